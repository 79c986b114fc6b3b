"""NumPy side of the LFAMD_TYPE_STAGED_Q80 image (the staged activations of the Q8_0-weight loader-wave batch body, csrc/gemm_lf.hip;
written by lfamd_rms_norm_quantize_b32 / lfamd_swiglu_quantize_b32, csrc/norm_quant.hip): its decoder and encoder, and what it holds
for given Q8_0 rows as oracle.quantize writes them.  Pinned without a GPU by tests/test_producer80_ref.py; used on the GPU by
tests/test_gpu_producers_q80.py.

The image (csrc/lfamd_internal.h, lfamd_q80_image_of), n_pad = n rounded up to 128, packed without padding:
    Xh        f16 [k / 128][n_pad][128]   f16(f32(f16(d)) * stage * code), rounded once from the exact product; inside the 256 bytes of a
                                          token and 128-weight quad, block blk, elements 4 j .. 4 j + 3 sit at byte
                                          (2 s + (j >> 2)) * 16 + (blk & 1) * 8 with s = 2 (j & 3) + (blk >> 1)
    stage     f32 [n_pad]                 2^(9 - ilogb(D)), D = f32(f16(max |y| of the row / 127)) * 127 = the row's largest stored d * 127
    tok_scale f32 [n_pad]                 2^(ilogb(D) - 9)
D zero or not finite: 1 and 1.  Padding tokens n .. n_pad: Xh zero, stage 1, tok_scale 1.
"""
from __future__ import annotations

import numpy as np

from llamafile_amd import ggml_types as T
from producer32_ref import b32_fields
from producer_ref import n_pad_of

f32 = np.float32


def _chunk_perm() -> np.ndarray:
    """f16 position within a token's quad (128 values) -> element index of the quad."""
    perm = np.empty(128, dtype=np.int64)
    for e in range(128):
        blk, j, r = e >> 5, (e & 31) >> 2, e & 3
        s = 2 * (j & 3) + (blk >> 1)
        byte = (2 * s + (j >> 2)) * 16 + (blk & 1) * 8 + 2 * r
        perm[byte // 2] = e
    assert sorted(perm.tolist()) == list(range(128))
    return perm


Q80_PERM = _chunk_perm()  # image position -> element
Q80_INV = np.argsort(Q80_PERM)  # element -> image position


def q80_image_offsets(k: int, n: int):
    """(n_pad, offset of stage, offset of tok_scale, total bytes)."""
    npad = n_pad_of(n)
    stage = npad * k * 2
    return npad, stage, stage + npad * 4, stage + npad * 8


def q80_image_size(k: int, n: int) -> int:
    return q80_image_offsets(k, n)[3]


def q80_image_decode(image: np.ndarray, k: int, n: int):
    """uint8 [q80_image_size] -> (Xh f16 [n_pad, k] in element order, stage f32 [n_pad], tok_scale f32 [n_pad])."""
    nq = k // 128
    npad, so, to, total = q80_image_offsets(k, n)
    assert image.size == total
    xh = image[:so].view(np.float16).reshape(nq, npad, 128)[:, :, Q80_INV].transpose(1, 0, 2).reshape(npad, k)
    return xh, image[so:to].view(np.float32).copy(), image[to:total].view(np.float32).copy()


def q80_image_encode(xh, stage, tok_scale, k: int, n: int) -> np.ndarray:
    """The inverse of q80_image_decode (arrays of n_pad tokens)."""
    nq = k // 128
    npad, so, to, total = q80_image_offsets(k, n)
    out = np.empty(total, dtype=np.uint8)
    q = np.asarray(xh, np.float16).reshape(npad, nq, 128).transpose(1, 0, 2)[:, :, Q80_PERM]
    out[:so] = np.ascontiguousarray(q).view(np.uint8).reshape(-1)
    out[so:to] = np.ascontiguousarray(stage, dtype=np.float32).view(np.uint8)
    out[to:] = np.ascontiguousarray(tok_scale, dtype=np.float32).view(np.uint8)
    return out


def q80_row_factors(d: np.ndarray):
    """d f16 [n, k / 32] (the stored block scales) -> (stage f32 [n], tok_scale f32 [n]).  f16(amax / 127) is monotonic in amax, so
    the row's largest stored |d| is f16(max |y| of the row / 127)."""
    D = (np.abs(d.astype(np.float32)).max(axis=1) * f32(127.0)).astype(np.float32)
    ok = (D > 0) & (D < f32(3.0e38))
    e = np.frexp(np.where(ok, D, f32(1.0)))[1].astype(np.int64) - 1  # ilogb
    stage = np.where(ok, np.ldexp(np.float64(1.0), 9 - e), 1.0).astype(np.float32)
    tok = np.where(ok, np.ldexp(np.float64(1.0), e - 9), 1.0).astype(np.float32)
    return stage, tok


def q80_image_model(q80_rows: np.ndarray, k: int):
    """What the image holds for the tokens whose quantize_row_q8_0 blocks are q80_rows: (Xh f16 [n, k], stage f32 [n], tok_scale f32
    [n]).  d * stage * code is exact in f64 (and in f32: 11 + 7 significant bits), so the conversion to f16 is its only rounding."""
    d, _, q = b32_fields(q80_rows, T.Q8_0, k)
    n = q80_rows.shape[0]
    stage, tok = q80_row_factors(d)
    with np.errstate(over="ignore", invalid="ignore"):
        v = d.astype(np.float64)[:, :, None] * stage.astype(np.float64)[:, None, None] * q.astype(np.float64)
        xh = v.reshape(n, k).astype(np.float16)
    return xh, stage, tok


def q80_image_of_rows(q80_rows: np.ndarray, k: int) -> np.ndarray:
    """The whole image, padding included, for n = len(q80_rows) tokens."""
    n = q80_rows.shape[0]
    npad = n_pad_of(n)
    xh, stage, tok = np.zeros((npad, k), np.float16), np.ones(npad, np.float32), np.ones(npad, np.float32)
    xh[:n], stage[:n], tok[:n] = q80_image_model(q80_rows, k)
    return q80_image_encode(xh, stage, tok, k, n)
