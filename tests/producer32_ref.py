"""NumPy side of the 32-block fused producers (lfamd_rms_norm_quantize_b32, lfamd_swiglu_quantize_b32: csrc/norm_quant.hip): the
fields of Q8_0 / Q8_1 rows, the decoder and encoder of the LFAMD_TYPE_STAGED_B32 image, what that image holds for given Q8_1 rows, and
the rows whose y is exact so that only the quantiser's rounding is under test.  Pinned without a GPU by tests/test_producer32_ref.py;
used on the GPU by tests/test_gpu_producers_b32.py.

The image (csrc/lfamd_internal.h, lfamd_b32_image_of), n_pad = n rounded up to 128, nb = k / 256, each part starting on 256 bytes:
    Xh  f16 [nb][n_pad][256]   codes as f16
    d8T f32 [nb * 8][n_pad]    f32(f16(d))
    sT  f32 [nb * 8][n_pad]    f32(f16(sum * d)), d not yet rounded
"""
from __future__ import annotations

import numpy as np

from llamafile_amd import ggml_types as T
from producer_ref import _up256, n_pad_of

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- Q8_0 / Q8_1 rows
def b32_fields(rows: np.ndarray, vdt: int, k: int):
    """Q8_0 / Q8_1 rows uint8 [n, k / 32 * (34 | 36)] -> (d f16 [n, nb32], s f16 [n, nb32] or None, codes int8 [n, nb32, 32])."""
    n, nb32 = rows.shape[0], k // 32
    bs = T.TYPE_SIZE[vdt]
    b = np.ascontiguousarray(rows).reshape(n, nb32, bs)
    d = np.ascontiguousarray(b[:, :, 0:2]).view(np.float16)[..., 0]
    s = np.ascontiguousarray(b[:, :, 2:4]).view(np.float16)[..., 0] if vdt == T.Q8_1 else None
    q = np.ascontiguousarray(b[:, :, bs - 32:]).view(np.int8)
    return d, s, q


# ------------------------------------------------------------------------------------------------------------------- the image
def b32_image_offsets(k: int, n: int):
    """(n_pad, offset of d8T, offset of sT, total bytes)."""
    nb, npad = k // 256, n_pad_of(n)
    d8t = _up256(npad * k * 2)
    st = d8t + _up256(nb * 8 * npad * 4)
    return npad, d8t, st, st + _up256(nb * 8 * npad * 4)


def b32_image_size(k: int, n: int) -> int:
    return b32_image_offsets(k, n)[3]


def b32_image_decode(image: np.ndarray, k: int, n: int):
    """uint8 [b32_image_size] -> (Xh f16 [n_pad, k], d8 f32 [n_pad, k / 32], s f32 [n_pad, k / 32]), token-major."""
    nb = k // 256
    npad, d8t, st, total = b32_image_offsets(k, n)
    assert image.size == total
    xh = image[:npad * k * 2].view(np.float16).reshape(nb, npad, 256).transpose(1, 0, 2).reshape(npad, k)
    d8 = image[d8t:d8t + nb * 8 * npad * 4].view(np.float32).reshape(nb * 8, npad).T
    s = image[st:st + nb * 8 * npad * 4].view(np.float32).reshape(nb * 8, npad).T
    return xh, d8, s


def b32_image_encode(xh, d8, s, k: int, n: int, fill: int = 0) -> np.ndarray:
    """The inverse of b32_image_decode (token-major arrays of n_pad tokens); bytes of no part are `fill`."""
    nb = k // 256
    npad, d8t, st, total = b32_image_offsets(k, n)
    out = np.full(total, fill, dtype=np.uint8)
    out[:npad * k * 2] = np.ascontiguousarray(np.asarray(xh, np.float16).reshape(npad, nb, 256).transpose(1, 0, 2)).view(np.uint8).reshape(-1)
    out[d8t:d8t + nb * 8 * npad * 4] = np.ascontiguousarray(np.asarray(d8, np.float32).T).view(np.uint8).reshape(-1)
    out[st:st + nb * 8 * npad * 4] = np.ascontiguousarray(np.asarray(s, np.float32).T).view(np.uint8).reshape(-1)
    return out


def b32_image_model(q81_rows: np.ndarray, k: int):
    """What the image holds for the tokens whose quantize_row_q8_1 blocks are q81_rows (Q8_0's d and codes are the same):
    (Xh f16 [n, k], d8 f32 [n, k / 32], s f32 [n, k / 32])."""
    d, s, q = b32_fields(q81_rows, T.Q8_1, k)
    return q.reshape(q.shape[0], k).astype(np.float16), d.astype(np.float32), s.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- rows with an exact y
def tie_values(k: int) -> np.ndarray:
    """f32 [k]: per 32-block 127 first (so d = amax / 127 = 1 and id = 1), then +-(j + 0.5) with alternating signs: every code is a
    tie, and roundf takes it away from zero (0.5 -> 1, -1.5 -> -2, 2.5 -> 3) where nearest-even gives 0, -2, 2."""
    j = np.arange(31)
    blk = np.concatenate([[127.0], (j + 0.5) * np.where(j % 2 == 0, 1.0, -1.0)]).astype(np.float32)
    return np.tile(blk, k // 32)


def tie_codes(k: int) -> np.ndarray:
    """int8 [k]: roundf of tie_values."""
    v = tie_values(k).astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int8)


def swiglu_tie_inputs(n: int, k: int, zero_block: int | None = None):
    """(gate, up) with silu(gate) * up == tie_values exactly: gate = 32 (1 + expf(-32) rounds to 1, so silu = 32) and up = v / 32.
    zero_block: that 32-block of every row is all zero (up = 0)."""
    v = tie_values(k)
    if zero_block is not None:
        v[32 * zero_block:32 * zero_block + 32] = 0.0
    g = np.full((n, k), 32.0, dtype=np.float32)
    u = np.tile((v / f32(32.0)).astype(np.float32), (n, 1))
    return g, u, np.tile(v, (n, 1))


def norm_tie_inputs(n: int, k: int, zero_block: int | None = None):
    """(x, weight, eps) with the norm's y == tie_values exactly: x = 2 everywhere (mean 4, scale 0.5 at eps = 0, x * scale = 1) and
    weight = v."""
    v = tie_values(k)
    if zero_block is not None:
        v[32 * zero_block:32 * zero_block + 32] = 0.0
    return np.full((n, k), 2.0, dtype=np.float32), v, 0.0, np.tile(v, (n, 1))
