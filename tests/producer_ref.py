"""CPU reference, image decoders and input generators for the fused producers (lfamd_rms_norm_quantize, lfamd_swiglu_quantize:
csrc/norm_quant.hip) and for lfamd_quantize_rows.  Plain NumPy: f32 steps where ggml rounds, f64 / exact sums elsewhere.  Pinned
without a GPU by tests/test_producer_ref.py; used on the GPU by tests/test_gpu_producers.py and tests/test_gpu_quantize_rows.py.

The arithmetic (norm_quant.hip header, include/lfamd_hip.h):
    RMS norm   S = sum_i (double)(x[i] * x[i]) (f32 products), mean = (float)(S / k), scale = 1.0f / sqrtf(mean + eps),
               y[i] = (x[i] * scale) * w[i]
    SwiGLU     y[i] = (g[i] / (1.0f + expf(-g[i]))) * u[i]
    Q8_K       per 256 values: first index of the largest |y| -> iscale = -128 / y[that], codes nearest-even clamped at 127,
               d = 1 / iscale, bsums of 16 (oracle.quantize is the yardstick; tests/test_extremes.py pins it)
and the two staged images, laid out as csrc/lfamd_internal.h (lfamd_i8_image_of, lfamd_kq_image_of) says.
"""
from __future__ import annotations

import math

import numpy as np

from extremes import extreme_activations

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------------------------ RMS norm
def rms_norm_ref(x: np.ndarray, w: np.ndarray | None, eps: float):
    """(y f32 [n, k], ambiguous bool [n]).  S is the exact sum of the f32 products; the kernel adds them in a tree and ggml in a
    loop, both in f64: within ~1e-14 relative of S.  A row is ambiguous when S moved by 1e-12 relative rounds to another f32 mean:
    only such a row may differ from y (it may equal either neighbour's result)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, k = x.shape
    y = np.empty_like(x)
    amb = np.zeros(n, dtype=bool)
    e = f32(eps)
    for r in range(n):
        S = math.fsum((x[r] * x[r]).astype(np.float64))
        mean = f32(S / k)
        amb[r] = f32(S * (1 - 1e-12) / k) != f32(S * (1 + 1e-12) / k)
        scale = f32(1.0) / np.sqrt(f32(mean + e))
        y[r] = x[r] * scale
        if w is not None:
            y[r] = y[r] * w
    return y, amb


# -------------------------------------------------------------------------------------------------------------------- SwiGLU
def swiglu_f32(g, u, e32):
    """The stated formula in f32 steps on a given f32 exp(-g)."""
    with np.errstate(over="ignore"):
        t = (f32(1.0) + e32).astype(np.float32)
        r = (g / t).astype(np.float32)
        return (r * u).astype(np.float32)


def swiglu_interval(g: np.ndarray, u: np.ndarray, n_ulp: int):
    """Element-wise (lo, hi) of the stated formula when expf(-g) is within n_ulp units (spacing of the rounded f64 value) of the f64
    exp.  Each step is monotone in the exponential, so the end points and the centre bracket.  An exponential that overflows f32 is
    inf, with the largest finite value as its neighbour."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e32 = np.exp(-g.astype(np.float64)).astype(np.float32)
        sp = np.spacing(e32)
        lo = np.maximum(e32 - f32(n_ulp) * sp, f32(0)).astype(np.float32)
        hi = (e32 + f32(n_ulp) * sp).astype(np.float32)
        over = np.isinf(e32)
        lo[over] = FLT_MAX if n_ulp > 0 else np.inf
        hi[over] = np.inf
    ys = np.stack([swiglu_f32(g, u, c) for c in (lo, e32, hi)])
    return ys.min(axis=0), ys.max(axis=0)


def outside(y: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> int:
    """How many elements of y are not inside [lo, hi] (a non-finite y counts)."""
    return int((~((y >= lo) & (y <= hi))).sum())


def smallest_n_ulp(y, g, u, top=4):
    """The smallest n_ulp in 0 .. top whose interval holds every element of y, and the counts outside for each; top + 1 if none."""
    counts = []
    for n in range(top + 1):
        counts.append(outside(y, *swiglu_interval(g, u, n)))
        if counts[-1] == 0:
            return n, counts
    return top + 1, counts


# ---------------------------------------------------------------------------------------------------------------- Q8_K blocks
def q8k_fields(rows: np.ndarray, k: int):
    """Q8_K rows uint8 [n, k / 256 * 292] -> (d f32 [n, nb], bsums int16 [n, nb, 16], codes int8 [n, nb, 256])."""
    n, nb = rows.shape[0], k // 256
    b = np.ascontiguousarray(rows).reshape(n, nb, 292)
    d = np.ascontiguousarray(b[:, :, 0:4]).view(np.float32)[..., 0]
    bs = np.ascontiguousarray(b[:, :, 4:36]).view(np.int16)
    q = np.ascontiguousarray(b[:, :, 36:292]).view(np.int8)
    return d, bs, q


# ------------------------------------------------------------------------------------------------- the int8 body's staged image
def _i8_perm():
    """byte position within a token's 256 -> code index: group g of eight codes c0 .. c7 sits at (g >> 2) * 32 + (g & 1) * 16 +
    ((g >> 1) & 1) * 8 as c0 c4 c1 c5 c2 c6 c3 c7."""
    perm = np.empty(256, dtype=np.int64)
    for g in range(32):
        at = (g >> 2) * 32 + (g & 1) * 16 + ((g >> 1) & 1) * 8
        for j, c in enumerate((0, 4, 1, 5, 2, 6, 3, 7)):
            perm[at + j] = 8 * g + c
    return perm


I8_PERM = _i8_perm()


def n_pad_of(n: int) -> int:
    return (n + 127) // 128 * 128


def i8_image_size(k: int, n: int) -> int:
    return n_pad_of(n) * (k // 256) * (256 + 4 + 32)


def i8_image_decode(image: np.ndarray, k: int, n: int):
    """uint8 [i8_image_size] -> (codes int8 [n_pad, nb, 256] in element order, d f32 [n_pad, nb], bsums f32 [n_pad, nb, 16]).
    Layout: Xq int8 [nb][n_pad][256], d8T f32 [nb][n_pad], Xs f16 [nb][n_pad][16], packed."""
    nb, npad = k // 256, n_pad_of(n)
    a, b = nb * npad * 256, nb * npad * 260
    assert image.size == i8_image_size(k, n)
    xq = image[:a].view(np.int8).reshape(nb, npad, 256)
    codes = np.empty_like(xq)
    codes[:, :, I8_PERM] = xq
    d = image[a:b].view(np.float32).reshape(nb, npad)
    xs = image[b:].view(np.float16).reshape(nb, npad, 16).astype(np.float32)
    return codes.transpose(1, 0, 2), d.T, xs.transpose(1, 0, 2)


def i8_image_encode(codes: np.ndarray, d: np.ndarray, bsums: np.ndarray) -> np.ndarray:
    """The inverse of i8_image_decode ([n_pad, nb, ...] arrays)."""
    xq = np.ascontiguousarray(codes.transpose(1, 0, 2)[:, :, I8_PERM]).view(np.uint8).reshape(-1)
    dd = np.ascontiguousarray(d.T, dtype=np.float32).view(np.uint8).reshape(-1)
    xs = np.ascontiguousarray(bsums.transpose(1, 0, 2)).astype(np.float16).view(np.uint8).reshape(-1)
    return np.concatenate([xq, dd, xs])


# ------------------------------------------------------------------------------------ the scaled f16 bodies' staged image
def _up256(v: int) -> int:
    return (v + 255) // 256 * 256


def scaled_image_offsets(k: int, n: int):
    """(n_pad, offset of tok_scale, offset of Xm, total bytes): each part starts on 256 bytes."""
    nb, npad = k // 256, n_pad_of(n)
    d8t = _up256(npad * k * 2)
    xm = d8t + _up256(nb * npad * 4)
    return npad, d8t, xm, xm + _up256(npad * nb * 32)


def scaled_image_size(k: int, n: int) -> int:
    return scaled_image_offsets(k, n)[3]


def scaled_image_decode(image: np.ndarray, k: int, n: int):
    """uint8 [scaled_image_size] -> (Xh f16 [n_pad, nb, 256], tok_scale f32 [n_pad], Xm f16 [n_pad, nb, 16]), as bit patterns'
    own dtypes.  Layout: Xh f16 [nb][n_pad][256], tok_scale f32 [n_pad], Xm f16 [nb][n_pad][16]."""
    nb = k // 256
    npad, d8t, xm, total = scaled_image_offsets(k, n)
    assert image.size == total
    xh = image[:npad * k * 2].view(np.float16).reshape(nb, npad, 256).transpose(1, 0, 2)
    ts = image[d8t:d8t + npad * 4].view(np.float32)
    m = image[xm:xm + npad * nb * 32].view(np.float16).reshape(nb, npad, 16).transpose(1, 0, 2)
    return xh, ts, m


def scaled_image_encode(xh, ts, xm, k: int, n: int, fill: int = 0) -> np.ndarray:
    npad, d8t, xmo, total = scaled_image_offsets(k, n)
    nb = k // 256
    out = np.full(total, fill, dtype=np.uint8)
    out[:npad * k * 2] = np.ascontiguousarray(xh.transpose(1, 0, 2)).view(np.uint8).reshape(-1)
    out[d8t:d8t + npad * 4] = np.ascontiguousarray(ts, dtype=np.float32).view(np.uint8)
    out[xmo:xmo + npad * nb * 32] = np.ascontiguousarray(xm.transpose(1, 0, 2)).view(np.uint8).reshape(-1)
    return out


def scaled_image_model(y: np.ndarray, q8k_rows: np.ndarray):
    """What the scaled image of the f32 rows y holds, from their Q8_K blocks: e = ilogb(max |y| of the row) - 9, tok_scale = 2^e,
    Xh = f16(f32(q) * (d * 2^-e)), Xm[j] = f16(f32(sum of codes 32 j .. 32 j + 31) * (d * 2^-e)) for j < 8 and 0 for j >= 8; an
    all-zero row has tok_scale = 1.  Returns (Xh f16 [n, nb, 256], tok_scale f32 [n], Xm f16 [n, nb, 16])."""
    n, k = y.shape
    d, _, q = q8k_fields(q8k_rows, k)
    amax = np.abs(y).max(axis=1)
    _, ex = np.frexp(amax)  # amax = f * 2^ex, f in [0.5, 1): ilogb = ex - 1
    e = np.where(amax > 0, ex - 1 - 9, 0).astype(np.int32)
    tok = np.ldexp(f32(1.0), e).astype(np.float32)
    inv = np.ldexp(f32(1.0), -e).astype(np.float32)
    xs = (d * inv[:, None]).astype(np.float32)
    xh = (q.astype(np.float32) * xs[:, :, None]).astype(np.float32).astype(np.float16)
    s32 = q.astype(np.int32).reshape(n, -1, 8, 32).sum(axis=3)
    xm = np.zeros((n, k // 256, 16), dtype=np.float16)
    xm[:, :, :8] = (s32.astype(np.float32) * xs[:, :, None]).astype(np.float32).astype(np.float16)
    return xh, tok, xm


def in_domain(y: np.ndarray) -> bool:
    """The producers' stated domain: finite, every row's largest |y| 0 or in [1e-30, 1e30], every 256-block's largest |y| 0 or
    >= 1e-30 (below that -128 / max overflows and the reference quantiser itself is undefined)."""
    a = np.abs(y)
    rmax = a.max(axis=1)
    bmax = a.reshape(y.shape[0], -1, 256).max(axis=2)
    return bool(np.isfinite(y).all() and (((rmax >= 1e-30) & (rmax <= 1e30)) | (rmax == 0)).all()
                and ((bmax >= 1e-30) | (bmax == 0)).all())


# ----------------------------------------------------------------------------------------------------------------- generators
WEIGHT_KINDS = ("none", "ones", "wide")


def norm_weight(kind: str, k: int, seed: int):
    """None; ones; or a wide one: magnitudes log-uniform in 1e-3 .. 1e3, a third negative, every 17th zero, channels 3 and k - 5 at
    1e3 (outliers), and for rows of at least three 256-blocks block 1 all zero and block 2 constant -0.5."""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(k, dtype=np.float32)
    assert kind == "wide"
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), k))
    w[rng.random(k) < 1 / 3] *= -1
    w = w.astype(np.float32)
    w[::17] = 0.0
    if k >= 768:
        w[256:512] = 0.0
        w[512:768] = -0.5
    w[3] = 1e3
    w[k - 5] = -1e3
    return w


def norm_input(n: int, k: int, seed: int, eps: float) -> np.ndarray:
    """extreme_activations; for eps == 0 the all-zero tokens (0 * 1 / sqrt(0) is not a number) become rows of 1e-7."""
    x = extreme_activations(n, k, seed)
    if eps == 0:
        zero = ~x.any(axis=1)
        x[zero] = f32(1e-7) * (np.random.default_rng(seed + 1).random((int(zero.sum()), k), dtype=np.float32) * 2 - 1)
    return x


GATE_KINDS = ("gauss3", "wide", "signed zeros", "tiny", "constant", "g alternating", "tie", "zero block")
G_CONSTANT, G_TIE = 4, 6


def swiglu_inputs(n: int, k: int, seed: int):
    """(gate, up) f32 [n, k].  up = extreme_activations (token j of kind j % 16); gate row j of kind gate_kind(j) = (j + j // 16) % 8,
    so that over 128 rows every gate kind meets every up kind (the constant, alternating and tie kinds set their row of up too):
      gauss3          3 x N(0, 1)
      wide            uniform -104 .. 90: expf(-g) overflows below ~ -88.7 (result -0 x up), 1 + expf(-g) = 1 above ~17
      signed zeros    +0 / -0 mixed: the whole row is zero
      tiny            |g| < 1e-3
      constant        g = 1, up = -0.75: every Q8_K code -128
      g alternating   g = +2, -2, ... with up = 0.75: silu(2) and silu(-2) differ, so the block maximum is at index 0
      tie             g = 2 with up = +c, -c, ... (even 256-blocks) or -c, +c, ... (odd): the largest |y| is shared by opposite
                      signs and the first index decides the sign of iscale; c is the row's largest |up|, or 1
      zero block      gauss3 with block 1 (block 0 of a one-block row) of the gate zero: a zero 256-block after the formula"""
    rng = np.random.default_rng(seed)
    u = extreme_activations(n, k, seed + 1)
    g = np.empty((n, k), dtype=np.float32)
    idx = np.arange(k)
    for j in range(n):
        kind = gate_kind(j)
        if kind == 0 or kind == 7:
            g[j] = (rng.standard_normal(k) * 3.0).astype(np.float32)
            if kind == 7:
                b = 1 if k >= 512 else 0
                g[j, 256 * b:256 * b + 256] = 0.0
        elif kind == 1:
            g[j] = rng.uniform(-104.0, 90.0, k).astype(np.float32)
        elif kind == 2:
            g[j] = np.where(rng.random(k) < 0.5, f32(0.0), f32(-0.0))
        elif kind == 3:
            g[j] = rng.uniform(-1e-3, 1e-3, k).astype(np.float32)
        elif kind == G_CONSTANT:
            g[j] = 1.0
            u[j] = -0.75
        elif kind == 5:
            g[j] = np.where(idx % 2 == 0, 2.0, -2.0)
            u[j] = 0.75
        else:
            c = f32(np.abs(u[j]).max()) or f32(1.0)
            g[j] = 2.0
            u[j] = c * np.where((idx + idx // 256) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return g, u


def gate_kind(j: int) -> int:
    return (j + j // 16) % len(GATE_KINDS)


def tie_rows(k: int, block: int, seed: int) -> np.ndarray:
    """f32 [4, k] for the plain quantisers: +1 / -1 alternating; -1 / +1 alternating; random rows whose every `block` has its
    largest |x| twice, the later one with the opposite sign (positive first, then negative first)."""
    rng = np.random.default_rng(seed)
    x = np.empty((4, k), dtype=np.float32)
    alt = np.where(np.arange(k) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x[0], x[1] = alt, -alt
    for r, sgn in ((2, 1.0), (3, -1.0)):
        v = (rng.random(k, dtype=np.float32) * 2 - 1).reshape(-1, block)
        v[:, 5] = f32(1.5 * sgn)
        v[:, block - 3] = f32(-1.5 * sgn)
        x[r] = v.reshape(-1)
    return x
