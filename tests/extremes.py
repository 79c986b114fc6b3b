"""Adversarial operands for the mat-mul bodies: GGUF weight bytes and f32 activations at the limits of every field.

synth.random_weights gives positive d in 2^-10 .. 2^-6, a positive second scale and uniform code bytes; real files do not look
like that (ggml's Q4_0 / Q5_0 quantisers store d = vmax / -8 or -16, Q4_1 / Q5_1 m is the block minimum, Q3_K / Q6_K / IQ4_XS
carry signed sub-block scales).  These generators start from synth.random_weights and overwrite bands of rows and some whole
blocks with the extremes of each field; the field offsets of every block type are written out below (include/lfamd_blocks.h).

Weight rows, by row % 8 (BAND_*):
  0 codes all minimum            1 codes all maximum          2 sub-block scales at their maximum (codes random)
  3 signed scales at their most negative (Q3_K -32, Q6_K -128, IQ4_XS -32); scales 0 where they are unsigned
  4 scales alternating min / max over maximal codes            5 .. 7 random codes and scales
then, over every row: the sign bit of d on every other block, a negative m / dmin on every third block (types that have one),
every fifth block's code bytes mirrored (x ^ 0xFF), d = 0 on block 5 mod 7, an f16-subnormal d (2^-20) on block 3 mod 7, and
row ZERO_ROW with d = dmin = 0 in every block.  Q8_0 codes never take -128 (the quantiser's rule).
"""
from __future__ import annotations

import numpy as np

from llamafile_amd import _hip, ggml_types as T, synth

BAND_MIN, BAND_MAX, BAND_SCMAX, BAND_SCNEG, BAND_ALT = 0, 1, 2, 3, 4
ZERO_ROW = 6  # every block: d = dmin = 0

# per type: byte ranges of the code fields (low bits and high bits alike) and of the sub-block scales, the f16 d offset, the
# f16 second-scale offset (dmin / m) or None, and the byte values of the scale field at its max / most negative (or 0)
_CODES = {
    T.Q4_0: [(2, 18)], T.Q4_1: [(4, 20)], T.Q5_0: [(2, 6), (6, 22)], T.Q5_1: [(4, 8), (8, 24)], T.Q8_0: [(2, 34)],
    T.Q2_K: [(16, 80)], T.Q3_K: [(0, 32), (32, 96)], T.Q4_K: [(16, 144)], T.Q5_K: [(16, 48), (48, 176)],
    T.Q6_K: [(0, 128), (128, 192)], T.IQ4_XS: [(8, 136)],
}
_SCALES = {T.Q2_K: (0, 16), T.Q3_K: (96, 108), T.Q4_K: (4, 16), T.Q5_K: (4, 16), T.Q6_K: (192, 208), T.IQ4_XS: (2, 8)}
_SC_MAX = {T.Q2_K: 0xFF, T.Q3_K: 0xFF, T.Q4_K: 0xFF, T.Q5_K: 0xFF, T.Q6_K: 0x7F, T.IQ4_XS: 0xFF}
_SC_MIN = {T.Q2_K: 0x00, T.Q3_K: 0x00, T.Q4_K: 0x00, T.Q5_K: 0x00, T.Q6_K: 0x80, T.IQ4_XS: 0x00}
SIGNED_SCALES = (T.Q3_K, T.Q6_K, T.IQ4_XS)
D_OFF = {t: synth._SCALE_OFF[t][0] for t in T.QUANT_WEIGHT_TYPES}
M_OFF = {t: synth._SCALE_OFF[t][1] for t in T.QUANT_WEIGHT_TYPES}

# the value of one weight of a block whose codes are all minimum / all maximum and whose sub-block scales are all at the byte
# value _SC_MAX (band 1) or _SC_MIN, as (code, sub-block scale, mins multiplier): w = d * sc * q - dmin * mm (K-quants),
# d * q + m (Q4_1 / Q5_1), d * q (the rest)
CODE_MIN = {T.Q4_0: -8, T.Q4_1: 0, T.Q5_0: -16, T.Q5_1: 0, T.Q8_0: -127, T.Q2_K: 0, T.Q3_K: -4, T.Q4_K: 0, T.Q5_K: 0,
            T.Q6_K: -32, T.IQ4_XS: -127}
CODE_MAX = {T.Q4_0: 7, T.Q4_1: 15, T.Q5_0: 15, T.Q5_1: 31, T.Q8_0: 127, T.Q2_K: 3, T.Q3_K: 3, T.Q4_K: 15, T.Q5_K: 31,
            T.Q6_K: 31, T.IQ4_XS: 113}
SC_MAX = {T.Q2_K: 15, T.Q3_K: 31, T.Q4_K: 63, T.Q5_K: 63, T.Q6_K: 127, T.IQ4_XS: 31}
SC_NEG = {T.Q2_K: 0, T.Q3_K: -32, T.Q4_K: 0, T.Q5_K: 0, T.Q6_K: -128, T.IQ4_XS: -32}
MIN_MAX = {T.Q2_K: 15, T.Q4_K: 63, T.Q5_K: 63}  # the 4- / 6-bit mins multiplier when every scale byte is _SC_MAX


def _blocks(raw, t):
    rows = raw.shape[0]
    return raw.reshape(rows, raw.shape[1] // T.TYPE_SIZE[t], T.TYPE_SIZE[t])


def _set_codes(blk, sel, t, byte):
    for a, b in _CODES[t]:
        blk[sel, ..., a:b] = byte
    if t == T.Q8_0 and byte == 0x00:  # minimum int8 code the quantiser emits: -127
        blk[sel, ..., 2:34] = 0x81
    if t == T.Q8_0 and byte == 0xFF:
        blk[sel, ..., 2:34] = 0x7F


def _f16(v):
    return np.array(v, dtype=np.float16).view(np.uint8)


def _get_f16(blk, off):
    return np.ascontiguousarray(blk[:, :, off:off + 2]).view(np.float16)[..., 0].astype(np.float32)


def _put_f16(blk, off, vals):
    blk[:, :, off:off + 2] = np.asarray(vals, dtype=np.float32).astype(np.float16)[..., None].view(np.uint8)


def extreme_weights(t: int, m: int, k: int, seed: int, real_scale: bool = False) -> np.ndarray:
    """Raw GGUF bytes [m, row_size(t, k)] of type t with the bands and blocks of the module docstring.  real_scale: the block
    scales are then moved by 2^-5 into the 2^-15 .. 2^-11 of real K-quant files (synth.rescale_blocks)."""
    raw = synth.random_weights(t, m, k, seed).copy()
    blk = _blocks(raw, t)
    nb = blk.shape[1]
    band = np.arange(m) % 8
    _set_codes(blk, band == BAND_MIN, t, 0x00)
    _set_codes(blk, band == BAND_MAX, t, 0xFF)
    _set_codes(blk, band == BAND_ALT, t, 0xFF)
    if t in _SCALES:
        a, b = _SCALES[t]
        blk[band == BAND_MIN, :, a:b] = _SC_MAX[t]
        blk[band == BAND_MAX, :, a:b] = _SC_MAX[t]
        blk[band == BAND_SCMAX, :, a:b] = _SC_MAX[t]
        blk[band == BAND_SCNEG, :, a:b] = _SC_MIN[t]
        blk[band == BAND_ALT, :, a:b] = np.tile(np.array([_SC_MIN[t], _SC_MAX[t]], np.uint8), (b - a + 1) // 2)[:b - a]
    # whole blocks, every row
    blk[:, 1::5] = _mirror_codes(blk[:, 1::5], t)
    d = _get_f16(blk, D_OFF[t])
    d[:, 1::2] = -d[:, 1::2]
    if M_OFF[t] is not None:
        mm = _get_f16(blk, M_OFF[t])
        mm[:, 1::3] = -mm[:, 1::3]
        mm[ZERO_ROW] = 0.0
        _put_f16(blk, M_OFF[t], mm)
    d[:, 5::7] = 0.0
    d[:, 3::7] = np.float32(2.0 ** -20) * np.where(np.arange(nb)[3::7] % 2, -1, 1)
    d[ZERO_ROW] = 0.0
    _put_f16(blk, D_OFF[t], d)
    if real_scale:
        synth.rescale_blocks(t, raw, 2.0 ** -5)
    return raw


def _mirror_codes(blk, t):
    blk = blk.copy()
    for a, b in _CODES[t]:
        blk[..., a:b] ^= 0xFF
    if t == T.Q8_0:
        q = blk[..., 2:34].view(np.int8)
        q[q == -128] = -127
    return blk


def edge_scale_weights(t: int, m: int, k: int, seed: int, inside: bool) -> np.ndarray:
    """Weights with a few blocks at the limit of the scaled batch bodies' f16 range, just inside or just outside it:
    Q4_K / Q5_K f16(|d| * 63) * 1024 against 65504, Q6_K |d| * 4064 against 65504, Q8_0 |d| * 127 against 65504 (the f16 image f16(d * q) of
    gemm_lf.hip).  Every other block keeps synth's scales; the edge blocks carry maximal codes and sub-block scales."""
    lim = {T.Q4_K: (1.0146484375, 1.015625), T.Q5_K: (1.0146484375, 1.015625), T.Q6_K: (16.109375, 16.125),
           T.Q8_0: (515.5, 516.0)}[t]
    raw = synth.random_weights(t, m, k, seed).copy()
    blk = _blocks(raw, t)
    sel = (np.arange(m) % 11 == 3)
    _set_codes(blk, sel, t, 0xFF)
    if t in _SCALES:
        a, b = _SCALES[t]
        blk[sel, :, a:b] = _SC_MAX[t]
    d = _get_f16(blk, D_OFF[t])
    v = lim[0] if inside else lim[1]
    d[sel, 0] = v
    d[sel, -1] = -v
    _put_f16(blk, D_OFF[t], d)
    return raw


# ------------------------------------------------------------------------------------------------------------------------
# activations, by token j % 16 (KINDS)
KINDS = ("1e-7", "2e-3", "zero block", "1e3", "3e5", "zero token", "constant blocks", "alternating", "1e-6 spread",
         "outlier channels", "1", "3e5 constant", "1e-7 b", "3e5 b", "1e3 b", "2e-3 b")
ZERO_TOKEN = 5
_MAG = {0: 1e-7, 1: 2e-3, 2: 1.0, 3: 1e3, 4: 3e5, 8: 1.0, 9: 1.0, 10: 1.0, 12: 1e-7, 13: 3e5, 14: 1e3, 15: 2e-3}


def extreme_activations(n: int, k: int, seed: int) -> np.ndarray:
    """f32 [n, k]: token j is of kind KINDS[j % 16] — per-token magnitudes 1e-7 .. 3e5, an all-zero token, a token with an
    all-zero 32-block and 256-block, constant blocks (Q8_K codes all -128, Q8_0 / Q8_1 codes +-127), full-scale alternating
    signs, one token whose 32-blocks alternate between 1 and 1e-6, outlier channels at 1e3x inside an ordinary token."""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, k), dtype=np.float32) * 2 - 1).astype(np.float32)
    nb32 = k // 32
    for j in range(n):
        kind = j % 16
        if kind in _MAG:
            x[j] *= np.float32(_MAG[kind])
        if kind == 2:
            x[j, 32:64] = 0.0
            if k >= 512:
                x[j, 256:512] = 0.0
        elif kind == ZERO_TOKEN:
            x[j] = 0.0
        elif kind == 6:
            sgn = np.where(np.arange(k) // 256 % 2 == 0, 1.0, -1.0).astype(np.float32)
            x[j] = np.float32(0.75) * sgn
        elif kind == 7:
            x[j] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0).astype(np.float32)
        elif kind == 8:
            x[j] *= np.repeat(np.where(np.arange(nb32) % 2 == 0, 1.0, 1e-6), 32).astype(np.float32)
        elif kind == 9:
            for c in (3, k // 2 + 7, k - 5):
                x[j, c] = np.float32(1e3) * (1.0 if c % 2 else -1.0)
        elif kind == 11:
            x[j] = np.float32(-3e5)
    return x


def for_vec_dot(x: np.ndarray, vec_dot_type: int) -> np.ndarray:
    """The activations a weight type can be fed.  Q8_1 blocks store d = amax / 127 and s = d * sum(q) as two f16 fields: beyond
    |x| ~ 2047 s overflows (quantize_row_q8_1 writes inf), and below |x| ~ 8e-3 d leaves f16's normal range while s does not, so
    the two fields stop describing the same block.  For Q4_1 / Q5_1 such tokens are scaled to a largest |x| of 1e3 and such
    32-blocks to one of 1e-2."""
    if vec_dot_type != T.Q8_1:
        return x
    x = x.copy()
    amax = np.abs(x).max(axis=1)
    x[amax > 1e3] *= (np.float32(1e3) / amax[amax > 1e3])[:, None]
    xb = x.reshape(x.shape[0], -1, 32)  # (32-blocks: the small side is a property of each block's own d)
    bmax = np.abs(xb).max(axis=2)
    small = (bmax > 0) & (bmax < 1e-2)
    xb[small] *= (np.float32(1e-2) / bmax[small])[:, None]
    return x


# ------------------------------------------------------------------------------------------------------------------------
# One entry per batch body the dispatcher can pick (test_gpu_operand_extremes.py feeds them the operands above,
# test_gpu_operand_layouts.py varies where their operands sit).  Flags by the names of CASE_FLAGS.
CASE_FLAGS = {"precise": _hip.FLAG_PRECISE, "narrow": _hip.FLAG_GEMM_NARROW, "plain": _hip.FLAG_GEMM_PLAIN,
              "q80_exact": _hip.FLAG_Q80_EXACT, "generic": _hip.FLAG_FORCE_GENERIC}
# (type, m, n, k, flags, expected answer of lfamd_mul_mat_is_exact or None)
CASES = [
    # small batch gemm_sb (SB_SHAPES: at most one row tile per CU): the int8 body for Q4_K at 4 tokens, f16 bodies at 9 .. 32
    (T.Q4_K, 1000, 4, 2048, (), True),
    (T.Q5_K, 1000, 9, 2048, (), True), (T.Q5_K, 1000, 32, 2048, (), True),
    (T.Q6_K, 1000, 9, 2048, (), True), (T.Q6_K, 1000, 17, 2048, (), True), (T.Q6_K, 1000, 32, 2048, (), True),
    # the int8 body: 4096 x 4096 x 512 class grid
    (T.Q4_K, 4096, 512, 4096, (), True),
    # scaled f16 bodies at 512 tokens: the 14336-row Q4_K grid (too many tiles for the int8 body), Q5_K, Q6_K
    (T.Q4_K, 14336, 512, 4096, (), False), (T.Q5_K, 4096, 512, 4096, (), False), (T.Q6_K, 4096, 512, 4096, (), False),
    # the exact-code f16 bodies
    (T.Q4_K, 1024, 200, 2048, ("precise",), True), (T.Q4_K, 1024, 200, 2048, ("narrow",), True),
    (T.Q4_K, 1024, 200, 2048, ("plain",), True), (T.Q5_K, 1024, 200, 2048, ("precise",), True),
    (T.Q5_K, 1024, 200, 2048, ("narrow",), True), (T.Q5_K, 1024, 200, 2048, ("plain",), True),
    (T.Q6_K, 1024, 200, 2048, ("precise",), None), (T.Q6_K, 1024, 200, 2048, ("narrow",), None),
    # canonical image (n > 8)
    (T.Q2_K, 256, 64, 1024, (), True), (T.Q3_K, 256, 64, 1024, (), True), (T.IQ4_XS, 256, 64, 1024, (), False),
    # legacy 32-blocks: P40, PCL
    (T.Q4_0, 256, 64, 1024, (), True), (T.Q4_1, 256, 64, 1024, (), True), (T.Q5_0, 256, 64, 1024, (), True),
    (T.Q5_1, 256, 64, 1024, (), True),
    # Q8_0: the f16 MFMA body by default; the bit-exact kernel by flag and for rows that are not whole 128-weight quads
    (T.Q8_0, 512, 200, 1024, (), False), (T.Q8_0, 512, 64, 1024, ("q80_exact",), True), (T.Q8_0, 512, 64, 1056, (), True),
    # the generic kernels: rows kept as GGUF rows (legacy types, not whole 256-weight groups)
    (T.Q4_0, 100, 40, 288, ("generic",), True), (T.Q4_1, 100, 40, 288, ("generic",), True),
    (T.Q5_0, 100, 40, 288, ("generic",), True), (T.Q5_1, 100, 40, 288, ("generic",), True),
    (T.Q8_0, 100, 40, 288, (), True), (T.Q4_0, 100, 3, 288, ("generic",), True),
]


def case_id(c):
    t, m, n, k, fl, _ = c
    return f"{T.NAMES[t]}-{m}x{n}x{k}" + ("-" + "+".join(fl) if fl else "")
