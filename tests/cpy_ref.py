"""NumPy restatement of lfamd_cpy (include/lfamd_hip.h): the scalar rules of ggml's quantize_row_<type>_reference as the reference's
device copies state them (ggml-cuda.cu.patch:4330-4722), in f32 with every product rounded before the add that follows it, and the
expected destination image of a call — the allocation as it was, with the destination's elements replaced and nothing else.

quantize(t, x): x f32 [blocks, 32] -> uint8 [blocks, type size].  All arithmetic on np.float32 arrays, so that every operation rounds
to f32 once; roundf (half away from zero) and the truncating casts are taken on exact f64 copies of f32 values."""
import numpy as np

from llamafile_amd import ggml_types as T

KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.float32)
BLOCK_TYPES = (T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL)
F32 = np.float32


def _f16_bytes(v):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(v.astype(np.float16)).view(np.uint8).reshape(-1, 2)


def _inverse(d):
    with np.errstate(divide="ignore"):
        return np.where(d != 0, F32(1.0) / d, F32(0.0)).astype(F32)


def _first_absmax(x):
    """vmax: the first element with the largest |x| (strict <, from amax = 0: an all-zero block keeps +0)."""
    a = np.abs(x)
    i = np.argmax(a, axis=1)
    v = x[np.arange(len(x)), i]
    return np.where(a.max(axis=1) > 0, v, F32(0.0)).astype(F32)


def _first(x, arg):
    return x[np.arange(len(x)), arg(x, axis=1)]  # argmin / argmax: the first of equal values (-0 == +0)


def _nibbles(codes):
    return (codes[:, :16] | codes[:, 16:] << 4).astype(np.uint8)


def _qh(codes):
    bits = ((codes >> 4) & 1).astype(np.uint32)
    return np.ascontiguousarray((bits << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)).view(np.uint8).reshape(-1, 4)


def _trunc_i8(v):
    return np.trunc(v.astype(np.float64)).astype(np.int64)


def iq4nl_index(y):
    """best_index_int8: the nearest codebook value, a tie to the upper index."""
    mu = 1 + (y[..., None] >= KVALUES[1:15]).sum(axis=-1)
    pick = np.where((y - KVALUES[mu - 1]).astype(F32) < (KVALUES[mu] - y).astype(F32), mu - 1, mu)
    return np.where(y <= KVALUES[0], 0, np.where(y >= KVALUES[15], 15, pick)).astype(np.int64)


def quantize(t, x):
    with np.errstate(over="ignore", invalid="ignore"):  # (inputs outside the call's domain still get the scalar rule's bytes)
        return _quantize(t, np.ascontiguousarray(x, dtype=F32).reshape(-1, 32))


def _quantize(t, x):
    if t == T.Q8_0:
        d = (np.abs(x).max(axis=1) / F32(127.0)).astype(F32)
        y = (x * _inverse(d)[:, None]).astype(np.float64)
        codes = (np.sign(y) * np.floor(np.abs(y) + 0.5)).astype(np.int8)
        return np.concatenate([_f16_bytes(d), codes.view(np.uint8)], axis=1)
    if t in (T.Q4_0, T.Q5_0, T.IQ4_NL):
        vmax = _first_absmax(x)
        d = (vmax / F32({T.Q4_0: -8.0, T.Q5_0: -16.0, T.IQ4_NL: -127.0}[t])).astype(F32)
        y = (x * _inverse(d)[:, None]).astype(F32)
        if t == T.IQ4_NL:
            codes = iq4nl_index(y)
            q = KVALUES[codes]
            w = (x * x).astype(F32)
            sumqx, sumq2 = np.zeros(len(x), F32), np.zeros(len(x), F32)
            for j in range(16):  # the reference's step: the pair (j, j + 16), each product chain left to right
                a, b = j, j + 16
                sumqx = (sumqx + ((w[:, a] * q[:, a]).astype(F32) * x[:, a] + (w[:, b] * q[:, b]).astype(F32) * x[:, b]).astype(F32)).astype(F32)
                sumq2 = (sumq2 + ((w[:, a] * q[:, a]).astype(F32) * q[:, a] + (w[:, b] * q[:, b]).astype(F32) * q[:, b]).astype(F32)).astype(F32)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(sumq2 > 0, sumqx / sumq2, d).astype(F32)
            return np.concatenate([_f16_bytes(d), _nibbles(codes)], axis=1)
        off, top = (F32(8.5), 15) if t == T.Q4_0 else (F32(16.5), 31)
        codes = np.minimum(top, _trunc_i8((y + off).astype(F32)))
        if t == T.Q4_0:
            return np.concatenate([_f16_bytes(d), _nibbles(codes)], axis=1)
        return np.concatenate([_f16_bytes(d), _qh(codes), _nibbles(codes & 15)], axis=1)
    if t in (T.Q4_1, T.Q5_1):
        lo, hi = _first(x, np.argmin), _first(x, np.argmax)
        d = ((hi - lo).astype(F32) / F32(15.0 if t == T.Q4_1 else 31.0)).astype(F32)
        y = ((x - lo[:, None]).astype(F32) * _inverse(d)[:, None]).astype(F32)
        codes = _trunc_i8((y + F32(0.5)).astype(F32))
        if t == T.Q4_1:
            return np.concatenate([_f16_bytes(d), _f16_bytes(lo), _nibbles(np.minimum(15, codes))], axis=1)
        return np.concatenate([_f16_bytes(d), _f16_bytes(lo), _qh(codes), _nibbles(codes & 15)], axis=1)
    raise ValueError(t)


def scale_of(t, raw):
    """|d| of each block, f64."""
    return np.abs(np.ascontiguousarray(raw[:, :2]).view(np.float16)[:, 0].astype(np.float64))


# ---- layouts
def unit_of(t):
    """(elements, bytes) of the unit lfamd_cpy moves: an element, or a 32-block."""
    return (32, T.TYPE_SIZE[t]) if t in BLOCK_TYPES else (1, 4 if t == T.F32 else 2)


def unit_offsets(t, ne, nb):
    """Byte offsets of the units of a tensor in flattened order (index 0 fastest)."""
    e = unit_of(t)[0]
    n = [ne[0] // e, ne[1], ne[2], ne[3]]
    o = np.zeros((n[3], n[2], n[1], n[0]), np.int64)
    for axis, d in zip((3, 2, 1, 0), range(4)):
        shape = [1, 1, 1, 1]
        shape[axis] = n[d]
        o = o + (np.arange(n[d], dtype=np.int64) * nb[d]).reshape(shape)
    return o.reshape(-1)


def gather(buf, base, t, ne, nb):
    """The tensor's units as bytes [units, unit size], flattened order, from the uint8 allocation buf."""
    idx = base + unit_offsets(t, ne, nb)[:, None] + np.arange(unit_of(t)[1])
    return buf[idx]


def convert(src_type, dst_type, units):
    """Source units (bytes) -> destination units (bytes)."""
    if src_type == dst_type:
        return units
    assert src_type == T.F32
    x = np.ascontiguousarray(units).view(F32)
    if dst_type == T.F16:
        return _f16_bytes(x.reshape(-1))
    return quantize(dst_type, x.reshape(-1, 32))


def expected_image(dst_buf, dst_base, dst_type, dst_ne, dst_nb, src_buf, src_base, src_type, src_ne, src_nb):
    """The destination allocation after the call: dst_buf with the destination's elements replaced, every other byte as it was."""
    s_ne = list(src_ne)
    if dst_type in BLOCK_TYPES and src_type == T.F32:  # the source in runs of 32 floats
        units = gather(src_buf, src_base, T.F32, s_ne, src_nb).reshape(-1, 128)
    else:
        units = gather(src_buf, src_base, src_type, s_ne, src_nb)
    out = dst_buf.copy()
    data = convert(src_type, dst_type, units)
    idx = dst_base + unit_offsets(dst_type, dst_ne, dst_nb)[:, None] + np.arange(unit_of(dst_type)[1])
    out[idx] = data
    return out
