"""lfamd_cpy without a device: the NumPy rules the device tests rely on (tests/cpy_ref.py) against the oracle's quantize_row_q8_0, the
error of the dequantised blocks, hand-made blocks at the rules' corners, and every refusal of the call in the order include/lfamd_hip.h
states — with a NULL stream and bogus non-NULL pointers, so a refusal that came after a device call would fault instead of answering."""
import ctypes as C

import numpy as np
import pytest

import cpy_ref as R
import iq4nl_ref
from llamafile_amd import _hip, ggml_types as T
from oracle import ora

OK, UNSUPPORTED, INVALID = 0, -1, -2
F32 = np.float32


def random_blocks(seed, n=256, lo=-12.0, hi=12.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 32)).astype(F32)
    x[n // 2:] *= np.exp(rng.uniform(lo, hi, (n - n // 2, 1))).astype(F32)  # scales from 6e-6 to 1.6e5
    x[::7, 5] = 0.0
    return x


def extreme_blocks():
    rows = [np.zeros(32), np.full(32, 65504.0 * 127), np.full(32, 1e30), np.full(32, -3e-39), np.r_[np.full(31, 1e-8), 3e4],
            np.arange(32) - 15.5, (np.arange(32) - 16) * 0.5, np.r_[1.0, -1.0, np.zeros(30)]]
    return np.array(rows, dtype=F32)


# ---- the rules
def test_q8_0_is_the_oracles_quantize_row_q8_0_bit_for_bit():
    for x in (random_blocks(1), random_blocks(2) * F32(1e-3), extreme_blocks()):
        want = ora.quantize(T.Q8_0, x.reshape(1, -1)).reshape(-1, 34)
        assert np.array_equal(R.quantize(T.Q8_0, x), want)


def dequantise(t, raw):
    if t == T.IQ4_NL:
        return iq4nl_ref.dequantize(raw.reshape(1, -1)).reshape(-1, 32).astype(np.float64)
    return ora.dequantize(t, np.ascontiguousarray(raw.reshape(1, -1)), raw.shape[0] * 32).reshape(-1, 32).astype(np.float64)


def exact_blocks(t, seed):
    """Blocks on which the stored f16 d (and m) are the rule's f32 d (and min) and x * id is exact: d a power of two, the elements
    multiples of d / 4.  There the issue's bounds are theorems of the rule; on arbitrary inputs the rounding of d to f16 moves a value
    by up to |code| * 2^-11 |d| more (test_the_f16_rounding_of_d_is_the_only_excess_on_random_blocks measures it)."""
    rng = np.random.default_rng(seed)
    n = 128
    e = F32(2.0) ** rng.integers(-10, 10, (n, 1)).astype(F32)
    if t == T.Q8_0:
        q = rng.integers(-127 * 4, 127 * 4 + 1, (n, 32))
        q[:, 0] = 127 * 4
    elif t in (T.Q4_0, T.Q5_0, T.IQ4_NL):
        top = {T.Q4_0: 8, T.Q5_0: 16, T.IQ4_NL: 127}[t] * 4
        q = rng.integers(-top, top + 1, (n, 32))
        q[:, 3] = -top
    else:
        top = (15 if t == T.Q4_1 else 31) * 4
        q = rng.integers(0, top + 1, (n, 32))
        q[:, 1], q[:, 2] = 0, top
        q = q + 4 * rng.integers(-8, 8, (n, 1))  # min = a multiple of d: exact in f16
    return (q.astype(F32) * (e / F32(4.0))).astype(F32)


@pytest.mark.parametrize("t", R.BLOCK_TYPES, ids=lambda t: T.NAMES[t])
def test_the_dequantised_blocks_are_within_the_rules_bound(t):
    """|x - dequantised| <= |d| / 2 for Q8_0, Q4_1, Q5_1 (round to nearest); <= |d| for Q4_0, Q5_0 (the top code is clamped: x * id
    + 8.5 in [16, 16.5] gives 15, one step short).
    IQ4_NL: with d0 = vmax / -127 the codes are the nearest codebook values of y = x / d0 in [-127, 127]; inside the codebook the
    distance is at most half the largest gap, (113 - 89) / 2 = 12, above its top value 113 at most 127 - 113 = 14: |x - d0 q| <= 14 |d0|.
    The refit replaces d0 by the stored d: |x - d q| <= |x - d0 q| + |d - d0| |q| <= 14 |d0| + 127 |d - d0|, with d as stored (so the
    f16 rounding of d is part of the movement)."""
    x = exact_blocks(t, 5)
    raw = R.quantize(t, x)
    err = np.abs(x.astype(np.float64) - dequantise(t, raw)).max(axis=1)
    d = R.scale_of(t, raw)
    if t == T.IQ4_NL:
        d0 = np.abs(R._first_absmax(x).astype(np.float64) / 127.0)
        bound = 14 * d0 + 127 * np.abs(d - d0)
    else:
        bound = d / 2 if t in (T.Q8_0, T.Q4_1, T.Q5_1) else d
    print(T.NAMES[t], "largest err / bound", (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("t", R.BLOCK_TYPES, ids=lambda t: T.NAMES[t])
def test_the_f16_rounding_of_d_is_the_only_excess_on_random_blocks(t):
    """On arbitrary inputs the same bounds hold up to what the format itself adds: the stored d is f16(d), which moves a dequantised
    value by up to |code| 2^-11 |d| (codes up to 127, 8, 16, 15, 31), the stored m of Q4_1 / Q5_1 by 2^-11 |m|, and the f32
    rounding of x * id a few 2^-24 of the largest element.  (Scales from 0.02 to 3000: every d a normal f16.)"""
    x = random_blocks(9, lo=-4.0, hi=8.0)
    raw = R.quantize(t, x)
    err = np.abs(x.astype(np.float64) - dequantise(t, raw)).max(axis=1)
    d = R.scale_of(t, raw)
    amax = np.abs(x.astype(np.float64)).max(axis=1)
    top = {T.Q8_0: 127, T.Q4_0: 8, T.Q5_0: 16, T.Q4_1: 15, T.Q5_1: 31, T.IQ4_NL: 127}[t]
    fmt = top * 2.0 ** -11 * d * (1 + 2.0 ** -10) + 2.0 ** -11 * amax * (t in (T.Q4_1, T.Q5_1)) + 2.0 ** -20 * amax
    if t == T.IQ4_NL:
        d0 = np.abs(R._first_absmax(x).astype(np.float64) / 127.0)
        bound = 14 * d0 + 127 * np.abs(d - d0)
    else:
        bound = d / 2 if t in (T.Q8_0, T.Q4_1, T.Q5_1) else d
    print(T.NAMES[t], "largest err / bound", (err / bound).max(), "blocks over the bare bound", int((err > bound).sum()), "of", len(x))
    assert (err <= bound + fmt).all()


def d_of(raw):
    return np.ascontiguousarray(raw[:, :2]).view(np.float16)[:, 0]


def codes4(raw, qs_at):
    qs = raw[:, qs_at:qs_at + 16]
    return np.concatenate([qs & 15, qs >> 4], axis=1)


def test_an_all_zero_block():
    z = np.zeros((1, 32), F32)
    q4, q8 = R.quantize(T.Q4_0, z), R.quantize(T.Q8_0, z)
    assert d_of(q4)[0] == 0 and (q4[0, 2:] == 0x88).all()
    assert d_of(q8)[0] == 0 and (q8[0, 2:] == 0).all()
    for t in R.BLOCK_TYPES:
        assert d_of(R.quantize(t, z))[0] == 0


@pytest.mark.parametrize("t", [T.Q4_0, T.Q5_0, T.IQ4_NL], ids=lambda t: T.NAMES[t])
def test_of_two_elements_of_equal_magnitude_the_first_decides_the_sign_of_d(t):
    x = np.zeros((2, 32), F32)
    x[0, 3], x[0, 7] = 2.0, -2.0
    x[1, 3], x[1, 7] = -2.0, 2.0
    d = d_of(R.quantize(t, x))
    assert d[0] < 0 < d[1]  # d = vmax / (a negative number)


@pytest.mark.parametrize("t", R.BLOCK_TYPES, ids=lambda t: T.NAMES[t])
def test_the_maximum_in_the_last_element(t):
    x = np.full((1, 32), 0.25, F32)
    x[0, 31] = -4.0
    raw = R.quantize(t, x)
    want = {T.Q8_0: 4.0 / 127, T.Q4_0: 0.5, T.Q5_0: 0.25, T.Q4_1: 4.25 / 15, T.Q5_1: 4.25 / 31}.get(t)
    if want is not None:
        assert d_of(raw)[0] == np.float16(F32(want))
    back = dequantise(t, raw)[0]
    assert abs(back[31] + 4.0) <= 0.01 * 4.0 + (4.0 / 127 if t == T.IQ4_NL else 0)
    if t == T.Q8_0:
        assert raw[0, 2 + 31] == np.uint8(-127 & 0xff)
    if t == T.Q4_0:
        assert codes4(raw, 2)[0, 31] == 0  # vmax = -4: d = 0.5, -4 / 0.5 + 8.5 = 0.5


def test_the_clamp_of_the_top_code():
    x = np.zeros((1, 32), F32)
    x[0, 0], x[0, 1], x[0, 2] = -8.0, 7.5, 8.0  # d = 1: 7.5 + 8.5 = 16.0 and 8 + 8.5 = 16.5 both give 16, clamped to 15
    c = codes4(R.quantize(T.Q4_0, x), 2)[0]
    assert (c[0], c[1], c[2], c[3]) == (0, 15, 15, 8)
    x[0, 0], x[0, 1], x[0, 2] = -16.0, 15.5, 16.0
    raw = R.quantize(T.Q5_0, x)
    qh = int(np.ascontiguousarray(raw[:, 2:6]).view(np.uint32)[0, 0])
    c = codes4(raw, 6)[0] | (((qh >> np.arange(32)) & 1) << 4)
    assert (c[0], c[1], c[2], c[3]) == (0, 31, 31, 16)


def test_a_block_whose_d_is_an_f16_subnormal():
    x = np.zeros((1, 32), F32)
    x[0, 9], x[0, 10] = 127 * 2.0 ** -20, -64 * 2.0 ** -20
    raw = R.quantize(T.Q8_0, x)
    assert np.ascontiguousarray(raw[:, :2]).view(np.uint16)[0, 0] == 0x0010  # 2^-20 = 16 x 2^-24
    assert raw[0, 2 + 9] == 127 and raw[0, 2 + 10] == np.uint8(-64 & 0xff)
    x4 = np.zeros((1, 32), F32)
    x4[0, 0], x4[0, 1] = -8 * 2.0 ** -22, 3 * 2.0 ** -22
    raw = R.quantize(T.Q4_0, x4)
    assert np.ascontiguousarray(raw[:, :2]).view(np.uint16)[0, 0] == 0x0004
    assert tuple(codes4(raw, 2)[0, :3]) == (0, 11, 8)


def test_the_iq4nl_index_takes_the_upper_entry_on_a_tie():
    y = np.array([-127.0, -200.0, 113.0, 150.0, 7.0, -115.5, 101.0, 100.9], F32)  # 7 = (1 + 13) / 2, -115.5 and 101 are midpoints too
    assert list(R.iq4nl_index(y)) == [0, 0, 15, 15, 9, 1, 15, 14]


# ---- the call's checks
PS, PD = 0x10000, 0x20002  # never dereferenced
ORDER = ["src_type", "src", "src_ne", "src_nb", "dst_type", "dst", "dst_ne", "dst_nb", "flags", "stream"]
# the K store of 3 tokens on 2 KV heads of 128: contiguous F32 [128, 2, 3] into a 1-D Q8_0 view, 2-byte aligned
GOOD = dict(src_type=T.F32, src=PS, src_ne=(128, 2, 3, 1), src_nb=(4, 512, 1024, 3072), dst_type=T.Q8_0, dst=PD, dst_ne=(768, 1, 1, 1),
            dst_nb=(34, 816, 816, 816), flags=0, stream=None)
F16_ROWS = dict(dst_type=T.F16, dst_nb=(2, 1536, 1536, 1536))


def call(**over):
    a = dict(GOOD, **over)
    for k in ("src_ne", "dst_ne"):
        a[k] = (C.c_long * 4)(*a[k]) if a[k] is not None else None
    for k in ("src_nb", "dst_nb"):
        a[k] = (C.c_size_t * 4)(*a[k]) if a[k] is not None else None
    return _hip.lib().lfamd_cpy(*[a[n] for n in ORDER])


def last_error():
    return _hip.lib().lfamd_last_error().decode()


def test_the_symbol_is_exported_and_listed():
    assert "lfamd_cpy" in _hip.EXPORTS
    assert _hip.lib().lfamd_abi_version() == 1


@pytest.mark.parametrize("side", ["src_ne", "dst_ne"])
@pytest.mark.parametrize("dim", range(4))
def test_1_a_negative_extent_is_invalid_before_everything(side, dim):
    ne = list(GOOD[side])
    ne[dim] = -1
    assert call(**{side: tuple(ne)}) == INVALID
    assert "lfamd_cpy" in last_error()
    assert call(**{side: tuple(ne), "dst_type": T.Q6_K, "src": None, "dst_ne": (0, 1, 1, -1) if side == "dst_ne" else (0, 1, 1, 1)}) == INVALID
    assert call(src_ne=None) == INVALID and call(dst_nb=None) == INVALID


@pytest.mark.parametrize("dim", range(4))
def test_2_an_empty_destination_is_ok_and_looks_at_nothing(dim):
    ne = [768, 1, 1, 1]
    ne[dim] = 0
    assert call(dst_ne=tuple(ne)) == OK
    assert call(dst_ne=tuple(ne), src=None, dst=None, src_type=T.BF16, dst_type=99, flags=7, src_nb=(3, 1, 1, 1), dst_nb=(1, 1, 1, 1)) == OK


PAIRS_REFUSED = [(T.F16, T.F32), (T.F32, T.BF16), (T.BF16, T.BF16), (T.F32, T.Q6_K), (T.F32, T.Q4_K), (T.F32, T.Q8_1), (T.Q8_0, T.Q4_0),
                 (T.Q8_0, T.F32), (T.F16, T.Q8_0), (T.Q6_K, T.Q6_K), (T.F32, T.IQ4_XS), (T.F32, 99), (-1, T.F32)]


@pytest.mark.parametrize("pair", PAIRS_REFUSED, ids=lambda p: f"{T.NAMES.get(p[0], p[0])}-{T.NAMES.get(p[1], p[1])}")
def test_3_an_unserved_pair_is_unsupported_before_the_invalid_arguments(pair):
    assert call(src_type=pair[0], dst_type=pair[1]) == UNSUPPORTED
    assert "lfamd_cpy" in last_error()
    assert call(src_type=pair[0], dst_type=pair[1], src=None, flags=1, src_nb=(3, 1, 1, 1), dst_ne=(767, 1, 1, 1)) == UNSUPPORTED


def test_3_more_elements_than_the_grid_takes_are_unsupported():
    big = (1 << 16, 1 << 15, 1, 1)  # 2^31 elements
    assert call(src_ne=big, dst_ne=big, **F16_ROWS) == UNSUPPORTED
    assert call(src_ne=(1 << 40, 1 << 40, 1 << 40, 2), dst_ne=big, src=None, flags=1, **F16_ROWS) == UNSUPPORTED
    ok = (1 << 16, (1 << 15) - 1, 1, 1)  # below the limit: the next check answers (a stride that is no multiple of 4)
    assert call(src_ne=ok, dst_ne=ok, src_nb=(4, 1 << 18, 6, 8), **F16_ROWS) == INVALID


SERVED = [(T.F32, T.F32), (T.F32, T.F16), (T.F16, T.F16)] + [(T.F32, t) for t in R.BLOCK_TYPES] + [(t, t) for t in R.BLOCK_TYPES]


@pytest.mark.parametrize("pair", SERVED, ids=lambda p: f"{T.NAMES[p[0]]}-{T.NAMES[p[1]]}")
def test_3_every_served_pair_passes_to_the_pointer_check(pair):
    assert call(src_type=pair[0], dst_type=pair[1], src=None) == INVALID
    assert "null pointer" in last_error()


INVALID_CASES = [dict(src=None), dict(dst=None), dict(dst_ne=(736, 1, 1, 1)), dict(src_ne=(128, 2, 4, 1)),
                 dict(src_ne=(48, 16, 1, 1), src_nb=(4, 192, 3072, 3072)), dict(dst_ne=(48, 16, 1, 1), dst_nb=(34, 51, 816, 816)),
                 dict(dst_nb=(36, 816, 816, 816)), dict(src_nb=(8, 1024, 2048, 6144)), dict(src_nb=(512, 4, 1024, 3072)),
                 dict(src_type=T.Q8_0, src_ne=(768, 1, 1, 1), src_nb=(36, 816, 816, 816)), dict(src=PS + 2), dict(dst=PD + 1),
                 dict(src_nb=(4, 514, 1028, 3084)), dict(src_nb=(4, 512, 1024, 3074)), dict(dst_nb=(34, 816, 817, 816)),
                 dict(dst=PD + 1, **F16_ROWS), dict(src_nb=(4, 508, 1016, 3048)), dict(src_nb=(4, 512, 508, 3072)),
                 dict(dst_ne=(384, 2, 1, 1), dst_nb=(34, 406, 816, 816)), dict(flags=1)]


@pytest.mark.parametrize("over", INVALID_CASES, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items())[:60])
def test_4_invalid_arguments_are_refused_before_any_device_call(over):
    assert call(**over) == INVALID
    assert "lfamd_cpy" in last_error()


def test_4_a_float_destination_takes_odd_extents_and_strided_elements():
    # what is invalid beside a block type is not beside F16: ne[0] = 48 (passes on to the flags, the last check)
    assert call(src_ne=(48, 16, 1, 1), src_nb=(4, 192, 3072, 3072), dst_ne=(48, 16, 1, 1), dst_type=T.F16, dst_nb=(2, 96, 1536, 1536), flags=2) == INVALID
    assert "flags" in last_error()
    assert call(src_ne=(3, 256, 1, 1), src_nb=(1024, 4, 3072, 3072), dst_ne=(3, 256, 1, 1), dst_type=T.F16, dst_nb=(2, 192, 49152, 49152),
                flags=2) == INVALID
    assert "flags" in last_error()
