"""Without a GPU: the interface of the 32-block fused producers (lfamd_rms_norm_quantize_b32, lfamd_swiglu_quantize_b32,
LFAMD_TYPE_STAGED_B32) as far as it answers without a device — the symbols load, the image size is the layout formula, the
predicate's truth table, the argument checks (which make no device call) — and tests/producer32_ref.py against itself and the
oracle: the image codec inverts, the tie rows are exact and round away from zero."""
import ctypes as C

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T
import producer32_ref as R32
import producer_ref as R

f32 = np.float32
B32 = 0x1002
LEGACY = (T.Q4_0, T.IQ4_NL, T.Q4_1, T.Q5_0, T.Q5_1)


def test_the_four_symbols_load():
    L = _hip.lib()
    assert _hip.TYPE_STAGED_B32 == B32
    for name in ("lfamd_staged_b32_size", "lfamd_mul_mat_takes_staged_b32", "lfamd_rms_norm_quantize_b32", "lfamd_swiglu_quantize_b32"):
        assert name in _hip.EXPORTS and getattr(L, name).argtypes is not None, name


@pytest.mark.parametrize("k", [256, 768, 4352])
def test_image_size_is_the_layout_formula(k):
    L = _hip.lib()
    for n in (1, 127, 128, 129, 300):
        npad, nb = (n + 127) // 128 * 128, k // 256
        up = lambda v: (v + 255) // 256 * 256  # noqa: E731
        want = up(npad * k * 2) + 2 * up(nb * 8 * npad * 4)
        assert L.lfamd_staged_b32_size(k, n) == want == R32.b32_image_size(k, n), (k, n)
        _, d8t, st, total = R32.b32_image_offsets(k, n)
        assert d8t % 256 == 0 and st % 256 == 0 and total % 256 == 0
    assert L.lfamd_staged_b32_size(96, 4) == 0 and L.lfamd_staged_b32_size(0, 4) == 0 and L.lfamd_staged_b32_size(256, -1) == 0


def test_takes_staged_b32_truth_table():
    L = _hip.lib()
    takes = L.lfamd_mul_mat_takes_staged_b32
    for t in LEGACY:
        assert takes(t, 4096, 4096, 512, 0) == 1, T.NAMES[t]
        assert takes(t, 4096, 4096, 9, 0) == 1, T.NAMES[t]
        assert takes(t, 4096, 4096, 8, 0) == 0, T.NAMES[t]
        assert takes(t, 4096, 96, 512, 0) == 0, T.NAMES[t]
        assert takes(t, 4096, 4096, 512, _hip.FLAG_FORCE_GENERIC) == 0, T.NAMES[t]
        assert takes(t, 0, 4096, 512, 0) == 0 and takes(t, 4096, 4096, 0, 0) == 0
    for t in (T.Q8_0, T.Q4_K, T.Q5_K, T.Q6_K, T.Q2_K, T.IQ4_XS, T.F16, T.F32):
        assert takes(t, 4096, 4096, 512, 0) == 0, T.NAMES[t]
    assert takes(99, 4096, 4096, 512, 0) == 0
    # the other two predicates do not claim these calls, and this one does not claim theirs
    assert L.lfamd_mul_mat_takes_staged(T.Q4_0, 4096, 4096, 512, 0) == 0 and L.lfamd_mul_mat_takes_staged_scaled(T.Q5_0, 4096, 4096, 512, 0) == 0


# ------------------------------------------------------------------------------ argument checks, without a device behind them
# Addresses that are never dereferenced: every case below must be refused before any launch.
A16, A4, A2 = 0x7F0000001000, 0x7F0000001004, 0x7F0000001002
INVALID, OK = -2, 0


def _norm(L, x=A16, xrb=1024, w=A16, n=4, k=256, vdt=T.Q8_0, yq=A16, yqrb=272, yf=A16, yfrb=1024):
    return L.lfamd_rms_norm_quantize_b32(C.c_void_p(x), xrb, C.c_void_p(w), 1e-5, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


def _swiglu(L, g=A16, grb=1024, u=A16, urb=1024, n=4, k=256, vdt=T.Q8_0, yq=A16, yqrb=272, yf=A16, yfrb=1024):
    return L.lfamd_swiglu_quantize_b32(C.c_void_p(g), grb, C.c_void_p(u), urb, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


INVALID_BOTH = {
    "k % 32": dict(k=48), "k = 0": dict(k=0), "nrows < 0": dict(n=-1), "d_yf on 4 bytes": dict(yf=A4), "yf stride": dict(yfrb=1028),
    "Q8_0 rows on an odd byte": dict(yq=A16 + 1), "Q8_0 stride odd": dict(yqrb=273), "Q8_0 stride short": dict(yqrb=270),
    "Q8_1 rows on 2 bytes": dict(vdt=T.Q8_1, yq=A2, yqrb=288), "Q8_1 stride": dict(vdt=T.Q8_1, yqrb=290),
    "Q8_1 stride short": dict(vdt=T.Q8_1, yqrb=284), "image with k = 96": dict(vdt=B32, k=96, yqrb=0),
    "image on 4 bytes": dict(vdt=B32, yq=A4), "Q8_K": dict(vdt=T.Q8_K, yqrb=292), "int8 image": dict(vdt=_hip.TYPE_STAGED_Q8K),
    "scaled image": dict(vdt=_hip.TYPE_STAGED_SCALED), "F32": dict(vdt=T.F32), "no output": dict(yq=0, yf=0),
}
INVALID_NORM = {**INVALID_BOTH, "null d_x": dict(x=0), "d_x on 4 bytes": dict(x=A4), "x stride": dict(xrb=1028), "d_weight on 4 bytes": dict(w=A4)}
INVALID_SWIGLU = {**INVALID_BOTH, "null d_gate": dict(g=0), "null d_up": dict(u=0), "d_gate on 4 bytes": dict(g=A4), "d_up on 4 bytes": dict(u=A4),
                  "gate stride": dict(grb=1028), "up stride": dict(urb=1032), "65409 rows": dict(n=65409)}


@pytest.mark.parametrize("what", INVALID_NORM)
def test_rms_norm_quantize_b32_refuses(what):
    L = _hip.lib()
    assert _norm(L, **INVALID_NORM[what]) == INVALID, what
    assert b"lfamd_rms_norm_quantize_b32" in L.lfamd_last_error()


@pytest.mark.parametrize("what", INVALID_SWIGLU)
def test_swiglu_quantize_b32_refuses(what):
    L = _hip.lib()
    assert _swiglu(L, **INVALID_SWIGLU[what]) == INVALID, what
    assert b"lfamd_swiglu_quantize_b32" in L.lfamd_last_error()


def test_zero_rows_is_ok_and_launches_nothing():
    L = _hip.lib()
    for vdt, yqrb in ((T.Q8_0, 272), (T.Q8_1, 288), (B32, 0)):
        assert _norm(L, n=0, vdt=vdt, yqrb=yqrb) == OK
        assert _swiglu(L, n=0, vdt=vdt, yqrb=yqrb) == OK
    # what is legal: rows that are no multiple of 256, Q8_0 rows on 2 bytes, a null weight, either output alone
    assert _norm(L, n=0, k=96, xrb=384, yfrb=384, yq=A2, yqrb=102, w=0) == OK
    assert _swiglu(L, n=0, k=4128, grb=16512, urb=16512, yfrb=16512, vdt=T.Q8_1, yq=A4, yqrb=4644) == OK
    assert _norm(L, n=0, yf=0) == OK and _norm(L, n=0, yq=0, vdt=T.F32) == OK


def test_the_existing_entry_points_still_refuse_these_formats():
    L = _hip.lib()
    z = C.c_void_p(A16)
    for vdt in (T.Q8_0, T.Q8_1, B32):
        assert L.lfamd_rms_norm_quantize(z, 1024, z, 1e-5, 4, 256, vdt, z, 292, z, 1024, None) == INVALID
        assert L.lfamd_swiglu_quantize(z, 1024, z, 1024, 4, 256, vdt, z, 292, z, 1024, None) == INVALID


def test_mat_mul_entry_points_answer_for_the_image_without_a_device():
    """The checks in front of the first launch: -1 where the call does not take the image, -2 for a null or misaligned one."""
    L = _hip.lib()
    z, ws = C.c_void_p(A16), C.c_void_p(0)
    def mm(t, m, k, n, img=A16, flags=0):
        return L.lfamd_mul_mat(t, z, m, k, B32, C.c_void_p(img), 0, n, z, m, ws, 0, flags, None)
    for t in (T.Q8_0, T.Q4_K, T.F16):
        assert mm(t, 256, 256, 64) == -1, T.NAMES[t]
    assert mm(T.Q4_0, 256, 256, 4) == -1 and mm(T.Q5_1, 256, 256, 64, flags=_hip.FLAG_FORCE_GENERIC) == -1
    assert mm(T.Q4_0, 256, 256, 64, img=0) == INVALID and mm(T.Q4_1, 256, 256, 64, img=A4) == INVALID
    one = (C.c_void_p * 1)(A16)
    m1 = (C.c_long * 1)(256)
    t1 = (C.c_int * 1)(T.Q4_0)
    assert L.lfamd_mul_mat_multi_types(1, t1, one, m1, 256, B32, z, 0, 64, one, m1, ws, 0, 0, None) == -1
    assert L.lfamd_mul_mat_multi(T.Q8_0, 1, one, m1, 256, B32, z, 0, 64, one, m1, ws, 0, 0, None) == -1
    assert L.lfamd_mul_mat_multi(T.Q4_0, 1, one, m1, 256, B32, C.c_void_p(A4), 0, 64, one, m1, ws, 0, 0, None) == INVALID
    plan = C.c_void_p(A16)
    assert L.lfamd_mul_mat_id(T.Q4_0, z, 256, 256, 4, B32, z, 0, 1, 16, plan, 2, z, ws, 0, 0, None) == -1
    assert L.lfamd_mul_mat_id_multi(T.Q4_0, 1, one, 256, 256, 4, B32, z, 0, 1, 16, plan, 2, one, ws, 0, 0, None) == -1


# ---------------------------------------------------------------------------------------------------- producer32_ref by itself
def test_image_round_trip():
    rng = np.random.default_rng(1)
    k, n = 768, 129
    npad = R.n_pad_of(n)
    xh = rng.integers(-127, 128, (npad, k)).astype(np.float16)
    d8 = rng.standard_normal((npad, k // 32)).astype(np.float32)
    s = rng.standard_normal((npad, k // 32)).astype(np.float32)
    img = R32.b32_image_encode(xh, d8, s, k, n, fill=0x5A)
    assert img.size == R32.b32_image_size(k, n)
    a, b, c = R32.b32_image_decode(img, k, n)
    assert np.array_equal(a.view(np.uint16), xh.view(np.uint16)) and np.array_equal(b.view(np.uint32), d8.view(np.uint32))
    assert np.array_equal(c.view(np.uint32), s.view(np.uint32))
    # token 1, weight 256 * 2 + 5 sits at ((2 * n_pad) + 1) * 256 + 5 of Xh; its block 2 * 8 + 0 at (16 * n_pad + 1) of d8T and sT
    _, d8t, st, _ = R32.b32_image_offsets(k, n)
    assert img[:npad * k * 2].view(np.float16)[(2 * npad + 1) * 256 + 5] == xh[1, 512 + 5]
    assert img[d8t:].view(np.float32)[16 * npad + 1] == d8[1, 16] and img[st:].view(np.float32)[16 * npad + 1] == s[1, 16]


def test_image_model_is_the_oracles_blocks(oracle):
    k = 512
    y = R.norm_input(20, k, 3, 1e-5)
    q80, q81 = oracle.quantize(T.Q8_0, y), oracle.quantize(T.Q8_1, y)
    d0, _, c0 = R32.b32_fields(q80, T.Q8_0, k)
    d1, s1, c1 = R32.b32_fields(q81, T.Q8_1, k)
    assert np.array_equal(d0.view(np.uint16), d1.view(np.uint16)) and np.array_equal(c0, c1)  # one image serves both formats
    xh, d8, s = R32.b32_image_model(q81, k)
    assert np.array_equal(xh.astype(np.int32).reshape(20, -1, 32), c1.astype(np.int32)) and np.array_equal(d8, d1.astype(np.float32))
    assert np.array_equal(s, s1.astype(np.float32))


def test_tie_rows_are_exact_and_round_away_from_zero(oracle):
    k = 96
    v = R32.tie_values(k)
    assert v[0] == 127 and v[1] == 0.5 and v[2] == -1.5 and v[3] == 2.5 and v[32] == 127
    assert R32.tie_codes(k)[:4].tolist() == [127, 1, -2, 3] and np.rint(v[1:4]).tolist() == [0, -2, 2]
    # SwiGLU: the stated formula in f32 steps gives v exactly
    g, u, want = R32.swiglu_tie_inputs(2, k)
    e = np.exp(-g.astype(np.float64)).astype(np.float32)
    assert (f32(1.0) + e == 1).all()
    assert np.array_equal(R.swiglu_f32(g, u, e), want)
    assert R.smallest_n_ulp(want, g, u)[0] == 0
    # the norm: the reference gives v exactly
    x, w, eps, want = R32.norm_tie_inputs(2, k)
    y, amb = R.rms_norm_ref(x, w, eps)
    assert not amb.any() and np.array_equal(y, want)
    # and the oracle's quantisers take every tie away from zero, with d = 1
    for vdt in (T.Q8_0, T.Q8_1):
        d, s, q = R32.b32_fields(oracle.quantize(vdt, want), vdt, k)
        assert (d == 1).all() and np.array_equal(q.reshape(2, k), np.tile(R32.tie_codes(k), (2, 1)))
        if s is not None:
            assert np.array_equal(s.astype(np.float32), q.astype(np.int32).sum(axis=2).astype(np.float32))
    # an all-zero block: d = 0, codes 0, s = 0
    _, _, want0 = R32.swiglu_tie_inputs(1, k, zero_block=1)
    d, s, q = R32.b32_fields(oracle.quantize(T.Q8_1, want0), T.Q8_1, k)
    assert d[0, 1] == 0 and s[0, 1] == 0 and (q[0, 1] == 0).all() and d[0, 0] == 1
