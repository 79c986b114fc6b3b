"""Without a GPU: the interface of the LFAMD_TYPE_STAGED_Q80 image (the staged activations of Q8_0-weight batches on gemm_lf_q80) as far
as it answers without a device — the symbols load, the image size is the layout formula, the predicate's truth table, the argument
checks of the producers and of every mat-mul entry point (which make no device call) — and tests/producer80_ref.py against itself and
the oracle: the codec inverts, and the decoded image times tok_scale is the f16-rounded d * code of the Q8_0 rows."""
import ctypes as C

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
import producer32_ref as R32
import producer80_ref as R80
import producer_ref as R

f32 = np.float32
Q80I = 0x1003
EXCLUDING = ("FLAG_PRECISE", "FLAG_Q80_EXACT", "FLAG_FORCE_GENERIC")


def test_the_symbols_load():
    L = _hip.lib()
    assert _hip.TYPE_STAGED_Q80 == Q80I
    for name in ("lfamd_staged_q80_size", "lfamd_mul_mat_takes_staged_q80", "lfamd_rms_norm_quantize_b32", "lfamd_swiglu_quantize_b32"):
        assert name in _hip.EXPORTS and getattr(L, name).argtypes is not None, name


@pytest.mark.parametrize("k", [128, 384, 4096, 14336])
def test_image_size_is_the_layout_formula(k):
    L = _hip.lib()
    ws = L.lfamd_mul_mat_workspace
    for n in (0, 1, 128, 129, 512):
        npad = (n + 127) // 128 * 128
        want = npad * k * 2 + npad * 8
        assert L.lfamd_staged_q80_size(k, n) == want == R80.q80_image_size(k, n), (k, n)
        if n > 8 and not L.lfamd_vendor_gemm_available():  # what the same call stages into (the workspace rounds up to 256 bytes)
            assert (want + 255) // 256 * 256 <= ws(T.Q8_0, 64, k, n)
    assert L.lfamd_staged_q80_size(160, 4) == 0 and L.lfamd_staged_q80_size(0, 4) == 0 and L.lfamd_staged_q80_size(128, -1) == 0


def test_takes_staged_q80_truth_table():
    L = _hip.lib()
    takes = L.lfamd_mul_mat_takes_staged_q80
    yes = 0 if L.lfamd_vendor_gemm_available() else 1  # (a process that opted into the vendor GEMM runs these batches there)
    assert takes(T.Q8_0, 4096, 4096, 512, 0) == yes
    for t in (T.Q4_0, T.Q4_K, T.F16):
        assert takes(t, 4096, 4096, 512, 0) == 0, T.NAMES[t]
    assert takes(T.Q8_0, 4096, 4096, 9, 0) == yes and takes(T.Q8_0, 4096, 4096, 8, 0) == 0
    assert takes(T.Q8_0, 64, 128, 64, 0) == yes and takes(T.Q8_0, 64, 160, 64, 0) == 0
    for name in EXCLUDING:
        assert takes(T.Q8_0, 4096, 4096, 512, getattr(_hip, name)) == 0, name
    assert takes(T.Q8_0, 4096, 4096, 512, _hip.FLAG_Q0_VREGS32) == yes  # (a host-variant flag: no say in the route)
    assert takes(T.Q8_0, 0, 4096, 512, 0) == 0 and takes(T.Q8_0, 4096, 4096, 0, 0) == 0 and takes(99, 4096, 4096, 512, 0) == 0
    # the P80 image the loaders address by a 32-bit byte offset: (m / 8) * (k / 128) * 1088 bytes below 4 GiB
    assert takes(T.Q8_0, 31_000_000, 128, 64, 0) == yes and takes(T.Q8_0, 32_000_000, 128, 64, 0) == 0
    # the other predicates do not claim these calls
    assert L.lfamd_mul_mat_takes_staged_b32(T.Q8_0, 4096, 4096, 512, 0) == 0 and L.lfamd_mul_mat_takes_staged(T.Q8_0, 4096, 4096, 512, 0) == 0
    assert L.lfamd_mul_mat_takes_staged_scaled(T.Q8_0, 4096, 4096, 512, 0) == 0


# ------------------------------------------------------------------------------ argument checks, without a device behind them
# Addresses that are never dereferenced: every case below must be refused before any launch.
A16, A8, A4 = 0x7F0000001000, 0x7F0000001008, 0x7F0000001004
INVALID, UNSUPPORTED, OK = -2, -1, 0


def _norm(L, x=A16, xrb=512, w=A16, n=4, k=128, vdt=Q80I, yq=A16, yqrb=0, yf=A16, yfrb=512):
    return L.lfamd_rms_norm_quantize_b32(C.c_void_p(x), xrb, C.c_void_p(w), 1e-5, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


def _swiglu(L, g=A16, grb=512, u=A16, urb=512, n=4, k=128, vdt=Q80I, yq=A16, yqrb=0, yf=A16, yfrb=512):
    return L.lfamd_swiglu_quantize_b32(C.c_void_p(g), grb, C.c_void_p(u), urb, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


INVALID_BOTH = {
    "k % 128 (a multiple of 32)": dict(k=160), "k % 128 (of 64)": dict(k=192), "k = 0": dict(k=0),
    "nrows < 0": dict(n=-1), "image on 8 bytes": dict(yq=A8), "image on 4 bytes": dict(yq=A4), "no output": dict(yq=0, yf=0),
    "d_yf on 4 bytes": dict(yf=A4), "yf stride": dict(yfrb=516),
}
INVALID_NORM = {**INVALID_BOTH, "null d_x": dict(x=0), "d_x on 4 bytes": dict(x=A4), "x stride": dict(xrb=516), "d_weight on 4 bytes": dict(w=A4)}
INVALID_SWIGLU = {**INVALID_BOTH, "null d_gate": dict(g=0), "null d_up": dict(u=0), "d_gate on 4 bytes": dict(g=A4), "d_up on 4 bytes": dict(u=A4),
                  "gate stride": dict(grb=516), "up stride": dict(urb=520), "65409 rows": dict(n=65409)}


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
    assert _norm(L, n=0) == OK and _swiglu(L, n=0) == OK
    # what is legal: yq_row_bytes is ignored, a half chunk (k % 256 == 128), a null weight, either output alone, 65408 rows' worth of checks
    assert _norm(L, n=0, yqrb=273) == OK and _swiglu(L, n=0, yqrb=1) == OK
    assert _norm(L, n=0, k=384, xrb=1536, yfrb=1536, w=0) == OK and _swiglu(L, n=0, k=4224, grb=16896, urb=16896, yfrb=16896) == OK
    assert _norm(L, n=0, yf=0) == OK and _norm(L, n=0, yq=0) == OK and _swiglu(L, n=0, yf=0) == OK and _swiglu(L, n=0, yq=0) == OK
    # d_yq = NULL writes f32 only, whatever vec_dot_type says: then the rows' rule k % 32 == 0 holds, not the image's
    assert _norm(L, n=0, k=160, xrb=640, yfrb=640, yq=0) == OK


def test_the_q8k_producers_refuse_the_image():
    L = _hip.lib()
    z = C.c_void_p(A16)
    assert L.lfamd_rms_norm_quantize(z, 1024, z, 1e-5, 4, 256, Q80I, z, 292, z, 1024, None) == INVALID
    assert L.lfamd_swiglu_quantize(z, 1024, z, 1024, 4, 256, Q80I, z, 292, z, 1024, None) == INVALID


def test_mat_mul_entry_points_answer_for_the_image_without_a_device():
    """The checks in front of the first launch: -1 where the call does not take the image, -2 for a null or misaligned one."""
    L = _hip.lib()
    if L.lfamd_vendor_gemm_available():  # (such a process runs Q8_0 batches on the vendor GEMM: no call takes the image)
        return
    z, ws = C.c_void_p(A16), C.c_void_p(0)

    def mm(t, m, k, n, img=A16, flags=0):
        return L.lfamd_mul_mat(t, z, m, k, Q80I, C.c_void_p(img), 0, n, z, m, ws, 0, flags, None)

    for t in (T.Q4_0, T.Q4_K, T.F16):
        assert mm(t, 256, 256, 64) == UNSUPPORTED, T.NAMES[t]
    assert mm(T.Q8_0, 256, 256, 8) == UNSUPPORTED and mm(T.Q8_0, 256, 160, 64) == UNSUPPORTED
    assert mm(T.Q8_0, 32_000_000, 128, 64) == UNSUPPORTED
    for name in EXCLUDING:
        assert mm(T.Q8_0, 256, 256, 64, flags=getattr(_hip, name)) == UNSUPPORTED, name
    assert mm(T.Q8_0, 256, 256, 64, img=0) == INVALID and mm(T.Q8_0, 256, 256, 64, img=A8) == INVALID
    one, two = (C.c_void_p * 1)(A16), (C.c_void_p * 2)(A16, A16)
    m1, m2 = (C.c_long * 1)(256), (C.c_long * 2)(256, 64)
    t1 = (C.c_int * 1)(T.Q8_0)
    assert L.lfamd_mul_mat_multi_types(1, t1, one, m1, 256, Q80I, z, 0, 64, one, m1, ws, 0, 0, None) == UNSUPPORTED
    multi = L.lfamd_mul_mat_multi
    assert multi(T.Q4_0, 1, one, m1, 256, Q80I, z, 0, 64, one, m1, ws, 0, 0, None) == UNSUPPORTED
    assert multi(T.Q4_K, 2, two, m2, 256, Q80I, z, 0, 64, two, m2, ws, 0, 0, None) == UNSUPPORTED
    assert multi(T.Q8_0, 2, two, m2, 256, Q80I, z, 0, 8, two, m2, ws, 0, 0, None) == UNSUPPORTED
    assert multi(T.Q8_0, 2, two, m2, 256, Q80I, z, 0, 64, two, m2, ws, 0, _hip.FLAG_Q80_EXACT, None) == UNSUPPORTED
    big = (C.c_long * 2)(256, 32_000_000)
    assert multi(T.Q8_0, 2, two, big, 128, Q80I, z, 0, 64, two, big, ws, 0, 0, None) == UNSUPPORTED
    assert multi(T.Q8_0, 1, one, m1, 256, Q80I, C.c_void_p(A8), 0, 64, one, m1, ws, 0, 0, None) == INVALID
    assert multi(T.Q8_0, 2, two, m2, 256, Q80I, C.c_void_p(A8), 0, 64, two, m2, ws, 0, 0, None) == INVALID
    assert multi(T.Q8_0, 2, two, m2, 256, Q80I, C.c_void_p(0), 0, 64, two, m2, ws, 0, 0, None) == INVALID
    short = (C.c_long * 2)(256, 63)  # the second matrix has ldc < m
    assert multi(T.Q8_0, 2, two, m2, 256, Q80I, z, 0, 64, two, short, ws, 0, 0, None) == INVALID
    plan = C.c_void_p(A16)
    assert L.lfamd_mul_mat_id(T.Q8_0, z, 256, 256, 4, Q80I, z, 0, 1, 16, plan, 2, z, ws, 0, 0, None) == UNSUPPORTED
    assert L.lfamd_mul_mat_id_multi(T.Q8_0, 1, one, 256, 256, 4, Q80I, z, 0, 1, 16, plan, 2, one, ws, 0, 0, None) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- producer80_ref by itself
def test_the_chunk_permutation_is_the_stated_one():
    # block 0, elements 0 .. 3 (j = 0) at byte 0; block 1 at byte 8; block 2 (s = 1) at byte 32; j = 1 (s = 2) at byte 64; j = 4 at byte 16
    P = R80.Q80_INV
    assert P[0] == 0 and P[3] == 3 and P[32] == 4 and P[64] == 16 and P[4] == 32 and P[16] == 8 and P[96 + 28 + 3] == 127


def test_image_round_trip(oracle):
    """Encode then decode is the identity on random Q8_0 rows: the three parts come back bit for bit, and the codes of the rows are
    recovered from the decoded image (Xh * tok_scale / d, to the nearest integer)."""
    k, n = 384, 129
    npad = R.n_pad_of(n)
    rows = oracle.quantize(T.Q8_0, synth.random_activations(n, k, 7))
    img = R80.q80_image_of_rows(rows, k)
    assert img.size == R80.q80_image_size(k, n) == npad * k * 2 + npad * 8
    xh, stage, tok = R80.q80_image_decode(img, k, n)
    mh, ms, mt = R80.q80_image_model(rows, k)
    assert np.array_equal(xh[:n].view(np.uint16), mh.view(np.uint16)) and np.array_equal(stage[:n], ms) and np.array_equal(tok[:n], mt)
    assert not xh[n:].any() and (stage[n:] == 1).all() and (tok[n:] == 1).all()
    assert np.array_equal(R80.q80_image_encode(xh, stage, tok, k, n), img)
    assert (stage * tok == 1).all()
    d, _, q = R32.b32_fields(rows, T.Q8_0, k)
    assert (d > 0).all()
    back = xh[:n].astype(np.float64).reshape(n, -1, 32) * tok[:n, None, None] / d.astype(np.float64)[:, :, None]
    assert np.array_equal(np.rint(back), q.astype(np.float64))  # (one f16 rounding of an 18-bit product: within 2^-11 of the code)
    # token 1, quad 2, element 5 of block 1 (j = 1, r = 1: byte 64 + 8 + 2) sits at ((2 * n_pad + 1) * 128 + 37) of Xh
    assert img[:npad * k * 2].view(np.float16)[(2 * npad + 1) * 128 + 37] == mh[1, 256 + 32 + 5]


def test_decoded_image_times_tok_scale_is_the_f16_rounded_d_times_code(oracle):
    """Rows whose every product d * code lies in f16's normal range: the power of two commutes with the one rounding, so the image
    holds f16(d * code) up to the token's exact factor.  The row's largest product lands in [512, 1024) before its rounding."""
    k, n = 256, 40
    y = synth.random_activations(n, k, 9) * np.exp2(np.arange(n) % 9 - 4).astype(np.float32)[:, None]
    rows = oracle.quantize(T.Q8_0, y)
    d, _, q = R32.b32_fields(rows, T.Q8_0, k)
    want = (d.astype(np.float32)[:, :, None] * q.astype(np.float32)).astype(np.float16).reshape(n, k)  # (the f32 product is exact)
    nz = want[want != 0]
    assert (np.abs(nz.astype(np.float32)) >= 2.0 ** -14).all() and np.isfinite(want).all()
    xh, stage, tok = R80.q80_image_decode(R80.q80_image_of_rows(rows, k), k, n)
    got = xh[:n].astype(np.float32) * tok[:n, None]
    assert np.array_equal(got, want.astype(np.float32))
    top = np.abs(xh[:n].astype(np.float32)).max(axis=1)
    assert ((top >= 512) & (top <= 1024)).all()  # (1024: a product within half an f16 step of it)


def test_rows_without_a_normalisation():
    """An all-zero row, and a row whose every stored d is zero (|y| / 127 below half of f16's smallest subnormal): stage = tok_scale = 1 and
    zero operands."""
    k = 128
    rows = np.zeros((2, k // 32 * 34), np.uint8)
    rows[1].reshape(-1, 34)[:, 2:] = 5  # codes without a scale
    xh, stage, tok = R80.q80_image_model(rows, k)
    assert not xh.any() and (stage == 1).all() and (tok == 1).all()
