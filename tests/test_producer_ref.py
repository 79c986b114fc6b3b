"""CPU-side pins of tests/producer_ref.py, the yardstick of tests/test_gpu_producers.py: the generators produce what they claim and
stay inside the producers' domain, no generated norm row sits on a rounding boundary of its mean, the SwiGLU interval tells the
stated formula from its re-orderings, the image decoders agree with the library's own sizes and invert their encoders — and the
argument checks of the producers and of lfamd_quantize_rows, which make no device call, answer without a device."""
import ctypes as C

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T
import producer_ref as R
from extremes import ZERO_TOKEN, extreme_activations

f32 = np.float32
KS = (256, 768, 4096, 11008, 14336, 28672)


# ----------------------------------------------------------------------------------------------------------------- the norm
@pytest.mark.parametrize("k", KS)
def test_no_generated_norm_row_is_ambiguous(k):
    """rms_norm_ref is a bit-exact yardstick only for rows whose mean does not change when the sum moves by 1e-12 relative."""
    for eps in (1e-5, 0.0):
        x = R.norm_input(48, k, k, eps)
        y, amb = R.rms_norm_ref(x, None, eps)
        print(f"k = {k}, eps = {eps}: {int(amb.sum())} of {len(amb)} rows ambiguous")
        assert not amb.any()
        assert np.isfinite(y).all()


def test_rms_norm_ref_is_the_sequential_f64_loop():
    """Against ggml's loop written out (sum += (double)(x * x) in order): the same bits on rows that are not ambiguous."""
    k, eps = 768, 1e-6
    x = R.norm_input(20, k, 3, eps)
    w = R.norm_weight("wide", k, 4)
    y, amb = R.rms_norm_ref(x, w, eps)
    assert not amb.any()
    for r in range(x.shape[0]):
        s = 0.0
        for v in x[r]:
            s += float(f32(v) * f32(v))
        scale = f32(1.0) / np.sqrt(f32(f32(s / k) + f32(eps)))
        want = (x[r] * scale).astype(np.float32) * w
        assert np.array_equal(want.view(np.uint32), y[r].view(np.uint32)), r


def test_norm_extremes_are_what_they_claim():
    k, eps = 4096, 1e-5
    x = R.norm_input(32, k, 7, eps)
    y, _ = R.rms_norm_ref(x, None, eps)
    assert (y[ZERO_TOKEN] == 0).all()  # the zero token: scale = 1 / sqrt(eps), y = 0
    assert np.mean(x[0].astype(np.float64) ** 2) < 1e-3 * eps  # a row whose mean of squares is far below eps
    assert np.abs(y[0]).max() < 1e-3
    assert 0.5 < np.sqrt(np.mean(y[4].astype(np.float64) ** 2)) < 1.5  # rows of 3e5: the magnitude is gone after the norm
    x0 = R.norm_input(32, k, 7, 0.0)
    assert x0.any(axis=1).all()  # eps = 0 only on rows that are not all zero
    w = R.norm_weight("wide", k, 8)
    i17 = np.arange(0, k, 17)
    assert (w[i17[(i17 < 512) | (i17 >= 768)]] == 0).all() and (w[256:512] == 0).all() and (w[512:768] == -0.5).all()
    assert w[3] == 1e3 and w[k - 5] == -1e3
    nzw = np.abs(w[w != 0])
    assert nzw.min() < 3e-3 and nzw.max() == 1e3 and 0.25 < (w < 0).mean() < 0.45
    assert (R.norm_weight("ones", k, 0) == 1).all() and R.norm_weight("none", k, 0) is None
    for kind in R.WEIGHT_KINDS:
        for e in (1e-5, 1e-6, 0.0):
            yy, _ = R.rms_norm_ref(R.norm_input(32, k, 7, e), R.norm_weight(kind, k, 8), e)
            assert R.in_domain(yy), (kind, e)
    # the alternating token (kind 7) under no weight: the block maximum is shared by opposite signs
    assert y[7, 0] == -y[7, 1] == np.abs(y[7]).max()


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
def test_swiglu_kinds_are_what_they_claim(oracle):
    g, u = R.swiglu_inputs(64, 1024, 9)
    with np.errstate(over="ignore"):
        e = np.exp(-g.astype(np.float64)).astype(np.float32)
    y = R.swiglu_f32(g, u, e)
    assert R.in_domain(y)
    kinds = [R.gate_kind(j) for j in range(64)]
    assert set(kinds) == set(range(len(R.GATE_KINDS)))
    assert len({(R.gate_kind(j), j % 16) for j in range(512)}) == 16 * len(R.GATE_KINDS)  # every gate kind meets every up kind
    q = oracle.quantize(T.Q8_K, y)
    d, bs, codes = R.q8k_fields(q, 1024)
    for j in range(64):
        kd = kinds[j]
        if kd == 1:  # wide: exponentials that overflow (result a zero) and sums that round to 1
            assert (g[j] < -89).any() and np.isinf(e[j][g[j] < -89]).all() and (y[j][g[j] < -89] == 0).all()
            assert (g[j] > 17).any() and (f32(1.0) + e[j][g[j] > 17] == 1).all()
        elif kd == 2:
            assert (y[j] == 0).all() and np.signbit(g[j]).any() and not np.signbit(g[j]).all() and (d[j] == 0).all()
        elif kd == 3:
            assert np.abs(g[j]).max() < 1e-3
        elif kd == R.G_CONSTANT:
            assert (codes[j] == -128).all()
        elif kd == 5:
            assert g[j, 0] == 2 and g[j, 1] == -2 and abs(y[j, 0]) > abs(y[j, 1])
        elif kd == R.G_TIE:
            yb = y[j].reshape(-1, 256)
            m = np.abs(yb).max(axis=1)
            assert (np.abs(yb) == m[:, None]).all() and m.min() > 0
            assert (yb[0::2, 0] > 0).all() and (yb[0::2, 1] < 0).all()  # even blocks: + first; the first index decides
            assert (yb[1::2, 0] < 0).all() and (yb[1::2, 1] > 0).all()
            assert (codes[j, 0::2, 0] == -128).all() and (codes[j, 0::2, 1] == 127).all()
            assert (codes[j, 1::2, 0] == -128).all() and (d[j, 0::2] < 0).all() and (d[j, 1::2] > 0).all()
        elif kd == 7:
            assert (y[j, 256:512] == 0).all() and (d[j, 1] == 0) and (codes[j, 1] == 0).all() and (bs[j, 1] == 0).all()


def test_swiglu_interval_has_teeth():
    """At the allowance of 2 units of expf, the stated formula with NumPy's f32 exp stays inside on all 262,144 elements; every
    re-ordering and exp2(-g * log2 e) leaves it.  The 2 is what NumPy's own f32 exp needs against the f64 exp on these inputs."""
    g, u = R.swiglu_inputs(64, 4096, 5)
    assert g.size == 262144
    lo, hi = R.swiglu_interval(g, u, 2)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = np.exp(-g)  # f32
        assert e.dtype == np.float32
        one = f32(1.0)
        t = one + e
        stated = (g / t) * u
        variants = {
            "(g * u) / t": (g * u) / t,
            "g * (1 / t) * u": (g * (one / t)) * u,
            "g * ((1 / t) * u)": g * ((one / t) * u),
            "exp2(-g * log2 e)": (g / (one + np.exp2(-g * f32(1.4426950408889634)))) * u,
        }
    n_stated = [R.outside(stated, *R.swiglu_interval(g, u, n)) for n in range(3)]
    print("stated formula, NumPy f32 exp: outside at 0 / 1 / 2 ulp:", n_stated)
    assert n_stated[2] == 0
    assert R.outside(stated, lo, hi) == 0
    for name, y in variants.items():
        fin = np.isfinite(y)
        out = R.outside(y[fin], lo[fin], hi[fin])
        print(f"{name}: {out} of {g.size} outside")
        assert out > 1000, name
    # the interval is not vacuous: on most elements it is a single value or two neighbours
    width = (hi.astype(np.float64) - lo) / np.maximum(np.spacing(np.abs(lo)), 1e-300)
    assert np.median(width) <= 4


def test_interval_end_points():
    g = np.array([-100.0, -88.0, 0.0, 30.0, 1.0], dtype=np.float32)
    u = np.array([2.0, 1.0, 5.0, 1.0, -1.0], dtype=np.float32)
    lo, hi = R.swiglu_interval(g, u, 2)
    assert hi[0] == 0 and lo[0] == f32(f32(-100.0) / R.FLT_MAX) * f32(2.0)  # overflow: inf and the largest finite value
    assert lo[2] == hi[2] == 0
    assert lo[3] == hi[3] == 30.0  # 1 + e rounds to 1 whatever the last bits of e
    assert lo[4] < hi[4] and lo[4] <= f32(-0.7310586) <= hi[4]  # negative up: the ends swap, min / max still bracket
    lo0, hi0 = R.swiglu_interval(g, u, 0)
    assert (lo0 == hi0).all()


# ------------------------------------------------------------------------------------------------------------ the two images
SIZES_K = (256, 512, 768, 4096, 4352, 11008, 14336, 16384, 16640, 28672)
SIZES_N = (1, 127, 128, 129, 512)


def test_image_sizes_are_the_librarys():
    L = _hip.lib()
    for k in SIZES_K:
        for n in SIZES_N:
            assert L.lfamd_staged_q8k_size(k, n) == R.i8_image_size(k, n), (k, n)
            assert L.lfamd_staged_scaled_size(k, n) == R.scaled_image_size(k, n), (k, n)
    assert L.lfamd_staged_q8k_size(500, 4) == 0 and L.lfamd_staged_scaled_size(0, 4) == 0 and L.lfamd_staged_scaled_size(256, -1) == 0


def test_i8_image_round_trip():
    assert sorted(R.I8_PERM.tolist()) == list(range(256))
    assert R.I8_PERM[:8].tolist() == [0, 4, 1, 5, 2, 6, 3, 7]  # group 0 at byte 0
    assert R.I8_PERM[16:24].tolist() == [8, 12, 9, 13, 10, 14, 11, 15]  # group 1 at byte 16
    assert R.I8_PERM[8:16].tolist() == [16, 20, 17, 21, 18, 22, 19, 23]  # group 2 at byte 8
    assert R.I8_PERM[32] == 32  # group 4 at byte 32
    rng = np.random.default_rng(1)
    k, n = 768, 129
    npad, nb = R.n_pad_of(n), k // 256
    codes = rng.integers(-128, 128, (npad, nb, 256)).astype(np.int8)
    d = rng.standard_normal((npad, nb)).astype(np.float32)
    bs = codes.astype(np.int32).reshape(npad, nb, 16, 16).sum(axis=3).astype(np.float32)
    assert np.abs(bs).max() <= 2048  # f16 holds every block sum exactly
    img = R.i8_image_encode(codes, d, bs)
    assert img.size == R.i8_image_size(k, n)
    c2, d2, b2 = R.i8_image_decode(img, k, n)
    assert np.array_equal(c2, codes) and np.array_equal(d2.view(np.uint32), d.view(np.uint32)) and np.array_equal(b2, bs)
    # token 1 of block 2 starts at ((2 * n_pad) + 1) * 256, its scale at the d8T offset + (2 * n_pad + 1) * 4
    at = (2 * npad + 1) * 256
    assert img[at:at + 4].view(np.int8).tolist() == [codes[1, 2, 0], codes[1, 2, 4], codes[1, 2, 1], codes[1, 2, 5]]
    assert img[nb * npad * 256 + (2 * npad + 1) * 4:][:4].view(np.float32)[0] == d[1, 2]


def test_scaled_image_round_trip_and_model(oracle):
    rng = np.random.default_rng(2)
    k, n = 512, 130
    npad, nb = R.n_pad_of(n), k // 256
    xh = rng.standard_normal((npad, nb, 256)).astype(np.float16)
    ts = rng.standard_normal(npad).astype(np.float32)
    xm = rng.standard_normal((npad, nb, 16)).astype(np.float16)
    img = R.scaled_image_encode(xh, ts, xm, k, n, fill=0x5A)
    a, b, c = R.scaled_image_decode(img, k, n)
    assert np.array_equal(a.view(np.uint16), xh.view(np.uint16)) and np.array_equal(b, ts) and np.array_equal(c.view(np.uint16), xm.view(np.uint16))
    _, d8t, xmo, total = R.scaled_image_offsets(k, n)
    assert d8t % 256 == 0 and xmo % 256 == 0 and total % 256 == 0
    assert (img[d8t + npad * 4:xmo] == 0x5A).all()  # only n_pad floats of the scale part are the image's
    # the model on extreme rows: operands are finite, normalised rows peak in [512, 1024], the zero row has scale 1
    y = extreme_activations(32, k, 3)
    q = oracle.quantize(T.Q8_K, y)
    mh, mt, mm = R.scaled_image_model(y, q)
    assert np.isfinite(mh.astype(np.float32)).all() and np.isfinite(mm.astype(np.float32)).all()
    peak = np.abs(mh.astype(np.float32)).reshape(32, -1).max(axis=1)
    live = np.abs(y).max(axis=1) > 0
    assert (peak[live] >= 511).all() and (peak[live] <= 1026).all()
    assert mt[ZERO_TOKEN] == 1 and (mh[ZERO_TOKEN] == 0).all()
    assert (np.log2(mt) == np.rint(np.log2(mt))).all()  # powers of two
    back = mh.astype(np.float32) * mt[:, None, None]  # the image times 2^e is the dequantised Q8_K row, to f16's precision
    d, _, codes = R.q8k_fields(q, k)
    want = codes.astype(np.float32) * d[:, :, None]
    assert np.all(np.abs(back - want) <= 2.0 ** -10 * np.abs(want) + 2.0 ** -24 * mt[:, None, None])
    assert (mm[:, :, 8:] == 0).all()


def test_tie_rows_tie():
    for block in (32, 256):
        x = R.tie_rows(1024, block, 1).reshape(4, -1, block)
        a = np.abs(x)
        first = a.argmax(axis=2)
        for r in range(4):
            m = a[r].max(axis=1)
            ties = (a[r] == m[:, None]).sum(axis=1)
            assert (ties >= 2).all()
            later = np.array([x[r, b][a[r, b] == m[b]][-1] for b in range(x.shape[1])])
            firstv = np.take_along_axis(x[r], first[r][:, None], axis=1)[:, 0]
            assert (np.sign(later) == -np.sign(firstv)).all()
    assert (R.tie_rows(512, 32, 1)[2].reshape(-1, 32)[:, 5] > 0).all() and (R.tie_rows(512, 32, 1)[3].reshape(-1, 32)[:, 5] < 0).all()


# ------------------------------------------------------------------------------ argument checks, without a device behind them
# Addresses that are never dereferenced: every case below must be refused before any launch.
A16, A4 = 0x7F0000001000, 0x7F0000001004
INVALID, OK = -2, 0
Q8K, STG, SCL = T.Q8_K, _hip.TYPE_STAGED_Q8K, _hip.TYPE_STAGED_SCALED


def _norm(L, x=A16, xrb=1024, w=A16, n=4, k=256, vdt=Q8K, yq=A16, yqrb=292, yf=A16, yfrb=1024):
    return L.lfamd_rms_norm_quantize(C.c_void_p(x), xrb, C.c_void_p(w), 1e-5, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


def _swiglu(L, g=A16, grb=1024, u=A16, urb=1024, n=4, k=256, vdt=Q8K, yq=A16, yqrb=292, yf=A16, yfrb=1024):
    return L.lfamd_swiglu_quantize(C.c_void_p(g), grb, C.c_void_p(u), urb, n, k, vdt, C.c_void_p(yq), yqrb, C.c_void_p(yf), yfrb, None)


INVALID_NORM = {
    "k % 256": dict(k=500), "k = 0": dict(k=0), "nrows < 0": dict(n=-1), "d_x on 4 bytes": dict(x=A4), "d_yf on 4 bytes": dict(yf=A4),
    "d_weight on 4 bytes": dict(w=A4), "x stride": dict(xrb=1028), "yf stride": dict(yfrb=1032), "q8k rows on 2 bytes": dict(yq=A16 + 2),
    "q8k stride": dict(yqrb=294), "int8 image on 4 bytes": dict(vdt=STG, yq=A4), "scaled image on 4 bytes": dict(vdt=SCL, yq=A4),
    "Q8_0": dict(vdt=T.Q8_0), "Q8_1": dict(vdt=T.Q8_1), "F32": dict(vdt=T.F32), "no output": dict(yq=0, yf=0),
}
INVALID_SWIGLU = {
    "k % 256": dict(k=500), "k = 0": dict(k=0), "nrows < 0": dict(n=-1), "d_gate on 4 bytes": dict(g=A4), "d_up on 4 bytes": dict(u=A4),
    "d_yf on 4 bytes": dict(yf=A4), "gate stride": dict(grb=1028), "up stride": dict(urb=1032), "yf stride": dict(yfrb=1028),
    "q8k rows on 2 bytes": dict(yq=A16 + 2), "q8k stride": dict(yqrb=294), "int8 image on 4 bytes": dict(vdt=STG, yq=A4),
    "scaled image on 4 bytes": dict(vdt=SCL, yq=A4), "Q8_0": dict(vdt=T.Q8_0), "Q8_1": dict(vdt=T.Q8_1), "F32": dict(vdt=T.F32),
    "no output": dict(yq=0, yf=0), "65409 rows": dict(n=65409), "null d_gate": dict(g=0), "null d_up": dict(u=0),
}


@pytest.mark.parametrize("what", INVALID_NORM)
def test_rms_norm_quantize_refuses(what):
    L = _hip.lib()
    assert _norm(L, **INVALID_NORM[what]) == INVALID, what
    assert b"lfamd_rms_norm_quantize" in L.lfamd_last_error()


@pytest.mark.parametrize("what", INVALID_SWIGLU)
def test_swiglu_quantize_refuses(what):
    L = _hip.lib()
    assert _swiglu(L, **INVALID_SWIGLU[what]) == INVALID, what
    assert b"lfamd_swiglu_quantize" in L.lfamd_last_error()


def test_zero_rows_is_ok_and_launches_nothing():
    L = _hip.lib()
    for vdt in (Q8K, STG, SCL):
        assert _norm(L, n=0, vdt=vdt) == OK
        assert _swiglu(L, n=0, vdt=vdt) == OK
    assert L.lfamd_quantize_rows(Q8K, C.c_void_p(A16), 0, 256, 1024, C.c_void_p(A16), 292, None) == OK


def test_rms_norm_quantize_refuses_a_null_input():
    """Before the check existed the alignment test passed for address 0 and the kernel was launched on a null row: with a device
    that is a fault, so this case runs only where there is none (there the launch itself failed with LFAMD_ERR_HIP)."""
    L = _hip.lib()
    if L.lfamd_device_count() > 0:
        pytest.skip("a device is present: a library without the check would launch a kernel that reads address 0")
    for vdt in (Q8K, STG, SCL):
        assert _norm(L, x=0, vdt=vdt) == INVALID, vdt


def _qrows(L, vdt=Q8K, x=A16, n=4, cols=256, xrb=1024, y=A16, yrb=292):
    return L.lfamd_quantize_rows(vdt, C.c_void_p(x), n, cols, xrb, C.c_void_p(y), yrb, None)


def test_quantize_rows_refuses():
    L = _hip.lib()
    assert _qrows(L, cols=250) == INVALID and _qrows(L, vdt=T.Q8_0, cols=48, yrb=68) == INVALID  # not a block multiple
    assert _qrows(L, yrb=291) == INVALID and _qrows(L, vdt=T.Q8_0, cols=64, yrb=67) == INVALID  # output rows too short
    assert _qrows(L, vdt=T.Q8_1, cols=64, yrb=71) == INVALID
    assert _qrows(L, vdt=T.F32) == -1
    assert _qrows(L, n=65536) == INVALID  # one grid row per input row


def test_quantize_rows_refuses_null_pointers():
    L = _hip.lib()
    if L.lfamd_device_count() > 0:
        pytest.skip("a device is present: a library without the check would launch a kernel on address 0")
    for vdt, cols, yrb in ((Q8K, 256, 292), (T.Q8_0, 64, 68), (T.Q8_1, 64, 72)):
        assert _qrows(L, vdt=vdt, cols=cols, yrb=yrb, x=0) == INVALID
        assert _qrows(L, vdt=vdt, cols=cols, yrb=yrb, y=0) == INVALID
