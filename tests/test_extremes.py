"""The adversarial operands of extremes.py on the CPU: every band decodes to what it claims, and the oracle the GPU tests compare
against agrees with a dequantise-to-f64 product at exactly these inputs, token by token."""
import numpy as np
import pytest

from llamafile_amd import ggml_types as T, synth
from extremes import (BAND_MAX, BAND_MIN, BAND_SCMAX, BAND_SCNEG, CODE_MAX, CODE_MIN, D_OFF, KINDS, M_OFF, MIN_MAX, SC_MAX,
                      SC_NEG, ZERO_ROW, ZERO_TOKEN, edge_scale_weights, extreme_activations, extreme_weights,
                      for_vec_dot)
from helpers import rel_err

TYPES = T.QUANT_WEIGHT_TYPES
K = 512


def _scale_fields(t, raw):
    blk = raw.reshape(raw.shape[0], -1, T.TYPE_SIZE[t])
    d = np.ascontiguousarray(blk[:, :, D_OFF[t]:D_OFF[t] + 2]).view(np.float16)[..., 0].astype(np.float32)
    mo = M_OFF[t]
    mm = None if mo is None else np.ascontiguousarray(blk[:, :, mo:mo + 2]).view(np.float16)[..., 0].astype(np.float32)
    return d, mm


def _block_value(t, d, mm, code, sc, mins):
    """One weight of a block with uniform code / sub-block scale / mins multiplier, in the reference's f32 order."""
    f = np.float32
    if t in (T.Q4_K, T.Q5_K, T.Q2_K):
        return f(d * f(sc)) * f(code) - f(mm * f(mins))
    if t in (T.Q3_K, T.Q6_K, T.IQ4_XS):
        return f(d * f(sc)) * f(code)
    if t in (T.Q4_1, T.Q5_1):
        return f(d * f(code)) + mm
    return f(d * f(code))


@pytest.mark.parametrize("t", TYPES, ids=lambda t: T.NAMES[t])
def test_bands_decode_to_what_they_claim(oracle, t):
    m = 16
    raw = extreme_weights(t, m, K, 3 + t)
    w = oracle.dequantize(t, raw, K)
    d, mm = _scale_fields(t, raw)
    bl = T.BLCK[t]
    nb = K // bl
    wb = w.reshape(m, nb, bl)
    assert np.isfinite(w).all()
    assert (w[ZERO_ROW] == 0).all()
    assert (d[:, 1::2] <= 0).all() and (d[:, 0::2] >= 0).all()  # sign bit of d on every other block
    if mm is not None:
        assert (mm[:, 1::3] <= 0).all() and (mm[:, 1::3] < 0).any()
    has_sc = t in SC_MAX
    for b in range(nb):
        mirrored = b % 5 == 1
        for row, code in ((BAND_MAX, CODE_MIN[t] if mirrored else CODE_MAX[t]),
                          (BAND_MIN, (126 if t == T.Q8_0 else CODE_MAX[t]) if mirrored else CODE_MIN[t])):
            for r in (row, row + 8):
                want = _block_value(t, d[r, b], None if mm is None else mm[r, b], code, SC_MAX.get(t, 1), MIN_MAX.get(t, 0))
                assert (wb[r, b] == want).all(), (r, b, wb[r, b][:4], want)
        if not has_sc and b % 7 == 5:  # d = 0 and no mins: exact zeros
            if mm is None:
                assert (wb[:, b] == 0).all()
            else:
                assert (wb[:, b] == mm[:, b][:, None]).all()  # Q4_1 / Q5_1: d * q + m = m
    if has_sc and SC_NEG[t] == 0:  # unsigned sub-block scales and mins all 0: the whole band is exact zeros
        assert (w[BAND_SCNEG::8] == 0).all()
    if t in (T.Q6_K, T.Q3_K, T.IQ4_XS):  # band 2 (scales at max) over random codes: every weight is d * sc * (a valid code)
        sc = SC_MAX[t]
        codes = wb[BAND_SCMAX] / (d[BAND_SCMAX][:, None] * np.float32(sc))
        live = d[BAND_SCMAX] != 0
        c = codes[live]
        assert (c >= CODE_MIN[t]).all() and (c <= CODE_MAX[t]).all() and (c == np.rint(c)).all()


@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0], ids=lambda t: T.NAMES[t])
def test_edge_scales_sit_either_side_of_the_limit(t):
    for inside in (True, False):
        raw = edge_scale_weights(t, 32, K, 5, inside)
        d, _ = _scale_fields(t, raw)
        big = np.float32(np.abs(d).max())
        if t in (T.Q4_K, T.Q5_K):  # the body's f16 constant -1024 * f16(d * sc)
            top = np.float32(np.float16(big * np.float32(63))) * 1024
        else:
            top = big * np.float32(4064 if t == T.Q6_K else 127)
        assert (top <= 65504) == inside, (big, top)
        assert np.isfinite(d).all()


def test_activation_kinds():
    n, k = 32, 1024
    x = extreme_activations(n, k, 1)
    assert np.isfinite(x).all()
    assert (x[ZERO_TOKEN] == 0).all() and (x[ZERO_TOKEN + 16] == 0).all()
    amax = np.abs(x).max(axis=1)
    assert amax[0] <= 1e-7 and 1e5 <= amax[4] <= 3e5 and amax[11] == np.float32(3e5)
    q8k = synth.quantize_activations(T.Q8_K, x).reshape(n, k // 256, 292)
    assert (q8k[6, :, 36:].view(np.int8) == -128).all()  # constant super-blocks: every Q8_K code -128
    assert (q8k[7, :, 36:].view(np.int8).reshape(-1)[0::2] == -128).all()
    q80 = synth.quantize_activations(T.Q8_0, x).reshape(n, k // 32, 34)
    assert (np.abs(q80[6, :, 2:].view(np.int8)) == 127).all()
    assert (np.abs(q80[7, :, 2:].view(np.int8)) == 127).all()
    assert (q80[2, 1, 2:] == 0).all() and (q80[2, 1, :2] == 0).all()  # an all-zero block: d = 0, codes 0
    bm = np.abs(x[8]).reshape(-1, 32).max(axis=1)
    assert bm[0::2].min() / bm[1::2].max() > 1e5  # one token whose blocks differ by six orders of magnitude


def _per_token_ok(C, G, tol):
    for j in range(G.shape[0]):
        if not np.any(G[j]):
            assert not np.any(C[j]), j
            continue
        assert rel_err(C[j], G[j]) <= tol, (j, KINDS[j % 16], rel_err(C[j], G[j]))


@pytest.mark.parametrize("t", TYPES, ids=lambda t: T.NAMES[t])
@pytest.mark.parametrize("real_scale", [False, True], ids=["synth_d", "real_d"])
def test_oracle_agrees_with_f64_on_extremes(oracle, t, real_scale):
    """Integer block dots + f32 scales (the oracle the GPU tests use) against dequantise-to-f64, per token against its own
    scale, on extreme weights x extreme activations: pins the reference at exactly the inputs the GPU tests feed it."""
    m, n, k = 40, 16, 1024
    A = extreme_weights(t, m, k, 40 + t, real_scale=real_scale)
    bt = T.VEC_DOT[t]
    x = for_vec_dot(extreme_activations(n, k, 41), bt)
    B = synth.quantize_activations(bt, x)
    ok, Cm = oracle.sgemm(t, A, bt, B, m, n, k, nth=2)
    assert ok == 1 and np.isfinite(Cm).all()
    G = oracle.f64_gemm(t, A, bt, B, m, n, k)
    assert (Cm[ZERO_TOKEN] == 0).all() and (Cm[:, ZERO_ROW] == 0).all()
    # Q8_1 keeps s = d * sum(q) as an f16 field of its own: the mins term m * s carries that rounding (2^-12 of it), the f64
    # product dequantises d * q instead
    _per_token_ok(Cm, G, 5e-5 if bt == T.Q8_1 else 5e-7)
