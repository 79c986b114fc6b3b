"""Every mat-mul body the dispatcher can pick, fed the adversarial operands of extremes.py (negative and zero d, f16-subnormal d,
negative mins, codes and sub-block scales at both ends, tokens from 1e-7 to 3e5, all-zero and constant blocks, outlier channels),
with f32 and with pre-quantised activations, against the oracle on a row x token sample, each token judged against its own
scale.

The bound of every case is the one lfamd_mul_mat_is_exact promises for the call: exact (the reference's integer arithmetic up to
the order of the f32 sums) -> 2e-6 normwise and no element beyond rtol 1e-5; otherwise the scaled f16 bodies' 1e-3 and rtol 1.5e-3;
each plus the rounding of the summed terms themselves (check()).  So this matrix is also the test of the predicate: no per-type
exception is written down here."""
import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
from extremes import CASES, CASE_FLAGS, ZERO_ROW, ZERO_TOKEN, KINDS, case_id, edge_scale_weights, extreme_activations, extreme_weights, for_vec_dot
from helpers import elem_err, rel_err

pytestmark = pytest.mark.gpu

EXACT = (2e-6, 1e-5)
SCALED = (1e-3, 1.5e-3)
F = CASE_FLAGS

_cache = {}


def _weights(t, m, k, seed, real_scale=False):
    key = ("w", t, m, k, seed, real_scale)
    if key not in _cache:
        _cache.clear()
        _cache[key] = extreme_weights(t, m, k, seed, real_scale=real_scale)
    return _cache[key]


def sample_rows(m):
    """The bands (rows 0 .. 15, ZERO_ROW among them), a stride through the rest, the last rows."""
    return np.unique(np.concatenate([np.arange(min(m, 24)), np.arange(24, m, max(1, m // 40)), np.arange(max(0, m - 8), m)]))


def sample_tokens(n):
    return np.arange(n) if n <= 40 else np.unique(np.concatenate([np.arange(32), np.arange(n - 8, n)]))


def oracle_sample(oracle, t, A, B, k, rows, cols):
    bt = T.VEC_DOT[t]
    ok, G = oracle.sgemm(t, np.ascontiguousarray(A[rows]), bt, np.ascontiguousarray(B[cols]), len(rows), len(cols), k, nth=8)
    assert ok == 1
    return G


def abs_products(oracle, t, A, x, k, rows, cols):
    """sum_l |w[i, l]| * |x[j, l]| of the sample, with |x| widened by a quantisation step: the size of the terms an output sums."""
    w = np.abs(oracle.dequantize(t, np.ascontiguousarray(A[rows]), k)).astype(np.float64)
    xs = np.abs(x[cols]).astype(np.float64)
    xs += xs.max(axis=1, keepdims=True) / 127.0
    return xs @ w.T


def rounding_unit(exact, k):
    """What one output may move per unit of sum |w| |x| on top of the relative bound: scaled operands round each operand of every
    product once in f16 (2^-11 each); exact bodies round f32 scale products and sums of k / 32 block terms, on both sides."""
    return 2.0 ** -10 if not exact else (k / 32) * 2.0 ** -23


def check(Cs, G, cols, rows, exact, what, zero_row=True, absprod=None, k=None):
    """Cs, G: [tokens, rows] of the sample.  Finite; all-zero token and d = dmin = 0 row give exactly 0; per token, on every row:
        max |C - G| <= tol * max |G| + u * max A        and every element  |C - G| <= rtol * (|G| + rms G) + u * A
    with (tol, rtol) = (2e-6, 1e-5) exact, (1e-3, 1.5e-3) scaled, A = sum |w| |x| and u = rounding_unit().  Where the products of an
    output do not cancel, A is about |G| and u * A is far below the relative term; where they do (constant, alternating and
    outlier tokens against rows of maximal codes or of 1000x scales), the rounding of the terms is what the result can be off by,
    and no arithmetic short of the exact one meets a bound relative to the result alone."""
    tol, rtol = EXACT if exact else SCALED
    assert np.isfinite(Cs).all(), (what, "non-finite outputs at tokens", sorted({KINDS[c % 16] for c in cols[~np.isfinite(Cs).all(axis=1)]}))
    for a, j in enumerate(cols):
        if j % 16 == ZERO_TOKEN:
            assert (Cs[a] == 0).all(), (what, "all-zero token", j)
    zr = np.where(rows == ZERO_ROW)[0]
    if zero_row and len(zr):
        assert (Cs[:, zr] == 0).all(), (what, "all-zero row")
    assert absprod is not None and k is not None
    u = rounding_unit(exact, k)
    bad = []
    for a, j in enumerate(cols):
        g = G[a].astype(np.float64)
        if not np.any(g):
            if np.any(Cs[a]):
                bad.append((int(j), KINDS[j % 16], "nonzero where the oracle is 0"))
            continue
        d = np.abs(Cs[a].astype(np.float64) - g)
        rms = float(np.sqrt(np.mean(g * g)))
        A = absprod[a]
        norm_ok = d.max() <= tol * np.abs(g).max() + u * A.max()
        over = d > rtol * (np.abs(g) + rms) + u * A
        if not norm_ok or over.any():
            bad.append((int(j), KINDS[j % 16], rel_err(Cs[a], g), float(over.mean()), float((d / (u * A + 1e-300)).max()),
                        rows[over][:4].tolist()))
    assert not bad, (what, "exact" if exact else "scaled", bad[:8])


def run(gpu, W, x, t, n, flags, f32in, B=None):
    k = x.shape[1]
    bt = T.VEC_DOT[t]
    if f32in:
        Bd = torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.uint8).view(n, k * 4)
        out = gpu.mul_mat(W, Bd, T.F32, n=n, flags=flags)
    else:
        out = gpu.mul_mat(W, torch.from_numpy(B).cuda(), bt, n=n, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def body_case(gpu, oracle, t, m, n, k, flag_names=(), seed=1, real_scale=False, A=None, expect_exact=None, both_bits=False,
              zero_row=True):
    """Run (t, m x k, n tokens, flags) on extreme operands with f32 and with pre-quantised activations; the bound comes from
    lfamd_mul_mat_is_exact (the upload's range check adds its flag, as mul_mat does)."""
    flags = gpu.host_variant_flags()
    for f in flag_names:
        flags |= F[f]
    A = _weights(t, m, k, seed, real_scale) if A is None else A
    bt = T.VEC_DOT[t]
    x = for_vec_dot(extreme_activations(n, k, seed + 100), bt)
    B = synth.quantize_activations(bt, x)
    W = gpu.upload_weights(t, A, m, k)
    call_flags = flags | (_exact_flag(t) if getattr(W, "exact_only", False) else 0)
    exact = bool(_hip.lib().lfamd_mul_mat_is_exact(t, m, k, n, call_flags))
    if expect_exact is not None:
        assert exact == expect_exact, ("lfamd_mul_mat_is_exact", T.NAMES[t], m, k, n, flag_names, exact)
    rows, cols = sample_rows(m), sample_tokens(n)
    G = oracle_sample(oracle, t, A, B, k, rows, cols)
    ap = abs_products(oracle, t, A, x, k, rows, cols)
    outs = []
    for f32in in (True, False):
        Cn = run(gpu, W, x, t, n, flags, f32in, B)
        check(Cn[np.ix_(cols, rows)], G, cols, rows, exact, (T.NAMES[t], m, n, k, flag_names, "f32" if f32in else "quantised"),
              zero_row=zero_row, absprod=ap, k=k)
        outs.append(Cn)
    if both_bits:
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "f32 and pre-quantised input differ"
    return W, exact


def _exact_flag(t):
    return _hip.FLAG_Q80_EXACT if t == T.Q8_0 else _hip.FLAG_PRECISE


# ---------------------------------------------------------------------------------------------------------------- decode GEMV
@pytest.mark.parametrize("t", T.QUANT_WEIGHT_TYPES, ids=lambda t: T.NAMES[t])
@pytest.mark.parametrize("real_scale", [False, True], ids=["synth_d", "real_d"])
def test_decode_gemv(gpu, oracle, t, real_scale):
    """n = 1, 3, 8 over 16 extreme tokens (one call per chunk): exact, and f32 input gives the bits of pre-quantised input."""
    m, k = 200, 1024
    A = _weights(t, m, k, 11, real_scale)
    bt = T.VEC_DOT[t]
    x = for_vec_dot(extreme_activations(16, k, 12), bt)
    B = synth.quantize_activations(bt, x)
    rows = sample_rows(m)
    G = oracle_sample(oracle, t, A, B, k, rows, np.arange(16))
    ap = abs_products(oracle, t, A, x, k, rows, np.arange(16))
    W = gpu.upload_weights(t, A, m, k)
    for n in (1, 3, 8):
        assert _hip.lib().lfamd_mul_mat_is_exact(t, m, k, n, gpu.host_variant_flags()) == 1
        for j0 in range(0, 16 - n + 1, n):
            cols = np.arange(j0, j0 + n)
            c32 = run(gpu, W, x[cols], t, n, None, True)
            cq = run(gpu, W, x[cols], t, n, None, False, np.ascontiguousarray(B[cols]))
            assert np.array_equal(c32.view(np.uint32), cq.view(np.uint32)), (T.NAMES[t], n, j0)
            check(cq[:, rows], G[cols], cols, rows, True, (T.NAMES[t], "gemv", n, j0), absprod=ap[cols], k=k)


# ------------------------------------------------------------------------------------------------------------- batch bodies
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_body(gpu, oracle, case):
    """The bound is the predicate's; where the case says what the predicate must answer, it is checked too."""
    t, m, n, k, fl, expect = case
    body_case(gpu, oracle, t, m, n, k, fl, seed=20 + t, expect_exact=expect, both_bits=n <= 32 and t in (T.Q4_K, T.Q5_K, T.Q6_K))


@pytest.mark.parametrize("t", [T.Q4_K, T.Q6_K, T.Q8_0, T.IQ4_XS], ids=lambda t: T.NAMES[t])
def test_batch_body_real_scale(gpu, oracle, t):
    """d moved into the 2^-15 .. 2^-11 of real files: d * sc of small sub-block scales becomes an f16 subnormal."""
    m, n, k = 1024, 200, 2048
    body_case(gpu, oracle, t, m, n, k, seed=30 + t, real_scale=True)


@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0], ids=lambda t: T.NAMES[t])
@pytest.mark.parametrize("inside", [True, False], ids=["inside", "outside"])
def test_scale_range_edge(gpu, oracle, t, inside):
    """Block scales just inside the scaled batch bodies' f16 range keep them, within their bound; just outside, the upload's range
    check flips the matrix to the exact arithmetic and the predicate's bound for that call holds (exact for Q4_K / Q5_K / Q8_0;
    Q6_K's exact-code body still rounds sc * (q - 32) above 2048).  Before the checks were right, Q4_K / Q5_K scales just under
    the old |d| * 63 < 64 overflowed f16(d * sc) * -1024 to inf, and Q8_0 had no check at all."""
    m, n, k = 1024, 200, 2048
    A = edge_scale_weights(t, m, k, 40 + t, inside)
    W, exact = body_case(gpu, oracle, t, m, n, k, seed=40 + t, A=A, zero_row=False)
    assert W.exact_only == (not inside), (T.NAMES[t], inside)
    assert exact == (not inside and t != T.Q6_K), (T.NAMES[t], inside, exact)


# ------------------------------------------------------------------------------------------------------------- MUL_MAT_ID
MMID = [(t, tokens, f) for t in (T.Q4_K, T.Q6_K) for tokens in (3, 150) for f in (False, True)] + [(T.Q4_0, 3, False), (T.Q4_0, 40, False)]


@pytest.mark.parametrize("t,tokens,f32in", MMID, ids=lambda v: None)  # (F32 activations: K-quant experts only)
def test_mul_mat_id(gpu, oracle, t, tokens, f32in):
    rows, cols, experts, thinkers = 96, 1024, 4, 2
    Ws = [extreme_weights(t, rows, cols, 60 + e) for e in range(experts)]
    packed = torch.cat([gpu.upload_weights(t, W, rows, cols).data for W in Ws])
    bt = T.VEC_DOT[t]
    x = for_vec_dot(extreme_activations(tokens, cols, 61), bt)
    xq = synth.quantize_activations(bt, x)
    plan = (np.arange(tokens * thinkers).reshape(tokens, thinkers) % experts).astype(np.int32)
    thought = torch.from_numpy(x).cuda().view(torch.uint8).view(tokens, cols * 4) if f32in else torch.from_numpy(xq).cuda()
    flags = gpu.host_variant_flags()
    res = gpu.mul_mat_id(packed, t, rows, cols, experts, thought, T.F32 if f32in else bt, 1, tokens,
                         torch.from_numpy(plan).cuda(), thinkers, flags=flags).cpu().numpy()
    exact = bool(_hip.lib().lfamd_mul_mat_is_exact(t, rows, cols, tokens, flags))
    allr = np.arange(rows)
    for e in range(experts):
        sel = [(tok, th) for tok in range(tokens) for th in range(thinkers) if plan[tok, th] == e]
        toks = np.array([tok for tok, _ in sel])
        ok, G = oracle.sgemm(t, Ws[e], bt, np.ascontiguousarray(xq[toks]), rows, len(toks), cols, nth=8)
        assert ok == 1
        got = np.stack([res[tok, th] for tok, th in sel])
        ap = abs_products(oracle, t, Ws[e], x, cols, allr, toks)
        check(got, G, toks, allr, exact, (T.NAMES[t], "mul_mat_id", tokens, e), absprod=ap, k=cols)


# ------------------------------------------------------------------------------------------ sibling matrices, one launch
@pytest.mark.parametrize("n", [1, 64, 512])
def test_multi_types_qkv(gpu, oracle, n):
    """attn_q / attn_k as Q4_K and attn_v as Q6_K on the same activations (mul_mat_multi_types): the dual GEMV at n = 1, one
    shared staging of the batch otherwise.  Mixed launches run the scaled bodies (the per-matrix predicate does not hold for
    them: include/lfamd_hip.h), so batches are held to the scaled bound."""
    k = 2048
    shapes = [(T.Q4_K, 512), (T.Q4_K, 256), (T.Q6_K, 256)]
    As = [extreme_weights(t, m, k, 70 + j) for j, (t, m) in enumerate(shapes)]
    Ws = [gpu.upload_weights(t, A, m, k) for (t, m), A in zip(shapes, As)]
    x = extreme_activations(n, k, 71)
    B = synth.quantize_activations(T.Q8_K, x)
    cols = sample_tokens(n)
    for f32in in (True, False):
        Bd = torch.from_numpy(x).cuda().view(torch.uint8).view(n, k * 4) if f32in else torch.from_numpy(B).cuda()
        outs = gpu.mul_mat_multi(Ws, Bd, T.F32 if f32in else T.Q8_K, n=n)
        torch.cuda.synchronize()
        for (t, m), A, o in zip(shapes, As, outs):
            rows = sample_rows(m)
            G = oracle_sample(oracle, t, A, B, k, rows, cols)
            ap = abs_products(oracle, t, A, x, k, rows, cols)
            check(o.cpu().numpy()[np.ix_(cols, rows)], G, cols, rows, n <= 8, (T.NAMES[t], "multi_types", n, f32in), absprod=ap, k=k)
