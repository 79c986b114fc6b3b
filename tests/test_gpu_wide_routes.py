"""The launch forms of the scaled-operand wide call that only the grid size selects (csrc/gemm_wide.hip: wide_go; DESIGN.md
section 34), each at the ragged edges of its tiles.  No flag selects a form, so every case first ASKS the library which form its
shape takes (lfamd_gemm_wide_plan_of, the function wide_go switches on; tests/test_gemm_wide_plan.py pins the same shapes without a
GPU) and then checks, on small k (256 .. 1024) so that every output can be compared:

  (a) every output against the oracle on the Q8_K-quantised activations, for f32 rows and for pre-quantised Q8_K rows, at the
      project's bounds of the scaled bodies (normwise 1e-3, no element beyond 1.5e-3 (|G| + rms)).  The inputs are chosen so that
      the f16 operands are exactly representable (wide_routes.representable / route_activations): the arithmetic itself then
      costs ~1e-7 (profiles/wide_routes_model_error.txt), and the figures printed here show anything a tile edge adds;
  (b) bits: `kr` against the same call on weights padded with random rows to whole 256-row blocks and on tokens padded to whole
      128-token tiles; the tail split against calls on the rows below the cut (reported `lw128`) and above it (`lw64`); the
      two-type launch against the separate calls; a rerun;
  (c) the destination through the raw entry points with ldc > m in a sentinel-filled buffer: nothing outside [0, n) x [0, m) is
      written, nothing inside is NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T
import wide_routes as R
from wide_routes import KR, LW128, SPLIT, LW64

pytestmark = pytest.mark.gpu

FILL = 0xC7  # as f32 -1.02e5: a sentinel that is no NaN
WORD = np.uint32(0x01010101 * FILL)
GUARD = 64


def _p(v):
    return C.c_void_p(v)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32_rows(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.uint8).view(x.shape[0], -1)


def launch(gpu, Ws, Bd, Btype, n, flags=0, ldc_extra=8):
    """lfamd_mul_mat (one matrix), lfamd_mul_mat_multi (one type) or lfamd_mul_mat_multi_types with every result at
    ldc = m + ldc_extra, 64 words (256 bytes) into a buffer of sentinel words, and a workspace of exactly the documented size.
    ldc_extra = 8 keeps ldc a multiple of 4 where m is one (the bodies' float4 stores), 5 never does (their scalar stores).
    Checks (c); returns f32 [n, m] each."""
    L = _hip.lib()
    cnt = len(Ws)
    k = Ws[0].cols
    flags |= gpu.host_variant_flags()
    assert not any(w.exact_only for w in Ws), "the weights left the scaled bodies' range: the call would run exact codes"
    ldcs = [w.rows + ldc_extra for w in Ws]
    bufs = [torch.full(((2 * GUARD + n * ld) * 4,), FILL, dtype=torch.uint8, device="cuda") for ld in ldcs]
    need = max(L.lfamd_mul_mat_workspace(w.type, w.rows, k, n) for w in Ws)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    st = _p(torch.cuda.current_stream().cuda_stream)
    pC = [b.data_ptr() + GUARD * 4 for b in bufs]
    brb = Bd.stride(0) if Btype != _hip.TYPE_STAGED_SCALED else 0
    if cnt == 1:
        rc = L.lfamd_mul_mat(Ws[0].type, _p(Ws[0].data.data_ptr()), Ws[0].rows, k, Btype, _p(Bd.data_ptr()), brb, n, _p(pC[0]), ldcs[0],
                             _p(ws.data_ptr()), need, flags, st)
    else:
        A = (C.c_void_p * cnt)(*[w.data.data_ptr() for w in Ws])
        Cs = (C.c_void_p * cnt)(*pC)
        ms = (C.c_long * cnt)(*[w.rows for w in Ws])
        ld = (C.c_long * cnt)(*ldcs)
        if len({w.type for w in Ws}) == 1:
            rc = L.lfamd_mul_mat_multi(Ws[0].type, cnt, A, ms, k, Btype, _p(Bd.data_ptr()), brb, n, Cs, ld, _p(ws.data_ptr()), need, flags, st)
        else:
            ts = (C.c_int * cnt)(*[w.type for w in Ws])
            rc = L.lfamd_mul_mat_multi_types(cnt, ts, A, ms, k, Btype, _p(Bd.data_ptr()), brb, n, Cs, ld, _p(ws.data_ptr()), need, flags, st)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.lfamd_last_error())
    outs = []
    for w, ld, b in zip(Ws, ldcs, bufs):
        h = b.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == WORD).all() and (h[GUARD + n * ld:] == WORD).all(), "words around the result were written"
        body = h[GUARD:GUARD + n * ld].reshape(n, ld)
        assert (body[:, w.rows:] == WORD).all(), "the gap between result columns (ldc > m) was written"
        out = body[:, :w.rows].copy().view(np.float32)
        assert not np.isnan(out).any()
        outs.append(out)
    return outs


def against_oracle(oracle, tag, ts, raws, B, n, k, outs):
    """(a): every output of every matrix; prints the figures in the style of DEFAULT_BODY_ERROR."""
    for j, (t, raw, out) in enumerate(zip(ts, raws, outs)):
        ok, G = oracle.sgemm(t, raw, T.Q8_K, B, raw.shape[0], n, k, nth=8)
        assert ok == 1
        err, frac, worst = R.figures(out, G)
        print(f"WIDE_ROUTE_ERROR {tag}[{j}] {T.NAMES[t]} m={raw.shape[0]} n={n} k={k}: normwise={err:.3e} frac_over_1.5e-3={frac:.6f} "
              f"worst_elem={worst:.3e}")
        assert err <= R.SCALED_TOL, (tag, j, err)
        assert frac == 0.0, (tag, j, frac, worst)


def upload(gpu, ts, raws, k):
    return [gpu.upload_weights(t, raw, raw.shape[0], k) for t, raw in zip(ts, raws)]


@pytest.mark.parametrize("run", R.RUNS, ids=[R.run_id(r) for r in R.RUNS])
def test_form_at_its_ragged_edges(gpu, oracle, run):
    """One case of wide_routes.CASES (its `what` names the edge): the form is asserted, then (a), (b) and (c) of the module docstring."""
    name, t, control = run
    form, _, ms, n, nb, what = R.CASES[name]
    k, ms = nb * 256, list(ms)
    assert R.call_form(t, ms, k, n)[0] == form, (name, what)  # BEFORE anything is launched
    ts = [t] * len(ms)
    raws, x, B = R.inputs(ms, t, n, k, R.seed_of(name), control)
    Ws = upload(gpu, ts, raws, k)
    xd = f32_rows(x)
    outs = launch(gpu, Ws, xd, T.F32, n)
    against_oracle(oracle, R.run_id(run) + " f32", ts, raws, B, n, k, outs)
    outs_q = launch(gpu, Ws, torch.from_numpy(B).cuda(), T.Q8_K, n)
    against_oracle(oracle, R.run_id(run) + " q8k", ts, raws, B, n, k, outs_q)
    again = launch(gpu, Ws, xd, T.F32, n, ldc_extra=5)  # (the rerun through the other store path)
    for a, b in zip(outs, again):
        assert np.array_equal(_bits(a), _bits(b)), "a rerun differs"

    if form == KR:
        # the same call on weights padded with random rows to whole 256-row blocks: the first m rows keep their bits
        pad = [(m + 255) // 256 * 256 for m in ms]
        assert R.call_form(t, pad, k, n)[0] == KR
        praws = [np.concatenate([raw, R.route_weights(t, p - m, k, 77 + j, control=True)]) if p > m else raw
                 for j, (raw, m, p) in enumerate(zip(raws, ms, pad))]
        pouts = launch(gpu, upload(gpu, ts, praws, k), xd, T.F32, n)
        for j, (a, b, m) in enumerate(zip(outs, pouts, ms)):
            assert np.array_equal(_bits(a), _bits(b[:, :m])), ("rows padded to 256", j)
        # ... and on tokens padded to whole 128-token tiles: the first n columns keep their bits
        n_pad = R.n_pad_of(n)
        assert R.call_form(t, ms, k, n_pad)[0] == KR
        xp = np.concatenate([x, R.route_activations(n_pad - n, k, 78)])
        touts = launch(gpu, Ws, f32_rows(xp), T.F32, n_pad)
        for j, (a, b) in enumerate(zip(outs, touts)):
            assert np.array_equal(_bits(a), _bits(b[:n])), ("tokens padded to 128", j)

    if form == SPLIT:
        _, lo, hi = R.plan_of(t, ms, nb, n, 0, parts=True)
        # the rows below the cut as ONE call, which the library reports as 128 x 128 tiles
        assert R.call_form(t, [p[2] for p in lo], k, n) == (LW128, 0, 1)
        lo_raws = [np.ascontiguousarray(raws[j][r0:r0 + rows]) for j, r0, rows, _ in lo]
        lo_outs = launch(gpu, upload(gpu, [t] * len(lo), lo_raws, k), xd, T.F32, n)
        for (j, r0, rows, _), o in zip(lo, lo_outs):
            assert np.array_equal(_bits(outs[j][:, r0:r0 + rows]), _bits(o)), ("below the cut", j, r0, rows)
        # the rows above it, each matrix alone on 128 x 64 tiles
        for j, r0, rows, _ in hi:
            assert R.call_form(t, [rows], k, n) == (LW64, 0, 1)
            o = launch(gpu, upload(gpu, [t], [np.ascontiguousarray(raws[j][r0:r0 + rows])], k), xd, T.F32, n)[0]
            assert np.array_equal(_bits(outs[j][:, r0:r0 + rows]), _bits(o)), ("above the cut", j, r0, rows)


def test_kr_below_257_tiles_on_the_staged_scaled_image(gpu, oracle):
    """Two Q4_K matrices of 196 tiles together.  The int8 body would take that grid; LFAMD_FLAG_GEMM_WIDE keeps it away (it cannot
    read LFAMD_TYPE_STAGED_SCALED, and a staged call of such a grid without the flag is LFAMD_ERR_UNSUPPORTED), and the launch is
    `kr` below 257 tiles.  On f32 rows against the oracle; then on the image lfamd_rms_norm_quantize staged, which must give the
    bits of the same call on the producer's f32 output (that output is no longer exactly representable, so it is tied to the
    oracle through the first half, not measured against it)."""
    L = _hip.lib()
    form, t, ms, n, nb = R.KR_STAGED
    k, ms = nb * 256, list(ms)
    assert R.call_form(t, ms, k, n, flags=R.FLAG_GEMM_WIDE)[0] == KR
    raws, x, B = R.inputs(ms, t, n, k, R.seed_of("kr-staged"))
    Ws = upload(gpu, [t, t], raws, k)
    outs = launch(gpu, Ws, f32_rows(x), T.F32, n, flags=_hip.FLAG_GEMM_WIDE)
    against_oracle(oracle, "kr-staged f32", [t, t], raws, B, n, k, outs)
    st = _p(torch.cuda.current_stream().cuda_stream)
    image = torch.full((L.lfamd_staged_scaled_size(k, n),), 0x5A, dtype=torch.uint8, device="cuda")
    xd = torch.from_numpy(x).cuda()
    w = torch.ones(k, dtype=torch.float32, device="cuda")
    yf = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    _hip.check(L.lfamd_rms_norm_quantize(_p(xd.data_ptr()), k * 4, _p(w.data_ptr()), 1e-5, n, k, _hip.TYPE_STAGED_SCALED,
                                         _p(image.data_ptr()), 0, _p(yf.data_ptr()), k * 4, st), "rms_norm_quantize (scaled image)")
    torch.cuda.synchronize()
    staged = launch(gpu, Ws, image, _hip.TYPE_STAGED_SCALED, n, flags=_hip.FLAG_GEMM_WIDE)
    same = launch(gpu, Ws, yf.view(torch.uint8).view(n, k * 4), T.F32, n, flags=_hip.FLAG_GEMM_WIDE)
    for a, b in zip(staged, same):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("pair", R.DUAL[0], ids=lambda p: f"{T.NAMES[p[0]]}+{T.NAMES[p[1]]}")
def test_two_types_in_one_launch_ragged(gpu, oracle, pair):
    """lfamd_lw_dual_go at 134 tiles with ragged last blocks in both groups and 100 of 128 tokens: against the oracle, and the
    Q5_K / Q6_K results against the bits of the separate calls (128 x 64 loader-wave tiles; a separate Q4_K call runs gemm_ks)."""
    _, ms, n, nb = R.DUAL
    k, ms, ts = nb * 256, list(ms), list(pair)
    ra, rb = R.row_blocks(ms[:1]), R.row_blocks(ms[1:])
    assert R.plan_lib().lfamd_gemm_wide_dual_ok(ra, rb, R.n_pad_of(n)) == 1
    raws, x, B = R.inputs(ms, ts, n, k, R.seed_of("dual"))
    Ws = upload(gpu, ts, raws, k)
    xd = f32_rows(x)
    outs = launch(gpu, Ws, xd, T.F32, n)
    tag = f"dual-{T.NAMES[ts[0]]}+{T.NAMES[ts[1]]}"
    against_oracle(oracle, tag + " f32", ts, raws, B, n, k, outs)
    against_oracle(oracle, tag + " q8k", ts, raws, B, n, k, launch(gpu, Ws, torch.from_numpy(B).cuda(), T.Q8_K, n))
    for a, b in zip(outs, launch(gpu, Ws, xd, T.F32, n, ldc_extra=5)):
        assert np.array_equal(_bits(a), _bits(b)), "a rerun differs"
    for j, (t, W) in enumerate(zip(ts, Ws)):
        if t != T.Q4_K:
            assert R.call_form(t, [ms[j]], k, n) == (LW64, 0, 1)
            assert np.array_equal(_bits(outs[j]), _bits(launch(gpu, [W], xd, T.F32, n)[0])), T.NAMES[t]
