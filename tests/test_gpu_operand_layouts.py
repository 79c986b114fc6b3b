"""Every mat-mul entry point of the C ABI with the arithmetic fixed and the LAYOUT of its operands varied, one axis at a time:
activation rows at a stride larger than the row, at a base inside an allocation, a result with ldc > m or starting 4 bytes into
its buffer, a workspace of exactly the documented size whose contents are 0x00 or 0xFF.  A layout must not change which products
are summed or in what order, so every accepted layout must give the BITS of the same call on the layout the rest of the suite
uses (contiguous rows at an allocation's base, ldc = m, a zero-filled workspace) — that baseline is held to the oracle, body by
body, by test_gpu_operand_extremes.py, test_gpu_decode_variants.py and test_gpu_parity.py.  One documented exception: float
weights at n <= 8 whose rows are not 16-byte aligned leave gemv_float for the generic kernel (api.hip, `aligned16(d_B)` under
mm_body::gemv_float); those are held to gemv_float's own bound, 2e-6 of oracle.f64_gemm.

Everything around the operands is a sentinel: the gaps between rows are 0xFF (an f32 NaN, a NaN block scale: a kernel that reads
a gap poisons its output) and must be unchanged afterwards, the result buffer is 0xC7 outside the m x n results, the workspace
has 64 guard bytes behind it.  Layouts the contract of include/lfamd_hip.h ("Operand layout") does not take — f32 rows of
quantised weights that are not 16-byte aligned (read as float4), rows below their format's alignment, a result off 4 bytes, a
workspace off 256 — must answer LFAMD_ERR_INVALID, a workspace one byte short LFAMD_ERR_WORKSPACE, with result and workspace
untouched.  No wrong-layout case leaves the test's own allocations: every buffer is larger than what any stride could reach."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, sgemm, synth
from extremes import CASES, CASE_FLAGS, case_id
from helpers import rel_err

pytestmark = pytest.mark.gpu

OK, INVALID, WORKSPACE = 0, -2, -4
B_FILL, C_FILL, GUARD = 0xFF, 0xC7, 0xA5
FLOATS = (T.F32, T.F16, T.BF16)
KQ = (T.Q4_K, T.Q5_K, T.Q6_K)
# the alignment of a row of each activation format, which is also the smallest step its stride can grow by
ALIGN = {T.F32: 4, T.F16: 2, T.BF16: 2, T.Q8_K: 4, T.Q8_1: 4, T.Q8_0: 2}


def _p(v):
    return C.c_void_p(v)


def _stream():
    return _p(torch.cuda.current_stream().cuda_stream)


_wcache = {}


def _weights(t, m, k, seed):
    """(raw rows, packed weights), the last one kept: consecutive test ids share a matrix."""
    key = (t, m, k, seed)
    if key not in _wcache:
        _wcache.clear()
        A = synth.random_weights(t, m, k, seed)
        _wcache[key] = (A, sgemm.upload_weights(t, A, m, k))
    return _wcache[key]


def _inputs(t_list, x):
    """f32 rows as bytes, and the rows in the vec_dot format of the weights."""
    ins = {T.F32: np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1)}
    bt = T.VEC_DOT[t_list[0]]
    assert all(T.VEC_DOT[t] == bt for t in t_list)
    if bt != T.F32:
        ins[bt] = synth.quantize_activations(bt, x)
    return ins


class MulMat:
    """One lfamd_mul_mat call."""

    def __init__(self, t, m, n, k, flag_names=(), seed=1):
        L = _hip.lib()
        self.t, self.m, self.n, self.k = t, m, n, k
        self.quantised = t not in FLOATS
        self.A, self.W = _weights(t, m, k, seed)
        self.flags = sgemm.host_variant_flags() | (self.W.exact_flag if self.W.exact_only else 0)
        for f in flag_names:
            self.flags |= CASE_FLAGS[f]
        self.inputs = _inputs([t], synth.random_activations(n, k, seed + 1))
        self.outs = [(m, n)]
        self.ws_need = L.lfamd_mul_mat_workspace(t, m, k, n)
        self.fixed_ldc = False

    def call(self, Btype, pB, brb, pCs, ldcs, pws, wsb):
        return _hip.lib().lfamd_mul_mat(self.t, _p(self.W.data.data_ptr()), self.m, self.k, Btype, _p(pB), brb, self.n, _p(pCs[0]), ldcs[0],
                                        _p(pws), wsb, self.flags, _stream())


class Multi:
    """lfamd_mul_mat_multi (one type) or lfamd_mul_mat_multi_types over sibling matrices of unequal height."""

    def __init__(self, shapes, n, k, typed, seed=5):
        L = _hip.lib()
        self.shapes, self.n, self.k, self.typed = shapes, n, k, typed
        self.quantised = True
        self.Ws = [sgemm.upload_weights(t, synth.random_weights(t, m, k, seed + j), m, k) for j, (t, m) in enumerate(shapes)]
        self.flags = sgemm.host_variant_flags()
        for w in self.Ws:
            self.flags |= w.exact_flag if w.exact_only else 0
        self.inputs = _inputs([t for t, _ in shapes], synth.random_activations(n, k, seed + 9))
        self.outs = [(m, n) for _, m in shapes]
        self.ws_need = max(L.lfamd_mul_mat_workspace(t, m, k, n) for t, m in shapes)
        self.fixed_ldc = False

    def call(self, Btype, pB, brb, pCs, ldcs, pws, wsb):
        L, cnt = _hip.lib(), len(self.shapes)
        A = (C.c_void_p * cnt)(*[w.data.data_ptr() for w in self.Ws])
        Cs = (C.c_void_p * cnt)(*pCs)
        ms = (C.c_long * cnt)(*[m for _, m in self.shapes])
        ld = (C.c_long * cnt)(*ldcs)
        if self.typed:
            ts = (C.c_int * cnt)(*[t for t, _ in self.shapes])
            return L.lfamd_mul_mat_multi_types(cnt, ts, A, ms, self.k, Btype, _p(pB), brb, self.n, Cs, ld, _p(pws), wsb, self.flags, _stream())
        return L.lfamd_mul_mat_multi(self.shapes[0][0], cnt, A, ms, self.k, Btype, _p(pB), brb, self.n, Cs, ld, _p(pws), wsb, self.flags,
                                     _stream())


class MulMatId:
    """One lfamd_mul_mat_id call: 4 experts of 96 x 1024, 2 thinkers; the `thought` rows are the strided operand."""

    def __init__(self, t, tokens, tasks, seed=40):
        L = _hip.lib()
        self.t, self.tokens, self.tasks = t, tokens, tasks
        self.rows, self.cols, self.experts, self.thinkers = 96, 1024, 4, 2
        self.quantised = True
        self.stack = torch.cat([sgemm.upload_weights(t, synth.random_weights(t, self.rows, self.cols, seed + e), self.rows, self.cols).data
                                for e in range(self.experts)])
        self.flags = sgemm.host_variant_flags()
        if t in KQ and tokens > 4:  # batches run on scaled operands: the stack's block scales are checked once (sgemm.mul_mat_id)
            ok = L.lfamd_scaled_gemm_ok(t, self.experts * ((self.rows + 31) // 32) * 32, self.cols, _p(self.stack.data_ptr()), _stream())
            assert ok >= 0
            self.flags |= 0 if ok else _hip.FLAG_PRECISE
        x = synth.random_activations(tokens * tasks, self.cols, seed + 7)
        bt = T.VEC_DOT[t]
        self.inputs = {bt: synth.quantize_activations(bt, x)}
        if t in KQ:  # (F32 activations: K-quant experts only)
            self.inputs[T.F32] = x.view(np.uint8).reshape(tokens * tasks, -1)
        rng = np.random.default_rng(seed)
        plan = np.stack([rng.permutation(self.experts)[:self.thinkers] for _ in range(tokens)]).astype(np.int32)
        self.plan = torch.from_numpy(plan).cuda()
        self.outs = [(self.rows, tokens * self.thinkers)]
        self.ws_need = L.lfamd_mul_mat_id_workspace(t, self.rows, self.cols, self.experts, tokens, self.thinkers)
        self.fixed_ldc = True

    def call(self, Btype, pB, brb, pCs, ldcs, pws, wsb):
        return _hip.lib().lfamd_mul_mat_id(self.t, _p(self.stack.data_ptr()), self.rows, self.cols, self.experts, Btype, _p(pB), brb, self.tasks,
                                           self.tokens, _p(self.plan.data_ptr()), self.thinkers, _p(pCs[0]), _p(pws), wsb, self.flags, _stream())


def run(spec, Btype, b_off=0, b_pad=0, c_off=0, ldc_extra=0, ws_fill=None, ws_off=0, ws_short=0, no_ws=False, expect=OK):
    """The call with its activation rows b_off bytes into a 0xFF buffer and row size + b_pad apart, every result c_off bytes into
    a 0xC7 buffer with ldc = m + ldc_extra, and the workspace: ws_fill None = zero-filled (the baseline), else exactly the documented
    size filled with that byte, ws_off bytes into a buffer with 64 guard bytes behind it; ws_short bytes are withheld from the
    size passed.  Checks the status, that the activations and their gaps, the guards and everything outside the m x n results
    are unchanged, and — for a refused call — that results and workspace are untouched.  Returns the results as uint32 [n, m]."""
    L = _hip.lib()
    rows = spec.inputs[Btype]
    nrow, rb = rows.shape
    stride = rb + b_pad
    hb = np.full(b_off + nrow * stride + 256, B_FILL, np.uint8)
    hb[b_off:b_off + nrow * stride].reshape(nrow, stride)[:, :rb] = rows
    dB = torch.from_numpy(hb).cuda()
    dCs, ldcs = [], []
    for m, ncols in spec.outs:
        ldcs.append(m + ldc_extra)
        dCs.append(torch.full((c_off + ncols * ldcs[-1] * 4 + 256,), C_FILL, dtype=torch.uint8, device="cuda"))
    need = spec.ws_need
    if ws_fill is None:
        dws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    else:
        dws = torch.full((ws_off + need + 64,), GUARD, dtype=torch.uint8, device="cuda")
        dws[ws_off:ws_off + need] = ws_fill
    hws = dws.cpu()
    for d in [dB, dws] + dCs:  # (the offsets above are offsets from an allocation's alignment)
        assert d.data_ptr() % 256 == 0
    pws, wsb = (0, 0) if no_ws or need == 0 else (dws.data_ptr() + ws_off, need - ws_short)
    rc = spec.call(Btype, dB.data_ptr() + b_off, stride, [d.data_ptr() + c_off for d in dCs], ldcs, pws, wsb)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lfamd_last_error())
    assert torch.equal(dB.cpu(), torch.from_numpy(hb)), "the activation rows or the gaps between them were written"
    after = dws.cpu()
    assert torch.equal(after[:ws_off], hws[:ws_off]) and torch.equal(after[ws_off + need:], hws[ws_off + need:]), "workspace guard written"
    out = []
    for (m, ncols), ldc, d in zip(spec.outs, ldcs, dCs):
        h = d.cpu().numpy()
        if expect != OK:
            assert (h == C_FILL).all(), "a refused call wrote into the result"
            continue
        end = c_off + ncols * ldc * 4
        assert (h[:c_off] == C_FILL).all() and (h[end:] == C_FILL).all(), "bytes around the result were written"
        body = h[c_off:end].view(np.uint32).reshape(ncols, ldc)
        assert (body[:, m:] == np.uint32(0x01010101 * C_FILL)).all(), "the gap between result columns (ldc > m) was written"
        out.append(body[:, :m].copy())
    if expect != OK:
        assert torch.equal(after, hws), "a refused call wrote into the workspace"
    return out


_scache = {}


def _spec(key, make):
    """The call and its baselines per activation type, the last one kept."""
    if key not in _scache:
        _scache.clear()
        _scache[key] = (make(), {})
    return _scache[key]


def baseline(spec, base, Btype):
    if Btype not in base:
        base[Btype] = run(spec, Btype)
        for o in base[Btype]:
            assert np.isfinite(o.view(np.float32)).all()
    return base[Btype]


def accepted(spec, Btype, b_off, stride):
    """The contract of include/lfamd_hip.h.  Every reader of f32 rows under quantised weights takes 16 bytes per lane —
    prep_f32_kernel, prep_scaled_kernel and prep80_kernel (prep.hip), sb_prep_kernel (gemm_sb.hip), the staging of gemm_i8.hip,
    gemm_lf.hip and gemm_q80.hip as float4, the decode GEMVs as 16-byte buffer loads (gemv_impl.h: buf_ld16 on make_rsrc(row)) —
    so a base or a stride that is not a multiple of 16 is refused, not run.  Rows in a vec_dot format are read field by field and
    code word by code word at offsets that are only block-aligned inside a contiguous row already (292-, 36-, 34-byte blocks):
    their natural alignment is a layout every body runs today.  Float weights take any element-aligned rows: the generic
    kernels and quantize.hip read elements, prep_float_kernel reads elements where a row is not aligned to its vector loads."""
    if Btype == T.F32 and spec.quantised:
        return b_off % 16 == 0 and stride % 16 == 0
    return b_off % ALIGN[Btype] == 0 and stride % ALIGN[Btype] == 0


def check_layout(spec, base, oracle, Btype, what, **kw):
    rb = spec.inputs[Btype].shape[1]
    b_off, stride = kw.get("b_off", 0), rb + kw.get("b_pad", 0)
    if not accepted(spec, Btype, b_off, stride):
        run(spec, Btype, expect=INVALID, **kw)
        return
    got = run(spec, Btype, **kw)
    want = baseline(spec, base, Btype)
    if not spec.quantised and spec.n <= 8 and (b_off % 16 or stride % 16):
        # the documented other body: mm_body::gemv_float needs aligned16(d_B) and a stride that keeps it, else the generic kernel
        # (api.hip).  Held to gemv_float's parity bound (test_gpu_parity.py::test_float_types_vs_oracle): 2e-6 of a double GEMM.
        G = oracle.f64_gemm(spec.t, spec.A, Btype, spec.inputs[Btype], spec.m, spec.n, spec.k)
        for o in (got[0], want[0]):
            err = rel_err(o.view(np.float32), G)
            assert err <= 2e-6, (what, T.NAMES[Btype], "gemv_float -> generic", err)
        return
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, T.NAMES[Btype], "matrix", j, "differs from the baseline in",
                                      int((g != w).sum()), "of", g.size, "outputs")


AXES = ("b_stride", "b_stride64", "b_base16", "b_base_elem", "c_ldc", "c_base4", "ws_zero", "ws_ff", "ws_short", "refusals")
ID_AXES = tuple(a for a in AXES if a != "c_ldc")  # (d_result has no leading dimension)


def vary(spec, base, oracle, axis, what):
    """One layout axis, for f32 rows and for rows in the vec_dot format."""
    for Btype in spec.inputs:
        a = ALIGN[Btype]
        w = (what, axis)
        if axis == "b_stride":  # f32: 16 bytes; quantised rows: the smallest step their alignment allows (Q8_K, Q8_1: 4; Q8_0: 2)
            check_layout(spec, base, oracle, Btype, w, b_pad=16 if Btype == T.F32 else a)
        elif axis == "b_stride64":
            check_layout(spec, base, oracle, Btype, w, b_pad=64 if Btype == T.F32 else 64 + a)
        elif axis == "b_stride_elem":  # (float weights: the element)
            check_layout(spec, base, oracle, Btype, w, b_pad=a)
        elif axis == "b_base16":
            check_layout(spec, base, oracle, Btype, w, b_off=16)
        elif axis == "b_base_elem":  # the operand's own alignment: 4 bytes for f32 (refused under quantised weights), the block's otherwise
            check_layout(spec, base, oracle, Btype, w, b_off=a)
        elif axis == "c_ldc":
            check_layout(spec, base, oracle, Btype, w, ldc_extra=5)
        elif axis == "c_base4":
            check_layout(spec, base, oracle, Btype, w, c_off=4)
        elif axis == "ws_zero":
            check_layout(spec, base, oracle, Btype, w, ws_fill=0x00)
        elif axis == "ws_ff":
            check_layout(spec, base, oracle, Btype, w, ws_fill=0xFF)
        elif axis == "ws_short":
            if spec.ws_need:
                run(spec, Btype, ws_fill=0xFF, ws_short=1, expect=WORKSPACE)
            else:  # a call whose documented workspace is 0 bytes takes NULL
                check_layout(spec, base, oracle, Btype, w, no_ws=True)
        else:  # refusals: below the format's alignment (base, stride), a result off 4 bytes, a workspace off 256
            assert a > 1
            run(spec, Btype, b_off=a // 2, expect=INVALID)
            run(spec, Btype, b_pad=a // 2, expect=INVALID)
            if Btype == T.F32 and spec.quantised:
                run(spec, Btype, b_pad=4, expect=INVALID)
                run(spec, Btype, b_off=8, ws_fill=0xFF, expect=INVALID)
            run(spec, Btype, c_off=2, expect=INVALID)
            if spec.ws_need:
                run(spec, Btype, ws_fill=0xFF, ws_off=16, expect=INVALID)


# ------------------------------------------------------------------------------------------------------------- batch bodies
# the cases of extremes.CASES that run the int8 body (lfamd_mul_mat_takes_staged) and the scaled f16 bodies (_takes_staged_scaled)
I8_CASES = {"Q4_K-4096x512x4096"}
SCALED_CASES = {"Q4_K-14336x512x4096", "Q5_K-4096x512x4096", "Q6_K-4096x512x4096"}


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_body_layout(gpu, oracle, case, axis):
    """Every body of extremes.CASES at the shape that table gives it, so the dispatcher picks what it picks there, and the
    module's own predicates say so: lfamd_mul_mat_is_exact answers what the table expects, lfamd_mul_mat_takes_staged is 1 for
    exactly the int8 case and lfamd_mul_mat_takes_staged_scaled for exactly the scaled f16 ones."""
    t, m, n, k, fl, expect = case
    spec, base = _spec(("mm", case), lambda: MulMat(t, m, n, k, fl, seed=20 + t))
    L = _hip.lib()
    if expect is not None:
        assert bool(L.lfamd_mul_mat_is_exact(t, m, k, n, spec.flags)) == expect
    assert L.lfamd_mul_mat_takes_staged(t, m, k, n, spec.flags) == (case_id(case) in I8_CASES), case_id(case)
    assert L.lfamd_mul_mat_takes_staged_scaled(t, m, k, n, spec.flags) == (case_id(case) in SCALED_CASES), case_id(case)
    vary(spec, base, oracle, axis, case_id(case))


# F16 / BF16 batches: the loader-wave body on the raw rows (float_lf) and, by a testing flag, the 128 x 128 body (float_wide);
# both stage the activations with prep_float_kernel, which reads whole vectors only where a row is aligned to them
FLOAT_BATCH = [(t, 256, 64, 1024, fl, True) for t in (T.F16, T.BF16) for fl in ((), ("plain",))] + [(T.F16, 100, 200, 512, (), True)]
FLOAT_AXES = AXES + ("b_stride_elem",)


@pytest.mark.parametrize("axis", FLOAT_AXES)
@pytest.mark.parametrize("case", FLOAT_BATCH, ids=case_id)
def test_float_batch_layout(gpu, oracle, case, axis):
    """Float weights take element-aligned rows (include/lfamd_hip.h), f32 or in the weight's own type: base + 4 / + 2 bytes and a
    stride of the row + 4 / + 2 bytes run the element-wise branch of prep_float_kernel and must give the bits of the vector loads."""
    t, m, n, k, fl, expect = case
    spec, base = _spec(("fb", case), lambda: MulMat(t, m, n, k, fl, seed=50 + t))
    L = _hip.lib()
    assert bool(L.lfamd_mul_mat_is_exact(t, m, k, n, spec.flags)) == expect
    assert L.lfamd_mul_mat_takes_staged(t, m, k, n, spec.flags) == 0 and L.lfamd_mul_mat_takes_staged_scaled(t, m, k, n, spec.flags) == 0
    vary(spec, base, oracle, axis, case_id(case))


# ---------------------------------------------------------------------------------------------------------------- decode GEMV
DECODE = [(t, m, k, n) for t in T.QUANT_WEIGHT_TYPES + (T.F16, T.BF16, T.F32) for m, k in ((48, 768), (8208, 1024), (33, 8192))
          for n in (1, 3, 8)]


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("t,m,k,n", DECODE, ids=[f"{T.NAMES[t]}-{m}x{n}x{k}" for t, m, k, n in DECODE])
def test_decode_gemv_layout(gpu, oracle, t, m, k, n, axis):
    """n = 1, 3, 8 on the three row depths / tile counts of test_gpu_decode_variants.py; every type, the float ones included."""
    spec, base = _spec(("gemv", t, m, k, n), lambda: MulMat(t, m, n, k, seed=300 + t))
    L = _hip.lib()
    assert L.lfamd_mul_mat_is_exact(t, m, k, n, spec.flags) == 1
    assert L.lfamd_mul_mat_takes_staged(t, m, k, n, spec.flags) == 0 and L.lfamd_mul_mat_takes_staged_scaled(t, m, k, n, spec.flags) == 0
    vary(spec, base, oracle, axis, (T.NAMES[t], m, k, n))


# --------------------------------------------------------------------------------------------------------- sibling matrices
TRIO = [(T.Q4_K, 512), (T.Q4_K, 256), (T.Q6_K, 128)]  # attn_q / attn_k / attn_v of a Q4_K_M file, unequal heights
MULTI = [(typed, n) for typed in (False, True) for n in (1, 4, 150)]


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("typed,n", MULTI, ids=[f"{'multi_types' if ty else 'multi'}-n{n}" for ty, n in MULTI])
def test_sibling_matrices_layout(gpu, oracle, typed, n, axis):
    """lfamd_mul_mat_multi on the two Q4_K matrices, lfamd_mul_mat_multi_types on the trio: the fused GEMVs (n = 1: the dual launch),
    the shared staging of the small-batch and the wide bodies."""
    spec, base = _spec(("multi", typed, n), lambda: Multi(TRIO if typed else TRIO[:2], n, 2048, typed))
    vary(spec, base, oracle, axis, ("multi_types" if typed else "multi", n))


# --------------------------------------------------------------------------------------------------------------- MUL_MAT_ID
MMID = [(t, tokens, tasks) for t in (T.Q4_K, T.Q6_K) for tokens in (3, 150) for tasks in (1, 2)] + [(T.Q4_0, 3, 1), (T.Q4_0, 3, 2)]


@pytest.mark.parametrize("axis", ID_AXES)
@pytest.mark.parametrize("t,tokens,tasks", MMID, ids=[f"{T.NAMES[t]}-{tok}tok-{ta}tasks" for t, tok, ta in MMID])
def test_mul_mat_id_layout(gpu, oracle, t, tokens, tasks, axis):
    """The decode launches that read the expert index themselves (3 tokens), the routed MFMA launch whose tables live in the
    workspace (150 tokens: cnt, poff, slot_row and src_row are all written by moe_route_kernel before anything reads them), and
    the gather / per-expert path of the other types (Q4_0); the `thought` rows are strided like B."""
    spec, base = _spec(("id", t, tokens, tasks), lambda: MulMatId(t, tokens, tasks))
    vary(spec, base, oracle, axis, (T.NAMES[t], "mul_mat_id", tokens, tasks))
