"""lfamd_flash_attn on the device (csrc/flash_attn.hip): GGML_OP_FLASH_ATTN_EXT on an F16 K / V cache, both routes.

Every case is built as a -fa graph hands it over: K and V as permuted cache views (memory [token][KV head][D + 8 halves], so
nb1 = n_head_kv * (2 D + 16) and nb2 = 2 D + 16) with the byte 0x7e — a NaN f16 — in every gap and in one whole row behind n_kv; Q with
NaN behind every row; the mask with a row stride beyond 2 n_kv, NaN in the gap and in three rows past n_q; dst pre-filled with a
sentinel.  Checked per case:
  (a) the per-row error of tests/fattn_ref.py against the f64 value on the operands as the route sees them: TOL_F32 (n_q <= 8),
      TOL_MMA (n_q > 8);
  (b) bit equality with calls on one head each;
  (c) every byte outside the D * n_head * n_q * ne3 results unchanged;
  (d) no NaN in the results (a padding lane that read memory, or exp(-inf - -inf), would put one there).
The f64 reference of each case is computed once per case; shapes are fattn_ref's pairwise subsets, then its edge cases: the column
counts, chunk counts, dead chunks, dead tiles and 128-tile segments the pairwise shapes never execute (a row that sees one key must
be that row of V bit for bit).  Last, the header's other claims: a row's bits do not depend on the call's other rows, the call runs
on the stream it is given and in a captured graph, and the workspace may hold anything and is written up to its stated need only."""
import numpy as np
import pytest

import fattn_ref as R
from batched_case import NAN32, Dev, span, strided
from llamafile_amd import _hip, ggml_types as T

GAP = 0x7e


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def fill_image(nbytes, view_shape, strides, values, dtype):
    img = np.full(nbytes, GAP, np.uint8)
    strided(img, dtype, view_shape, strides)[...] = values
    return img


def build(Q, K, V, mask, mask_aligned):
    """The byte images and strides (nb3, nb2, nb1) of one case."""
    ne3, n_head, n_q, D = Q.shape
    kvh, n_kv = K.shape[1], K.shape[2]
    q_nb = (n_head * n_q * (4 * D + 16), n_q * (4 * D + 16), 4 * D + 16)
    q_img = np.full(span(Q.shape, q_nb + (4,), 4) // 4 + 4, NAN32, np.uint32)
    strided(q_img, np.uint32, Q.shape, q_nb + (4,))[...] = Q.view(np.uint32)
    row = 2 * D + 16
    kv_nb = ((n_kv + 1) * kvh * row, row, kvh * row)  # one more token row behind n_kv, all NaN
    kv_bytes = ne3 * kv_nb[0]
    k_img = fill_image(kv_bytes, K.shape, kv_nb + (2,), K.view(np.uint16), np.uint16)
    v_img = fill_image(kv_bytes, V.shape, kv_nb + (2,), V.view(np.uint16), np.uint16)
    m_img, m_nb1 = None, 0
    if mask is not None:
        m_nb1 = (2 * n_kv + 2 + 15) // 16 * 16 if mask_aligned else 2 * (n_kv + 3)
        m_img = fill_image((n_q + 3) * m_nb1, mask.shape, (m_nb1, 2), mask.astype(np.float16).view(np.uint16), np.uint16)
    d_nb = (n_q * n_head * (4 * D + 16), 4 * D + 16, n_head * (4 * D + 16))  # (nb3, nb1, nb2): element (i3, j, h, l)
    return q_img, q_nb, k_img, v_img, kv_nb, m_img, m_nb1, d_nb


def sentinel(words):
    return (np.arange(words, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32) | np.uint32(0x7f800001)


def fa_call(dev, pq, q_nb, pk, pv, kv_nb, pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, scale, pd, d_nb, ws=None, expect=0, ws_bytes=None,
            stream=None):
    """One call.  ws: a device tensor to use as the workspace (a fresh one where the call needs one and none is given); ws_bytes: the
    length the call is told of (lfamd_flash_attn_workspace() by default)."""
    need = dev.lib.lfamd_flash_attn_workspace(D, n_q, n_kv, n_head, kvh, ne3)
    if need and ws is None:
        ws = dev.torch.empty(need, dtype=dev.torch.uint8, device="cuda")
    rc = dev.lib.lfamd_flash_attn(pq, q_nb[2], q_nb[1], q_nb[0], T.F16, pk, kv_nb[2], kv_nb[1], kv_nb[0], T.F16, pv, kv_nb[2], kv_nb[1], kv_nb[0],
                                  pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, float(scale), 0.0, pd, d_nb[1], d_nb[2], d_nb[0],
                                  ws.data_ptr() if ws is not None else None, need if ws_bytes is None else ws_bytes, 0, stream)
    assert rc == expect, _hip.lib().lfamd_last_error()
    return ws


class Loaded:
    """One case on the device, laid out as build() says, and its result by one call on all heads."""

    def __init__(self, dev, case, mask_aligned, scale=None):
        self.dev, self.case = dev, case
        self.D, self.kvh, self.group, self.ne3, self.n_q, self.n_kv, _, _ = case
        self.Q, self.K, self.V, self.mask, self.scale = R.inputs_of(case, scale=scale)
        self.n_head = self.kvh * self.group
        q_img, self.q_nb, k_img, v_img, self.kv_nb, m_img, self.m_nb1, self.d_nb = build(self.Q, self.K, self.V, self.mask, mask_aligned)
        self.hq, self.hk, self.hv = dev.put(q_img.view(np.uint8), 0), dev.put(k_img, 0), dev.put(v_img, 0)
        self.hm = dev.put(m_img, 0 if mask_aligned else 2) if m_img is not None else None
        self.pm = dev.ptr(self.hm) if self.hm else None

    def call(self, pd, d_nb, ws=None, ws_bytes=None, n_kv=None):
        """All heads and rows into dst at pd."""
        return fa_call(self.dev, self.dev.ptr(self.hq), self.q_nb, self.dev.ptr(self.hk), self.dev.ptr(self.hv), self.kv_nb, self.pm, self.m_nb1,
                       self.D, self.n_q, n_kv or self.n_kv, self.n_head, self.kvh, self.ne3, self.scale, pd, d_nb, ws, ws_bytes=ws_bytes)

    def rows(self, i3, h, j0, n, n_head=1, ws=None):
        """Rows j0 .. j0 + n - 1 of head h (of heads h .. h + n_head - 1: n_head == self.n_head, h == 0) of slice i3 by a call of
        their own: the Q and mask bases moved to row j0, K and V as they are.  Returns (the bits [n][n_head][D], the workspace)."""
        dev = self.dev
        kvh = 1 if n_head == 1 else self.kvh
        one = dev.put(np.full(n * n_head * self.D * 4, 0xff, np.uint8), 0)
        one_nb = (n * n_head * self.D * 4, self.D * 4, n_head * self.D * 4)  # (nb3, nb1, nb2)
        pq = dev.ptr(self.hq) + i3 * self.q_nb[0] + h * self.q_nb[1] + j0 * self.q_nb[2]
        off = i3 * self.kv_nb[0] + (h // self.group) * self.kv_nb[1]
        pm = self.pm + j0 * self.m_nb1 if self.pm else None
        ws = fa_call(dev, pq, self.q_nb, dev.ptr(self.hk) + off, dev.ptr(self.hv) + off, self.kv_nb, pm, self.m_nb1, self.D, n, self.n_kv, n_head,
                     kvh, 1, self.scale, dev.ptr(one), one_nb, ws)
        return dev.get(one).view(np.uint32).reshape(n, n_head, self.D), ws

    def full(self):
        """The bits [ne3][n_q][n_head][D] of the call on all heads into a sentinel dst; (c) and (d) of the module's docstring."""
        dev = self.dev
        dsh, dst_strides = (self.ne3, self.n_q, self.n_head, self.D), (self.d_nb[0], self.d_nb[2], self.d_nb[1], 4)
        d_img = sentinel(span(dsh, dst_strides, 4) // 4 + 16)
        hd = dev.put(d_img.view(np.uint8), 0)
        self.call(dev.ptr(hd), self.d_nb)
        out = dev.get(hd).view(np.uint32).copy()
        got = strided(out, np.uint32, dsh, dst_strides).copy()
        strided(out, np.uint32, dsh, dst_strides)[...] = strided(d_img, np.uint32, dsh, dst_strides)
        assert np.array_equal(out, d_img), "bytes outside the results were written"
        assert not np.isnan(got.view(np.float32)).any(), "NaN in the results"
        return got


def run_case(dev, case, mask_aligned, scale=None):
    D, kvh, group, ne3, n_q, n_kv, _, _ = case
    ld = Loaded(dev, case, mask_aligned, scale)
    got = ld.full()  # (c), (d)
    res = got.view(np.float32)
    # (a)
    route = R.route_of(n_q)
    ref, a = R.ref64(ld.Q, ld.K, ld.V, ld.mask, ld.scale, route)
    err = R.row_err(res, ref, a)
    tol = R.TOL_F32 if route == "decode" else R.TOL_MMA
    print(R.case_id(case), route, "err", err, "tol", tol)
    assert err <= tol, (R.case_id(case), err)
    # (b) the same rows by calls on one head each: the same bits
    ws = None
    for i3 in range(ne3):
        for h in range(ld.n_head):
            single, ws = ld.rows(i3, h, 0, n_q, ws=ws)
            assert np.array_equal(single[:, 0], got[i3, :, h]), ("a row's bits depend on the call's other heads", i3, h)
    return ld, got


@pytest.mark.gpu
@pytest.mark.parametrize("i,case", list(enumerate(R.decode_cases())), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else None)
def test_decode_route(dev, i, case):
    run_case(dev, case, mask_aligned=i % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("i,case", list(enumerate(R.prefill_cases())), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else None)
def test_prefill_route(dev, i, case):
    run_case(dev, case, mask_aligned=i % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", [2, 17])
def test_a_misaligned_k_base_is_invalid_and_leaves_dst_untouched(dev, n_q):
    case = (128, 2, 4, 1, n_q, 65, "causal", None)
    Q, K, V, mask, scale = R.inputs_of(case)
    q_img, q_nb, k_img, v_img, kv_nb, m_img, m_nb1, d_nb = build(Q, K, V, mask, True)
    d_img = sentinel(span((1, n_q, 8, 128), (d_nb[0], d_nb[2], d_nb[1], 4), 4) // 4 + 16)
    hq, hk, hv, hd, hm = dev.put(q_img.view(np.uint8), 0), dev.put(k_img, 8), dev.put(v_img, 0), dev.put(d_img.view(np.uint8), 0), dev.put(m_img, 0)
    fa_call(dev, dev.ptr(hq), q_nb, dev.ptr(hk), dev.ptr(hv), kv_nb, dev.ptr(hm), m_nb1, 128, n_q, 65, 8, 2, 1, scale, dev.ptr(hd), d_nb, expect=-2)
    assert np.array_equal(dev.get(hd).view(np.uint32), d_img)


# ---- the edges: column counts, chunk counts, dead chunks, tiles and segments (fattn_ref.decode_edge_cases / prefill_edge_cases)
def both_alignments(cases):
    """Every case with its mask 16-byte aligned and at the + 2 base with the stride 2 (n_kv + 3); a case without a mask once."""
    return [pytest.param(c, al, id=R.case_id(c) + ("" if c[6] is None else "-m16" if al else "-m2")) for c in cases
            for al in ((True, False) if c[6] is not None else (True,))]


def assert_rows_are_their_one_key(ld, got):
    """A row that sees one key t: p = 1, l = 1, and an f16 V value times 1 added to zeros in f32 is that value: dst is V[t], bit for
    bit, whichever lane group, wave, chunk, half or tile the key falls into."""
    keys = R.onehot_keys(ld.case[6], ld.n_q, ld.n_kv)
    want = ld.V.astype(np.float32)[:, :, keys].transpose(0, 2, 1, 3)  # [ne3][n_q][kv head][D]
    want = np.repeat(want, ld.group, axis=2)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case,aligned", both_alignments(R.decode_edge_cases()))
def test_decode_route_edges(dev, case, aligned):
    ld, got = run_case(dev, case, aligned)
    if case[6] == "onehot":
        assert_rows_are_their_one_key(ld, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case,aligned", both_alignments(R.prefill_edge_cases()))
def test_prefill_route_edges(dev, case, aligned):
    ld, got = run_case(dev, case, aligned)
    if case[6] in ("onehot", "diag"):
        assert_rows_are_their_one_key(ld, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case,scale", R.scale_cases(), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else f"scale{v}")
def test_a_zero_and_a_negative_scale(dev, case, scale):
    ld, got = run_case(dev, case, True, scale)
    if scale == 0.0:  # every key weighs the same: the plain mean of V
        Vx = np.repeat(ld.V.astype(np.float64), ld.group, axis=1)
        mean = np.broadcast_to(Vx.mean(axis=2)[:, None], got.shape)
        a = np.broadcast_to(np.abs(Vx).mean(axis=2)[:, None], got.shape)
        err = R.row_err(got.view(np.float32), mean, a)
        print("against the mean of V", err)
        assert err <= (R.TOL_F32 if R.route_of(ld.n_q) == "decode" else R.TOL_MMA)


# ---- the header's other claims
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["m16", "m2"])
@pytest.mark.parametrize("case", [(128, 2, 4, 1, 8, 3 * R.CHUNK + 7, "causal70", None), (64, 1, 3, 1, 2, R.CHUNK + 1, "causal", None)], ids=R.case_id)
def test_decode_rows_do_not_depend_on_the_calls_other_rows(dev, case, aligned):
    """'The bits of a result row are a function of that row's own operands, D and n_kv alone': every row again by an n_q = 1 call on
    its head, the Q and mask bases moved to the row."""
    ld = Loaded(dev, case, aligned)
    got = ld.full()
    ws = None
    for h in range(ld.n_head):
        for j in range(ld.n_q):
            single, ws = ld.rows(0, h, j, 1, ws=ws)
            assert np.array_equal(single[0, 0], got[0, j, h]), ("a row's bits depend on the call's other rows", h, j)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["m16", "m2"])
@pytest.mark.parametrize("case", [(128, 1, 1, 1, 130, 1000, "window:40", None), (64, 2, 4, 1, 300, 300, "window:40", None)], ids=R.case_id)
def test_prefill_rows_do_not_depend_on_the_calls_other_rows(dev, case, aligned):
    """Rows 100 .. 112 and 119 .. 127 again by calls on those rows alone (n_q = 13 and 9, all heads).  There the rows sit in wave 0
    of a work-group that holds nothing else, so which tiles the work-group loads and which halves the wave computes differ from the
    large call: the bits must not."""
    ld = Loaded(dev, case, aligned)
    got = ld.full()
    for j0, n in ((100, 13), (119, 9)):
        part, _ = ld.rows(0, 0, j0, n, n_head=ld.n_head)
        assert np.array_equal(part, got[0, j0:j0 + n]), ("a row's bits depend on the call's other rows", j0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(128, 2, 4, 1, 2, 3 * R.CHUNK + 7, "causal", None), (64, 1, 1, 1, 8, 3 * R.CHUNK + 7, "bias", None)], ids=R.case_id)
def test_the_workspace_may_hold_anything_and_is_written_up_to_its_stated_need_only(dev, case):
    ld = Loaded(dev, case, True)
    want = ld.full()  # (a fresh workspace)
    need = dev.lib.lfamd_flash_attn_workspace(ld.D, ld.n_q, ld.n_kv, ld.n_head, ld.kvh, ld.ne3)
    assert need > 0
    ws = dev.torch.full((need + 64,), GAP, dtype=dev.torch.uint8, device="cuda")  # NaN everywhere, 64 bytes more than needed
    hd = dev.put(np.full(want.size * 4, 0xff, np.uint8), 0)
    d_nb = (ld.n_q * ld.n_head * ld.D * 4, ld.D * 4, ld.n_head * ld.D * 4)
    ld.call(dev.ptr(hd), d_nb, ws, ws_bytes=need + 64)
    assert np.array_equal(dev.get(hd).view(np.uint32).reshape(want.shape), want), "the result depends on what the workspace held"
    assert bool((ws[need:] == GAP).all()), "bytes behind the workspace's stated need were written"
    # the buffer as a call at another n_kv leaves it: stale finite values
    ld.call(dev.ptr(hd), d_nb, ws, ws_bytes=need + 64, n_kv=2 * R.CHUNK + 3)
    ld.call(dev.ptr(hd), d_nb, ws, ws_bytes=need + 64)
    assert np.array_equal(dev.get(hd).view(np.uint32).reshape(want.shape), want), "the result depends on the previous call's partials"
    assert bool((ws[need:] == GAP).all())


def graph_case():
    """Body of test_calls_on_a_stream_and_in_a_captured_graph; runs in a process of its own (see there)."""
    import torch
    from llamafile_amd import sgemm
    sgemm.init(0)
    lib = _hip.lib()
    shapes = [(128, 2, 4, 2, 3 * R.CHUNK + 7), (64, 2, 4, 33, 257)]  # a split decode call (with a workspace), a prefill call
    jobs = []
    for D, kvh, group, n_q, n_kv in shapes:
        heads = kvh * group
        Q = torch.zeros((heads, n_q, D), device="cuda")
        K, V = (torch.zeros((kvh, n_kv, D), dtype=torch.float16, device="cuda") for _ in range(2))
        M = torch.from_numpy(R.make_mask("causal", n_q, n_kv, None)).to(torch.float16).cuda()
        dst = torch.zeros((n_q, heads, D), device="cuda")
        need = lib.lfamd_flash_attn_workspace(D, n_q, n_kv, heads, kvh, 1)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        jobs.append((D, kvh, group, n_q, n_kv, Q, K, V, M, dst, ws, need))
    assert jobs[0][-1] > 0 and jobs[1][-1] == 0

    def issue(stream):
        for D, kvh, group, n_q, n_kv, Q, K, V, M, dst, ws, need in jobs:
            heads = kvh * group
            rc = lib.lfamd_flash_attn(Q.data_ptr(), D * 4, n_q * D * 4, heads * n_q * D * 4, T.F16, K.data_ptr(), D * 2, n_kv * D * 2, kvh * n_kv * D * 2,
                                      T.F16, V.data_ptr(), D * 2, n_kv * D * 2, kvh * n_kv * D * 2, M.data_ptr(), n_kv * 2, D, n_q, n_kv, heads, kvh, 1,
                                      1.0 / np.sqrt(D), 0.0, dst.data_ptr(), D * 4, heads * D * 4, n_q * heads * D * 4,
                                      ws.data_ptr() if need else None, need, 0, stream)
            assert rc == 0, lib.lfamd_last_error()

    def rewrite(seed):
        for D, kvh, group, n_q, n_kv, Q, K, V, M, dst, ws, need in jobs:
            q, k, v, _, _ = R.make_inputs(D, kvh, group, 1, n_q, n_kv, None, None, seed)
            Q.copy_(torch.from_numpy(q[0])), K.copy_(torch.from_numpy(k[0])), V.copy_(torch.from_numpy(v[0]))
            dst.zero_()
        torch.cuda.synchronize()

    def results():
        torch.cuda.synchronize()
        return [j[9].clone() for j in jobs]

    def same(got, want, what):
        for g, w in zip(got, want):
            assert torch.isfinite(w).all() and w.abs().sum() > 0
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), what

    want = {}
    for seed in (1, 2):  # eager, NULL stream (also loads the kernels before the capture)
        rewrite(seed)
        issue(None)
        want[seed] = results()
    side = torch.cuda.Stream()
    rewrite(2)
    issue(side.cuda_stream)
    side.synchronize()
    same(results(), want[2], "a non-default stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: three kernel nodes
        issue(torch.cuda.current_stream().cuda_stream)
    for seed in (1, 2):
        rewrite(seed)
        g.replay()
        same(results(), want[seed], ("replay", seed))
    print("graph case ok")


@pytest.mark.gpu
def test_calls_on_a_stream_and_in_a_captured_graph(gpu):
    """'Asynchronous on `stream`, graph-capturable': a split decode call (two launches and the workspace) and a prefill call on a
    non-default stream, then captured with torch.cuda.graph on the capture stream as one chain and replayed twice with Q, K and V
    rewritten in place, give the bits of the eager NULL-stream calls.  The capture runs in a fresh child process, as the other
    capture tests of this suite do (tests/test_gpu_get_rows.py says why)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_flash_attn as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
