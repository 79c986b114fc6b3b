"""lfamd_flash_attn_q on the device (csrc/flash_attn.hip): GGML_OP_FLASH_ATTN_EXT on a Q8_0 / Q4_0 K and V cache, both routes, both pairs.

Every case is built as a -fa graph hands it over, and hostile: the cache memory is [token][KV head][D / 32 blocks + 2 gap bytes], so
successive rows alternate between a base = 0 and = 2 (mod 4); the byte 0x7e stands in every gap and in one whole token row behind n_kv
(a gap read as d is an f16 NaN); the K base sits 2 bytes past a 16-byte boundary.  Q, mask and dst are laid out as
tests/test_gpu_flash_attn.py: build does it.  Checked per case:
  (a) the per-row error against the f64 value on the operands as the route sees them (tests/fattn_q_ref.py): TOL_F32 on the f32
      d * code (n_q <= 8), TOL_MMA on f16(d * code) (n_q > 8);
  (b) bit equality with calls on one head each;
  (c) every byte outside the results unchanged, no NaN in the results (test_gpu_flash_attn.Loaded.full);
  (d) n_q > 8: bit equality with lfamd_flash_attn on an F16 cache holding f16(d * code) — the header's contract;
  (e) a row that sees one key is that key's V row, bit for bit: the f32 d * code (n_q <= 8), f16(d * code) widened (n_q > 8).
The cases of a list run inside one test per pair (run_cases), each printing its figures and failing under its own id."""
import numpy as np
import pytest

import fattn_q_ref as QR
import fattn_ref as R
import test_gpu_flash_attn as F
from batched_case import Dev, span, strided
from llamafile_amd import _hip, ggml_types as T

GAP = F.GAP
PAIRS = pytest.mark.parametrize("t", QR.TYPES, ids=QR.type_name)


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def cache_image(raw):
    """raw blocks uint8 [ne3][kv heads][n_kv][row] -> (the byte image, (nb3, nb2, nb1)): memory [token][kv head][row + 2 gap bytes],
    one more token row behind n_kv, GAP wherever no block lies."""
    ne3, kvh, n_kv, row = raw.shape
    nb = ((n_kv + 1) * kvh * (row + 2), row + 2, kvh * (row + 2))
    img = np.full(ne3 * nb[0], GAP, np.uint8)
    strided(img, np.uint8, raw.shape, nb + (1,))[...] = raw
    return img, nb


def call(dev, t, pq, q_nb, pk, pv, kv_nb, pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, scale, pd, d_nb, ws=None, expect=0, ws_bytes=None, stream=None):
    """One lfamd_flash_attn_q call on the pair (t, t); the workspace as in test_gpu_flash_attn.fa_call."""
    need = dev.lib.lfamd_flash_attn_workspace(D, n_q, n_kv, n_head, kvh, ne3)
    if need and ws is None:
        ws = dev.torch.empty(need, dtype=dev.torch.uint8, device="cuda")
    rc = dev.lib.lfamd_flash_attn_q(pq, q_nb[2], q_nb[1], q_nb[0], t, pk, kv_nb[2], kv_nb[1], kv_nb[0], t, pv, kv_nb[2], kv_nb[1], kv_nb[0],
                                    pm, m_nb1, D, n_q, n_kv, n_head, kvh, ne3, float(scale), 0.0, pd, d_nb[1], d_nb[2], d_nb[0],
                                    ws.data_ptr() if ws is not None else None, need if ws_bytes is None else ws_bytes, 0, stream)
    assert rc == expect, _hip.lib().lfamd_last_error()
    return ws


class Loaded(F.Loaded):
    """One case on the device.  f16_twin=False: the raw blocks in the hostile layout, calls through lfamd_flash_attn_q.
    f16_twin=True: an F16 cache holding f16(d * code) in test_gpu_flash_attn's layout, calls through lfamd_flash_attn.
    K / V (host): the operands as the case's route sees them."""

    def __init__(self, dev, case, mask_aligned, t, f16_twin=False):
        self.dev, self.case, self.t, self.twin = dev, case, t, f16_twin
        self.D, self.kvh, self.group, self.ne3, self.n_q, self.n_kv, _, _ = case
        self.Q, Kraw, Vraw, self.K, self.V, self.mask, self.scale = QR.inputs_of(case, t)
        self.n_head = self.kvh * self.group
        K16, V16 = self.K.astype(np.float16), self.V.astype(np.float16)
        q_img, self.q_nb, k_img, v_img, self.kv_nb, m_img, self.m_nb1, self.d_nb = F.build(self.Q, K16, V16, self.mask, mask_aligned)
        k_at = 0
        if not f16_twin:
            (k_img, self.kv_nb), (v_img, _), k_at = cache_image(Kraw), cache_image(Vraw), 2
        self.hq, self.hk, self.hv = dev.put(q_img.view(np.uint8), 0), dev.put(k_img, k_at), dev.put(v_img, 0)
        self.hm = dev.put(m_img, 0 if mask_aligned else 2) if m_img is not None else None
        self.pm = dev.ptr(self.hm) if self.hm else None

    def _call(self, *a, **kw):
        return F.fa_call(self.dev, *a, **kw) if self.twin else call(self.dev, self.t, *a, **kw)

    def call(self, pd, d_nb, ws=None, ws_bytes=None, n_kv=None, expect=0, stream=None):
        return self._call(self.dev.ptr(self.hq), self.q_nb, self.dev.ptr(self.hk), self.dev.ptr(self.hv), self.kv_nb, self.pm, self.m_nb1, self.D,
                          self.n_q, n_kv or self.n_kv, self.n_head, self.kvh, self.ne3, self.scale, pd, d_nb, ws, ws_bytes=ws_bytes, expect=expect,
                          stream=stream)

    def rows(self, i3, h, j0, n, n_head=1, ws=None):
        """As test_gpu_flash_attn.Loaded.rows: rows j0 .. j0 + n - 1 of head h (or of all heads) of slice i3 by a call of their own."""
        dev = self.dev
        kvh = 1 if n_head == 1 else self.kvh
        one = dev.put(np.full(n * n_head * self.D * 4, 0xff, np.uint8), 0)
        one_nb = (n * n_head * self.D * 4, self.D * 4, n_head * self.D * 4)
        pq = dev.ptr(self.hq) + i3 * self.q_nb[0] + h * self.q_nb[1] + j0 * self.q_nb[2]
        off = i3 * self.kv_nb[0] + (h // self.group) * self.kv_nb[1]
        pm = self.pm + j0 * self.m_nb1 if self.pm else None
        ws = self._call(pq, self.q_nb, dev.ptr(self.hk) + off, dev.ptr(self.hv) + off, self.kv_nb, pm, self.m_nb1, self.D, n, self.n_kv, n_head, kvh, 1,
                        self.scale, dev.ptr(one), one_nb, ws)
        return dev.get(one).view(np.uint32).reshape(n, n_head, self.D), ws


def assert_rows_are_their_one_key(ld, got):
    """test_gpu_flash_attn.assert_rows_are_their_one_key for block values: p = 1, l = 1, and a value times 1 added to the zeros of
    the accumulator is that value bit for bit — but for -0, which a negative d gives every code 0 (an F16 cache of random values
    holds none): -0 + 0 is +0, so the row is V[t] + 0."""
    keys = R.onehot_keys(ld.case[6], ld.n_q, ld.n_kv)
    want = ld.V.astype(np.float32)[:, :, keys].transpose(0, 2, 1, 3) + np.float32(0)  # [ne3][n_q][kv head][D]
    want = np.repeat(want, ld.group, axis=2)
    assert (ld.V == 0).any(), "the inputs have no zero code to make the remark above matter"
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32))


def run_case(dev, case, mask_aligned, t):
    D, kvh, group, ne3, n_q, n_kv, kind, _ = case
    ld = Loaded(dev, case, mask_aligned, t)
    got = ld.full()  # (c)
    route = R.route_of(n_q)
    ref, a = R.ref64(ld.Q, ld.K, ld.V, ld.mask, ld.scale, route)
    err = R.row_err(got.view(np.float32), ref, a)
    tol = R.TOL_F32 if route == "decode" else R.TOL_MMA
    print(QR.type_name(t), R.case_id(case), route, "err", err, "tol", tol)
    if route == "prefill":  # (d), before (a): where both miss, this one says more
        twin = Loaded(dev, case, mask_aligned, t, f16_twin=True).full()
        assert np.array_equal(got, twin), "not the bits of lfamd_flash_attn on an F16 cache holding f16(d * code)"
    assert err <= tol, (R.case_id(case), err)  # (a)
    ws = None
    for i3 in range(ne3):  # (b)
        for h in range(ld.n_head):
            single, ws = ld.rows(i3, h, 0, n_q, ws=ws)
            assert np.array_equal(single[:, 0], got[i3, :, h]), ("a row's bits depend on the call's other heads", i3, h)
    if kind in ("onehot", "diag"):  # (e)
        assert_rows_are_their_one_key(ld, got)
    return ld, got


def run_cases(dev, cases, t):
    """run_case on every (case, mask alignment) of a list in ONE test: the suite keeps one test id per list and pair, not one per
    case.  Every case runs whatever the others did; the failures are reported together, each under its case's id."""
    failed = []
    for case, aligned in cases:
        name = R.case_id(case) + ("" if case[6] is None else "-m16" if aligned else "-m2")
        try:
            run_case(dev, case, aligned, t)
        except AssertionError as e:
            failed.append((name, str(e)[:400]))
    assert not failed, failed


def alternating(cases):
    """The pairwise lists as tests/test_gpu_flash_attn.py runs them: the mask 16-byte aligned in every other case."""
    return [(c, i % 2 == 0) for i, c in enumerate(cases)]


def both_alignments(cases):
    """Every masked case with its mask 16-byte aligned and at the + 2 base; a case without a mask once."""
    return [(c, al) for c in cases for al in ((True, False) if c[6] is not None else (True,))]


@pytest.mark.gpu
@PAIRS
def test_decode_route(dev, t):
    run_cases(dev, alternating(R.decode_cases()), t)


@pytest.mark.gpu
@PAIRS
def test_decode_route_edges(dev, t):
    run_cases(dev, both_alignments(QR.decode_edge_cases()), t)


@pytest.mark.gpu
@PAIRS
def test_prefill_route(dev, t):
    run_cases(dev, alternating(R.prefill_cases()), t)


@pytest.mark.gpu
@PAIRS
def test_prefill_route_edges(dev, t):
    run_cases(dev, both_alignments(QR.prefill_edge_cases()), t)


@pytest.mark.gpu
@PAIRS
def test_decode_rows_do_not_depend_on_the_calls_other_rows(dev, t):
    """Every row again by an n_q = 1 call on its head, the Q and mask bases moved to the row: the same bits."""
    ld = Loaded(dev, (128, 2, 4, 1, 8, 3 * R.CHUNK + 7, "causal70", None), True, t)
    got = ld.full()
    ws = None
    for h in range(ld.n_head):
        for j in range(ld.n_q):
            single, ws = ld.rows(0, h, j, 1, ws=ws)
            assert np.array_equal(single[0, 0], got[0, j, h]), ("a row's bits depend on the call's other rows", h, j)


@pytest.mark.gpu
@PAIRS
def test_an_odd_k_base_is_invalid_and_leaves_dst_untouched(dev, t):
    for n_q in (2, 17):  # either route
        ld = Loaded(dev, (128, 2, 4, 1, n_q, 65, "causal", None), True, t)
        dsh, strides = (1, n_q, 8, 128), (ld.d_nb[0], ld.d_nb[2], ld.d_nb[1], 4)
        d_img = F.sentinel(span(dsh, strides, 4) // 4 + 16)
        hd = dev.put(d_img.view(np.uint8), 0)
        odd = (ld.hk[0], ld.hk[1] - 1, ld.hk[2])  # the buffer one byte earlier: an odd base, inside the allocation
        call(dev, t, dev.ptr(ld.hq), ld.q_nb, dev.ptr(odd), dev.ptr(ld.hv), ld.kv_nb, ld.pm, ld.m_nb1, 128, n_q, 65, 8, 2, 1, ld.scale, dev.ptr(hd),
             ld.d_nb, expect=-2)
        assert "a K / V base or stride is not a multiple of 2" in _hip.lib().lfamd_last_error().decode(), n_q
        assert np.array_equal(dev.get(hd).view(np.uint32), d_img), n_q


@pytest.mark.gpu
@PAIRS
def test_the_workspace_may_hold_anything_and_a_short_one_is_refused(dev, t):
    ld = Loaded(dev, (128, 2, 4, 1, 2, 3 * R.CHUNK + 7, "causal", None), True, t)
    want = ld.full()  # (a fresh workspace)
    need = dev.lib.lfamd_flash_attn_workspace(ld.D, ld.n_q, ld.n_kv, ld.n_head, ld.kvh, ld.ne3)
    assert need > 0
    ws = dev.torch.full((need + 64,), GAP, dtype=dev.torch.uint8, device="cuda")  # NaN everywhere, 64 bytes more than needed
    hd = dev.put(np.full(want.size * 4, 0xff, np.uint8), 0)
    d_nb = (ld.n_q * ld.n_head * ld.D * 4, ld.D * 4, ld.n_head * ld.D * 4)
    ld.call(dev.ptr(hd), d_nb, ws, ws_bytes=need + 64)
    assert np.array_equal(dev.get(hd).view(np.uint32).reshape(want.shape), want), "the result depends on what the workspace held"
    assert bool((ws[need:] == GAP).all()), "bytes behind the workspace's stated need were written"
    before = dev.get(hd).copy()
    ld.call(dev.ptr(hd), d_nb, ws, ws_bytes=need - 1, expect=-4)  # LFAMD_ERR_WORKSPACE
    assert np.array_equal(dev.get(hd), before)


def graph_case():
    """Body of test_a_call_on_a_stream_and_in_a_captured_graph; runs in a process of its own (see there)."""
    import torch
    from llamafile_amd import sgemm
    sgemm.init(0)
    lib = _hip.lib()
    D, kvh, group, n_q, n_kv, t = 128, 2, 4, 2, 3 * R.CHUNK + 7, T.Q8_0  # a split decode call: two launches and the workspace
    heads, row = kvh * group, QR.row_bytes(t, D)
    Q = torch.zeros((heads, n_q, D), device="cuda")
    K, V = (torch.zeros((kvh, n_kv, row), dtype=torch.uint8, device="cuda") for _ in range(2))
    M = torch.from_numpy(R.make_mask("causal", n_q, n_kv, None)).to(torch.float16).cuda()
    dst = torch.zeros((n_q, heads, D), device="cuda")
    need = lib.lfamd_flash_attn_workspace(D, n_q, n_kv, heads, kvh, 1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def issue(stream):
        rc = lib.lfamd_flash_attn_q(Q.data_ptr(), D * 4, n_q * D * 4, heads * n_q * D * 4, t, K.data_ptr(), row, n_kv * row, kvh * n_kv * row,
                                    t, V.data_ptr(), row, n_kv * row, kvh * n_kv * row, M.data_ptr(), n_kv * 2, D, n_q, n_kv, heads, kvh, 1,
                                    1.0 / np.sqrt(D), 0.0, dst.data_ptr(), D * 4, heads * D * 4, n_q * heads * D * 4, ws.data_ptr(), need, 0, stream)
        assert rc == 0, lib.lfamd_last_error()

    def rewrite(seed):
        q, k, v, _, _ = R.make_inputs(D, kvh, group, 1, n_q, n_kv, None, None, seed)
        Q.copy_(torch.from_numpy(q[0])), K.copy_(torch.from_numpy(QR.quantise(t, k)[0])), V.copy_(torch.from_numpy(QR.quantise(t, v)[0]))
        dst.zero_()
        torch.cuda.synchronize()

    def result():
        torch.cuda.synchronize()
        return dst.clone()

    def same(got, want, what):
        assert torch.isfinite(want).all() and want.abs().sum() > 0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what

    want = {}
    for seed in (1, 2):  # eager, NULL stream (also loads the kernels before the capture)
        rewrite(seed)
        issue(None)
        want[seed] = result()
    assert not torch.equal(want[1], want[2])
    side = torch.cuda.Stream()
    rewrite(2)
    issue(side.cuda_stream)
    side.synchronize()
    same(result(), want[2], "a non-default stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # the single call: a chain of two kernel nodes
        issue(torch.cuda.current_stream().cuda_stream)
    for seed in (1, 2):
        rewrite(seed)
        g.replay()
        same(result(), want[seed], ("replay", seed))
    print("graph case ok")


@pytest.mark.gpu
def test_a_call_on_a_stream_and_in_a_captured_graph(gpu):
    """One split decode call on a non-default stream, then captured with torch.cuda.graph as a graph of that single call and replayed
    twice with Q, K and V rewritten in place: the bits of the eager NULL-stream calls.  In a fresh child process, as
    tests/test_gpu_flash_attn.py does it."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_flash_attn_q as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
