"""The fused producers in front of every mat-mul of a layer (lfamd_rms_norm_quantize, lfamd_swiglu_quantize: csrc/norm_quant.hip,
six kernels) in all three output formats — Q8_K rows, the int8 body's image, the scaled f16 bodies' image — held to the CPU
reference of tests/producer_ref.py on adversarial inputs:

  f32 output    the norm bit for bit (no generated row is ambiguous: tests/test_producer_ref.py); SwiGLU inside the interval of
                the stated formula with expf within n_ulp units of the f64 exp, the smallest n_ulp printed and held to <= 2
  Q8_K rows     byte for byte oracle.quantize of the kernel's own f32 output
  both images   decoded from their documented layouts, field by field, against the same blocks / the power-of-two model;
                padding tokens all zero, guard bytes behind the image untouched; mismatches counted per field, zero asserted
  arguments     the same bytes whichever outputs are requested and with d_weight = NULL or ones; padded row strides on every
                operand with sentinels in the gaps; outputs that start 16 (f32, images) or 4 (Q8_K rows) bytes into their allocation
  consumers     the mat-mul on each image gives the bits of the same mat-mul on the producer's f32 output, which is within the
                bounds of tests/test_gpu_operand_extremes.py of the oracle
  a captured graph of norm -> image -> mat-mul, and the argument errors, every output keeping its sentinel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
import producer_ref as R
from extremes import extreme_activations
from test_gpu_operand_extremes import abs_products, check, oracle_sample, sample_rows, sample_tokens

pytestmark = pytest.mark.gpu

Q8K, STG, SCL = T.Q8_K, _hip.TYPE_STAGED_Q8K, _hip.TYPE_STAGED_SCALED
FMT = {Q8K: "q8k_rows", STG: "i8_image", SCL: "scaled_image"}
SENT = 0x5A
GUARD = 256

ROW_SHAPES = [(1, 256), (129, 256), (7, 768), (512, 768), (512, 4096), (1, 4096), (7, 4352), (129, 4352), (129, 11008), (7, 11008),
              (512, 14336), (1, 14336), (7, 16384), (129, 16384), (1, 16640), (512, 16640), (129, 28672), (7, 28672)]
IMAGE_SHAPES = [(1, 256), (300, 256), (127, 768), (128, 768), (512, 4096), (129, 4096), (300, 4352), (127, 4352), (128, 11008),
                (1, 11008), (512, 14336), (129, 14336), (127, 16384), (300, 16384), (128, 16640), (512, 16640), (129, 28672),
                (1, 28672)]
BENCH_SHAPES = ((512, 4096), (512, 14336))
CASES = [(Q8K, n, k) for n, k in ROW_SHAPES] + [(f, n, k) for f in (STG, SCL) for n, k in IMAGE_SHAPES]
NORM_CONFIGS = (("wide", 1e-5), ("none", 1e-6), ("ones", 1e-5), ("wide", 0.0))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sentinel(nbytes):
    return torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _rows_in(a, pad):
    """numpy f32 [n, k] -> a device buffer whose rows are k + pad floats apart, 1e30 in the gaps (a read of them shows)."""
    n, k = a.shape
    t = torch.full((n, k + pad), 1e30, dtype=torch.float32, device="cuda")
    t[:, :k] = torch.from_numpy(a)
    return t


def out_size(fmt, n, k):
    L = _hip.lib()
    return {Q8K: n * T.row_size(Q8K, k), STG: L.lfamd_staged_q8k_size(k, n), SCL: L.lfamd_staged_scaled_size(k, n)}[fmt]


class Outputs:
    """Sentinel-filled output buffers: f32 rows 16 bytes into their allocation and k + pf floats apart, Q8_K rows 4 bytes in and
    row_size + pq bytes apart, an image 16 bytes in; GUARD bytes behind each.  fetch() checks head, gaps and guard."""

    def __init__(self, fmt, n, k, q=True, f=True, strided=False):
        self.fmt, self.n, self.k = fmt, n, k
        self.pf, self.pq = (4, 4) if strided else (0, 0)
        self.rs = T.row_size(Q8K, k)
        self.qoff = 4 if fmt == Q8K else 16
        self.qbytes = n * (self.rs + self.pq) if fmt == Q8K else out_size(fmt, n, k)
        self.fbuf = _sentinel(16 + n * (k + self.pf) * 4 + GUARD) if f else None
        self.qbuf = _sentinel(self.qoff + self.qbytes + GUARD) if q else None

    def args(self):
        """(vec_dot_type, d_yq, yq_row_bytes, d_yf, yf_row_bytes)"""
        yq = _ptr(self.qbuf, self.qoff) if self.qbuf is not None else C.c_void_p(0)
        yf = _ptr(self.fbuf, 16) if self.fbuf is not None else C.c_void_p(0)
        return self.fmt, yq, (self.rs + self.pq if self.fmt == Q8K else 0), yf, (self.k + self.pf) * 4

    def fetch(self):
        """(f32 [n, k] or None, Q8_K rows uint8 [n, row_size] / image bytes or None)"""
        torch.cuda.synchronize()
        n, k = self.n, self.k
        yf = yq = None
        if self.fbuf is not None:
            a = self.fbuf.cpu().numpy()
            body = a[16:16 + n * (k + self.pf) * 4].reshape(n, (k + self.pf) * 4)
            assert (a[:16] == SENT).all() and (a[16 + body.size:] == SENT).all() and (body[:, k * 4:] == SENT).all(), "f32 rows: a gap or guard byte was written"
            yf = np.ascontiguousarray(body[:, :k * 4]).view(np.float32)
        if self.qbuf is not None:
            a = self.qbuf.cpu().numpy()
            assert (a[:self.qoff] == SENT).all() and (a[self.qoff + self.qbytes:] == SENT).all(), FMT[self.fmt] + ": a byte in front of or behind the output was written"
            body = a[self.qoff:self.qoff + self.qbytes]
            if self.fmt == Q8K:
                body = body.reshape(n, self.rs + self.pq)
                assert (body[:, self.rs:] == SENT).all(), "Q8_K rows: a gap byte was written"
                body = np.ascontiguousarray(body[:, :self.rs])
            yq = body
        return yf, yq


def produce(producer, ins, out, w=None, eps=1e-5, pad_in=0):
    """One producer call.  ins: (x,) for the norm, (gate, up) for SwiGLU, numpy f32 [n, k]; w: numpy [k] or None."""
    L = _hip.lib()
    n, k = ins[0].shape
    dev = [_rows_in(a, pad_in) for a in ins]
    rb = (k + pad_in) * 4
    vdt, yq, yqrb, yf, yfrb = out.args()
    if producer == "rms_norm":
        wd = torch.from_numpy(w).cuda() if w is not None else None
        rc = L.lfamd_rms_norm_quantize(_ptr(dev[0]), rb, _ptr(wd) if wd is not None else C.c_void_p(0), eps, n, k, vdt, yq, yqrb, yf, yfrb, _stream())
    else:
        rc = L.lfamd_swiglu_quantize(_ptr(dev[0]), rb, _ptr(dev[1]), rb, n, k, vdt, yq, yqrb, yf, yfrb, _stream())
    assert rc == 0, (rc, L.lfamd_last_error())
    torch.cuda.synchronize()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _count(field, got, want, counts):
    bad = int((_bits(got) != _bits(want)).sum())
    counts[field] = (bad, int(np.asarray(got).size))
    return bad


def check_quantised(fmt, yq, yf, n, k, oracle, what):
    """The quantised output against the kernel's own f32 output: Q8_K rows byte for byte; the images field by field."""
    want_q = oracle.quantize(Q8K, yf)
    counts = {}
    if fmt == Q8K:
        d, bs, codes = R.q8k_fields(yq, k)
        wd, wbs, wc = R.q8k_fields(want_q, k)
        _count("d", d, wd, counts), _count("bsums", bs, wbs, counts), _count("codes", codes, wc, counts)
        _count("bytes", yq, want_q, counts)
    else:
        npad, nb = R.n_pad_of(n), k // 256
        wd, wbs, wc = R.q8k_fields(want_q, k)
        if fmt == STG:
            codes, d, xs = R.i8_image_decode(yq, k, n)
            assert np.abs(wbs).max() <= 2048  # f16 holds every block sum exactly
            _count("codes", codes[:n], wc, counts), _count("d", d[:n], wd, counts)
            _count("bsums", np.ascontiguousarray(xs[:n]).astype(np.float16), wbs.astype(np.float16), counts)
            _count("padding codes", codes[n:], np.zeros((npad - n, nb, 256), np.int8), counts)
            _count("padding d", d[n:], np.zeros((npad - n, nb), np.float32), counts)
            _count("padding bsums", np.ascontiguousarray(xs[n:]), np.zeros((npad - n, nb, 16), np.float32), counts)
            whole = np.zeros((npad, nb, 256), np.int8), np.zeros((npad, nb), np.float32), np.zeros((npad, nb, 16), np.float32)
            whole[0][:n], whole[1][:n], whole[2][:n] = wc, wd, wbs
            _count("bytes", yq, R.i8_image_encode(*whole), counts)
        else:
            assert R.in_domain(yf), what
            xh, ts, xm = R.scaled_image_decode(yq, k, n)
            mh, mt, mm = R.scaled_image_model(yf, want_q)
            _count("Xh", xh[:n], mh, counts), _count("tok_scale", ts[:n], mt, counts), _count("Xm", xm[:n], mm, counts)
            _count("padding Xh", xh[n:], np.zeros((npad - n, nb, 256), np.float16), counts)
            _count("padding tok_scale", ts[n:], np.zeros(npad - n, np.float32), counts)
            _count("padding Xm", xm[n:], np.zeros((npad - n, nb, 16), np.float16), counts)
    print(what, FMT[fmt], "mismatches per field (of):", counts)
    assert all(b == 0 for b, _ in counts.values()), (what, counts)


def same_bytes(a, b, what):
    assert a is not None and b is not None
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


def _case_id(c):
    return f"{FMT[c[0]]}-{c[1]}x{c[2]}"


# ------------------------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_rms_norm_quantize(gpu, oracle, case):
    fmt, n, k = case
    kind, eps = ("none", 1e-5) if (n, k) in BENCH_SHAPES and fmt != Q8K else NORM_CONFIGS[CASES.index(case) % 4]
    x = R.norm_input(n, k, k + n, eps)
    w = R.norm_weight(kind, k, k)
    what = ("rms_norm", n, k, kind, eps)
    want, amb = R.rms_norm_ref(x, w, eps)
    assert not amb.any()
    # every operand strided, both outputs
    yf, yq = produce("rms_norm", (x,), Outputs(fmt, n, k, strided=True), w, eps, pad_in=64).fetch()
    bad = int((yf.view(np.uint32) != want.view(np.uint32)).sum())
    print(what, FMT[fmt], f"f32: {bad} of {yf.size} words differ from the reference")
    assert bad == 0
    check_quantised(fmt, yq, yf, n, k, oracle, what)
    # dense, and only one of the outputs (the second is the staged prefill pass's call when fmt is an image and kind is none)
    yf2, yq2 = produce("rms_norm", (x,), Outputs(fmt, n, k), w, eps).fetch()
    _, yq3 = produce("rms_norm", (x,), Outputs(fmt, n, k, f=False), w, eps).fetch()
    yf4, _ = produce("rms_norm", (x,), Outputs(fmt, n, k, q=False), w, eps).fetch()
    same_bytes(yf2, yf, "dense f32"), same_bytes(yf4, yf, "f32 alone")
    same_bytes(yq2, yq, "dense"), same_bytes(yq3, yq, "quantised alone")
    # d_weight = NULL is a weight of ones
    _, a = produce("rms_norm", (x,), Outputs(fmt, n, k, f=False), None, eps).fetch()
    fb, b = produce("rms_norm", (x,), Outputs(fmt, n, k), np.ones(k, np.float32), eps).fetch()
    same_bytes(a, b, "NULL weight vs ones")
    if kind != "wide":
        same_bytes(a, yq, "NULL weight vs ones"), same_bytes(fb, yf, "ones")


# --------------------------------------------------------------------------------------------------------------------- SwiGLU
N_ULP_LIMIT = 2  # what NumPy's own f32 exp needs against the f64 exp on these inputs (tests/test_producer_ref.py)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_swiglu_quantize(gpu, oracle, case):
    fmt, n, k = case
    g, u = R.swiglu_inputs(n, k, 3 * k + n)
    what = ("swiglu", n, k)
    yf, yq = produce("swiglu", (g, u), Outputs(fmt, n, k, strided=True), pad_in=64).fetch()
    assert np.isfinite(yf).all()
    n_ulp, outside = R.smallest_n_ulp(yf, g, u)
    print(what, FMT[fmt], f"f32: smallest n_ulp = {n_ulp}; outside the interval at 0, 1, ... ulp: {outside} of {yf.size}")
    assert n_ulp <= N_ULP_LIMIT
    check_quantised(fmt, yq, yf, n, k, oracle, what)
    yf2, yq2 = produce("swiglu", (g, u), Outputs(fmt, n, k)).fetch()
    _, yq3 = produce("swiglu", (g, u), Outputs(fmt, n, k, f=False)).fetch()
    yf4, _ = produce("swiglu", (g, u), Outputs(fmt, n, k, q=False)).fetch()
    same_bytes(yf2, yf, "dense f32"), same_bytes(yf4, yf, "f32 alone")
    same_bytes(yq2, yq, "dense"), same_bytes(yq3, yq, "quantised alone")


def test_swiglu_quantize_at_its_row_limit(gpu, oracle):
    """65,408 rows, the most lfamd_swiglu_quantize takes: one grid row per token of the padded image."""
    n, k = 65408, 256
    rng = np.random.default_rng(8)
    g = (rng.standard_normal((n, k)) * 3.0).astype(np.float32)
    u = (rng.random((n, k), dtype=np.float32) * 2 - 1) * rng.choice(np.float32([1e-3, 1.0, 1e3]), (n, 1))
    u[5::16] = 0.0
    for fmt in (Q8K, STG, SCL):
        yf, yq = produce("swiglu", (g, u), Outputs(fmt, n, k)).fetch()
        if fmt == Q8K:
            assert R.smallest_n_ulp(yf, g, u)[0] <= N_ULP_LIMIT
        check_quantised(fmt, yq, yf, n, k, oracle, ("swiglu", n, k))


# ------------------------------------------------------------------------------------------------- the ends of the domain
@pytest.mark.parametrize("scale", [1e27, 1e-27], ids=["1e27", "1e-27"])
@pytest.mark.parametrize("fmt", [Q8K, STG, SCL], ids=lambda f: FMT[f])
@pytest.mark.parametrize("producer", ["rms_norm", "swiglu"])
def test_near_the_ends_of_the_domain(gpu, oracle, producer, fmt, scale):
    """Outputs whose rows peak around 1e27 and around 1e-27, inside the stated domain (row and block maxima in [1e-30, 1e30]):
    -128 / max, d * 2^-e and the row's power of two are then far from 1 but finite."""
    n, k = 32, 768
    if producer == "rms_norm":
        ins, eps = (R.norm_input(n, k, 11, 0.0),), 0.0
        w = (np.float32(scale) * np.random.default_rng(12).uniform(0.5, 1.0, k) * np.where(np.arange(k) % 3 == 0, -1, 1)).astype(np.float32)
        want, amb = R.rms_norm_ref(ins[0], w, eps)
        assert not amb.any()
    else:
        u = extreme_activations(n, k, 13)
        top = np.abs(u).max(axis=1, keepdims=True)
        u = (u / np.where(top > 0, top, 1) * np.float32(scale)).astype(np.float32)
        ins, w, eps = ((np.random.default_rng(14).standard_normal((n, k)) * 3.0).astype(np.float32), u), None, 0.0
    yf, yq = produce(producer, ins, Outputs(fmt, n, k), w, eps).fetch()
    assert R.in_domain(yf)
    top = np.abs(yf).max(axis=1)
    assert (top[top > 0] > scale / 100).all() and (top < scale * 100).all()
    if producer == "rms_norm":
        assert np.array_equal(yf.view(np.uint32), want.view(np.uint32))
    else:
        assert R.smallest_n_ulp(yf, *ins)[0] <= N_ULP_LIMIT
    check_quantised(fmt, yq, yf, n, k, oracle, (producer, "scale", scale))


# -------------------------------------------------------------------------------------------------------------- the consumers
def _mul_mat(L, W, Btype, B, brb, n, flags, ws):
    out = torch.empty((n, W.rows), dtype=torch.float32, device="cuda")
    rc = L.lfamd_mul_mat(W.type, _ptr(W.data), W.rows, W.cols, Btype, B, brb, n, _ptr(out), W.rows, _ptr(ws), ws.numel(), flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    return out


def _multi_types(L, Ws, k, Btype, B, brb, n, flags, ws):
    cnt = len(Ws)
    outs = [torch.empty((n, w.rows), dtype=torch.float32, device="cuda") for w in Ws]
    A = (C.c_void_p * cnt)(*[w.data.data_ptr() for w in Ws])
    Cs = (C.c_void_p * cnt)(*[o.data_ptr() for o in outs])
    ms = (C.c_long * cnt)(*[w.rows for w in Ws])
    ts = (C.c_int * cnt)(*[w.type for w in Ws])
    rc = L.lfamd_mul_mat_multi_types(cnt, ts, A, ms, k, Btype, B, brb, n, Cs, ms, _ptr(ws), ws.numel(), flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    return outs


@pytest.mark.parametrize("k", [4096, 4352, 16384, 16640])  # either side of the mat-mul's own staging forms (k / 256 <= 16, <= 64, above)
@pytest.mark.parametrize("producer", ["rms_norm", "swiglu"])
def test_consumers_at_extremes(gpu, oracle, producer, k):
    """The mat-mul on each image gives the bits of the same mat-mul on the producer's f32 output (Q4_K on the int8 image; Q4_K on a
    grid that takes the scaled image, Q5_K, Q6_K, and one mixed-type call of three matrices on the scaled image), and that f32-path
    result is within the bounds of tests/test_gpu_operand_extremes.py of the oracle, token by token, the zero token exactly 0."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    n = 300
    if producer == "rms_norm":
        ins, w = (extreme_activations(n, k, k + 1),), R.norm_weight("wide", k, k + 2)
    else:
        g = (np.random.default_rng(k + 3).standard_normal((n, k)) * 3.0).astype(np.float32)
        ins, w = (g, extreme_activations(n, k, k + 4)), None
    images = {}
    for fmt in (STG, SCL):
        yf, img = produce(producer, ins, Outputs(fmt, n, k), w).fetch()
        images[fmt] = torch.from_numpy(img).cuda()  # (a fresh allocation: 16-byte aligned)
    assert R.in_domain(yf)
    yfd = torch.from_numpy(yf).cuda()
    Bq = oracle.quantize(Q8K, yf)
    cols = sample_tokens(n)
    singles = [(T.Q4_K, 4096, STG), (T.Q4_K, 1024, SCL), (T.Q5_K, 1024, SCL), (T.Q6_K, 1024, SCL)]
    Ws = {}
    for t, m, fmt in singles:
        takes = L.lfamd_mul_mat_takes_staged if fmt == STG else L.lfamd_mul_mat_takes_staged_scaled
        assert takes(t, m, k, n, flags) == 1, (T.NAMES[t], m, k, n, FMT[fmt])
        A = synth.random_weights(t, m, k, 50 + t)
        Wt = Ws[(t, m)] = gpu.upload_weights(t, A, m, k)
        ws = torch.empty(max(16, L.lfamd_mul_mat_workspace(t, m, k, n)), dtype=torch.uint8, device="cuda")
        got = _mul_mat(L, Wt, fmt, _ptr(images[fmt]), 0, n, flags, ws)
        want = _mul_mat(L, Wt, T.F32, _ptr(yfd), k * 4, n, flags, ws)
        torch.cuda.synchronize()
        diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
        print(producer, k, T.NAMES[t], m, FMT[fmt], f"{diff} of {got.numel()} words differ between the image and the f32 rows")
        assert diff == 0
        rows = sample_rows(m)
        G = oracle_sample(oracle, t, A, Bq, k, rows, cols)
        ap = abs_products(oracle, t, A, yf, k, rows, cols)
        exact = bool(L.lfamd_mul_mat_is_exact(t, m, k, n, flags))
        check(want.cpu().numpy()[np.ix_(cols, rows)], G, cols, rows, exact, (producer, T.NAMES[t], m, n, k), zero_row=False, absprod=ap, k=k)
    trio = [Ws[(T.Q4_K, 4096)], Ws[(T.Q4_K, 1024)], Ws[(T.Q6_K, 1024)]]
    ws = torch.empty(max(16, max(L.lfamd_mul_mat_workspace(w_.type, w_.rows, k, n) for w_ in trio)), dtype=torch.uint8, device="cuda")
    got = _multi_types(L, trio, k, SCL, _ptr(images[SCL]), 0, n, flags, ws)
    want = _multi_types(L, trio, k, T.F32, _ptr(yfd), k * 4, n, flags, ws)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- a captured graph
def graph_case():
    """Body of test_norm_image_mat_mul_in_a_captured_graph; runs in a process of its own."""
    from llamafile_amd import sgemm as gpu
    gpu.init(0)
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    n, k, m, eps = 512, 768, 2048, 1e-5
    assert L.lfamd_mul_mat_takes_staged(T.Q4_K, m, k, n, flags) == 1
    W = gpu.upload_weights(T.Q4_K, synth.random_weights(T.Q4_K, m, k, 5), m, k)
    wd = torch.from_numpy(R.norm_weight("wide", k, 6)).cuda()
    x = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    image = _sentinel(L.lfamd_staged_q8k_size(k, n))
    out = torch.zeros((n, m), dtype=torch.float32, device="cuda")
    none = C.c_void_p(0)

    def chain(img, o):
        st = _stream()
        assert L.lfamd_rms_norm_quantize(_ptr(x), k * 4, _ptr(wd), eps, n, k, STG, _ptr(img), 0, none, 0, st) == 0
        assert L.lfamd_mul_mat(T.Q4_K, _ptr(W.data), m, k, STG, _ptr(img), 0, n, _ptr(o), m, none, 0, flags, st) == 0

    x.copy_(torch.from_numpy(R.norm_input(n, k, 1, eps)))
    chain(image, out)  # (loads the kernels before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: two kernel nodes
        chain(image, out)
    for seed in (2, 3):
        x.copy_(torch.from_numpy(R.norm_input(n, k, seed, eps)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        img2, out2 = _sentinel(image.numel()), torch.zeros_like(out)
        chain(img2, out2)
        torch.cuda.synchronize()
        assert out.any() and torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(image, img2), seed
    print("graph case ok")


def test_norm_image_mat_mul_in_a_captured_graph(gpu):
    """norm -> int8 image -> lfamd_mul_mat captured once as a single chain and replayed twice with new input contents equals the
    uncaptured calls each time.  In a fresh child process, for the reason test_get_rows_in_a_captured_graph gives."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_producers as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_every_output_untouched(gpu):
    """LFAMD_ERR_INVALID with every output still holding its sentinel; nrows = 0 is LFAMD_OK with nothing written.  (Null input
    pointers are refused too: tests/test_producer_ref.py, on a machine without a device.)"""
    L = _hip.lib()
    n, k = 4, 512
    st = _stream()
    x = torch.ones((n, k + 4), dtype=torch.float32, device="cuda")
    w = torch.ones(k + 4, dtype=torch.float32, device="cuda")
    rs = T.row_size(Q8K, k)
    yf = _sentinel(n * k * 4 + 64)
    yq = _sentinel(max(n * rs, L.lfamd_staged_q8k_size(k, n), L.lfamd_staged_scaled_size(k, n)) + 64)
    base = dict(x=(x, 0), xrb=(k + 4) * 4, w=(w, 0), g=(x, 0), grb=(k + 4) * 4, n=n, k=k, vdt=Q8K, yq=(yq, 0), yqrb=rs, yf=(yf, 0), yfrb=k * 4)

    def p(v):
        return C.c_void_p(0) if v is None else _ptr(*v)

    def norm(**kw):
        a = {**base, **kw}
        return L.lfamd_rms_norm_quantize(p(a["x"]), a["xrb"], p(a["w"]), 1e-5, a["n"], a["k"], a["vdt"], p(a["yq"]), a["yqrb"], p(a["yf"]), a["yfrb"], st)

    def swiglu(**kw):
        a = {**base, **kw}
        return L.lfamd_swiglu_quantize(p(a["g"]), a["grb"], p(a["x"]), a["xrb"], a["n"], a["k"], a["vdt"], p(a["yq"]), a["yqrb"], p(a["yf"]), a["yfrb"], st)

    common = [dict(k=500), dict(k=0), dict(n=-1), dict(x=(x, 4)), dict(yf=(yf, 4)), dict(xrb=(k + 1) * 4), dict(yfrb=(k + 1) * 4),
              dict(yq=(yq, 2)), dict(yqrb=rs + 2), dict(vdt=STG, yq=(yq, 4)), dict(vdt=SCL, yq=(yq, 8)), dict(vdt=T.Q8_0), dict(vdt=T.Q8_1),
              dict(vdt=T.F32), dict(yq=None, yf=None)]
    for kw in common + [dict(w=(w, 4))]:
        assert norm(**kw) == -2, ("rms_norm", kw)
    for kw in common + [dict(g=(x, 4)), dict(grb=(k + 2) * 4), dict(n=65409)]:
        assert swiglu(**kw) == -2, ("swiglu", kw)
    for vdt in (Q8K, STG, SCL):
        assert norm(n=0, vdt=vdt) == 0 and swiglu(n=0, vdt=vdt) == 0
    torch.cuda.synchronize()
    assert bool((yf == SENT).all()) and bool((yq == SENT).all())
    # and the calls are served once the arguments are right
    assert norm() == 0 and swiglu(vdt=STG, yqrb=0) == 0
    torch.cuda.synchronize()
    assert not bool((yf[:n * k * 4] == SENT).all()) and bool((yf[n * k * 4:] == SENT).all())
