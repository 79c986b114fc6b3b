"""The fused producers for the 32-block activation formats (lfamd_rms_norm_quantize_b32, lfamd_swiglu_quantize_b32:
csrc/norm_quant.hip) in their three output formats — Q8_0 rows, Q8_1 rows, the LFAMD_TYPE_STAGED_B32 image — and the mat-muls
behind them:

  f32 output    as tests/test_gpu_producers.py holds the Q8_K producers': the norm bit for bit against producer_ref.rms_norm_ref
                (a row may differ only where the reference calls it ambiguous), SwiGLU inside the interval of the stated formula
                at expf within N_ULP_LIMIT units
  rows          byte for byte oracle.quantize of the kernel's own f32 output, for rows of one block up to 43 chunks, whole and
                partial last chunks; sentinels in front of, between and behind the rows
  the image     decoded from its documented layout, field by field (Xh, d8T, sT, their paddings), mismatches counted, zero asserted
  rounding      rows whose y is exact and whose every code is a tie: roundf's 1, -2, 3, not nearest-even's 0, -2, 2
  consumers     decode GEMVs on the producer's strided rows give the bits they give on lfamd_quantize_rows' rows, within the bound of
                tests/test_gpu_operand_extremes.py of the oracle; batches on the image give the bits of the same call on the f32
                rows and leave the workspace alone
  a captured graph of norm -> image -> mat-mul, and the argument errors, every output keeping its sentinel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
import iq4nl_ref as NL
import producer32_ref as R32
import producer_ref as R
from extremes import extreme_activations, for_vec_dot
from test_gpu_operand_extremes import abs_products, check, oracle_sample
from test_gpu_producers import GUARD, N_ULP_LIMIT, NORM_CONFIGS, SENT, _bits, _count, _ptr, _rows_in, _sentinel, _stream, same_bytes

pytestmark = pytest.mark.gpu

Q80, Q81, B32 = T.Q8_0, T.Q8_1, _hip.TYPE_STAGED_B32
FMT = {Q80: "q8_0_rows", Q81: "q8_1_rows", B32: "b32_image"}
QOFF = {Q80: 2, Q81: 4, B32: 16}  # how far into its allocation the quantised output starts: the format's own alignment and no more

# one block; less than a chunk; a chunk and a partial one; four chunks and a partial one (every wave of the norm's work-group has
# one); more than 16 chunks, whole and partial
ROW_SHAPES = [(1, 32), (7, 96), (129, 288), (7, 1056), (1, 4096), (129, 4352), (7, 11008)]
IMAGE_SHAPES = [(1, 256), (127, 768), (128, 768), (129, 4352), (300, 256)]
STRIDED = {(7, 1056), (127, 768)}  # the shape of each format whose operands are all strided and offset
CASES = [(f, n, k) for f in (Q80, Q81) for n, k in ROW_SHAPES] + [(B32, n, k) for n, k in IMAGE_SHAPES]


def out_size(fmt, n, k):
    return _hip.lib().lfamd_staged_b32_size(k, n) if fmt == B32 else n * T.row_size(fmt, k)


class Outputs:
    """Sentinel-filled output buffers, in the manner of test_gpu_producers.Outputs: f32 rows 16 bytes into their allocation and
    k + pf floats apart; Q8_0 rows 2 bytes in with a 2-byte gap, Q8_1 rows 4 bytes in with a 4-byte gap (strided), an image 16 bytes
    in; GUARD bytes behind each.  fetch() checks head, gaps and guard."""

    def __init__(self, fmt, n, k, q=True, f=True, strided=False):
        self.fmt, self.n, self.k = fmt, n, k
        self.pf = 4 if strided else 0
        self.pq = QOFF[fmt] if strided and fmt != B32 else 0
        self.rs = T.row_size(fmt, k) if fmt != B32 else 0
        self.qoff = QOFF[fmt]
        self.qbytes = n * (self.rs + self.pq) if fmt != B32 else out_size(fmt, n, k)
        self.fbuf = _sentinel(16 + n * (k + self.pf) * 4 + GUARD) if f else None
        self.qbuf = _sentinel(self.qoff + self.qbytes + GUARD) if q else None

    def args(self):
        """(vec_dot_type, d_yq, yq_row_bytes, d_yf, yf_row_bytes)"""
        yq = _ptr(self.qbuf, self.qoff) if self.qbuf is not None else C.c_void_p(0)
        yf = _ptr(self.fbuf, 16) if self.fbuf is not None else C.c_void_p(0)
        return self.fmt, yq, self.rs + self.pq, yf, (self.k + self.pf) * 4

    def fetch(self):
        """(f32 [n, k] or None, rows uint8 [n, row_size] / image bytes or None)"""
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
            if self.fmt != B32:
                body = body.reshape(n, self.rs + self.pq)
                assert (body[:, self.rs:] == SENT).all(), FMT[self.fmt] + ": a gap byte was written"
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
        rc = L.lfamd_rms_norm_quantize_b32(_ptr(dev[0]), rb, _ptr(wd) if wd is not None else C.c_void_p(0), eps, n, k, vdt, yq, yqrb, yf, yfrb, _stream())
    else:
        rc = L.lfamd_swiglu_quantize_b32(_ptr(dev[0]), rb, _ptr(dev[1]), rb, n, k, vdt, yq, yqrb, yf, yfrb, _stream())
    assert rc == 0, (rc, L.lfamd_last_error())
    torch.cuda.synchronize()
    return out


def check_quantised(fmt, yq, yf, n, k, oracle, what):
    """The quantised output against the kernel's own f32 output: rows byte for byte; the image field by field."""
    counts = {}
    if fmt != B32:
        want = oracle.quantize(fmt, yf)
        d, s, q = R32.b32_fields(yq, fmt, k)
        wd, ws, wq = R32.b32_fields(want, fmt, k)
        _count("d", d, wd, counts), _count("codes", q, wq, counts)
        if s is not None:
            _count("s", s, ws, counts)
        _count("bytes", yq, want, counts)
    else:
        npad = R.n_pad_of(n)
        mh, md, ms = R32.b32_image_model(oracle.quantize(Q81, yf), k)
        xh, d8, s = R32.b32_image_decode(yq, k, n)
        _count("Xh", xh[:n], mh, counts), _count("d8T", d8[:n], md, counts), _count("sT", s[:n], ms, counts)
        _count("padding Xh", xh[n:], np.zeros((npad - n, k), np.float16), counts)
        _count("padding d8T", d8[n:], np.zeros((npad - n, k // 32), np.float32), counts)
        _count("padding sT", s[n:], np.zeros((npad - n, k // 32), np.float32), counts)
        whole = np.zeros((npad, k), np.float16), np.zeros((npad, k // 32), np.float32), np.zeros((npad, k // 32), np.float32)
        whole[0][:n], whole[1][:n], whole[2][:n] = mh, md, ms
        _count("bytes", yq, R32.b32_image_encode(*whole, k, n), counts)
    print(what, FMT[fmt], "mismatches per field (of):", counts)
    assert all(b == 0 for b, _ in counts.values()), (what, counts)


def _case_id(c):
    return f"{FMT[c[0]]}-{c[1]}x{c[2]}"


# ------------------------------------------------------------------------------------------------------- bytes against the oracle
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_rms_norm_quantize_b32(gpu, oracle, case):
    fmt, n, k = case
    kind, eps = NORM_CONFIGS[CASES.index(case) % 4]
    x = R.norm_input(n, k, k + n, eps)
    w = R.norm_weight(kind, k, k)
    what = ("rms_norm", n, k, kind, eps)
    want, amb = R.rms_norm_ref(x, w, eps)
    strided = (n, k) in STRIDED
    yf, yq = produce("rms_norm", (x,), Outputs(fmt, n, k, strided=strided), w, eps, pad_in=4 if strided else 0).fetch()
    diff = (yf.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    print(what, FMT[fmt], f"f32: {int(diff.sum())} of {n} rows differ from the reference, {int(amb.sum())} rows are ambiguous")
    assert not (diff & ~amb).any()
    check_quantised(fmt, yq, yf, n, k, oracle, what)
    if strided:  # the same bytes where nothing is strided or padded
        yf2, yq2 = produce("rms_norm", (x,), Outputs(fmt, n, k), w, eps).fetch()
        same_bytes(yf2, yf, "dense f32"), same_bytes(yq2, yq, "dense")
    if k % 256 == 0 and fmt != B32:  # y is the Q8_K producer's, bit for bit
        L = _hip.lib()
        xd, wd = torch.from_numpy(x).cuda(), (torch.from_numpy(w).cuda() if w is not None else None)
        ref = torch.empty((n, k), dtype=torch.float32, device="cuda")
        assert L.lfamd_rms_norm_quantize(_ptr(xd), k * 4, _ptr(wd) if wd is not None else C.c_void_p(0), eps, n, k, T.Q8_K, C.c_void_p(0), 0,
                                         _ptr(ref), k * 4, _stream()) == 0
        torch.cuda.synchronize()
        same_bytes(ref.cpu().numpy(), yf, "y of lfamd_rms_norm_quantize")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_swiglu_quantize_b32(gpu, oracle, case):
    fmt, n, k = case
    g, u = R.swiglu_inputs(n, k, 3 * k + n)
    what = ("swiglu", n, k)
    strided = (n, k) in STRIDED
    yf, yq = produce("swiglu", (g, u), Outputs(fmt, n, k, strided=strided), pad_in=4 if strided else 0).fetch()
    assert np.isfinite(yf).all()
    n_ulp, outside = R.smallest_n_ulp(yf, g, u)
    print(what, FMT[fmt], f"f32: smallest n_ulp = {n_ulp}; outside the interval at 0, 1, ... ulp: {outside} of {yf.size}")
    assert n_ulp <= N_ULP_LIMIT
    check_quantised(fmt, yq, yf, n, k, oracle, what)
    if strided:
        yf2, yq2 = produce("swiglu", (g, u), Outputs(fmt, n, k)).fetch()
        same_bytes(yf2, yf, "dense f32"), same_bytes(yq2, yq, "dense")
    if k % 256 == 0 and fmt != B32:  # y is the Q8_K producer's, bit for bit
        L = _hip.lib()
        gd, ud = torch.from_numpy(g).cuda(), torch.from_numpy(u).cuda()
        ref = torch.empty((n, k), dtype=torch.float32, device="cuda")
        assert L.lfamd_swiglu_quantize(_ptr(gd), k * 4, _ptr(ud), k * 4, n, k, T.Q8_K, C.c_void_p(0), 0, _ptr(ref), k * 4, _stream()) == 0
        torch.cuda.synchronize()
        same_bytes(ref.cpu().numpy(), yf, "y of lfamd_swiglu_quantize")


# ------------------------------------------------------------------------------------------------------------ ties and rounding
@pytest.mark.parametrize("fmt", [Q80, Q81, B32], ids=lambda f: FMT[f])
@pytest.mark.parametrize("producer", ["rms_norm", "swiglu"])
def test_ties_round_away_from_zero(gpu, oracle, producer, fmt):
    """y is exact on these rows (tests/test_producer32_ref.py), so the quantiser alone is under test: per 32-block 127, 0.5, -1.5,
    2.5, ... gives d = 1 and codes 127, 1, -2, 3, ...; one block of the row is all zero: d = 0, codes 0, s = 0."""
    n, k = 3, 256 if fmt == B32 else 96
    zb = 1
    if producer == "rms_norm":
        x, w, eps, v = R32.norm_tie_inputs(n, k, zero_block=zb)
        yf, yq = produce(producer, (x,), Outputs(fmt, n, k), w, eps).fetch()
    else:
        g, u, v = R32.swiglu_tie_inputs(n, k, zero_block=zb)
        yf, yq = produce(producer, (g, u), Outputs(fmt, n, k)).fetch()
    same_bytes(yf, v, "y is exact")
    codes = np.tile(R32.tie_codes(k), (n, 1)).reshape(n, k // 32, 32)
    codes[:, zb] = 0
    want_d = np.ones((n, k // 32), np.float32)
    want_d[:, zb] = 0
    want_s = codes.astype(np.int32).sum(axis=2).astype(np.float32)
    assert codes[0, 0, :4].tolist() == [127, 1, -2, 3]
    if fmt == B32:
        xh, d8, s = R32.b32_image_decode(yq, k, n)
        got_q, got_d, got_s = xh[:n].astype(np.int32).reshape(n, -1, 32), d8[:n], s[:n]
    else:
        d, s, q = R32.b32_fields(yq, fmt, k)
        got_q, got_d, got_s = q.astype(np.int32), d.astype(np.float32), (s.astype(np.float32) if s is not None else None)
    assert np.array_equal(got_q, codes.astype(np.int32)), (got_q[0, 0, :8], codes[0, 0, :8])
    assert np.array_equal(got_d, want_d)
    if got_s is not None:
        assert np.array_equal(got_s, want_s)
    check_quantised(fmt, yq, yf, n, k, oracle, (producer, "ties"))


@pytest.mark.parametrize("fmt", [Q80, Q81, B32], ids=lambda f: FMT[f])
def test_block_maximum_shared_by_opposite_signs(gpu, oracle, fmt):
    """producer_ref.tie_rows through the norm with no weight: every 32-block's largest |y| occurs twice with opposite signs.  d =
    amax / 127 does not see the sign, so the codes do not depend on which comes first; the bytes are the oracle's."""
    k = 256 if fmt == B32 else 352
    x = R.tie_rows(k, 32, 21)
    yf, yq = produce("rms_norm", (x,), Outputs(fmt, 4, k), None, 1e-6).fetch()
    a = np.abs(yf.reshape(4, -1, 32))
    assert ((a == a.max(axis=2, keepdims=True)).sum(axis=2) >= 2).all()
    check_quantised(fmt, yq, yf, 4, k, oracle, ("rms_norm", "tie_rows"))


# ---------------------------------------------------------------------------------------------------------- output independence
@pytest.mark.parametrize("fmt", [Q80, Q81, B32], ids=lambda f: FMT[f])
@pytest.mark.parametrize("producer", ["rms_norm", "swiglu"])
def test_each_output_is_the_same_alone(gpu, producer, fmt):
    n, k = (130, 512) if fmt == B32 else (9, 1056)
    if producer == "rms_norm":
        ins, w = (R.norm_input(n, k, 31, 1e-5),), R.norm_weight("wide", k, 32)
    else:
        ins, w = R.swiglu_inputs(n, k, 33), None
    yf, yq = produce(producer, ins, Outputs(fmt, n, k), w).fetch()
    _, yq2 = produce(producer, ins, Outputs(fmt, n, k, f=False), w).fetch()
    yf3, none = produce(producer, ins, Outputs(fmt, n, k, q=False), w).fetch()
    assert none is None
    same_bytes(yq2, yq, "quantised alone"), same_bytes(yf3, yf, "f32 alone")
    if producer == "rms_norm":  # d_weight = NULL is a weight of ones
        _, a = produce(producer, ins, Outputs(fmt, n, k, f=False), None).fetch()
        _, b = produce(producer, ins, Outputs(fmt, n, k, f=False), np.ones(k, np.float32)).fetch()
        same_bytes(a, b, "NULL weight vs ones")


# ---------------------------------------------------------------------------------------------------------- consumers at decode
def _mul_mat(L, W, Btype, B, brb, n, flags, ws):
    out = torch.zeros((n, W.rows), dtype=torch.float32, device="cuda")
    rc = L.lfamd_mul_mat(W.type, _ptr(W.data), W.rows, W.cols, Btype, B, brb, n, _ptr(out), W.rows, _ptr(ws), ws.numel(), flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    return out


def _reference(oracle, t, A, Bq, y, k, rows, cols):
    """(oracle results [tokens, rows] of the sample, sum |w| |x|) — IQ4_NL from tests/iq4nl_ref.py, the others from the oracle."""
    if t != T.IQ4_NL:
        return oracle_sample(oracle, t, A, Bq, k, rows, cols), abs_products(oracle, t, A, y, k, rows, cols)
    G = NL.dot_ref(np.ascontiguousarray(A[rows]), np.ascontiguousarray(Bq[cols])).astype(np.float32)
    xs = np.abs(y[cols]).astype(np.float64)
    xs += xs.max(axis=1, keepdims=True) / 127.0
    return G, xs @ np.abs(NL.dequantize(np.ascontiguousarray(A[rows]))).astype(np.float64).T


DECODE_TYPES = (T.Q8_0, T.Q4_0, T.IQ4_NL, T.Q5_0, T.Q4_1, T.Q5_1)


@pytest.mark.parametrize("k", [256, 4352])
@pytest.mark.parametrize("t", DECODE_TYPES, ids=lambda t: T.NAMES[t])
def test_decode_gemv_on_the_producers_rows(gpu, oracle, t, k):
    """n = 1 and n = 7 on rows the norm wrote 2 / 4 bytes into their buffer with a gap between them: the bits of the same call on
    lfamd_quantize_rows' dense rows (the bytes are equal, so alignment and stride are what this guards), within the oracle's bound."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    m, n = 64, 7
    vdt = T.VEC_DOT[t]
    x = for_vec_dot(extreme_activations(n, k, k + t), vdt)
    w = np.random.default_rng(k + t).uniform(0.5, 2.0, k).astype(np.float32)
    out = produce("rms_norm", (x,), Outputs(vdt, n, k, strided=True), w, 1e-5, pad_in=4)
    yf, yq = out.fetch()
    dense = gpu.quantize_rows(vdt, torch.from_numpy(yf).cuda())
    torch.cuda.synchronize()
    same_bytes(dense.cpu().numpy(), yq, "lfamd_quantize_rows of y")
    A = synth.random_weights(t, m, k, 40 + t)
    W = gpu.upload_weights(t, A, m, k)
    ws = torch.empty(max(16, L.lfamd_mul_mat_workspace(t, m, k, n)), dtype=torch.uint8, device="cuda")
    rows, cols = np.arange(m), np.arange(n)
    G, ap = _reference(oracle, t, A, yq, yf, k, rows, cols)
    stride, rs = out.rs + out.pq, out.rs
    for n_call, j0 in ((7, 0), (1, 3), (1, 5)):
        got = _mul_mat(L, W, vdt, _ptr(out.qbuf, out.qoff + j0 * stride), stride, n_call, flags, ws)
        want = _mul_mat(L, W, vdt, _ptr(dense, j0 * rs), rs, n_call, flags, ws)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (T.NAMES[t], k, n_call, j0)
        c = cols[j0:j0 + n_call]
        check(got.cpu().numpy(), G[c], c, rows, True, (T.NAMES[t], "decode on producer rows", k, n_call, j0), zero_row=False, absprod=ap[c], k=k)


# --------------------------------------------------------------------------------------------------------- consumers on the image
IMAGE_TYPES = (T.Q4_0, T.IQ4_NL, T.Q4_1, T.Q5_0, T.Q5_1)


@pytest.mark.parametrize("k", [256, 4352])
@pytest.mark.parametrize("t", IMAGE_TYPES, ids=lambda t: T.NAMES[t])
def test_batches_on_the_image(gpu, t, k):
    """lfamd_mul_mat on the image gives the bits of the same call on the producer's f32 rows (the same body on the same operand
    bytes, no K split), and the workspace handed to it keeps its sentinel: no staging launch ran."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    m = 192
    W = gpu.upload_weights(t, synth.random_weights(t, m, k, 60 + t), m, k)
    for n in (9, 129):
        assert L.lfamd_mul_mat_takes_staged_b32(t, m, k, n, flags) == 1
        x = for_vec_dot(extreme_activations(n, k, k + n), T.VEC_DOT[t])
        yf, img = produce("rms_norm", (x,), Outputs(B32, n, k), R.norm_weight("ones", k, 0), 1e-5).fetch()
        image, yfd = torch.from_numpy(img).cuda(), torch.from_numpy(yf).cuda()  # (fresh allocations: 16-byte aligned)
        need = max(16, L.lfamd_mul_mat_workspace(t, m, k, n))
        ws, ws_img = torch.empty(need, dtype=torch.uint8, device="cuda"), _sentinel(need)
        got = _mul_mat(L, W, B32, _ptr(image), 0, n, flags, ws_img)
        want = _mul_mat(L, W, T.F32, _ptr(yfd), k * 4, n, flags, ws)
        torch.cuda.synchronize()
        diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
        print(T.NAMES[t], k, n, f"{diff} of {got.numel()} words differ between the image and the f32 rows")
        assert diff == 0 and bool(want.any())
        assert bool((ws_img == SENT).all()), "the workspace was written"
        # and without any workspace at all
        got.zero_()
        rc = L.lfamd_mul_mat(t, _ptr(W.data), m, k, B32, _ptr(image), 0, n, _ptr(got), m, C.c_void_p(0), 0, flags, _stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_multi_on_the_image(gpu):
    """lfamd_mul_mat_multi, two Q4_0 matrices on one image at 129 tokens: the bits of the call on the f32 rows."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    k, n, ms = 768, 129, (192, 64)
    Ws = [gpu.upload_weights(T.Q4_0, synth.random_weights(T.Q4_0, m, k, 70 + m), m, k) for m in ms]
    yf, img = produce("swiglu", R.swiglu_inputs(n, k, 71), Outputs(B32, n, k)).fetch()
    image, yfd = torch.from_numpy(img).cuda(), torch.from_numpy(yf).cuda()
    need = max(16, max(L.lfamd_mul_mat_workspace(T.Q4_0, m, k, n) for m in ms))
    A = (C.c_void_p * 2)(*[w.data.data_ptr() for w in Ws])
    mm = (C.c_long * 2)(*ms)

    def multi(Btype, B, brb, ws):
        outs = [torch.zeros((n, m), dtype=torch.float32, device="cuda") for m in ms]
        Cs = (C.c_void_p * 2)(*[o.data_ptr() for o in outs])
        rc = L.lfamd_mul_mat_multi(T.Q4_0, 2, A, mm, k, Btype, B, brb, n, Cs, mm, _ptr(ws), ws.numel(), flags, _stream())
        assert rc == 0, L.lfamd_last_error()
        torch.cuda.synchronize()
        return outs

    ws_img = _sentinel(need)
    got = multi(B32, _ptr(image), 0, ws_img)
    want = multi(T.F32, _ptr(yfd), k * 4, torch.empty(need, dtype=torch.uint8, device="cuda"))
    for a, b in zip(got, want):
        assert bool(b.any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool((ws_img == SENT).all())
    # a set with a matrix that does not take the image (n <= 8 rows of it would; a K-quant never does) is refused whole
    Cs = (C.c_void_p * 2)(*[o.data_ptr() for o in got])
    assert L.lfamd_mul_mat_multi(T.Q4_K, 2, A, mm, k, B32, _ptr(image), 0, n, Cs, mm, _ptr(ws_img), need, flags, _stream()) == -1


# ---------------------------------------------------------------------------------------------------------- a captured graph
def graph_case():
    """Body of test_norm_b32_image_mat_mul_in_a_captured_graph; runs in a process of its own."""
    from llamafile_amd import sgemm as gpu
    gpu.init(0)
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    n, k, m, eps = 130, 768, 256, 1e-5
    assert L.lfamd_mul_mat_takes_staged_b32(T.Q5_1, m, k, n, flags) == 1
    W = gpu.upload_weights(T.Q5_1, synth.random_weights(T.Q5_1, m, k, 5), m, k)
    wd = torch.from_numpy(R.norm_weight("wide", k, 6)).cuda()
    x = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    image = _sentinel(L.lfamd_staged_b32_size(k, n))
    out = torch.zeros((n, m), dtype=torch.float32, device="cuda")
    none = C.c_void_p(0)

    def chain(img, o):
        st = _stream()
        assert L.lfamd_rms_norm_quantize_b32(_ptr(x), k * 4, _ptr(wd), eps, n, k, B32, _ptr(img), 0, none, 0, st) == 0
        assert L.lfamd_mul_mat(T.Q5_1, _ptr(W.data), m, k, B32, _ptr(img), 0, n, _ptr(o), m, none, 0, flags, st) == 0

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


def test_norm_b32_image_mat_mul_in_a_captured_graph(gpu):
    """norm -> 32-block image -> lfamd_mul_mat captured once as a single chain and replayed twice with new input contents equals
    the uncaptured calls each time.  In a fresh child process, as test_gpu_producers does it."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_producers_b32 as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_every_output_untouched(gpu):
    """LFAMD_ERR_INVALID with every output still holding its sentinel; the image handed to a call that does not take it is
    LFAMD_ERR_UNSUPPORTED with the result untouched; then a correct call is served."""
    L = _hip.lib()
    n, k = 4, 512
    st = _stream()
    x = torch.ones((n, k + 4), dtype=torch.float32, device="cuda")
    w = torch.ones(k + 4, dtype=torch.float32, device="cuda")
    rs0, rs1 = T.row_size(Q80, k), T.row_size(Q81, k)
    yf = _sentinel(n * k * 4 + 64)
    yq = _sentinel(max(n * rs1, L.lfamd_staged_b32_size(k, n)) + 64)
    base = dict(x=(x, 0), xrb=(k + 4) * 4, w=(w, 0), g=(x, 0), grb=(k + 4) * 4, n=n, k=k, vdt=Q80, yq=(yq, 0), yqrb=rs0, yf=(yf, 0), yfrb=k * 4)

    def p(v):
        return C.c_void_p(0) if v is None else _ptr(*v)

    def norm(**kw):
        a = {**base, **kw}
        return L.lfamd_rms_norm_quantize_b32(p(a["x"]), a["xrb"], p(a["w"]), 1e-5, a["n"], a["k"], a["vdt"], p(a["yq"]), a["yqrb"], p(a["yf"]), a["yfrb"], st)

    def swiglu(**kw):
        a = {**base, **kw}
        return L.lfamd_swiglu_quantize_b32(p(a["g"]), a["grb"], p(a["x"]), a["xrb"], a["n"], a["k"], a["vdt"], p(a["yq"]), a["yqrb"], p(a["yf"]), a["yfrb"], st)

    common = [dict(k=48), dict(k=96, vdt=B32), dict(k=0), dict(n=-1), dict(vdt=T.Q8_K, yqrb=584), dict(vdt=_hip.TYPE_STAGED_Q8K),
              dict(vdt=_hip.TYPE_STAGED_SCALED), dict(vdt=T.F32), dict(x=(x, 4)), dict(yf=(yf, 4)), dict(xrb=(k + 1) * 4), dict(yfrb=(k + 1) * 4),
              dict(yq=(yq, 1)), dict(yqrb=rs0 + 1), dict(yqrb=rs0 - 2), dict(vdt=Q81, yq=(yq, 2), yqrb=rs1), dict(vdt=Q81, yqrb=rs1 + 2),
              dict(vdt=Q81, yqrb=rs1 - 4), dict(vdt=B32, yq=(yq, 8)), dict(yq=None, yf=None)]
    for kw in common + [dict(w=(w, 4))]:
        assert norm(**kw) == -2, ("rms_norm", kw)
    for kw in common + [dict(g=(x, 4)), dict(grb=(k + 2) * 4), dict(n=65409)]:
        assert swiglu(**kw) == -2, ("swiglu", kw)
    for vdt, rb in ((Q80, rs0), (Q81, rs1), (B32, 0)):
        assert norm(n=0, vdt=vdt, yqrb=rb) == 0 and swiglu(n=0, vdt=vdt, yqrb=rb) == 0
    torch.cuda.synchronize()
    assert bool((yf == SENT).all()) and bool((yq == SENT).all())
    # the image in front of calls that do not take it: Q8_0 weights, a K-quant, a decode batch
    flags = gpu.host_variant_flags()
    m, nt = 64, 16
    image = torch.zeros(L.lfamd_staged_b32_size(k, nt), dtype=torch.uint8, device="cuda")
    res = _sentinel(nt * m * 4)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for t, n_call in ((T.Q8_0, nt), (T.Q4_K, nt), (T.Q4_0, 4)):
        W = gpu.upload_weights(t, synth.random_weights(t, m, k, 80 + t), m, k)
        assert L.lfamd_mul_mat_takes_staged_b32(t, m, k, n_call, flags) == 0
        assert L.lfamd_mul_mat(t, _ptr(W.data), m, k, B32, _ptr(image), 0, n_call, _ptr(res), m, _ptr(ws), ws.numel(), flags, st) == -1, T.NAMES[t]
    torch.cuda.synchronize()
    assert bool((res == SENT).all())
    # and the calls are served once the arguments are right
    assert norm() == 0 and swiglu(vdt=B32, yqrb=0) == 0
    W = gpu.upload_weights(T.Q4_0, synth.random_weights(T.Q4_0, m, k, 90), m, k)
    assert L.lfamd_mul_mat(T.Q4_0, _ptr(W.data), m, k, B32, _ptr(image), 0, nt, _ptr(res), m, _ptr(ws), ws.numel(), flags, st) == 0
    torch.cuda.synchronize()
    assert not bool((yf[:n * k * 4] == SENT).all()) and bool((yf[n * k * 4:] == SENT).all())
    assert bool((yq[:L.lfamd_staged_b32_size(k, n)] != SENT).any()) and bool((yq[L.lfamd_staged_b32_size(k, n):] == SENT).all())
    assert bool((res.view(torch.float32) == 0).all())  # a zero image times anything
