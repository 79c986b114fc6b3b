"""The LFAMD_TYPE_STAGED_Q80 image — the staged activations of Q8_0-weight batches on gemm_lf_q80 (csrc/gemm_lf.hip) — as an output of
lfamd_rms_norm_quantize_b32 / lfamd_swiglu_quantize_b32 (csrc/norm_quant.hip) and as an input of lfamd_mul_mat / lfamd_mul_mat_multi:

  image bytes   all of them, padding included, against tests/producer80_ref.py applied to oracle.quantize of the kernel's own f32
                output; and against the workspace a lfamd_mul_mat call on that f32 output leaves behind (Xh over all n_pad tokens,
                stage / tok_scale over the tokens the in-call staging writes)
  edges         a 3e5 row, a 1e-7 row (every stored d is zero: no normalisation), an all-zero row, a row with an all-zero block
  rounding      rows whose y is exact and whose every code is a tie: roundf's 1, -2, 3
  each output   the image alone, the f32 rows alone, both: the same bytes
  consumers     the mat-mul on the image gives the bits of the same call on the producer's f32 rows and leaves the workspace alone
                (or has none); within the bounds tests/test_gpu_gemm_lf.py holds this body to of the oracle; sibling matrices in one
                launch; a failing call enqueues nothing; a captured graph; the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
from helpers import elem_err, rel_err
import producer32_ref as R32
import producer80_ref as R80
import producer_ref as R
from test_gpu_producers import GUARD, NORM_CONFIGS, SENT, _count, _ptr, _rows_in, _sentinel, _stream, same_bytes

pytestmark = pytest.mark.gpu

Q80I = _hip.TYPE_STAGED_Q80
PRODUCERS = ("rms_norm", "swiglu")
KS = (128, 384, 640, 4224)  # a half chunk alone; a chunk and a half; two and a half; every wave's share ends in the half chunk
NS = (1, 9, 127, 128, 129, 300)


def produce(producer, ins, w=None, eps=1e-5, q=True, f=True, pad_in=0):
    """One producer call into sentinel-filled buffers (the image and the f32 rows 16 bytes into their allocations, GUARD bytes
    behind): (f32 [n, k] or None, image bytes or None); head and guard are checked."""
    L = _hip.lib()
    n, k = ins[0].shape
    size = L.lfamd_staged_q80_size(k, n)
    qbuf = _sentinel(16 + size + GUARD) if q else None
    fbuf = _sentinel(16 + n * k * 4 + GUARD) if f else None
    dev = [_rows_in(a, pad_in) for a in ins]
    rb = (k + pad_in) * 4
    yq = _ptr(qbuf, 16) if q else C.c_void_p(0)
    yf = _ptr(fbuf, 16) if f else C.c_void_p(0)
    if producer == "rms_norm":
        wd = torch.from_numpy(w).cuda() if w is not None else None
        rc = L.lfamd_rms_norm_quantize_b32(_ptr(dev[0]), rb, _ptr(wd) if wd is not None else C.c_void_p(0), eps, n, k, Q80I, yq, 12345, yf, k * 4, _stream())
    else:
        rc = L.lfamd_swiglu_quantize_b32(_ptr(dev[0]), rb, _ptr(dev[1]), rb, n, k, Q80I, yq, 12345, yf, k * 4, _stream())
    assert rc == 0, (rc, L.lfamd_last_error())
    torch.cuda.synchronize()
    out_f = out_q = None
    if f:
        a = fbuf.cpu().numpy()
        assert (a[:16] == SENT).all() and (a[16 + n * k * 4:] == SENT).all(), "f32 rows: a byte in front of or behind them was written"
        out_f = a[16:16 + n * k * 4].view(np.float32).reshape(n, k).copy()
    if q:
        a = qbuf.cpu().numpy()
        assert (a[:16] == SENT).all() and (a[16 + size:] == SENT).all(), "the image: a byte in front of or behind it was written"
        out_q = a[16:16 + size].copy()
    return out_f, out_q


def inputs(producer, n, k, seed):
    """(ins, weight, eps) inside the image's domain: every block's amax / 127 at most 65504."""
    if producer == "rms_norm":
        kind, eps = NORM_CONFIGS[seed % 4]
        return (R.norm_input(n, k, k + n, eps),), R.norm_weight(kind, k, k), eps
    g, u = R.swiglu_inputs(n, k, 3 * k + n)
    with np.errstate(over="ignore"):
        y = np.abs(g.astype(np.float64) / (1.0 + np.exp(-g.astype(np.float64))) * u.astype(np.float64)).max(axis=1)
    big = y > 4e6  # (a 3e5 row of up under a gate of 90: scaled by a power of two, so every other property of the row stays)
    u[big] *= np.exp2(-np.ceil(np.log2(y[big] / 4e6))).astype(np.float32)[:, None]
    return (g, u), None, 0.0


_W = {}


def tiny_weights(gpu, k):
    if k not in _W:
        _W[k] = gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, 8, k, 300 + k), 8, k)
    return _W[k]


def in_call_staging(gpu, y, k, Btype=T.F32):
    """The workspace a lfamd_mul_mat call of Q8_0 weights on the rows y (f32 [n, k], or Q8_0 blocks uint8 [n, k / 32 * 34]) leaves
    behind: (Xh f16 [n_pad, k], stage [n_pad], tok_scale [n_pad], n' = the tokens it staged).  Batches take this body from nine tokens
    on: fewer rows are followed by all-zero rows, which the staging writes as it finds padding tokens (zero operands, factors of 1)."""
    L = _hip.lib()
    n = y.shape[0]
    n2 = max(n, 9)
    rows = np.zeros((n2, y.shape[1]), y.dtype)
    rows[:n] = y
    W = tiny_weights(gpu, k)
    assert L.lfamd_mul_mat_takes_staged_q80(T.Q8_0, 8, k, n2, gpu.host_variant_flags()) == 1
    need = L.lfamd_mul_mat_workspace(T.Q8_0, 8, k, n2)
    size = L.lfamd_staged_q80_size(k, n2)
    assert size == L.lfamd_staged_q80_size(k, n) and need >= size
    ws = _sentinel(need)
    yd = torch.from_numpy(rows).cuda()
    out = torch.empty((n2, 8), dtype=torch.float32, device="cuda")
    rc = L.lfamd_mul_mat(T.Q8_0, _ptr(W.data), 8, k, Btype, _ptr(yd), rows.shape[1] * rows.itemsize, n2, _ptr(out), 8, _ptr(ws), need,
                         gpu.host_variant_flags(), _stream())
    assert rc == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    return R80.q80_image_decode(ws.cpu().numpy()[:size], k, n2) + (n2,)


def check_image(gpu, oracle, img, yf, n, k, what):
    """Every byte of the image against the model on the kernel's own f32 rows, then against the in-call staging of those rows.

    The in-call staging of f32 rows keeps roundf's result as a float, so a y with its sign bit set (a y of -0.0 among them) that rounds
    to code 0 is staged as -0.0 (0x8000) there.  A Q8_0 block has no such code, so neither the model of the image (first reference)
    nor the in-call staging of Q8_0 rows holds it, and no sum the GEMM forms can tell the two zeros apart.  The two references of the
    f32 rows therefore differ in exactly those sign bits; the image follows the blocks.  Against the f32 call's workspace every other
    bit is compared, and every -0.0 it holds where the image holds +0 must sit on a y with the sign bit set whose code is 0; against
    the workspace of the same call on the Q8_0 rows of y, all bits."""
    counts = {}
    npad = R.n_pad_of(n)
    assert np.isfinite(yf).all() and np.abs(yf).max() / 127 <= 65504  # the image's domain
    q80 = oracle.quantize(T.Q8_0, yf)
    mh, ms, mt = R80.q80_image_model(q80, k)
    xh, stage, tok = R80.q80_image_decode(img, k, n)
    _count("Xh", xh[:n], mh, counts), _count("stage", stage[:n], ms, counts), _count("tok_scale", tok[:n], mt, counts)
    _count("padding Xh", xh[n:], np.zeros((npad - n, k), np.float16), counts)
    _count("padding stage", stage[n:], np.ones(npad - n, np.float32), counts)
    _count("padding tok_scale", tok[n:], np.ones(npad - n, np.float32), counts)
    _count("bytes", img, R80.q80_image_of_rows(q80, k), counts)
    sh, ss, st, n2 = in_call_staging(gpu, yf, k)
    bits = np.ascontiguousarray(sh).view(np.uint16)
    # (a -0.0 the image holds too — a negative code under a stored d of zero — is compared like any other value)
    neg0 = (bits == 0x8000) & (np.ascontiguousarray(xh).view(np.uint16) == 0)
    codes = R32.b32_fields(q80, T.Q8_0, k)[2].reshape(n, k)
    assert not neg0[n:].any() and (np.signbit(yf[neg0[:n]]) & (codes[neg0[:n]] == 0)).all(), "a -0.0 of the in-call staging that is no negative y of code 0"
    _count("Xh of the in-call staging of the f32 rows (its -0.0 read as 0)", xh, np.where(neg0, np.uint16(0), bits), counts)
    _count("stage of the in-call staging", stage[:n], ss[:n], counts), _count("tok_scale of the in-call staging", tok[:n], st[:n], counts)
    qh, qs, qt, _ = in_call_staging(gpu, q80, k, T.Q8_0)
    _count("Xh of the in-call staging of the Q8_0 rows", xh, qh, counts)
    _count("stage of that staging", stage[:n], qs[:n], counts), _count("tok_scale of that staging", tok[:n], qt[:n], counts)
    counts["-0.0 in the f32 call's workspace"] = (0, int(neg0.sum()))
    print(what, "mismatches per field (of):", counts)
    assert all(b == 0 for b, _ in counts.values()), (what, counts)


# ------------------------------------------------------------------------------------------------------------------- image bytes
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("producer", PRODUCERS)
def test_image_bytes(gpu, oracle, producer, k, n):
    ins, w, eps = inputs(producer, n, k, KS.index(k) + NS.index(n))
    yf, img = produce(producer, ins, w, eps, pad_in=4 if n == 9 else 0)
    assert np.isfinite(yf).all()
    if producer == "rms_norm":
        want, amb = R.rms_norm_ref(ins[0], w, eps)
        assert not ((yf.view(np.uint32) != want.view(np.uint32)).any(axis=1) & ~amb).any()
    check_image(gpu, oracle, img, yf, n, k, (producer, n, k))


# ----------------------------------------------------------------------------------------------------- per-token scale at its edges
def edge_inputs(producer, n, k):
    """Rows 0 .. 3: scaled by 3e5, scaled by 1e-7, all zero, one all-zero block; the rest ordinary.  SwiGLU: gate = 32 and up = v / 32
    give y = v exactly; the norm: eps = 1e12 pins the scale near 1e-6 for every row and a weight of 1e6 undoes it."""
    v = synth.random_activations(n, k, 21).astype(np.float32)
    v[0] *= np.float32(3e5)
    v[1] *= np.float32(1e-7)
    v[2] = 0.0
    v[3, 32:64] = 0.0
    if producer == "swiglu":
        return (np.full((n, k), 32.0, np.float32), (v / np.float32(32.0)).astype(np.float32)), None, 0.0
    return (v,), np.full(k, 1e6, np.float32), 1e12


@pytest.mark.parametrize("producer", PRODUCERS)
def test_per_token_scale_at_its_edges(gpu, oracle, producer):
    L = _hip.lib()
    n, k, m = 12, 256, 64
    ins, w, eps = edge_inputs(producer, n, k)
    yf, img = produce(producer, ins, w, eps)
    check_image(gpu, oracle, img, yf, n, k, (producer, "edges"))
    xh, stage, tok = R80.q80_image_decode(img, k, n)
    top = np.abs(yf).max(axis=1)
    assert top[0] > 1e5 and stage[0] <= 2.0 ** -7 and stage[0] * tok[0] == 1  # the 3e5 row is brought down ...
    assert 512 <= np.abs(xh[0].astype(np.float32)).max() <= 1024             # ... to [512, 1024]
    assert 0 < top[1] < 1e-6 and stage[1] == 1 and tok[1] == 1 and not xh[1].any()  # every stored d of the 1e-7 row is zero
    assert top[2] == 0 and stage[2] == 1 and tok[2] == 1 and not xh[2].any()
    assert not xh[3, 32:64].any() and xh[3, :32].any() and stage[3] > 1
    W = gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 22), m, k)
    got, want = image_and_f32_calls(gpu, W, img, yf, n)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(want[0].any()) and not bool(want[1:3].any())


# ------------------------------------------------------------------------------------------------------------ ties and rounding
@pytest.mark.parametrize("producer", PRODUCERS)
def test_ties_round_away_from_zero(gpu, oracle, producer):
    """y is exact on these rows (tests/test_producer32_ref.py), so the quantiser alone is under test: per 32-block 127, 0.5, -1.5,
    2.5, ... gives d = 1 and codes 127, 1, -2, 3, ...; D = 127, so stage = 8 and the image holds 8 * code.  One block is all zero."""
    n, k, zb = 3, 384, 1
    if producer == "rms_norm":
        x, w, eps, v = R32.norm_tie_inputs(n, k, zero_block=zb)
        yf, img = produce(producer, (x,), w, eps)
    else:
        g, u, v = R32.swiglu_tie_inputs(n, k, zero_block=zb)
        yf, img = produce(producer, (g, u))
    same_bytes(yf, v, "y is exact")
    codes = np.tile(R32.tie_codes(k), (n, 1)).astype(np.float32)
    codes[:, 32 * zb:32 * zb + 32] = 0
    assert codes[0, :4].tolist() == [127, 1, -2, 3]
    xh, stage, tok = R80.q80_image_decode(img, k, n)
    assert (stage[:n] == 8).all() and (tok[:n] == 0.125).all()
    assert np.array_equal(xh[:n].astype(np.float32), 8 * codes), (xh[0, :8], codes[0, :8])
    check_image(gpu, oracle, img, yf, n, k, (producer, "ties"))


# ---------------------------------------------------------------------------------------------------------- output independence
@pytest.mark.parametrize("producer", PRODUCERS)
def test_each_output_is_the_same_alone(gpu, producer):
    n, k = 130, 640
    ins, w, eps = inputs(producer, n, k, 0)
    yf, img = produce(producer, ins, w, eps)
    none, img2 = produce(producer, ins, w, eps, f=False)
    yf3, none3 = produce(producer, ins, w, eps, q=False)
    assert none is None and none3 is None
    same_bytes(img2, img, "the image alone"), same_bytes(yf3, yf, "f32 alone")
    # and y is the other producers' y, bit for bit (Q8_0 rows of the same entry point)
    L = _hip.lib()
    dev = [torch.from_numpy(a).cuda() for a in ins]
    ref = torch.empty((n, k), dtype=torch.float32, device="cuda")
    if producer == "rms_norm":
        wd = torch.from_numpy(w).cuda() if w is not None else None
        rc = L.lfamd_rms_norm_quantize_b32(_ptr(dev[0]), k * 4, _ptr(wd) if wd is not None else C.c_void_p(0), eps, n, k, T.Q8_0, C.c_void_p(0), 0,
                                           _ptr(ref), k * 4, _stream())
    else:
        rc = L.lfamd_swiglu_quantize_b32(_ptr(dev[0]), k * 4, _ptr(dev[1]), k * 4, n, k, T.Q8_0, C.c_void_p(0), 0, _ptr(ref), k * 4, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    same_bytes(ref.cpu().numpy(), yf, "y of the Q8_0-row format")


# --------------------------------------------------------------------------------------------------------- consumers on the image
def image_and_f32_calls(gpu, W, img, yf, n, ldc=None, fill=0.0, no_ws=False):
    """(result of lfamd_mul_mat on the image, result of the same call on the f32 rows); the workspace handed to the first call must
    keep its sentinel (no_ws: it gets none at all)."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    m, k = W.rows, W.cols
    ldc = ldc or m
    assert L.lfamd_mul_mat_takes_staged_q80(T.Q8_0, m, k, n, flags) == 1
    image, yfd = torch.from_numpy(img).cuda(), torch.from_numpy(yf).cuda()  # (fresh allocations: 16-byte aligned)
    need = max(16, L.lfamd_mul_mat_workspace(T.Q8_0, m, k, n))
    ws, ws_img = torch.empty(need, dtype=torch.uint8, device="cuda"), _sentinel(need)
    got = torch.full((n, ldc), fill, dtype=torch.float32, device="cuda")
    want = torch.full((n, ldc), fill, dtype=torch.float32, device="cuda")
    rc = L.lfamd_mul_mat(T.Q8_0, _ptr(W.data), m, k, Q80I, _ptr(image), 0, n, _ptr(got), ldc, C.c_void_p(0) if no_ws else _ptr(ws_img),
                         0 if no_ws else need, flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    rc = L.lfamd_mul_mat(T.Q8_0, _ptr(W.data), m, k, T.F32, _ptr(yfd), k * 4, n, _ptr(want), ldc, _ptr(ws), need, flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    assert bool((ws_img == SENT).all()), "the workspace was written"
    return got, want


# (4224, 520, 128): 264 tiles of 128 x 64, so the 128-token tile; (520, 150, 256): ldc = m + 24
MM_SHAPES = [(5, 9, 128), (40, 33, 384), (129, 65, 256), (1000, 129, 640), (4224, 520, 128), (4300, 513, 256), (520, 150, 256)]
_ORACLE_SHAPES = {(129, 65, 256), (1000, 129, 640)}


@pytest.mark.parametrize("shape", MM_SHAPES, ids=str)
def test_mat_mul_on_the_image(gpu, oracle, shape):
    m, n, k = shape
    ldc, fill = (m + 24, 7.0) if shape == (520, 150, 256) else (m, 0.0)
    producer = PRODUCERS[MM_SHAPES.index(shape) % 2]
    A = synth.random_weights(T.Q8_0, m, k, 131)
    W = gpu.upload_weights(T.Q8_0, A, m, k)
    x = synth.random_activations(n, k, 132)
    ins = (x,) if producer == "rms_norm" else (np.full((n, k), 32.0, np.float32), x)
    yf, img = produce(producer, ins, None, 1e-5)
    got, want = image_and_f32_calls(gpu, W, img, yf, n, ldc, fill)
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(shape, producer, f"{diff} of {got.numel()} words differ between the image and the f32 rows")
    assert diff == 0 and bool(want[:, :m].any())
    assert bool((got[:, m:] == fill).all())  # the columns past m keep their fill
    got2, _ = image_and_f32_calls(gpu, W, img, yf, n, ldc, fill, no_ws=True)  # d_ws = NULL, ws_bytes = 0
    assert torch.equal(got2.view(torch.int32), want.view(torch.int32))
    if shape in _ORACLE_SHAPES:  # the bounds tests/test_gpu_gemm_lf.py holds this body to
        v = oracle.variant("zen4" if gpu.host_variant_flags() & _hip.FLAG_Q0_VREGS32 else "avx2")
        ok, G = oracle.sgemm(T.Q8_0, A, T.Q8_0, oracle.quantize(T.Q8_0, yf), m, n, k, nth=8, v=v)
        assert ok == 1
        Cd = got.cpu().numpy()
        e = rel_err(Cd, G)
        frac, worst = elem_err(Cd, G, rtol=3e-3)
        print(shape, f"against the oracle: rel_err {e:.3g}, beyond rtol 3e-3: {frac} (worst {worst})")
        assert not np.isnan(Cd).any() and e <= 1e-3 and frac == 0.0, (e, frac, worst)


@pytest.mark.parametrize("count", [2, 3, 4])
def test_multi_on_the_image(gpu, count):
    """lfamd_mul_mat_multi on the image: one launch over the concatenated row blocks, the bits of separate calls on the f32 rows; a
    call whose second matrix has ldc < m is refused with every output still holding its fill."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    k, n = 512, 90
    ms = [300, 40, 7, 1030][:count]
    Ws = [gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 170 + i), m, k) for i, m in enumerate(ms)]
    g, u = np.full((n, k), 32.0, np.float32), synth.random_activations(n, k, 175)
    yf, img = produce("swiglu", (g, u))
    image, yfd = torch.from_numpy(img).cuda(), torch.from_numpy(yf).cuda()
    A = (C.c_void_p * count)(*[w.data.data_ptr() for w in Ws])
    mm = (C.c_long * count)(*ms)
    outs = [torch.full((n, m), 7.0, dtype=torch.float32, device="cuda") for m in ms]
    Cs = (C.c_void_p * count)(*[o.data_ptr() for o in outs])
    short = (C.c_long * count)(*[m - (j == 1) for j, m in enumerate(ms)])
    ws = _sentinel(1 << 16)
    rc = L.lfamd_mul_mat_multi(T.Q8_0, count, A, mm, k, Q80I, _ptr(image), 0, n, Cs, short, _ptr(ws), ws.numel(), flags, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and all(bool((o == 7.0).all()) for o in outs)
    rc = L.lfamd_mul_mat_multi(T.Q8_0, count, A, mm, k, Q80I, _ptr(image), 0, n, Cs, mm, _ptr(ws), ws.numel(), flags, _stream())
    assert rc == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    assert bool((ws == SENT).all())
    for W, o in zip(Ws, outs):
        sep = gpu.mul_mat(W, yfd.view(torch.uint8), T.F32, n=n)
        assert bool(sep.any()) and torch.equal(o.view(torch.int32), sep.view(torch.int32))
    # without any workspace
    outs2 = [torch.zeros((n, m), dtype=torch.float32, device="cuda") for m in ms]
    Cs2 = (C.c_void_p * count)(*[o.data_ptr() for o in outs2])
    assert L.lfamd_mul_mat_multi(T.Q8_0, count, A, mm, k, Q80I, _ptr(image), 0, n, Cs2, mm, C.c_void_p(0), 0, flags, _stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, outs2))


def test_multi_of_more_than_four_matrices_runs_one_gemm_each(gpu):
    """Five matrices do not fit one launch: one GEMM per matrix on the one image, the same bits."""
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    k, n, ms = 128, 20, [16, 9, 130, 8, 40]
    Ws = [gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 190 + i), m, k) for i, m in enumerate(ms)]
    yf, img = produce("rms_norm", (synth.random_activations(n, k, 195),))
    image, yfd = torch.from_numpy(img).cuda(), torch.from_numpy(yf).cuda()
    A = (C.c_void_p * 5)(*[w.data.data_ptr() for w in Ws])
    mm = (C.c_long * 5)(*ms)
    outs = [torch.zeros((n, m), dtype=torch.float32, device="cuda") for m in ms]
    Cs = (C.c_void_p * 5)(*[o.data_ptr() for o in outs])
    assert L.lfamd_mul_mat_multi(T.Q8_0, 5, A, mm, k, Q80I, _ptr(image), 0, n, Cs, mm, C.c_void_p(0), 0, flags, _stream()) == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    for W, o in zip(Ws, outs):
        sep = gpu.mul_mat(W, yfd.view(torch.uint8), T.F32, n=n)
        assert bool(sep.any()) and torch.equal(o.view(torch.int32), sep.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- a captured graph
def graph_case():
    """Body of test_producer_image_mat_mul_in_a_captured_graph; runs in a process of its own."""
    from llamafile_amd import sgemm as gpu
    gpu.init(0)
    L = _hip.lib()
    flags = gpu.host_variant_flags()
    n, k, m, eps = 130, 384, 256, 1e-5
    assert L.lfamd_mul_mat_takes_staged_q80(T.Q8_0, m, k, n, flags) == 1
    W = gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 5), m, k)
    wd = torch.from_numpy(R.norm_weight("wide", k, 6)).cuda()
    x = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    image = _sentinel(L.lfamd_staged_q80_size(k, n))
    out = torch.zeros((n, m), dtype=torch.float32, device="cuda")
    none = C.c_void_p(0)

    def chain(img, o):
        st = _stream()
        assert L.lfamd_rms_norm_quantize_b32(_ptr(x), k * 4, _ptr(wd), eps, n, k, Q80I, _ptr(img), 0, none, 0, st) == 0
        assert L.lfamd_mul_mat(T.Q8_0, _ptr(W.data), m, k, Q80I, _ptr(img), 0, n, _ptr(o), m, none, 0, flags, st) == 0

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


def test_producer_image_mat_mul_in_a_captured_graph(gpu):
    """norm -> Q80 image -> lfamd_mul_mat captured once as a single chain and replayed twice with new input contents equals the
    uncaptured calls each time.  In a fresh child process, as test_gpu_producers does it."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_producers_q80 as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_on_a_live_device(gpu):
    """The table of tests/test_producer80_ref.py with a device behind it (its addresses are never dereferenced: a call that got past
    its checks would fault), then on real buffers: every output keeps its sentinel, and a correct call is served afterwards."""
    import test_producer80_ref as cpu
    L = _hip.lib()
    for what in cpu.INVALID_NORM:
        cpu.test_rms_norm_quantize_b32_refuses(what)
    for what in cpu.INVALID_SWIGLU:
        cpu.test_swiglu_quantize_b32_refuses(what)
    cpu.test_zero_rows_is_ok_and_launches_nothing()
    cpu.test_the_q8k_producers_refuse_the_image()
    cpu.test_mat_mul_entry_points_answer_for_the_image_without_a_device()
    cpu.test_takes_staged_q80_truth_table()
    torch.cuda.synchronize()
    flags = gpu.host_variant_flags()
    n, k, m = 16, 256, 64
    st = _stream()
    x = torch.ones((n, k), dtype=torch.float32, device="cuda")
    size = L.lfamd_staged_q80_size(k, n)
    image, yf, res = _sentinel(size + 64), _sentinel(n * k * 4), _sentinel(n * m * 4)
    none = C.c_void_p(0)
    assert L.lfamd_rms_norm_quantize_b32(_ptr(x), k * 4, none, 1e-5, n, k, Q80I, _ptr(image, 8), 0, _ptr(yf), k * 4, st) == -2
    assert L.lfamd_swiglu_quantize_b32(_ptr(x), k * 4, _ptr(x), k * 4, n, 192, Q80I, _ptr(image), 0, _ptr(yf), k * 4, st) == -2
    assert L.lfamd_rms_norm_quantize(_ptr(x), k * 4, none, 1e-5, n, k, Q80I, _ptr(image), 0, _ptr(yf), k * 4, st) == -2
    W8 = gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 80), m, k)
    W4 = gpu.upload_weights(T.Q4_0, synth.random_weights(T.Q4_0, m, k, 81), m, k)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def mm(W, n_call, img_off=0, fl=0):
        return L.lfamd_mul_mat(W.type, _ptr(W.data), m, k, Q80I, _ptr(image, img_off), 0, n_call, _ptr(res), m, _ptr(ws), ws.numel(), flags | fl, st)

    assert mm(W4, n) == -1 and mm(W8, 8) == -1 and mm(W8, n, fl=_hip.FLAG_Q80_EXACT) == -1 and mm(W8, n, fl=_hip.FLAG_PRECISE) == -1
    assert mm(W8, n, img_off=8) == -2
    torch.cuda.synchronize()
    assert bool((image == SENT).all()) and bool((yf == SENT).all()) and bool((res == SENT).all())
    # and the calls are served once the arguments are right
    assert L.lfamd_rms_norm_quantize_b32(_ptr(x), k * 4, none, 1e-5, n, k, Q80I, _ptr(image), 0, _ptr(yf), k * 4, st) == 0
    assert mm(W8, n) == 0
    torch.cuda.synchronize()
    assert bool((image[size:] == SENT).all()) and not bool((res == SENT).all()) and bool(torch.isfinite(res.view(torch.float32)).all())
