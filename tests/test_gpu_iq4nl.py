"""IQ4_NL (ggml type 20) on the device: pack / unpack, get_rows, the decode GEMV, the 128 x 128 MFMA batches, RAW rows through the
generic kernel, sibling matrices, MUL_MAT_ID and the ggml backend interface, against tests/iq4nl_ref.py (the CPU oracle does not
know the type).

Bounds.  Every body is exact integer block dots with f32 scale products, so a result differs from iq4nl_ref.dot_ref only by the
order of its f32 sums: 2e-6 normwise (test_gpu_parity.DEFAULT_TOL) and no element beyond helpers.elem_err's rtol 1e-5, the rule
of the exact bodies (test_gpu_gemm_i8.py).  Extreme operands are judged by that rule on the whole sample and, token by token, by
test_gpu_operand_extremes.check (each token against its own scale, plus the rounding of the summed terms where they cancel)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
import extremes
import iq4nl_ref as R
from helpers import elem_err, rel_err
from test_gpu_operand_extremes import check as check_tokens, sample_rows, sample_tokens

pytestmark = pytest.mark.gpu

NL = T.IQ4_NL
RAW_K = (288, 2080, 4000)  # row lengths that are not whole 256-weight groups: what an IQ4_XS file stores as IQ4_NL
TOL = 2e-6
SENT = 0x5A
DT = {"F32": (torch.float32, np.uint32), "F16": (torch.float16, np.uint16)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights(m, k, gen="plain", seed=31):
    return synth.random_weights(NL, m, k, seed) if gen == "plain" else R.extreme_weights(m, k, seed)


def tokens(n, k, gen="plain", seed=32):
    return synth.random_activations(n, k, seed) if gen == "plain" else extremes.extreme_activations(n, k, seed)


def run(gpu, W, x, f32in, n=None, flags=None, ldc=None, out=None):
    n = x.shape[0] if n is None else n
    if f32in:
        B, bt = torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.uint8).view(x.shape[0], -1), T.F32
    else:
        B, bt = torch.from_numpy(R.activations(x)).cuda(), T.Q8_0
    c = gpu.mul_mat(W, B, bt, n=n, flags=flags, ldc=ldc, out=out)
    torch.cuda.synchronize()
    return c.cpu().numpy()


def judge(C, raw, x, gen, what):
    """C: f32 [n, m] of the call.  A row x token sample against dot_ref."""
    m, k = raw.shape[0], x.shape[1]
    rows, cols = sample_rows(m), sample_tokens(x.shape[0])
    sub = np.ascontiguousarray(raw[rows])
    G = R.dot_ref(sub, R.activations(x[cols]))
    Cs = C[np.ix_(cols, rows)]
    assert np.isfinite(Cs).all(), what
    err = rel_err(Cs, G)
    frac, worst = elem_err(Cs, G, rtol=1e-5)
    print(f"IQ4_NL {what}: normwise {err:.3e}, elements over rtol 1e-5: {frac}, worst {worst:.3e}")
    assert err <= TOL, (what, err)
    assert frac == 0.0, (what, frac, worst)
    if gen == "extreme":
        xs = np.abs(x[cols]).astype(np.float64)
        xs += xs.max(axis=1, keepdims=True) / 127.0
        ap = xs @ np.abs(R.dequantize(sub)).astype(np.float64).T
        check_tokens(Cs, G, cols, rows, True, what, absprod=ap, k=k)
        small = rows % 8 != R.BAND_BIG  # ... and the ordinary rows without the |d| = 65504 ones in their rms
        check_tokens(Cs[:, small], G[:, small], cols, rows[small], True, what, absprod=ap[:, small], k=k)


# ------------------------------------------------------------------------------------------------------------------------
# pack / unpack

@pytest.mark.parametrize("m,k", [(67, 256), (128, 4096), (33, 14336), (64, 288), (67, 2080), (40, 4000)])
@pytest.mark.parametrize("gen", ["plain", "extreme"])
def test_pack_is_q40s_image_and_unpack_inverts_it(gpu, m, k, gen):
    raw = weights(m, k, gen)
    W = gpu.upload_weights(NL, raw, m, k)
    W40 = gpu.upload_weights(T.Q4_0, raw, m, k)
    assert W.data.numel() == W40.data.numel() == _hip.lib().lfamd_packed_size(NL, m, k) > 0
    assert torch.equal(W.data, W40.data)  # the nibbles are indices instead of codes: the same bytes in the same places
    back = gpu.unpack_weights(W)
    assert np.array_equal(back.cpu().numpy(), raw)
    assert torch.equal(gpu.upload_weights(NL, back, m, k).data, W.data)  # pack(unpack(pack)) = pack
    if k % 256:
        assert np.array_equal(W.data.cpu().numpy().reshape(m, -1), raw)  # RAW: the GGUF rows


@pytest.mark.parametrize("k", [1024, 288])
def test_pack_reads_strided_raw_rows(gpu, k):
    m, rb = 45, T.row_size(NL, k)
    raw = weights(m, k)
    wide = np.full((m, rb + 30), SENT, dtype=np.uint8)
    wide[:, :rb] = raw
    src = torch.from_numpy(wide).cuda()
    L = _hip.lib()
    size = L.lfamd_packed_size(NL, m, k)
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lfamd_pack_weights(NL, m, k, C.c_void_p(src.data_ptr()), rb + 30, C.c_void_p(out.data_ptr()), st) == 0
    back = torch.full((m, rb + 7), SENT, dtype=torch.uint8, device="cuda")
    assert L.lfamd_unpack_weights(NL, m, k, C.c_void_p(out.data_ptr()), C.c_void_p(back.data_ptr()), rb + 7, st) == 0
    torch.cuda.synchronize()
    b = back.cpu().numpy()
    assert np.array_equal(b[:, :rb], raw) and (b[:, rb:] == SENT).all()
    assert L.lfamd_pack_weights(NL, m, k, C.c_void_p(src.data_ptr()), rb - 1, C.c_void_p(out.data_ptr()), st) == -2  # stride below a row


# ------------------------------------------------------------------------------------------------------------------------
# get_rows

def want_bits(raw, dt):
    with np.errstate(over="ignore"):
        w = R.dequantize(raw)
        return w.view(np.uint32) if dt == "F32" else w.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m,k", [(33, 256), (67, 1024), (128, 4096), (8200, 512), (64, 288), (67, 2080), (40, 4000)])
def test_whole_matrix_dequantisation_bit_for_bit(gpu, m, k, gen, dt):
    raw = weights(m, k, gen)
    W = gpu.upload_weights(NL, raw, m, k)
    got = gpu.dequantize(W, DT[dt][0]).cpu().numpy().view(DT[dt][1])
    want = want_bits(raw, dt)
    bad = int((got != want).sum())
    print(f"IQ4_NL get_rows {m} x {k} {gen} {dt}: {bad} of {want.size} differ")
    assert got.shape == want.shape and bad == 0


@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("k", [1024, 2080])
def test_index_lists_ranges_and_padded_outputs(gpu, k, dt):
    rows = 67
    raw = weights(rows, k, "extreme")
    W = gpu.upload_weights(NL, raw, rows, k)
    want = want_bits(raw, dt)
    tdt, ndt = DT[dt]
    esz = np.dtype(ndt).itemsize
    sent = int.from_bytes(bytes([SENT]) * esz, "little")
    idx = [66, 0, 5, 5, 64, -1, 31, 32, 65, rows, 0, 66, 17]  # repeats, the ragged last tile, two ids outside [0, rows)
    ids = torch.tensor(idx, dtype=torch.int32, device="cuda")
    pad = 24
    out = torch.full((len(idx), (k + pad) * esz), SENT, dtype=torch.uint8, device="cuda").view(tdt)
    gpu.get_rows(W, ids, tdt, out=out)
    got = out.cpu().numpy().view(ndt)
    for s, r in enumerate(idx):
        if 0 <= r < rows:
            assert (got[s, :k] == want[r]).all(), (s, r)
        else:
            assert (got[s, :k] == sent).all(), (s, r)
    assert (got[:, k:] == sent).all()
    for row0, n in ((29, rows - 29), (3, 5), (0, rows)):  # longer and shorter than a tile, the whole matrix
        got = gpu.get_rows(W, None, tdt, row0=row0, n=n).cpu().numpy().view(ndt)
        assert (got == want[row0:row0 + n]).all(), (row0, n)
    flat = torch.full(((rows * (k + 1) + 1) * esz,), SENT, dtype=torch.uint8, device="cuda").view(tdt)  # unaligned base and stride
    gpu.get_rows(W, None, tdt, out=flat[1:].view(rows, k + 1))
    g2 = flat.cpu().numpy().view(ndt)
    assert (g2[1:].reshape(rows, k + 1)[:, :k] == want).all()
    assert g2[0] == sent and (g2[1:].reshape(rows, k + 1)[:, k] == sent).all()


# ------------------------------------------------------------------------------------------------------------------------
# decode, n <= 8

DECODE = [(m, k) for k in (256, 1024, 4096, 14336) for m in (16, 67, 4096, 8200)] + [(67, k) for k in RAW_K] + [(4096, 288)]


@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m,k", DECODE, ids=lambda v: str(v))
def test_decode_every_column_count(gpu, m, k, gen):
    raw = weights(m, k, gen)
    W = gpu.upload_weights(NL, raw, m, k)
    x8 = tokens(8, k, gen)
    for n in range(1, 9):
        x = x8[:n]  # (extremes.KINDS go by token index)
        assert _hip.lib().lfamd_mul_mat_is_exact(NL, m, k, n, 0) == 1
        c_f = run(gpu, W, x, True)
        c_q = run(gpu, W, x, False)
        judge(c_f, raw, x, gen, f"decode {m} x {k} n={n} f32")
        judge(c_q, raw, x, gen, f"decode {m} x {k} n={n} q8_0")
        both = rel_err(c_f, c_q)  # fused and separate staging of the same activations
        assert both <= 1e-6, (m, k, n, both)


@pytest.mark.parametrize("k", [1024, 14336, 288])
def test_decode_leaves_the_slack_of_a_wider_result_alone(gpu, k):
    m, n, ldc = 67, 3, 67 + 9
    raw = weights(m, k)
    W = gpu.upload_weights(NL, raw, m, k)
    x = tokens(n, k)
    for f32in in (True, False):
        out = torch.full((n, ldc), float("nan"), dtype=torch.float32, device="cuda")
        c = run(gpu, W, x, f32in, ldc=ldc, out=out)
        assert np.isnan(c[:, m:]).all()
        judge(c[:, :m], raw, x, "plain", f"decode ldc {k} f32in={f32in}")


def test_decode_full_size_output_matrix(gpu):
    """128256 x 4096, one token: the long walk (63 half-tiles per work-group), in the item form the plan picks for the type."""
    m, k = 128256, 4096
    raw = synth.random_weights_torch(NL, m, k, 5)
    W = gpu.upload_weights(NL, raw, m, k)
    x = tokens(1, k)
    c_f, c_q = run(gpu, W, x, True), run(gpu, W, x, False)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(64, m, 997), np.arange(m - 64, m)]))
    G = R.dot_ref(raw[torch.from_numpy(rows).cuda()].cpu().numpy(), R.activations(x))
    for c in (c_f, c_q):
        err = rel_err(c[:, rows], G)
        frac, worst = elem_err(c[:, rows], G, rtol=1e-5)
        print(f"IQ4_NL decode 128256 x 4096: normwise {err:.3e} worst element {worst:.3e}")
        assert err <= TOL and frac == 0.0, (err, frac, worst)
    assert rel_err(c_f, c_q) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# batches, n > 8

@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("n", [9, 24, 33, 128, 512])
@pytest.mark.parametrize("m,k", [(67, 256), (300, 4096), (130, 14336), (4099, 1024)], ids=lambda v: str(v))
def test_batches_on_the_mfma_body(gpu, m, k, n, gen):
    raw = weights(m, k, gen)
    W = gpu.upload_weights(NL, raw, m, k)
    x = tokens(n, k, gen)
    assert _hip.lib().lfamd_mul_mat_is_exact(NL, m, k, n, 0) == 1
    for f32in in (True, False):
        judge(run(gpu, W, x, f32in), raw, x, gen, f"batch {m} x {k} n={n} f32in={f32in}")


@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("k", RAW_K)
@pytest.mark.parametrize("n", [9, 40])
def test_raw_row_lengths_run_the_generic_kernel(gpu, k, n, gen):
    m = 67
    raw = weights(m, k, gen)
    W = gpu.upload_weights(NL, raw, m, k)
    x = tokens(n, k, gen)
    assert _hip.lib().lfamd_mul_mat_is_exact(NL, m, k, n, 0) == 1
    for f32in in (True, False):
        c = run(gpu, W, x, f32in)
        judge(c, raw, x, gen, f"generic {m} x {k} n={n} f32in={f32in}")
        forced = run(gpu, W, x, f32in, flags=gpu.host_variant_flags() | _hip.FLAG_FORCE_GENERIC)
        assert np.array_equal(c.view(np.uint32), forced.view(np.uint32))  # RAW rows: the flag changes nothing


def test_force_generic_is_refused_on_the_packed_image(gpu):
    m, k = 64, 512
    W = gpu.upload_weights(NL, weights(m, k), m, k)
    for n in (1, 20):
        with pytest.raises(_hip.LfamdError):  # as for Q4_0: the P40 image is not a layout the generic kernels read
            run(gpu, W, tokens(n, k), True, flags=_hip.FLAG_FORCE_GENERIC)


# ------------------------------------------------------------------------------------------------------------------------
# siblings, experts, the backend interface, the host plug-in

@pytest.mark.parametrize("n", [1, 64])
def test_three_sibling_matrices_against_separate_calls(gpu, n):
    k, ms = 1024, [96, 40, 130]
    raws = [weights(m, k, seed=60 + i) for i, m in enumerate(ms)]
    Ws = [gpu.upload_weights(NL, r, m, k) for r, m in zip(raws, ms)]
    x = tokens(n, k)
    xd = torch.from_numpy(x).cuda().view(torch.uint8).view(n, -1)
    fused = gpu.mul_mat_multi(Ws, xd, T.F32, n=n)
    for W, r, f in zip(Ws, raws, fused):
        sep = gpu.mul_mat(W, xd, T.F32, n=n).cpu().numpy()
        f = f.cpu().numpy()
        if n == 1:  # one fused GEMV launch: its wave layout may differ from the lone matrix's (f32 sum order)
            assert rel_err(f, sep) <= 1e-6
        else:       # one call per matrix: the same launches
            assert np.array_equal(f.view(np.uint32), sep.view(np.uint32))
        judge(f, r, x, "plain", f"multi n={n} m={W.rows}")


@pytest.mark.parametrize("tokens_,tasks", [(1, 1), (1, 2), (5, 1), (5, 2)])
def test_mul_mat_id_gathers_per_expert(gpu, tokens_, tasks):
    rows, cols, experts, thinkers = 96, 512, 8, 2
    Ws = [weights(rows, cols, seed=900 + e) for e in range(experts)]
    packed = torch.cat([gpu.upload_weights(NL, W, rows, cols).data for W in Ws])
    x = synth.random_activations(tokens_ * tasks, cols, 77)
    xq = R.activations(x)
    plan = np.random.default_rng(5).integers(0, experts, size=(tokens_, thinkers)).astype(np.int32)
    if tokens_ > 1:
        plan[-1, -1] = experts + 3  # out of range: its result row stays untouched
    res = gpu.mul_mat_id(packed, NL, rows, cols, experts, torch.from_numpy(xq).cuda(), T.Q8_0, tasks, tokens_,
                         torch.from_numpy(plan).cuda(), thinkers, prefill=-7.0)
    torch.cuda.synchronize()
    res = res.cpu().numpy()
    for tok in range(tokens_):
        for th in range(thinkers):
            ex = int(plan[tok, th])
            if ex >= experts:
                assert (res[tok, th] == -7.0).all()
                continue
            row = tok * tasks + th % tasks
            G = R.dot_ref(Ws[ex], xq[row:row + 1])
            assert rel_err(res[tok, th], G[0]) <= TOL, (tok, th)
            frac, worst = elem_err(res[tok, th], G[0], rtol=1e-5)
            assert frac == 0.0, (tok, th, worst)


@pytest.fixture(scope="module")
def host_exes():
    d = os.path.join(ROOT, "tests", "backend_host")
    out = []
    for name in ("backend_host", "backend_host_iq4nl"):
        exe, src = os.path.join(d, name), os.path.join(d, name + ".c")
        newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(d, "backend_host.c")))
        if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
            subprocess.check_call(["gcc", "-O1", "-Wall", "-o", exe, src, "-ldl"])
        out.append(exe)
    return out


@pytest.mark.parametrize("m,k,n", [(96, 1024, 1), (160, 768, 64), (64, 288, 3)], ids=lambda v: str(v))
def test_mul_mat_node_through_the_backend_interface(gpu, host_exes, tmp_path, m, k, n):
    """A host whose type table names "iq4_nl" is served (f32 src1, quantised on the device to Q8_0); one that does not know type 20
    still links, and supports_op declines the tensor (the host program's exit code 11)."""
    old_host, host = host_exes
    raw, x = weights(m, k, seed=7), tokens(n, k, seed=8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    raw.tofile(wp)
    x.tofile(xp)
    args = [_hip.HIP_SO, "mulmat", str(NL), str(m), str(k), str(n), "1", str(wp), str(xp), str(op)]
    r = subprocess.run([host] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    got = np.fromfile(op, dtype=np.float32).reshape(n, m)
    judge(got, raw, x, "plain", f"backend {m} x {k} n={n}")
    r = subprocess.run([old_host] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 11, (r.returncode, r.stderr)


def test_the_host_plug_in_declines_the_type_like_the_reference(gpu):
    """llamafile_sgemm's table is the reference's x86 table, which has no IQ4_NL: false, and ggml's own vec_dot runs."""
    lib = C.CDLL(_hip.HOST_SO)
    lib.llamafile_sgemm.restype = C.c_bool
    lib.llamafile_sgemm.argtypes = [C.c_long] * 3 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long] + [C.c_int] * 5
    A, B = weights(4, 256), R.activations(tokens(1, 256))
    Cm = np.full((1, 4), 3.0, dtype=np.float32)
    assert not lib.llamafile_sgemm(4, 1, 8, A.ctypes.data, 8, B.ctypes.data, 8, Cm.ctypes.data, 4, 0, 1, NL, T.Q8_0, T.F32)
    assert not lib.llamafile_sgemm(4, 1, 8, A.ctypes.data, 8, B.ctypes.data, 8, Cm.ctypes.data, 4, 0, 1, NL, T.F32, T.F32)
    assert (Cm == 3.0).all()
    A40 = synth.random_weights(T.Q4_0, 4, 256, 1)
    assert lib.llamafile_sgemm(4, 1, 8, A40.ctypes.data, 8, B.ctypes.data, 8, Cm.ctypes.data, 4, 0, 1, T.Q4_0, T.Q8_0, T.F32)
