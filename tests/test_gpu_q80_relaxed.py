"""GPU: the relaxed-order Q8_0 decode GEMV (LFAMD_FLAG_Q80_RELAXED; csrc/gemv_q80r_impl.h).

Reference: for each output the f64 sum G of its 8 * k / 32 terms t = (f32(dA) * f32(dB)) * dot4, built from the same Q8_0 weights
and the same Q8_0-quantised activations (tests/q80r_ref.py).  Bounds: 2e-6 normwise (helpers.rel_err — the project's figure for
exact-integer bodies, helpers.q80_batch_tol) and |C - G| <= 2e-6 * sum |t| for every element.  The order model of q80r_ref.py
lands ten times inside both (tests/test_q80r_ref.py), so a kernel that adds the right terms in any fixed order passes and one that
drops, doubles or mis-scales a block does not.  The largest matrix is 64 x 14336; the tall ones have k = 128."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
from extremes import extreme_activations, extreme_weights, for_vec_dot
from helpers import rel_err
import q80r_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = _hip.FLAG_Q80_RELAXED
KS = (32, 96, 128, 160, 544, 4096, 4224, 14336)
MS = (1, 7, 8, 9, 40, 64)
NS = (1, 2, 5, 8)
NORM, ELEM = 2e-6, 2e-6
SENTINEL = 12345.5


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


def relaxed_plan(work, k, nc=1, count=1):
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    p = Plan()
    assert L.lfamd_gemv_plan_of(4, T.Q8_0, nc, work, 0, k, count, L.lfamd_num_cus(), C.byref(p)) == 0
    return p


_refs = {}


def case(k, m=64, n=8, seed=0):
    """Weights, f32 activations, their Q8_0 rows and (G, S) for m x k, n columns: computed once, shared, never written."""
    key = (k, m, n, seed)
    if key not in _refs:
        A = synth.random_weights(T.Q8_0, m, k, 700 + k + seed)
        x = synth.random_activations(n, k, 701 + k + seed)
        B = synth.quantize_activations(T.Q8_0, x)
        G, S = q80r_ref.f64_reference(A, B)
        for a in (A, x, B, G, S):
            a.setflags(write=False)
        _refs[key] = (A, x, B, G, S)
    return _refs[key]


def padded_rows(rows_u8, pad=64):
    """[n, row_bytes] on the device with `pad` bytes between the rows: b_row_bytes above the row size."""
    n, rb = rows_u8.shape
    big = torch.zeros((n, rb + pad), dtype=torch.uint8, device="cuda")
    big[:, :rb] = torch.from_numpy(np.array(rows_u8)).cuda()
    return big[:, :rb]


def f32_rows(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1)


def run(gpu, W, rows, bt, n, flags, ldc=None):
    """One lfamd_mul_mat into a pre-filled [n + 1, ldc] buffer; returns the m x n result after checking that nothing else changed."""
    ldc = W.rows + 3 if ldc is None else ldc
    out = torch.full((n + 1, ldc), SENTINEL, dtype=torch.float32, device="cuda")
    gpu.mul_mat(W, rows, bt, n=n, out=out, ldc=ldc, flags=flags)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:n, W.rows:] == SENTINEL).all() and (o[n] == SENTINEL).all(), "bytes outside the m x n result were written"
    return np.ascontiguousarray(o[:n, :W.rows])


def within_bounds(Cn, G, S, what):
    fin = np.isfinite(G) & np.isfinite(S)
    assert fin.any(), what
    assert np.isfinite(Cn[fin]).all(), what
    d = np.abs(Cn.astype(np.float64) - G)
    print(what, "normwise", rel_err(Cn[fin], G[fin]), "elementwise / sum|t|", float((d[fin] / np.maximum(S[fin], 1e-300)).max()))
    assert rel_err(Cn[fin], G[fin]) <= NORM, (what, rel_err(Cn[fin], G[fin]))
    assert (d[fin] <= ELEM * S[fin]).all(), (what, float((d[fin] / np.maximum(S[fin], 1e-300)).max()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("k", KS)
def test_shapes(gpu, k):
    """One block, a partial quad, fewer quads than waves, even and uneven quads per wave, the deep row; m around the 8-row group;
    every column count's kernel; f32 rows and Q8_0 rows, b_row_bytes above the row size, ldc > m, a pre-filled result."""
    A, x, B, G, S = case(k)
    assert lib().lfamd_mul_mat_is_bit_exact(T.Q8_0, 64, k, 1, R) == 0
    flags = gpu.host_variant_flags() | R
    for m in MS:
        W = gpu.upload_weights(T.Q8_0, A[:m].copy(), m, k)
        for n in NS:
            c32 = run(gpu, W, padded_rows(f32_rows(x[:n])), T.F32, n, flags)
            cq = run(gpu, W, padded_rows(B[:n], pad=6), T.Q8_0, n, flags)
            within_bounds(c32, G[:n, :m], S[:n, :m], ("f32 rows", m, k, n))
            within_bounds(cq, G[:n, :m], S[:n, :m], ("Q8_0 rows", m, k, n))


def lib():
    return _hip.lib()


def test_one_two_and_three_items_per_work_group(gpu):
    """m chosen from the plan of this device so that a work-group walks 1, 2 and 3 items (k = 128: the matrices stay small)."""
    k, cus = 128, lib().lfamd_num_cus()
    ms = {1: 8 * cus - 3, 2: 8 * cus + 8, 3: 16 * cus + 5}
    A, x, B, G, S = case(k, m=max(ms.values()), n=2, seed=5)
    flags = gpu.host_variant_flags() | R
    for per_wg, m in ms.items():
        items = (m + 7) // 8
        p = relaxed_plan(items, k)
        assert -(-items // p.grid) == per_wg and p.grid <= cus, (m, p.grid)
        W = gpu.upload_weights(T.Q8_0, A[:m].copy(), m, k)
        for n in (1, 2):
            within_bounds(run(gpu, W, padded_rows(f32_rows(x[:n])), T.F32, n, flags), G[:n, :m], S[:n, :m], ("items per wg", per_wg, n))


# ------------------------------------------------------------------------------------------------------- 2. extreme operands
@pytest.mark.parametrize("real_scale", [False, True], ids=["synth_d", "real_d"])
def test_extreme_operands(gpu, real_scale):
    """tests/extremes.py's Q8_0 weights (negative, zero and subnormal d, codes at both ends) and tokens (1e-7 .. 3e5, zero and
    constant blocks, outliers), as test_gpu_operand_extremes.py feeds the exact kernel: the same G, wherever it is finite."""
    m, k = 200, 1024
    A = extreme_weights(T.Q8_0, m, k, 11, real_scale=real_scale)
    x = for_vec_dot(extreme_activations(16, k, 12), T.Q8_0)
    B = synth.quantize_activations(T.Q8_0, x)
    G, S = q80r_ref.f64_reference(A, B)
    W = gpu.upload_weights(T.Q8_0, A.copy(), m, k)
    flags = gpu.host_variant_flags() | R
    for n in (1, 3, 8):
        for j0 in range(0, 16 - n + 1, n):
            c32 = run(gpu, W, padded_rows(f32_rows(x[j0:j0 + n])), T.F32, n, flags)
            cq = run(gpu, W, padded_rows(np.ascontiguousarray(B[j0:j0 + n])), T.Q8_0, n, flags)
            assert np.array_equal(bits(c32), bits(cq)), (n, j0)
            for j in range(n):  # each token against its own scale
                within_bounds(cq[j:j + 1], G[j0 + j:j0 + j + 1], S[j0 + j:j0 + j + 1], ("extremes", real_scale, n, j0 + j))


# ---------------------------------------------------------------------------------------------------------------- 3. siblings
@pytest.mark.parametrize("count", [2, 3, 4, 6])
@pytest.mark.parametrize("n", [1, 3])
def test_siblings_equal_separate_calls(gpu, count, n):
    """lfamd_mul_mat_multi on matrices of unequal heights, some no multiple of 8: the bits of one lfamd_mul_mat per matrix (the
    plan's waves and chunk depend on k alone, so the order of every sum is the same in both)."""
    k = 544
    ms = [96, 40, 7, 130, 9, 64][:count]
    singles = {(relaxed_plan((m + 7) // 8, k).nw, relaxed_plan((m + 7) // 8, k).ch) for m in ms}
    fused_rgs = sum((m + 7) // 8 for m in ms[:4])
    assert singles == {(relaxed_plan(fused_rgs, k, count=min(count, 4)).nw, relaxed_plan(fused_rgs, k, count=min(count, 4)).ch)}
    As = [synth.random_weights(T.Q8_0, m, k, 800 + i) for i, m in enumerate(ms)]
    Ws = [gpu.upload_weights(T.Q8_0, a, m, k) for a, m in zip(As, ms)]
    x = synth.random_activations(n, k, 801)
    B = synth.quantize_activations(T.Q8_0, x)
    flags = gpu.host_variant_flags() | R
    for rows, bt in ((f32_rows(x), T.F32), (B, T.Q8_0)):
        Bd = torch.from_numpy(np.array(rows)).cuda()
        fused = gpu.mul_mat_multi(Ws, Bd, bt, n=n, flags=flags)
        torch.cuda.synchronize()
        for W, a, f in zip(Ws, As, fused):
            sep = gpu.mul_mat(W, Bd, bt, n=n, flags=flags).cpu().numpy()
            assert np.array_equal(bits(f.cpu().numpy()), bits(sep)), (W.rows, bt)
            G, S = q80r_ref.f64_reference(a, B)
            within_bounds(sep, G, S, ("sibling", W.rows, n))


# -------------------------------------------------------------------------------------------------------------- 4. equal bits
@pytest.mark.parametrize("k", [160, 4096, 14336])
def test_equal_bits(gpu, k):
    m = 64
    A, x, B, G, S = case(k)
    W = gpu.upload_weights(T.Q8_0, A.copy(), m, k)
    flags = gpu.host_variant_flags() | R
    x8, q8 = padded_rows(f32_rows(x)), padded_rows(B)
    c8 = run(gpu, W, x8, T.F32, 8, flags)
    assert np.array_equal(bits(c8), bits(run(gpu, W, x8, T.F32, 8, flags))), "two runs of one call differ"
    assert np.array_equal(bits(c8), bits(run(gpu, W, q8, T.Q8_0, 8, flags))), "f32 rows and their Q8_0 rows differ"
    for c in range(8):  # column c of the n = 8 call == the n = 1 call on that column, in both formats
        assert np.array_equal(bits(c8[c:c + 1]), bits(run(gpu, W, x8[c:c + 1], T.F32, 1, flags))), c
        assert np.array_equal(bits(c8[c:c + 1]), bits(run(gpu, W, q8[c:c + 1], T.Q8_0, 1, flags))), c
    for n in (2, 5):
        assert np.array_equal(bits(c8[:n]), bits(run(gpu, W, x8[:n], T.F32, n, flags))), n
    # m does not enter either: the first 9 rows alone
    W9 = gpu.upload_weights(T.Q8_0, A[:9].copy(), 9, k)
    assert np.array_equal(bits(c8[:, :9]), bits(run(gpu, W9, x8, T.F32, 8, flags)))


def test_the_order_model_gives_the_kernels_bits(gpu):
    """tests/q80r_ref.py states the kernel's order; on rows of every kind of quad count the two agree in all bits."""
    for k in (32, 160, 544, 4224):
        A, x, B, G, S = case(k)
        W = gpu.upload_weights(T.Q8_0, A.copy(), 64, k)
        got = run(gpu, W, padded_rows(B[:2]), T.Q8_0, 2, gpu.host_variant_flags() | R)
        want = q80r_ref.relaxed_model(A, B[:2], relaxed_plan(8, k).nw)
        assert np.array_equal(bits(got), bits(want)), (k, float(np.abs(got - want).max()))


def graph_case():
    """Body of test_graph_replay_equals_eager; runs in a process of its own (see there)."""
    from llamafile_amd import sgemm as gpu
    gpu.init(0)
    k, m, n = 4096, 64, 2
    A, x, B, G, S = case(k)
    W = gpu.upload_weights(T.Q8_0, A.copy(), m, k)
    flags = gpu.host_variant_flags() | R
    Bd = torch.from_numpy(f32_rows(x[:n]).copy()).cuda()
    eager = gpu.mul_mat(W, Bd, T.F32, n=n, flags=flags).cpu().numpy()  # (loads the kernel before the capture)
    out = torch.zeros((n, m), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: one kernel node
        gpu.mul_mat(W, Bd, T.F32, n=n, out=out, flags=flags)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(eager))
    within_bounds(eager, G[:n], S[:n], "graph case")
    print("graph case ok")


def test_graph_replay_equals_eager(gpu):
    """One relaxed call captured with torch.cuda.graph and replayed twice gives the eager call's bits.  In a fresh child process,
    as test_gpu_get_rows.py does it: what a capture leaves behind in torch and the HIP runtime breaks a later test of this process
    that needs three streams side by side on the process's few hardware queues (tests/test_gpu_tp_rehearsal.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_q80_relaxed as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------- 5. it really is the other kernel
def test_the_flag_selects_another_kernel_and_only_where_it_says(gpu):
    k, m = 4096, 64
    A, x, B, G, S = case(k)
    W = gpu.upload_weights(T.Q8_0, A.copy(), m, k)
    hv = gpu.host_variant_flags()
    q1 = padded_rows(B[:1])
    relaxed, exact = run(gpu, W, q1, T.Q8_0, 1, hv | R), run(gpu, W, q1, T.Q8_0, 1, hv)
    within_bounds(relaxed, G[:1], S[:1], "relaxed")
    within_bounds(exact, G[:1], S[:1], "exact")
    assert (bits(relaxed) != bits(exact)).any(), "the relaxed call gave the chain's bits in every output"
    P, X = _hip.FLAG_PRECISE, _hip.FLAG_Q80_EXACT
    assert np.array_equal(bits(run(gpu, W, q1, T.Q8_0, 1, hv | P | R)), bits(run(gpu, W, q1, T.Q8_0, 1, hv | P)))
    assert np.array_equal(bits(run(gpu, W, q1, T.Q8_0, 1, hv | X | R)), bits(exact))
    # n = 9: a batch, the flag is ignored (same body, same bits; 160-weight rows run the bit-exact batch kernel, 4096 the MFMA body)
    x9 = synth.random_activations(9, k, 77)
    B9 = torch.from_numpy(synth.quantize_activations(T.Q8_0, x9)).cuda()
    assert np.array_equal(bits(run(gpu, W, B9, T.Q8_0, 9, hv | R)), bits(run(gpu, W, B9, T.Q8_0, 9, hv)))
    A2, _, _, _, _ = case(160)
    W2 = gpu.upload_weights(T.Q8_0, A2.copy(), m, 160)
    B92 = torch.from_numpy(synth.quantize_activations(T.Q8_0, synth.random_activations(9, 160, 78))).cuda()
    assert np.array_equal(bits(run(gpu, W2, B92, T.Q8_0, 9, hv | R)), bits(run(gpu, W2, B92, T.Q8_0, 9, hv)))


# ------------------------------------------------------------------------------------------------------------- 6. host shim
def test_host_shim_reads_the_switch(gpu, tmp_path):
    """LFAMD_Q80_RELAXED=1 in the environment of a FRESH child process (the shim reads it once, when it loads the module): its
    llamafile_sgemm Q8_0 vecdot is lfamd_mul_mat with the flag, bit for bit; without the variable it is the bit-exact chain."""
    m, n, k = 64, 1, 4096
    A, x, B, G, S = case(k)
    np.save(tmp_path / "A.npy", A)
    np.save(tmp_path / "B.npy", np.ascontiguousarray(B[:n]))
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("LFAMD_Q80_RELAXED", "LFAMD_Q80_EXACT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    got = {}
    for name, extra in (("relaxed", {"LFAMD_Q80_RELAXED": "1"}), ("default", {})):
        out = tmp_path / f"{name}.npy"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "q80r_shim_child.py"), str(tmp_path / "A.npy"), str(tmp_path / "B.npy"),
                            str(out), str(m), str(n), str(k)], env={**env, **extra}, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = np.load(out)
    W = gpu.upload_weights(T.Q8_0, A.copy(), m, k)
    hv = gpu.host_variant_flags()
    Bd = torch.from_numpy(np.array(B[:n])).cuda()
    within_bounds(got["relaxed"], G[:n], S[:n], "shim, relaxed")
    assert np.array_equal(bits(got["relaxed"]), bits(run(gpu, W, Bd, T.Q8_0, n, hv | R)))
    assert np.array_equal(bits(got["default"]), bits(run(gpu, W, Bd, T.Q8_0, n, hv)))
    assert (bits(got["relaxed"]) != bits(got["default"])).any()
