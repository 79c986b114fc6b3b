"""The ggml backend routes a MUL_MAT node whose src0 is a 32-block tensor OUTSIDE a weights buffer, under several src1 slices — KQ on a
quantised K cache — to ONE lfamd_mul_mat_batched_q call (csrc/ggml_backend_lfamd.hip: run_mul_mat); weights buffers, K-quants and
LFAMD_BACKEND_NO_BATCHED=1 keep the routes they had.  Driven from the C host program that plays llamafile's side
(tests/backend_host/backend_host.c): mode `mulmat <t> 48 128 <n> 3` is src0 [48][128] under three src1 slices; the program computes the
graph four times and between them clears the buffer, expects exact zeros and uploads the tensor again, so a stale private copy of
src0 would show.  (The multi-KV-head permuted layout is covered at the C ABI, tests/test_gpu_mul_mat_batched_q.py: the host program's
`attn` mode is F16-only.)"""
import os
import subprocess

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
from helpers import rel_err
import block32_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")
M, K, NB2 = 48, 128, 3


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("backend_host") / "backend_host")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-o", exe, SRC, "-ldl"])
    return exe


def mulmat(host_exe, tmp_path, t, m, k, n, nb2, env):
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp), x.tofile(xp)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), str(nb2), str(wp), str(xp), str(op)],
                       capture_output=True, text=True, timeout=300, env={**os.environ, "LFAMD_BACKEND_STATS": "1", **env})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    return r, W, x, np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m)


def block_k_calls(r):
    calls = [int(line.split()[1]) for line in r.stderr.splitlines() if line.endswith("block-K calls")]
    assert len(calls) == 1, r.stderr
    return calls[0]


ORDINARY = {"BACKEND_HOST_NO_WEIGHTS_USAGE": "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_0, T.Q5_1], ids=lambda t: T.NAMES[t])
def test_block_src0_in_an_ordinary_buffer_is_one_call(gpu, oracle, host_exe, tmp_path, t, n):
    bt = T.VEC_DOT[t]
    r, W, x, got = mulmat(host_exe, tmp_path, t, M, K, n, NB2, ORDINARY)
    assert block_k_calls(r) == 4, r.stderr  # one per graph run
    # the two earlier lines are still there, unchanged
    assert "ggml_backend_lfamd: 0 batched calls" in r.stderr and "sibling calls" in r.stderr, r.stderr
    for s in range(NB2):
        Bq = oracle.quantize(bt, x[s * n:(s + 1) * n])
        G = oracle.f64_gemm(t, W, bt, Bq, M, n, K)
        room = 0.0
        if t == T.Q5_1:  # (f64_gemm takes s without its f16 rounding: tests/block32_ref.py; the call's own sums, and f64_gemm within that room)
            room = block32_ref.stored_s_allowance(t, W, Bq) / np.abs(G).max()
            assert rel_err(got[s * n:(s + 1) * n], block32_ref.sums_ref(t, W, Bq)) <= 2e-6
        e = rel_err(got[s * n:(s + 1) * n], G)
        print(T.NAMES[t], n, s, "%.3g" % e, "room %.3g" % room)
        assert e <= 2e-6 + room
    # LFAMD_BACKEND_NO_BATCHED=1: the loop over the slices, within its own bounds (check_mul_mat of tests/test_backend_glue.py)
    r, W, x, got = mulmat(host_exe, tmp_path, t, M, K, n, NB2, {**ORDINARY, "LFAMD_BACKEND_NO_BATCHED": "1"})
    assert block_k_calls(r) == 0, r.stderr
    v = oracle.variant("zen4")
    for s in range(NB2):
        ok, G = oracle.sgemm(t, W, bt, synth.quantize_activations(bt, x[s * n:(s + 1) * n]), M, n, K, v=v)
        assert ok == 1
        g = got[s * n:(s + 1) * n]
        if t == T.Q8_0 and n <= 8:
            assert np.array_equal(g.view(np.uint32), G.view(np.uint32))
        else:
            assert rel_err(g, G) <= (1e-3 if n > 8 else 2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_0], ids=lambda t: T.NAMES[t])
def test_weights_buffers_keep_their_resident_image(gpu, host_exe, tmp_path, t):
    r, _, _, _ = mulmat(host_exe, tmp_path, t, M, K, 5, NB2, {})
    assert block_k_calls(r) == 0, r.stderr


@pytest.mark.gpu
def test_k_quants_keep_their_route(gpu, host_exe, tmp_path):
    r, _, _, _ = mulmat(host_exe, tmp_path, T.Q4_K, 64, 512, 3, 2, ORDINARY)
    assert block_k_calls(r) == 0, r.stderr
    assert "ggml_backend_lfamd: 0 batched calls" in r.stderr, r.stderr
