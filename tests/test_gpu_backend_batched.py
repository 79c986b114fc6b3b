"""The ggml backend routes an F16 MUL_MAT node with several src1 slices — the attention products KQ and KQV — to ONE
lfamd_mul_mat_batched call (csrc/ggml_backend_lfamd.hip: run_mul_mat); LFAMD_BACKEND_NO_BATCHED=1 restores the loop over the
slices.  Driven from the C host program that plays llamafile's side (tests/backend_host/backend_host.c)."""
import os
import subprocess

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
from helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("backend_host") / "backend_host")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-o", exe, SRC, "-ldl"])
    return exe


def run_host(host_exe, args, env):
    r = subprocess.run([host_exe, _hip.HIP_SO] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1", **env})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    return r


def check_f16_rule(got, W16, x, n):
    """The F16 rule of the backend's mat-mul nodes: ggml hands f16 weights their activations rounded to f16 (n > 2) or as f32; the
    module keeps f32 activations for n <= 8 — at least as accurate.  So: within 2e-6 of one of the two f64 products, and within 1e-3
    of the f16-activation one.  got [n][m], W16 f16 [m][k], x f32 [n][k]."""
    W = W16.astype(np.float64)
    G16 = x.astype(np.float16).astype(np.float64) @ W.T
    G32 = x.astype(np.float64) @ W.T
    assert min(rel_err(got, G16), rel_err(got, G32)) <= 2e-6 and rel_err(got, G16) <= 1e-3, (rel_err(got, G16), rel_err(got, G32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("group", [1, 4])
def test_attention_node_is_one_batched_call(gpu, host_exe, tmp_path, group, n):
    """KQ as llama.cpp builds it (permuted F16 K cache, permuted Q, `group` query heads per KV head): one batched call per graph
    run (the host program computes the graph twice); with LFAMD_BACKEND_NO_BATCHED=1 none, and the same rule for the results."""
    k, n_kv, kv_heads = 128, 96, 2
    heads = kv_heads * group
    rng = np.random.default_rng(60 + group + n)
    K = (rng.random((n_kv, kv_heads, k), dtype=np.float32) * 2 - 1).astype(np.float16)
    Q = (rng.random((n, heads, k), dtype=np.float32) * 2 - 1).astype(np.float32)
    kp, qp, op = tmp_path / "k.bin", tmp_path / "q.bin", tmp_path / "o.bin"
    K.tofile(kp), Q.tofile(qp)
    for env, calls in (({}, 2), ({"LFAMD_BACKEND_NO_BATCHED": "1"}, 0)):
        r = run_host(host_exe, ["attn", k, n_kv, kv_heads, heads, n, kp, qp, op], env)
        assert f"ggml_backend_lfamd: {calls} batched calls" in r.stderr, r.stderr
        got = np.fromfile(op, dtype=np.float32).reshape(heads, n, n_kv)
        for h in range(heads):
            check_f16_rule(got[h], K[:, h // group, :], Q[:, h, :], n)


@pytest.mark.gpu
def test_the_switch_is_on_for_a_number_other_than_zero(gpu, host_exe, tmp_path):
    """The truth rule of every LFAMD_* switch of the backend (env_on): LFAMD_BACKEND_NO_BATCHED=0 leaves the batched call in, =1
    takes it out."""
    k, n_kv, kv_heads, heads, n = 128, 96, 2, 2, 1
    rng = np.random.default_rng(7)
    K = (rng.random((n_kv, kv_heads, k), dtype=np.float32) * 2 - 1).astype(np.float16)
    Q = (rng.random((n, heads, k), dtype=np.float32) * 2 - 1).astype(np.float32)
    kp, qp, op = tmp_path / "k.bin", tmp_path / "q.bin", tmp_path / "o.bin"
    K.tofile(kp), Q.tofile(qp)
    for value, calls in (("0", 2), ("1", 0)):
        r = run_host(host_exe, ["attn", k, n_kv, kv_heads, heads, n, kp, qp, op], {"LFAMD_BACKEND_NO_BATCHED": value})
        assert f"ggml_backend_lfamd: {calls} batched calls" in r.stderr, (value, r.stderr)


def _mulmat(host_exe, tmp_path, t, m, k, n, nb2):
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp), x.tofile(xp)
    r = run_host(host_exe, ["mulmat", t, m, k, n, nb2, wp, xp, op], {})
    return r, W, x, np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m)


@pytest.mark.gpu
def test_f16_weights_under_broadcast_slices_take_the_batched_call(gpu, host_exe, tmp_path):
    """src0 one F16 slice, src1 three: r2 = 3 heads over one matrix."""
    m, k, n, nb2 = 48, 256, 5, 3
    r, W, x, got = _mulmat(host_exe, tmp_path, T.F16, m, k, n, nb2)
    calls = [int(line.split()[1]) for line in r.stderr.splitlines() if line.endswith("batched calls")]
    assert calls and calls[0] >= 1, r.stderr
    W16 = np.ascontiguousarray(W).view(np.float16).reshape(m, k)
    for s in range(nb2):
        check_f16_rule(got[s * n:(s + 1) * n], W16, x[s * n:(s + 1) * n], n)


@pytest.mark.gpu
def test_quantised_weights_keep_their_route(gpu, host_exe, tmp_path):
    r, _, _, _ = _mulmat(host_exe, tmp_path, T.Q4_K, 64, 512, 3, 2)
    assert "ggml_backend_lfamd: 0 batched calls" in r.stderr, r.stderr
