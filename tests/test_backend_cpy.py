"""GGML_OP_CPY through the GPU-module boundary (csrc/ggml_backend_lfamd.hip), driven by tests/backend_host/cpy_host.c: a host whose
operator table names CPY at a number of its own.  What supports_op takes and declines, the off switch, a host whose table lacks the
name; one graph_compute that stores a token's K and V into a cache in the module's buffers and attends over it; and a Q8_0 K store
whose bytes are tests/cpy_ref.py's."""
import os
import subprocess

import numpy as np
import pytest

import cpy_ref as C
import fattn_ref as R
from llamafile_amd import _hip, ggml_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "cpy_host.c")
BASE = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")
EXE = os.path.join(ROOT, "tests", "backend_host", "cpy_host")
D, KVH, HEADS, N_CTX, HEAD, N_KV, MASK_ROWS = 128, 2, 8, 8, 5, 6, 32  # cpy_host.c's cache and node
WIDTH = D * KVH


@pytest.fixture(scope="module")
def host_exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(BASE)):
        subprocess.check_call(["gcc", "-O1", "-Wall", "-o", EXE, SRC, "-ldl", "-lm"])
    return EXE


def supports(host_exe, case, **env):
    r = subprocess.run([host_exe, _hip.HIP_SO, "decline", case], capture_output=True, text=True, timeout=120, env={**os.environ, **env})
    assert r.returncode == 0, (case, r.returncode, r.stderr)
    return r.stdout.strip()


def test_the_host_program_builds(host_exe):
    """(runs without a device: the program compiles against the module's headers)"""
    assert os.path.exists(host_exe)


@pytest.mark.gpu
@pytest.mark.parametrize("case,want", [("control", "accepted"), ("control_f16", "accepted"), ("control_move", "accepted"),
                                       ("control_view_offs", "accepted"), ("dst_q6_k", "declined"), ("src_f16_dst_f32", "declined"),
                                       ("nelements", "declined"), ("ne0_32", "declined"), ("strided_src", "declined"),
                                       ("view_offs_odd", "declined")])
def test_supports_op(gpu, host_exe, case, want):
    assert supports(host_exe, case) == want


@pytest.mark.gpu
def test_the_switch_declines_the_op(gpu, host_exe):
    assert supports(host_exe, "control", LFAMD_BACKEND_NO_CPY="1") == "declined"


@pytest.mark.gpu
def test_a_host_without_the_name_links_and_is_never_offered_the_op(gpu, host_exe):
    assert supports(host_exe, "control", CPY_HOST_NO_NAME="1") == "declined"
    assert supports(host_exe, "control_f16", CPY_HOST_NO_NAME="1") == "declined"


def sentinel_halves(n):
    """Distinct f16 NaNs: a cell the graph should not have read or written shows up in the result or in the read-back."""
    return (np.arange(n, dtype=np.uint32) * 7 % 0x1ff + 0x7e01).astype(np.uint16)


@pytest.mark.gpu
def test_one_graph_stores_k_and_v_and_attends_over_the_cache(gpu, host_exe, tmp_path):
    Q, K, V, mask, _ = R.make_inputs(D, KVH, HEADS // KVH, 1, 1, N_KV, "bias", None, seed=11)
    rng = np.random.default_rng(12)
    k_cur, v_cur = (rng.standard_normal(WIDTH) * 1.5).astype(np.float32), (rng.standard_normal(WIDTH) * 1.5).astype(np.float32)
    caches = []
    for X in (K, V):  # cells 0 .. 4 hold keys / values, the rest the sentinel; memory [cell][kv head][D]
        c = sentinel_halves(N_CTX * WIDTH)
        c[:HEAD * WIDTH] = np.ascontiguousarray(X[0].transpose(1, 0, 2))[:HEAD].reshape(-1).view(np.uint16)
        caches.append(c)
    m_mem = np.zeros((MASK_ROWS, N_KV), np.float16)
    m_mem[:1] = mask.astype(np.float16)
    names = ["kc", "vc", "k", "v", "q", "m", "out", "kc_out", "vc_out"]
    paths = [str(tmp_path / f"{n}.bin") for n in names]
    for a, p in zip((caches[0], caches[1], k_cur, v_cur, np.ascontiguousarray(Q[0].transpose(1, 0, 2)), m_mem), paths):
        a.tofile(p)
    r = subprocess.run([host_exe, _hip.HIP_SO, "store"] + paths, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    assert "ggml_backend_lfamd: 2 cpy calls" in r.stderr and "ggml_backend_lfamd: 1 flash-attn calls" in r.stderr
    # the caches: cell 5 is f16(k_cur) / f16(v_cur), every other byte as it was
    want_caches = []
    for c, cur, p in zip(caches, (k_cur, v_cur), paths[7:9]):
        want = c.copy()
        want[HEAD * WIDTH:(HEAD + 1) * WIDTH] = cur.astype(np.float16).view(np.uint16)
        assert np.array_equal(np.fromfile(p, dtype=np.uint16), want)
        want_caches.append(want)
    # the attention over cells 0 .. 5 of the cache contents computed here, to fattn_ref's tolerance of the n_q <= 8 route
    Kc, Vc = (np.ascontiguousarray(w[:N_KV * WIDTH].view(np.float16).reshape(N_KV, KVH, D).transpose(1, 0, 2))[None] for w in want_caches)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    ref, a = R.ref64(Q, Kc, Vc, mask, scale, "decode")
    got = np.fromfile(paths[6], dtype=np.float32).reshape(1, 1, HEADS, D)
    err = R.row_err(got, ref, a)
    print("attention over the stored cache: err", err, "tol", R.TOL_F32)
    assert np.isfinite(got).all() and err <= R.TOL_F32


@pytest.mark.gpu
@pytest.mark.parametrize("n_tok", [1, 3])
def test_a_q8_0_k_store_has_the_reference_bytes(gpu, host_exe, tmp_path, n_tok):
    rng = np.random.default_rng(20 + n_tok)
    k_cur = (rng.standard_normal(WIDTH * n_tok) * np.exp(rng.uniform(-2, 2, WIDTH * n_tok))).astype(np.float32)
    pk, po = str(tmp_path / "k.bin"), str(tmp_path / "kc.bin")
    k_cur.tofile(pk)
    r = subprocess.run([host_exe, _hip.HIP_SO, "kq8", pk, str(n_tok), po], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    assert "ggml_backend_lfamd: 1 cpy calls" in r.stderr
    row = T.row_size(T.Q8_0, WIDTH)
    before = ((np.arange(N_CTX * row, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8)
    ne = (WIDTH * n_tok, 1, 1, 1)
    want = C.expected_image(before, 2 * row, T.Q8_0, ne, (34, row * n_tok, row * n_tok, row * n_tok), k_cur.view(np.uint8), 0, T.F32,
                            (D, KVH, n_tok, 1), (4, 4 * D, 4 * WIDTH, 4 * WIDTH * n_tok))
    assert np.array_equal(np.fromfile(po, dtype=np.uint8), want)
