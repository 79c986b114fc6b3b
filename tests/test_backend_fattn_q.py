"""GGML_OP_FLASH_ATTN_EXT on a Q8_0 / Q4_0 K and V cache through the GPU-module boundary (csrc/ggml_backend_lfamd.hip), driven by
tests/backend_host/fattn_q_host.c.  What supports_op takes and declines; one graph_compute that stores three tokens' K and V into Q8_0
caches with two CPY nodes and attends over the 65 keys, against the direct lfamd_cpy + lfamd_flash_attn_q calls on the same layouts
(the same bytes: the glue adds no arithmetic) and the reference; the statistics lines; a 775-key decode node through the context's
workspace."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fattn_q_ref as QR
import fattn_ref as R
from batched_case import Dev
from llamafile_amd import _hip, ggml_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "fattn_q_host.c")
BASE = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")
EXE = os.path.join(ROOT, "tests", "backend_host", "fattn_q_host")
D, N_KV, KVH, HEADS, MASK_ROWS, WIDTH, N_CTX, HEAD, N_TOK = 128, 65, 2, 8, 32, 256, 72, 62, 3  # fattn_q_host.c's nodes
ROW = QR.row_bytes(T.Q8_0, D)
CELL = KVH * ROW


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
def test_supports_op_accepts_the_pairs(gpu, host_exe):
    """The Q8_0 pair and the Q4_0 pair, and the same with K a view at a 2-byte-aligned offset."""
    got = {case: supports(host_exe, case) for case in ("q8_0", "q4_0", "q8_0_view2", "q4_0_view2")}
    assert set(got.values()) == {"accepted"}, got


@pytest.mark.gpu
def test_supports_op_declines(gpu, host_exe):
    cases = ("q8_0_k_f16_v", "f16_k_q8_0_v", "q8_0_k_q4_0_v", "q4_1", "d96", "prec_f32", "max_bias", "v_ne1", "view_odd")
    got = {case: supports(host_exe, case) for case in cases}
    assert set(got.values()) == {"declined"}, got


@pytest.mark.gpu
def test_the_switch_declines_the_op(gpu, host_exe):
    got = {case: supports(host_exe, case, LFAMD_BACKEND_NO_FLASH_ATTN="1") for case in ("q8_0", "q4_0")}
    assert set(got.values()) == {"declined"}, got


def arr4(ctype, v):
    return (ctype * 4)(*v)


def direct_attention(dev, t, q_mem, hk, hv, m_mem, n_q, n_kv):
    """lfamd_flash_attn_q on device caches laid out [cell][kv head][row of blocks]: the bits [n_q][HEADS][D]."""
    row = QR.row_bytes(t, D)
    hq, hm = dev.put(q_mem.view(np.uint8).reshape(-1), 0), dev.put(m_mem.view(np.uint8).reshape(-1), 0)
    hd = dev.put(np.full(n_q * HEADS * D * 4, 0xff, np.uint8), 0)
    op_scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    need = dev.lib.lfamd_flash_attn_workspace(D, n_q, n_kv, HEADS, KVH, 1)
    ws = dev.torch.empty(max(need, 16), dtype=dev.torch.uint8, device="cuda")
    rc = dev.lib.lfamd_flash_attn_q(dev.ptr(hq), HEADS * D * 4, D * 4, n_q * HEADS * D * 4, t, dev.ptr(hk), KVH * row, row, n_kv * KVH * row,
                                    t, dev.ptr(hv), KVH * row, row, n_kv * KVH * row, dev.ptr(hm), n_kv * 2, D, n_q, n_kv, HEADS, KVH, 1,
                                    op_scale, 0.0, dev.ptr(hd), D * 4, HEADS * D * 4, n_q * HEADS * D * 4, ws.data_ptr() if need else None, need, 0, None)
    assert rc == 0, _hip.lib().lfamd_last_error()
    return dev.get(hd).view(np.uint32).reshape(n_q, HEADS, D), np.float32(op_scale)


def operands_of(t, cache_bytes, n_kv, route):
    """The cache's first n_kv cells as the route's operands [1][kv heads][n_kv][D]."""
    raw = cache_bytes[:n_kv * KVH * QR.row_bytes(t, D)].reshape(n_kv, KVH, -1).transpose(1, 0, 2)[None]
    return QR.as_route_sees(route, QR.dequantise(t, np.ascontiguousarray(raw)))


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", [3, 17])
def test_one_graph_stores_three_tokens_and_attends_over_the_cache(gpu, host_exe, tmp_path, n_q):
    Q, K, V, mask, _ = R.make_inputs(D, KVH, HEADS // KVH, 1, n_q, N_KV, "causal", None, seed=21 + n_q)
    rng = np.random.default_rng(22)
    k_cur, v_cur = ((rng.standard_normal(WIDTH * N_TOK) * 1.5).astype(np.float32) for _ in range(2))
    caches = []
    for X in (K, V):  # cells 0 .. 61 hold quantised keys / values, the rest 0x7e (a NaN d); memory [cell][kv head][row]
        c = np.full(N_CTX * CELL, 0x7e, np.uint8)
        c[:HEAD * CELL] = QR.quantise(T.Q8_0, np.ascontiguousarray(X[0].transpose(1, 0, 2))[:HEAD]).reshape(-1)
        caches.append(c)
    m_mem = np.zeros((MASK_ROWS, N_KV), np.float16)
    m_mem[:n_q] = mask.astype(np.float16)
    q_mem = np.ascontiguousarray(Q[0].transpose(1, 0, 2))
    names = ["kc", "vc", "k", "v", "q", "m", "out", "kc_out", "vc_out"]
    paths = [str(tmp_path / f"{n}.bin") for n in names]
    for a, p in zip((caches[0], caches[1], k_cur, v_cur, q_mem, m_mem), paths):
        a.tofile(p)
    r = subprocess.run([host_exe, _hip.HIP_SO, "store"] + paths + [str(n_q)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    assert "ggml_backend_lfamd: 2 cpy calls" in r.stderr and "ggml_backend_lfamd: 1 flash-attn calls" in r.stderr
    got = np.fromfile(paths[6], dtype=np.uint32).reshape(n_q, HEADS, D)
    got_caches = [np.fromfile(p, dtype=np.uint8) for p in paths[7:9]]
    # the direct calls on the same layouts: lfamd_cpy of each store, then lfamd_flash_attn_q
    dev = Dev()
    ne, nb = (WIDTH * N_TOK, 1, 1, 1), (34, CELL * N_TOK, CELL * N_TOK, CELL * N_TOK)
    handles = []
    for c, cur, src_ne in zip(caches, (k_cur, v_cur), ((D, KVH, N_TOK, 1), (WIDTH, N_TOK, 1, 1))):
        hc, hs = dev.put(c, 0), dev.put(cur.view(np.uint8), 0)
        src_nb = (4, 4 * src_ne[0], 4 * src_ne[0] * src_ne[1], 4 * WIDTH * N_TOK)
        rc = dev.lib.lfamd_cpy(T.F32, dev.ptr(hs), arr4(ctypes.c_long, src_ne), arr4(ctypes.c_size_t, src_nb), T.Q8_0, dev.ptr(hc) + HEAD * CELL,
                               arr4(ctypes.c_long, ne), arr4(ctypes.c_size_t, nb), 0, None)
        assert rc == 0, _hip.lib().lfamd_last_error()
        handles.append(hc)
    for hc, back in zip(handles, got_caches):
        assert np.array_equal(dev.get(hc), back), "the graph's stores are not the direct lfamd_cpy's bytes"
    direct, scale = direct_attention(dev, T.Q8_0, q_mem, handles[0], handles[1], m_mem, n_q, N_KV)
    assert np.array_equal(got, direct), "the node's result is not the direct call's bytes"
    # and the reference on the cache contents, to the route's tolerance
    route = R.route_of(n_q)
    Kc, Vc = (operands_of(T.Q8_0, c, N_KV, route) for c in got_caches)
    ref, a = R.ref64(Q, Kc, Vc, mask, scale, route)
    err = R.row_err(got.view(np.float32)[None], ref, a)
    tol = R.TOL_F32 if route == "decode" else R.TOL_MMA
    print("attention over the stored cache: err", err, "tol", tol)
    assert np.isfinite(got.view(np.float32)).all() and err <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("t", QR.TYPES, ids=QR.type_name)
def test_graph_compute_of_a_decode_node_through_the_contexts_workspace(gpu, host_exe, tmp_path, t):
    n_q, n_kv = 1, 3 * R.CHUNK + 7  # 775 keys: the split route
    Q, K, V, mask, _ = R.make_inputs(D, KVH, HEADS // KVH, 1, n_q, n_kv, "bias", None, seed=4)
    q_mem = np.ascontiguousarray(Q[0].transpose(1, 0, 2))
    k_mem, v_mem = (QR.quantise(t, np.ascontiguousarray(X[0].transpose(1, 0, 2))).reshape(-1) for X in (K, V))
    m_mem = np.zeros((MASK_ROWS, n_kv), np.float16)
    m_mem[:n_q] = mask.astype(np.float16)
    paths = [str(tmp_path / f"{n}.bin") for n in "qkvmo"]
    for a, p in zip((q_mem, k_mem, v_mem, m_mem), paths):
        a.tofile(p)
    r = subprocess.run([host_exe, _hip.HIP_SO, "run", T.NAMES[t].lower()] + paths + [str(n_q), str(n_kv), str(MASK_ROWS)], capture_output=True,
                       text=True, timeout=300, env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    assert "ggml_backend_lfamd: 1 flash-attn calls" in r.stderr
    got = np.fromfile(paths[4], dtype=np.uint32).reshape(n_q, HEADS, D)
    dev = Dev()
    direct, scale = direct_attention(dev, t, q_mem, dev.put(k_mem, 0), dev.put(v_mem, 0), m_mem, n_q, n_kv)
    assert np.array_equal(got, direct)
    ref, a = R.ref64(Q, operands_of(t, k_mem, n_kv, "decode"), operands_of(t, v_mem, n_kv, "decode"), mask, scale, "decode")
    assert R.row_err(got.view(np.float32)[None], ref, a) <= R.TOL_F32
