"""GGML_OP_FLASH_ATTN_EXT through the GPU-module boundary (csrc/ggml_backend_lfamd.hip), driven by tests/backend_host/fattn_host.c:
a host whose operator table names FLASH_ATTN_EXT at a number of its own.  What supports_op takes and declines, one graph_compute of
a grouped-query node against the direct lfamd_flash_attn call on the same operands (the same bytes: the glue adds no arithmetic),
the statistics line, the off switch, and a host whose table lacks the name."""
import os
import subprocess

import numpy as np
import pytest

import fattn_ref as R
from batched_case import Dev
from llamafile_amd import _hip, ggml_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "fattn_host.c")
BASE = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")
EXE = os.path.join(ROOT, "tests", "backend_host", "fattn_host")
D, N_Q, N_KV, KVH, HEADS, MASK_ROWS = 128, 17, 65, 2, 8, 32  # fattn_host.c's node


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
@pytest.mark.parametrize("case,want", [("control", "accepted"), ("control_nomask", "accepted"), ("control_view_offs16", "accepted"),
                                       ("d96", "declined"), ("max_bias", "declined"), ("prec_f32", "declined"), ("q4_0_k", "declined"),
                                       ("view_offs", "declined")])
def test_supports_op(gpu, host_exe, case, want):
    assert supports(host_exe, case) == want


@pytest.mark.gpu
def test_the_switch_declines_the_op(gpu, host_exe):
    assert supports(host_exe, "control", LFAMD_BACKEND_NO_FLASH_ATTN="1") == "declined"


@pytest.mark.gpu
def test_a_host_without_the_name_links_and_is_never_offered_the_op(gpu, host_exe):
    assert supports(host_exe, "control", FATTN_HOST_NO_NAME="1") == "declined"
    assert supports(host_exe, "control_nomask", FATTN_HOST_NO_NAME="1") == "declined"


# each the accepted 'control' node with one change: what flash_attn_supported (csrc/ggml_backend_lfamd.hip) reads from ggml's structs,
# and what it leaves to lfamd_flash_attn_check (heads_3kv, slices, mask_nb1_odd, k_nb1_8; q_nb1_short and k_nb1_short: rows half a row
# apart, multiples of 16 — nodes that graph_compute would fail)
ONE_CHANGE = ["q_f16", "v_f32", "dst_f16", "q_nb0", "dst_strided", "v_ne1", "v_ne2", "k_ne3", "heads_3kv", "slices", "dst_ne1", "mask_f32",
              "mask_ne0", "mask_ne1", "mask_ne2", "mask_nb1_odd", "k_nb1_8", "q_nb1_short", "k_nb1_short"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ONE_CHANGE)
def test_supports_op_declines_the_control_node_with_one_change(gpu, host_exe, case):
    assert supports(host_exe, case) == "declined"


def graph_nodes(host_exe, tmp_path, shapes, explicit=True):
    """One graph_compute of one node per (n_q, n_kv, mask rows, mask kind, seed) through fattn_host; explicit=False: the program's
    default node, no dimensions on the command line.  Per node: the results' bits [n_q][HEADS][D] and the inputs; and stderr."""
    argv, nodes = [], []
    for i, (n_q, n_kv, rows, kind, seed) in enumerate(shapes):
        Q, K, V, mask, scale = R.make_inputs(D, KVH, HEADS // KVH, 1, n_q, n_kv, kind, None, seed=seed)
        q_mem = np.ascontiguousarray(Q[0].transpose(1, 0, 2))  # [n_q][heads][D]
        k_mem = np.ascontiguousarray(K[0].transpose(1, 0, 2))  # [n_kv][kv heads][D]
        v_mem = np.ascontiguousarray(V[0].transpose(1, 0, 2))
        m_mem = np.zeros((rows, n_kv), np.float16)
        m_mem[:n_q] = mask.astype(np.float16)
        paths = [tmp_path / f"{n}{i}.bin" for n in "qkvmo"]
        for a, p in zip((q_mem, k_mem, v_mem, m_mem), paths):
            a.tofile(p)
        argv += [str(p) for p in paths] + ([str(n_q), str(n_kv), str(rows)] if explicit else [])
        nodes.append(dict(n_q=n_q, n_kv=n_kv, Q=Q, K=K, V=V, mask=mask, mem=(q_mem, k_mem, v_mem, m_mem), out=paths[4]))
    r = subprocess.run([host_exe, _hip.HIP_SO, "run"] + argv, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    for n in nodes:
        n["got"] = np.fromfile(n["out"], dtype=np.uint32).reshape(n["n_q"], HEADS, D)
    return nodes, r.stderr


def assert_node_is_the_direct_call(dev, node, tol):
    """The bytes of the direct call on the same layouts (the glue adds no arithmetic), and the reference within the route's tolerance."""
    n_q, n_kv = node["n_q"], node["n_kv"]
    hq, hk, hv, hm = (dev.put(a.view(np.uint8).reshape(-1), 0) for a in node["mem"])
    hd = dev.put(np.full(n_q * HEADS * D * 4, 0xff, np.uint8), 0)
    op_scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    need = dev.lib.lfamd_flash_attn_workspace(D, n_q, n_kv, HEADS, KVH, 1)
    ws = dev.torch.empty(max(need, 16), dtype=dev.torch.uint8, device="cuda")
    rc = dev.lib.lfamd_flash_attn(dev.ptr(hq), HEADS * D * 4, D * 4, n_q * HEADS * D * 4, T.F16, dev.ptr(hk), KVH * D * 2, D * 2, n_kv * KVH * D * 2,
                                  T.F16, dev.ptr(hv), KVH * D * 2, D * 2, n_kv * KVH * D * 2, dev.ptr(hm), n_kv * 2, D, n_q, n_kv, HEADS, KVH, 1,
                                  op_scale, 0.0, dev.ptr(hd), D * 4, HEADS * D * 4, n_q * HEADS * D * 4, ws.data_ptr() if need else None, need, 0, None)
    assert rc == 0, _hip.lib().lfamd_last_error()
    direct = dev.get(hd).view(np.uint32).reshape(n_q, HEADS, D)
    assert np.array_equal(node["got"], direct)
    route = R.route_of(n_q)
    ref, a = R.ref64(node["Q"], node["K"], node["V"], node["mask"], np.float32(op_scale), route)
    assert R.row_err(node["got"].view(np.float32)[None], ref, a) <= tol


@pytest.mark.gpu
def test_graph_compute_issues_one_call_with_the_direct_calls_bytes(gpu, host_exe, tmp_path):
    nodes, err = graph_nodes(host_exe, tmp_path, [(N_Q, N_KV, MASK_ROWS, "causal", 3)], explicit=False)
    assert "ggml_backend_lfamd: 1 flash-attn calls" in err
    assert_node_is_the_direct_call(Dev(), nodes[0], R.TOL_MMA)


DECODE_NODE = (1, 3 * R.CHUNK + 7, MASK_ROWS, "bias", 4)  # n_q = 1 on 775 keys: the split route, through the context's workspace


@pytest.mark.gpu
def test_graph_compute_of_a_decode_node(gpu, host_exe, tmp_path):
    nodes, err = graph_nodes(host_exe, tmp_path, [DECODE_NODE])
    assert "ggml_backend_lfamd: 1 flash-attn calls" in err
    assert_node_is_the_direct_call(Dev(), nodes[0], R.TOL_F32)


@pytest.mark.gpu
def test_the_contexts_workspace_grows_between_two_decode_nodes(gpu, host_exe, tmp_path):
    """775 keys, then 2055: the second node needs more workspace than the context holds from the first."""
    nodes, err = graph_nodes(host_exe, tmp_path, [DECODE_NODE, (1, 2055, MASK_ROWS, "bias", 5)])
    assert "ggml_backend_lfamd: 2 flash-attn calls" in err
    dev = Dev()
    for n in nodes:
        assert_node_is_the_direct_call(dev, n, R.TOL_F32)
