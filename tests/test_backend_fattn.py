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


@pytest.mark.gpu
def test_graph_compute_issues_one_call_with_the_direct_calls_bytes(gpu, host_exe, tmp_path):
    Q, K, V, mask, scale = R.make_inputs(D, KVH, HEADS // KVH, 1, N_Q, N_KV, "causal", None, seed=3)
    q_mem = np.ascontiguousarray(Q[0].transpose(1, 0, 2))  # [n_q][heads][D]
    k_mem = np.ascontiguousarray(K[0].transpose(1, 0, 2))  # [n_kv][kv heads][D]
    v_mem = np.ascontiguousarray(V[0].transpose(1, 0, 2))
    m_mem = np.zeros((MASK_ROWS, N_KV), np.float16)
    m_mem[:N_Q] = mask.astype(np.float16)
    paths = [tmp_path / n for n in ("q.bin", "k.bin", "v.bin", "m.bin", "o.bin")]
    for a, p in zip((q_mem, k_mem, v_mem, m_mem), paths):
        a.tofile(p)
    r = subprocess.run([host_exe, _hip.HIP_SO, "run"] + [str(p) for p in paths], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "LFAMD_BACKEND_STATS": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)
    assert "ggml_backend_lfamd: 1 flash-attn calls" in r.stderr
    got = np.fromfile(paths[4], dtype=np.uint32).reshape(N_Q, HEADS, D)
    # the direct call on the same layouts
    dev = Dev()
    hq, hk, hv, hm = (dev.put(a.view(np.uint8).reshape(-1), 0) for a in (q_mem, k_mem, v_mem, m_mem))
    hd = dev.put(np.full(N_Q * HEADS * D * 4, 0xff, np.uint8), 0)
    op_scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    rc = dev.lib.lfamd_flash_attn(dev.ptr(hq), HEADS * D * 4, D * 4, N_Q * HEADS * D * 4, T.F16, dev.ptr(hk), KVH * D * 2, D * 2, N_KV * KVH * D * 2,
                                  T.F16, dev.ptr(hv), KVH * D * 2, D * 2, N_KV * KVH * D * 2, dev.ptr(hm), N_KV * 2, D, N_Q, N_KV, HEADS, KVH, 1,
                                  op_scale, 0.0, dev.ptr(hd), D * 4, HEADS * D * 4, N_Q * HEADS * D * 4, None, 0, 0, None)
    assert rc == 0, _hip.lib().lfamd_last_error()
    direct = dev.get(hd).view(np.uint32).reshape(N_Q, HEADS, D)
    assert np.array_equal(got, direct)
    ref, a = R.ref64(Q, K, V, mask, np.float32(op_scale), "prefill")
    assert R.row_err(got.view(np.float32)[None], ref, a) <= R.TOL_MMA
