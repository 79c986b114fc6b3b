"""The GPU-module boundary: the 12 ms_abi symbols llamafile/cuda.c:726-737 imports, driven
from a C host program that plays llamafile's side (tests/backend_host/backend_host.c): dlopen, symbol import,
ggml_cuda_link with a ggml_backend_api callback table, buffers, set_tensor, supports_op, graph_compute, get_tensor."""
import os
import subprocess

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
from helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "backend_host", "backend_host.c")
EXE = os.path.join(ROOT, "tests", "backend_host", "backend_host")


@pytest.fixture(scope="module")
def host_exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        subprocess.check_call(["gcc", "-O1", "-Wall", "-o", EXE, SRC, "-ldl"])
    return EXE


def test_module_exports_the_twelve_symbols_and_links_or_declines(host_exe):
    """On a box without an MI355X ggml_cuda_link answers false (llamafile then falls back to the CPU, cuda.c:744-752)."""
    out = subprocess.run([host_exe, _hip.HIP_SO, "exports"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] in ("linked", "nolink")


@pytest.mark.gpu
def test_a_host_with_other_struct_layouts_is_declined(gpu, host_exe, tmp_path):
    """The recalled struct layouts are cross-checked through the host's own accessors (ggml_nbytes, ggml_nelements,
    ggml_element_size, ggml_is_contiguous, ggml_backend_buffer_get_usage): when they disagree with what the module reads from the
    structs, supports_op says no (the host program exits 11 = "supports_op says no") and the module says why, once."""
    t, m, k, n = T.Q4_K, 64, 512, 3
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    synth.random_weights(t, m, k, 7).tofile(wp)
    synth.random_activations(n, k, 8).tofile(xp)
    args = [host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), "1", str(wp), str(xp), str(op)]
    ok = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0, ok.stderr
    bad = subprocess.run(args, capture_output=True, text=True, timeout=300, env={**os.environ, "BACKEND_HOST_SKEW": "1"})
    assert bad.returncode == 11, (bad.returncode, bad.stderr)
    assert "do not match this module's layouts" in bad.stderr


@pytest.mark.gpu
def test_matrices_only_switch_keeps_layer_buffers_on_the_host(gpu, host_exe):
    """with LFAMD_BACKEND_MATRICES_ONLY=1 only the split (matrix) buffer type is device memory, so norm
    weights, the KV cache and compute buffers stay with ggml's CPU backend."""
    for env, want in (({}, "layer=device matrix=device"), ({"LFAMD_BACKEND_MATRICES_ONLY": "1"}, "layer=host matrix=device")):
        r = subprocess.run([host_exe, _hip.HIP_SO, "bufts"], capture_output=True, text=True, timeout=120, env={**os.environ, **env})
        assert r.returncode == 0 and r.stdout.strip() == want, (r.stdout, r.stderr)


def check_mul_mat(oracle, got, t, W, x, m, k, n, nb2):
    bt = T.VEC_DOT[t]
    if t == T.F16:
        # ggml hands f16 weights their activations rounded to f16 (n > 2) or as f32 (n <= 2, tinyblas_cpu_sgemm.inc:121-136);
        # the module keeps f32 activations for n <= 8: at least as accurate — within f16 rounding of either form
        G16 = oracle.f64_gemm(t, W, T.F16, synth.quantize_activations(T.F16, x), m, n * nb2, k)
        G32 = oracle.f64_gemm(t, W, T.F32, synth.quantize_activations(T.F32, x), m, n * nb2, k)
        assert min(rel_err(got, G16), rel_err(got, G32)) <= 2e-6 and rel_err(got, G16) <= 1e-3
        return
    v = oracle.variant("zen4")  # the module passes LFAMD_FLAG_Q0_VREGS32 (AVX512 build of tinyBLAS_Q0)
    for s in range(nb2):  # every slice is its own llamafile_sgemm problem (the Q0 Kahan geometry depends on n)
        ok, G = oracle.sgemm(t, W, bt, synth.quantize_activations(bt, x[s * n:(s + 1) * n]), m, n, k, v=v)
        assert ok == 1
        g = got[s * n:(s + 1) * n]
        if t == T.Q8_0:
            assert np.array_equal(g.view(np.uint32), G.view(np.uint32))
        else:
            assert rel_err(g, G) <= (1e-3 if n > 8 else 2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("t,m,k,n,nb2", [(T.Q4_K, 96, 1024, 1, 1), (T.Q4_K, 160, 768, 40, 1), (T.Q6_K, 64, 512, 3, 2), (T.Q8_0, 72, 256, 1, 1),
                                         (T.F16, 48, 256, 5, 3), (T.Q5_K, 32, 512, 12, 1), (T.Q4_0, 64, 256, 2, 1)],
                         ids=lambda v: str(v))
def test_mul_mat_node_through_the_backend_interface(gpu, oracle, host_exe, tmp_path, t, m, k, n, nb2):
    """GGML_OP_MUL_MAT with f32 src1 and dims-2 broadcast (src1 has nb2 slices, src0 one): what
    ggml_compute_forward_mul_mat computes — quantise src1 rows to the type's vec_dot format, llamafile_sgemm per slice."""
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp)
    x.tofile(xp)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), str(nb2), str(wp), str(xp), str(op)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    got = np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m)
    check_mul_mat(oracle, got, t, W, x, m, k, n, nb2)


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,tasks", [(1, 1), (3, 2), (20, 1)])
def test_mul_mat_id_node_through_the_backend_interface(gpu, oracle, host_exe, tmp_path, tokens, tasks):
    t, m, k, experts, thinkers = T.Q4_K, 64, 512, 6, 2
    W = np.stack([synth.random_weights(t, m, k, 50 + e) for e in range(experts)])
    x = synth.random_activations(tokens * tasks, k, 9).reshape(tokens, tasks, k)
    rng = np.random.default_rng(4)
    ids = np.stack([rng.permutation(experts)[:thinkers] for _ in range(tokens)]).astype(np.int32)
    wp, xp, ip, op = (tmp_path / n for n in ("w.bin", "x.bin", "i.bin", "o.bin"))
    W.tofile(wp), x.tofile(xp), ids.tofile(ip)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmatid", str(t), str(m), str(k), str(experts), str(thinkers), str(tasks), str(tokens),
                        str(wp), str(xp), str(ip), str(op)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    got = np.fromfile(op, dtype=np.float32).reshape(tokens, thinkers, m)
    q = oracle.quantize(T.Q8_K, x.reshape(-1, k))
    G = np.zeros_like(got)
    for tk in range(tokens):
        for th in range(thinkers):
            ok, c = oracle.sgemm(t, W[ids[tk, th]], T.Q8_K, q[tk * tasks + th % tasks][None, :], m, 1, k)
            assert ok == 1
            G[tk, th] = c[0]
    # (normwise over the whole result like the other batch tests: more than 4 tokens run the grouped MFMA launch on scaled
    # f16 operands, whose per-output error is ~7e-4 of the outputs' rms at k = 512)
    assert rel_err(got, G) <= (1e-3 if tokens > 4 else 2e-6)


TWO = {"LFAMD_BACKEND_DEVICES": "0,0"}  # two logical devices on the one GPU of the box: the multi-device paths, rehearsed


@pytest.mark.gpu
def test_device_list_is_what_the_module_reports(gpu, host_exe):
    """ggml_backend_cuda_get_device_count (ggml-cuda.cu.patch:19532): every gfx950 device of the process by default,
    LFAMD_BACKEND_DEVICES restricts / repeats; ordinals that do not exist are dropped."""
    import torch
    visible = torch.cuda.device_count()
    for env, want in (({}, f"count={visible}"), (TWO, "count=2"), ({"LFAMD_BACKEND_DEVICES": "0,99,0,0"}, "count=3"),
                      ({"LFAMD_BACKEND_DEVICES": "99"}, "count=0")):
        r = subprocess.run([host_exe, _hip.HIP_SO, "exports"], capture_output=True, text=True, timeout=120, env={**os.environ, **env})
        assert r.returncode == 0 and r.stdout.split()[1] == want, (env, r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("t,m,k,n,nb2,split,main", [(T.Q4_K, 1024, 512, 1, 1, "1,1", 0), (T.Q4_K, 1280, 512, 40, 1, "0.3,0.7", 1),
                                                    (T.Q6_K, 768, 512, 3, 2, "1,1", 0), (T.Q8_0, 512, 256, 1, 1, "0,0", 1),
                                                    (T.F16, 520, 256, 5, 1, "1,3", 0), (T.Q4_K, 96, 1024, 2, 1, "1,1", 0),
                                                    (T.Q5_K, 512, 512, 12, 1, "1,0", 1)], ids=lambda v: str(v))
def test_row_split_mul_mat_over_two_devices(gpu, oracle, host_exe, tmp_path, t, m, k, n, nb2, split, main):
    """--split-mode row (ggml_backend_cuda_split_buffer_type, ggml-cuda.cu.patch:17123-17450; ggml_cuda_op_mul_mat with split
    src0, :18060-18330): the matrix's rows are cut at the tensor_split fractions over the logical devices, each computes its
    columns of the result, dst is assembled on the main device.  Same oracle, same tolerances as the one-device node; the host
    program also checks set_tensor / get_tensor round-trip, clear() and the re-upload on the split buffer."""
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp)
    x.tofile(xp)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), str(nb2), str(wp), str(xp), str(op)],
                       capture_output=True, text=True, timeout=300,
                       env={**os.environ, **TWO, "BACKEND_HOST_SPLIT": split, "BACKEND_HOST_MAIN": str(main)})
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    assert "weights in ROCm-lfamd_Split" in r.stderr
    check_mul_mat(oracle, np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m), t, W, x, m, k, n, nb2)


@pytest.mark.gpu
def test_expert_stack_in_a_split_buffer_stays_whole(gpu, oracle, host_exe, tmp_path):
    """llama.cpp places expert tensors in the matrix buffer type too; the reference refuses MUL_MAT_ID there
    (ggml-cuda.cu.patch:18501), this module keeps the stack whole on the first device and serves it."""
    t, m, k, experts, thinkers, tokens, tasks = T.Q4_K, 64, 512, 6, 2, 3, 1
    W = np.stack([synth.random_weights(t, m, k, 50 + e) for e in range(experts)])
    x = synth.random_activations(tokens * tasks, k, 9).reshape(tokens, tasks, k)
    rng = np.random.default_rng(4)
    ids = np.stack([rng.permutation(experts)[:thinkers] for _ in range(tokens)]).astype(np.int32)
    wp, xp, ip, op = (tmp_path / n for n in ("w.bin", "x.bin", "i.bin", "o.bin"))
    W.tofile(wp), x.tofile(xp), ids.tofile(ip)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmatid", str(t), str(m), str(k), str(experts), str(thinkers), str(tasks), str(tokens),
                        str(wp), str(xp), str(ip), str(op)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, **TWO, "BACKEND_HOST_SPLIT": "1,1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    got = np.fromfile(op, dtype=np.float32).reshape(tokens, thinkers, m)
    q = oracle.quantize(T.Q8_K, x.reshape(-1, k))
    for tk in range(tokens):
        for th in range(thinkers):
            ok, c = oracle.sgemm(t, W[ids[tk, th]], T.Q8_K, q[tk * tasks + th % tasks][None, :], m, 1, k)
            assert ok == 1 and rel_err(got[tk, th], c[0]) <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("t,m,k,n", [(T.Q4_K, 1024, 1024, 1), (T.Q6_K, 512, 512, 1), (T.Q4_K, 768, 512, 5), (T.Q8_0, 256, 256, 1), (T.F16, 128, 256, 2),
                                     (T.Q4_K, 512, 512, 20)], ids=lambda v: str(v))
def test_sibling_mul_mat_nodes_run_as_one_call(gpu, oracle, host_exe, tmp_path, t, m, k, n):
    """graph_compute (ggml-cuda.cu.patch:18945) sees attn_q / attn_k / attn_v and ffn_gate / ffn_up back to back over one src1:
    up to four such MUL_MAT nodes with at most 8 activation rows go out as ONE lfamd_mul_mat_multi_types call.  The host
    program puts a second node with its own copy of the weights behind the first and requires identical bytes from both;
    the result is held against the oracle as for a single node; LFAMD_BACKEND_NO_SIBLING_FUSION=1 runs them one by one."""
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp)
    x.tofile(xp)
    outs = []
    for env in ({}, {"LFAMD_BACKEND_NO_SIBLING_FUSION": "1"}):
        r = subprocess.run([host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), "1", str(wp), str(xp), str(op)],
                           capture_output=True, text=True, timeout=300,
                           env={**os.environ, "BACKEND_HOST_PAIR": "1", "LFAMD_BACKEND_STATS": "1", **env})
        assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
        # (the host program computes the graph four times; more than 8 rows: no fusion, the batch bodies take one matrix each)
        assert f"{0 if env or n > 8 else 4} sibling calls" in r.stderr, r.stderr
        outs.append(np.fromfile(op, dtype=np.float32).reshape(n, m))
        check_mul_mat(oracle, outs[-1], t, W, x, m, k, n, 1)
    if n == 1:
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))  # one column: the fused launch is the same arithmetic


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,weights_usage", [(1, True), (3, True), (12, True), (3, False)])
def test_sibling_mul_mat_id_nodes_run_as_one_call(gpu, oracle, host_exe, tmp_path, tokens, weights_usage):
    """ffn_gate_exps and ffn_up_exps of a layer (same src1, same ids) behind each other: one lfamd_mul_mat_id_multi call up to 4 tokens."""
    t, m, k, experts, thinkers, tasks = T.Q4_K, 64, 512, 6, 2, 1
    W = np.stack([synth.random_weights(t, m, k, 50 + e) for e in range(experts)])
    x = synth.random_activations(tokens * tasks, k, 9).reshape(tokens, tasks, k)
    rng = np.random.default_rng(4)
    ids = np.stack([rng.permutation(experts)[:thinkers] for _ in range(tokens)]).astype(np.int32)
    wp, xp, ip, op = (tmp_path / n for n in ("w.bin", "x.bin", "i.bin", "o.bin"))
    W.tofile(wp), x.tofile(xp), ids.tofile(ip)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmatid", str(t), str(m), str(k), str(experts), str(thinkers), str(tasks), str(tokens),
                        str(wp), str(xp), str(ip), str(op)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "BACKEND_HOST_PAIR": "1", "LFAMD_BACKEND_STATS": "1",
                            **({} if weights_usage else {"BACKEND_HOST_NO_WEIGHTS_USAGE": "1"})})
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    # (expert stacks outside a weights buffer share the context's one scratch image: such nodes must run one by one)
    assert f"{4 if tokens <= 4 and weights_usage else 0} sibling calls" in r.stderr, r.stderr
    got = np.fromfile(op, dtype=np.float32).reshape(tokens, thinkers, m)
    q = oracle.quantize(T.Q8_K, x.reshape(-1, k))
    G = np.zeros_like(got)
    for tk in range(tokens):
        for th in range(thinkers):
            ok, c = oracle.sgemm(t, W[ids[tk, th]], T.Q8_K, q[tk * tasks + th % tasks][None, :], m, 1, k)
            assert ok == 1
            G[tk, th] = c[0]
    assert rel_err(got, G) <= (1e-3 if tokens > 4 else 2e-6)


# ----------------------------------------------------------------------------------------------------------------------------
# The layouts of a real llama.cpp graph (the tests above build every tensor contiguous and alone at its buffer's base)
def _run_host(host_exe, args, env=None, code=0):
    r = subprocess.run([host_exe, _hip.HIP_SO] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env={**os.environ, **(env or {})})
    assert r.returncode == code and (code or r.stdout.strip() == "ok"), (r.returncode, r.stdout, r.stderr)
    return r


def _mmid_inputs(tmp_path, tokens, tasks, experts=6, thinkers=2, t=T.Q4_K, m=64, k=512):
    """Expert stack, activations and the argsort result: I32 [tokens][experts], a permutation of ALL expert ids per token.  The
    node's ids are its first `thinkers` columns, so a reader that ignores nb[1] = experts * 4 takes valid but other experts."""
    W = np.stack([synth.random_weights(t, m, k, 50 + e) for e in range(experts)])
    x = synth.random_activations(tokens * tasks, k, 9).reshape(tokens, tasks, k)
    rng = np.random.default_rng(4)
    parent = np.stack([rng.permutation(experts) for _ in range(tokens)]).astype(np.int32)
    wp, xp, ip, op = (tmp_path / n for n in ("w.bin", "x.bin", "i.bin", "o.bin"))
    W.tofile(wp), x.tofile(xp), parent.tofile(ip)
    return W, x, parent, ["mulmatid_view", t, m, k, experts, thinkers, tasks, tokens, wp, xp, ip, op], op


def _mmid_expected(oracle, W, x, ids, t, m, k, tasks):
    tokens, thinkers = ids.shape
    q = oracle.quantize(T.Q8_K, x.reshape(-1, k))
    G = np.zeros((tokens, thinkers, m), np.float32)
    for tk in range(tokens):
        for th in range(thinkers):
            ok, c = oracle.sgemm(t, W[ids[tk, th]], T.Q8_K, q[tk * tasks + th % tasks][None, :], m, 1, k)
            assert ok == 1
            G[tk, th] = c[0]
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("tasks", [1, 2])
@pytest.mark.parametrize("tokens", [1, 3, 20])
def test_mul_mat_id_with_ids_viewed_from_the_argsort_result(gpu, oracle, host_exe, tmp_path, tokens, tasks):
    """What every MUL_MAT_ID node of a real MoE model looks like: ids is a view with nb[1] = n_expert * 4 (run_mul_mat_id's
    hipMemcpy2D into ctx->plan).  Oracle and tolerances of test_mul_mat_id_node_through_the_backend_interface."""
    t, m, k, thinkers = T.Q4_K, 64, 512, 2
    W, x, parent, args, op = _mmid_inputs(tmp_path, tokens, tasks)
    _run_host(host_exe, args)
    got = np.fromfile(op, dtype=np.float32).reshape(tokens, thinkers, m)
    G = _mmid_expected(oracle, W, x, parent[:, :thinkers], t, m, k, tasks)
    # (more than 4 tokens: normwise over the whole result, as that test explains — the scaled f16 operands of the grouped launch
    # put single outputs ~7e-4 of the rms off, and one 64-output row was measured at 1.3e-3 of its own maximum.  A row computed
    # with another expert's weights is off by the size of the outputs themselves, which either norm shows.)
    assert rel_err(got, G) <= (1e-3 if tokens > 4 else 2e-6)
    if tokens <= 4:  # exact arithmetic: every (token, thinker) row by itself
        for tk in range(tokens):
            for th in range(thinkers):
                assert rel_err(got[tk, th], G[tk, th]) <= 2e-6, (tk, th, int(parent[tk, th]))


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", [1, 3])
def test_sibling_mul_mat_id_nodes_share_a_viewed_ids(gpu, oracle, host_exe, tmp_path, tokens):
    """ffn_gate_exps + ffn_up_exps over the same strided ids: still ONE lfamd_mul_mat_id_multi call per graph run."""
    t, m, k, thinkers, tasks = T.Q4_K, 64, 512, 2, 1
    W, x, parent, args, op = _mmid_inputs(tmp_path, tokens, tasks)
    r = _run_host(host_exe, args, {"BACKEND_HOST_PAIR": "1", "LFAMD_BACKEND_STATS": "1"})
    assert "4 sibling calls" in r.stderr, r.stderr
    got = np.fromfile(op, dtype=np.float32).reshape(tokens, thinkers, m)
    G = _mmid_expected(oracle, W, x, parent[:, :thinkers], t, m, k, tasks)
    for tk in range(tokens):
        for th in range(thinkers):
            assert rel_err(got[tk, th], G[tk, th]) <= 2e-6, (tk, th)


def _weights_args(tmp_path, k, n, mats, x):
    args = ["weights", k, n, len(mats)]
    for j, (t, m, W) in enumerate(mats):
        p = tmp_path / f"w{j}.bin"
        W.tofile(p)
        args += [t, m, p]
    xp = tmp_path / "x.bin"
    x.tofile(xp)
    return args + [xp, tmp_path / "out"]


def _check_nodes(oracle, path, mats, x, k, n):
    got = np.fromfile(path, dtype=np.float32)
    o = 0
    for t, m, W in mats:
        check_mul_mat(oracle, got[o:o + n * m].reshape(n, m), t, W, x, m, k, n, 1)
        o += n * m
    assert o == got.size


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 20])
def test_weights_sharing_a_buffer_are_invalidated_one_by_one(gpu, oracle, host_exe, tmp_path, n):
    """Three matrices of different type and shape at aligned offsets of ONE weights buffer (how llama.cpp lays a model out; the
    packed copies are keyed by raw address and dropped over the written tensor's range).  set_tensor into the middle one alone
    makes ITS node the new product and leaves the others — results and bytes — alone; a partial set_tensor of whole rows at an
    offset shows too; so does cpy_tensor into the last one.  The host program checks the read-back of every matrix after every
    step (exit 16)."""
    k = 512
    shapes = [(T.Q4_K, 96), (T.Q6_K, 64), (T.Q4_0, 72)]
    mats = [(t, m, synth.random_weights(t, m, k, 7 + j)) for j, (t, m) in enumerate(shapes)]
    x = synth.random_activations(n, k, 8)
    new_mid = synth.random_weights(T.Q6_K, 64, k, 70)
    new_last = synth.random_weights(T.Q4_0, 72, k, 71)
    row0, nrows = 16, 24
    pm, pl = tmp_path / "mid.bin", tmp_path / "last.bin"
    new_mid.tofile(pm), new_last.tofile(pl)
    _run_host(host_exe, _weights_args(tmp_path, k, n, mats, x) + [1, pm, row0, nrows, 2, pl])
    mixed = new_mid.copy()
    mixed[row0:row0 + nrows] = mats[1][2][row0:row0 + nrows]
    steps = [mats, [mats[0], (T.Q6_K, 64, new_mid), mats[2]], [mats[0], (T.Q6_K, 64, mixed), mats[2]],
             [mats[0], (T.Q6_K, 64, mixed), (T.Q4_0, 72, new_last)]]
    for s, want in enumerate(steps):
        _check_nodes(oracle, str(tmp_path / "out") + f".{s}", want, x, k, n)
    # the updates are visible at all: the middle node moved in step 1, and only it
    o = [np.fromfile(str(tmp_path / "out") + f".{s}", dtype=np.float32) for s in range(4)]
    a, b = n * 96, n * (96 + 64)
    assert np.array_equal(o[0][:a], o[1][:a]) and np.array_equal(o[0][b:], o[1][b:]) and not np.array_equal(o[0][a:b], o[1][a:b])
    assert not np.array_equal(o[1][a:b], o[2][a:b]) and np.array_equal(o[2][:b], o[3][:b]) and not np.array_equal(o[2][b:], o[3][b:])


@pytest.mark.gpu
@pytest.mark.parametrize("mix", ["Q4_K+Q4_K+Q6_K", "Q4_K+IQ4_XS+Q6_K"])
@pytest.mark.parametrize("n", [1, 3, 20])
def test_qkv_siblings_as_a_model_has_them(gpu, oracle, host_exe, tmp_path, n, mix):
    """attn_q / attn_k / attn_v of a *_K_M file: unequal row counts and types over one src1, in one weights buffer.  Tolerances and
    the sibling-call count of test_sibling_mul_mat_nodes_run_as_one_call (the host program computes the graph twice here)."""
    k = 1024
    shapes = [(T.BY_NAME[name], m) for name, m in zip(mix.split("+"), (512, 128, 128))]
    mats = [(t, m, synth.random_weights(t, m, k, 17 + j)) for j, (t, m) in enumerate(shapes)]
    x = synth.random_activations(n, k, 18)
    for env in ({}, {"LFAMD_BACKEND_NO_SIBLING_FUSION": "1"}):
        r = _run_host(host_exe, _weights_args(tmp_path, k, n, mats, x), {"LFAMD_BACKEND_STATS": "1", **env})
        assert f"{0 if env or n > 8 else 2} sibling calls" in r.stderr, r.stderr
        _check_nodes(oracle, str(tmp_path / "out") + ".0", mats, x, k, n)


@pytest.mark.gpu
@pytest.mark.parametrize("t,m,k,n,nb2", [(T.Q4_K, 96, 1024, 1, 1), (T.Q4_K, 160, 768, 40, 1), (T.Q6_K, 64, 512, 3, 2), (T.Q8_0, 72, 256, 1, 1),
                                         (T.F16, 48, 256, 5, 3), (T.Q5_K, 32, 512, 12, 1), (T.Q4_0, 64, 256, 2, 1)], ids=lambda v: str(v))
def test_mul_mat_node_with_a_strided_src1_view(gpu, oracle, host_exe, tmp_path, t, m, k, n, nb2):
    """src1 is a view with nb[1] = (k + 4) * 4 (a slice of a wider tensor); the four floats behind every row are NaN."""
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    parent = np.full((n * nb2, k + 4), np.nan, np.float32)
    parent[:, :k] = x
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp), parent.tofile(xp)
    _run_host(host_exe, ["mulmat_xview", t, m, k, n, nb2, wp, xp, op])
    check_mul_mat(oracle, np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m), t, W, x, m, k, n, nb2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [128, 256])
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("group", [1, 4])
def test_attention_kq_with_permuted_operands(gpu, oracle, host_exe, tmp_path, group, n, k):
    """KQ as llama.cpp builds it: src0 the F16 K cache permuted (nb[1] > nb[2]) in an ordinary buffer, src1 Q permuted, `group`
    query heads per KV head (get_packed per slice, the have02 reuse of run_mul_mat), both at non-zero offsets of their buffers.
    Each head against the F16 rule of check_mul_mat."""
    n_kv, kv_heads = 96, 2
    heads = kv_heads * group
    rng = np.random.default_rng(60 + group + n)
    K = (rng.random((n_kv, kv_heads, k), dtype=np.float32) * 2 - 1).astype(np.float16)
    Q = (rng.random((n, heads, k), dtype=np.float32) * 2 - 1).astype(np.float32)
    kp, qp, op = tmp_path / "k.bin", tmp_path / "q.bin", tmp_path / "o.bin"
    K.tofile(kp), Q.tofile(qp)
    _run_host(host_exe, ["attn", k, n_kv, kv_heads, heads, n, kp, qp, op])
    got = np.fromfile(op, dtype=np.float32).reshape(heads, n, n_kv)
    for h in range(heads):
        Kh = np.ascontiguousarray(K[:, h // group, :]).view(np.uint8).reshape(n_kv, k * 2)
        check_mul_mat(oracle, got[h], T.F16, Kh, np.ascontiguousarray(Q[:, h, :]), n_kv, k, n, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("t,m,k,n,nb2", [(T.F16, 48, 256, 5, 3), (T.F16, 64, 256, 40, 1), (T.F16, 40, 96, 12, 2)], ids=lambda v: str(v))
def test_float_weights_take_f32_rows_at_any_stride(gpu, oracle, host_exe, tmp_path, t, m, k, n, nb2):
    """What supports_op accepts it must compute: F16 weights over a src1 view with nb[1] = (k + 1) * 4 — rows that are only 4-byte
    aligned (the generic kernel at n <= 8 and for rows that are not whole 256-element groups, the element-wise staging of
    prep_float_kernel in front of the MFMA body at n = 40); the float behind every row is NaN.  The F16 rule of check_mul_mat."""
    W = synth.random_weights(t, m, k, 7)
    x = synth.random_activations(n * nb2, k, 8)
    parent = np.full((n * nb2, k + 1), np.nan, np.float32)
    parent[:, :k] = x
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    W.tofile(wp), parent.tofile(xp)
    _run_host(host_exe, ["mulmat_xodd", t, m, k, n, nb2, wp, xp, op])
    check_mul_mat(oracle, np.fromfile(op, dtype=np.float32).reshape(nb2 * n, m), t, W, x, m, k, n, nb2)


# every declined case alters one thing of an accepted node; the control beside it alters the same thing harmlessly
DECLINED = ["f16_src1", "dst_noncontig", "f16w_src0_transposed", "k_mismatch", "k_not_block", "id_ids_not_i32", "id_stack_noncontig",
            "src1_row_stride", "src1_base", "src1_view_offs", "id_src1_base", "id_q4_0_experts", "id_more_thinkers_than_experts"]
ACCEPTED = ["control_mm", "control_id", "control_f16w", "control_k_block", "control_f16w_src1_row_stride", "control_src1_row_stride16",
            "control_src1_base16", "control_id_src1_base16", "control_src1_view_offs16"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", DECLINED + ACCEPTED)
def test_supports_op_declines_what_the_module_would_refuse(gpu, host_exe, what):
    """supports_op answers no — and the host program never calls graph_compute — for nodes outside the module's contract: the
    operator's own shape rules, the operand layouts lfamd_mul_mat / lfamd_mul_mat_id refuse (include/lfamd_hip.h: f32 rows of
    quantised weights off 16 bytes) and expert types lfamd_mul_mat_id takes no F32 activations for.  The controls are the same
    node with the altered field moved by a harmless amount: accepted (and computed by the tests above)."""
    r = subprocess.run([host_exe, _hip.HIP_SO, "decline", what], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.strip() == ("declined" if what in DECLINED else "accepted"), (what, r.stdout, r.stderr)
