"""Reading resident weights back on the device: lfamd_get_rows (GGML_OP_GET_ROWS, to_fp32 / to_fp16) and lfamd_unpack_weights.

Every comparison is on bit patterns with zero mismatches allowed: get_rows against oracle.c's ora_dequantize_row (pinned to its
stated operation order by tests/test_dequant_abi.py; F16 = that f32 value rounded to nearest-even, numpy's astype), unpack against
the GGUF bytes that were packed.  No case is skipped: a type or shape a call declines fails its test."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
import extremes
from helpers import make_case, rel_err

pytestmark = pytest.mark.gpu

BLOCK32 = (T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.Q8_0)
FLOATS = (T.F32, T.F16, T.BF16)
SHAPES = {t: [(33, 256), (67, 1024), (128, 4096)] + ([(64, 96)] if t in BLOCK32 else []) + ([(40, 2048)] if t == T.Q8_0 else [])
          for t in T.QUANT_WEIGHT_TYPES}
QCASES = [(t, s) for t in T.QUANT_WEIGHT_TYPES for s in SHAPES[t]]
QIDS = [f"{T.NAMES[t]}-{s[0]}x{s[1]}" for t, s in QCASES]
FCASES = [(t, s) for t in FLOATS for s in [(33, 256), (67, 1024), (5, 77)]]
FIDS = [f"{T.NAMES[t]}-{s[0]}x{s[1]}" for t, s in FCASES]
DT = {"F32": (torch.float32, np.uint32), "F16": (torch.float16, np.uint16)}
SENT = 0x5A


def weights(t, rows, cols, gen, seed=23):
    if t in FLOATS:
        raw = synth.random_weights(t, rows, cols, seed).copy()
        if gen == "extreme":  # signed zeros, subnormals, the largest finite values, infinities; F32 values that overflow / go subnormal in F16
            if t == T.F32:
                v = raw.view(np.float32).reshape(rows, cols)
                sp = np.array([0.0, -0.0, 1e-45, -1e-40, 3.4e38, -3.4e38, np.inf, -np.inf, 65504.0, 65520.0, 65519.99, 6e-8, 2.98e-8,
                               -2.99e-8, 6.1e-5, 1e30], np.float32)
            elif t == T.F16:
                v = raw.view(np.float16).reshape(rows, cols)
                sp = np.array([0.0, -0.0, 6e-8, -6e-8, 6.1e-5, 65504.0, -65504.0, np.inf, -np.inf], np.float16)
            else:
                v = raw.view(np.uint16).reshape(rows, cols)
                sp = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x477F, 0x4780, 0x3300, 0x3280, 0x3880], np.uint16)
            v[:, ::3] = np.resize(sp, v[:, ::3].shape)
        return raw
    return synth.random_weights(t, rows, cols, seed) if gen == "plain" else extremes.extreme_weights(t, rows, cols, seed)


def want_bits(oracle, t, raw, cols, dt):
    with np.errstate(over="ignore"):
        w = oracle.dequantize(t, np.ascontiguousarray(raw), cols)
        return w.view(np.uint32) if dt == "F32" else w.astype(np.float16).view(np.uint16)


def bits(x, dt):
    return x.cpu().numpy().view(DT[dt][1])


def mismatches(got, want):
    return int((got != want).sum())


@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("t,shape", QCASES + FCASES, ids=QIDS + FIDS)
def test_whole_matrix_dequantisation_is_the_oracle_bit_for_bit(gpu, oracle, t, shape, gen, dt):
    rows, cols = shape
    raw = weights(t, rows, cols, gen)
    W = gpu.upload_weights(t, raw, rows, cols)
    got = bits(gpu.dequantize(W, DT[dt][0]), dt)
    want = want_bits(oracle, t, raw, cols, dt)
    bad = mismatches(got, want)
    print(f"{T.NAMES[t]} {shape} {gen} {dt}: {bad} of {want.size} differ")
    assert got.shape == want.shape and bad == 0


@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("t", T.QUANT_WEIGHT_TYPES + FLOATS, ids=lambda t: T.NAMES[t])
def test_index_lists_ranges_padding_and_out_of_range_indices(gpu, oracle, t, dt):
    rows, cols = 67, 1024
    raw = weights(t, rows, cols, "extreme")
    W = gpu.upload_weights(t, raw, rows, cols)
    want = want_bits(oracle, t, raw, cols, dt)
    tdt, ndt = DT[dt]
    esz = np.dtype(ndt).itemsize
    sent = int.from_bytes(bytes([SENT]) * esz, "little")
    # unsorted, repeats, first and last row, rows of the ragged last tile (64 .. 66), and two indices outside [0, rows)
    idx = [66, 0, 5, 5, 64, -1, 31, 32, 65, rows, 0, 66, 17]
    ids = torch.tensor(idx, dtype=torch.int32, device="cuda")
    pad = 24  # elements: out_row_bytes wider than the row
    out = torch.full((len(idx), (cols + pad) * esz), SENT, dtype=torch.uint8, device="cuda").view(tdt)
    assert out.shape == (len(idx), cols + pad)
    gpu.get_rows(W, ids, tdt, out=out)
    got = bits(out, dt)
    for s, r in enumerate(idx):
        if 0 <= r < rows:
            assert mismatches(got[s, :cols], want[r]) == 0, (s, r)
        else:
            assert (got[s, :cols] == sent).all(), (s, r)
    assert (got[:, cols:] == sent).all()
    # a range: d_ids == NULL, row0 > 0, through the last (ragged) tile
    got = bits(gpu.get_rows(W, None, tdt, row0=29, n=rows - 29), dt)
    assert mismatches(got, want[29:]) == 0
    # n_ids == 0: LFAMD_OK, nothing written
    out.view(torch.uint8).fill_(SENT)
    gpu.get_rows(W, ids, tdt, n=0, out=out)
    gpu.get_rows(W, None, tdt, row0=rows, n=0, out=out)
    assert (bits(out, dt) == sent).all()
    # an unaligned output (base and stride not multiples of 16 bytes): the element-store path
    flat = torch.full(((rows * (cols + 1) + 1) * esz,), SENT, dtype=torch.uint8, device="cuda").view(tdt)
    o2 = flat[1:].view(rows, cols + 1)
    gpu.get_rows(W, None, tdt, out=o2)
    g2 = bits(flat, dt)
    assert mismatches(g2[1:].reshape(rows, cols + 1)[:, :cols], want) == 0
    assert g2[0] == sent and (g2[1:].reshape(rows, cols + 1)[:, cols] == sent).all()


def test_argument_errors_launch_nothing(gpu):
    rows, cols = 40, 512
    W = gpu.upload_weights(T.Q4_K, synth.random_weights(T.Q4_K, rows, cols, 3), rows, cols)
    L = _hip.lib()
    out = torch.full((rows, cols), 7.0, dtype=torch.float32, device="cuda")
    raw = torch.full((rows, T.row_size(T.Q4_K, cols)), SENT, dtype=torch.uint8, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    p, o, i, st, null = W.data.data_ptr(), out.data_ptr(), ids.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream), None
    UNS, INV = -1, -2
    cases = [
        (UNS, (99, p, rows, cols, i, 0, 4, T.F32, o, cols * 4, st)),            # unknown weight type
        (UNS, (T.Q4_K, p, rows, cols, i, 0, 4, T.BF16, o, cols * 4, st)),       # out_type neither F32 nor F16
        (INV, (T.Q4_K, p, rows, cols - 32, i, 0, 4, T.F32, o, cols * 4, st)),   # cols not a block multiple
        (INV, (T.Q4_K, p, rows, cols, i, 0, 4, T.F32, o, cols * 4 - 4, st)),    # out_row_bytes smaller than a row
        (INV, (T.Q4_K, p, rows, cols, i, 0, 4, T.F32, o, cols * 4 + 2, st)),    # ... not a multiple of the element
        (INV, (T.Q4_K, null, rows, cols, i, 0, 4, T.F32, o, cols * 4, st)),     # null image
        (INV, (T.Q4_K, p, rows, cols, i, 0, 4, T.F32, null, cols * 4, st)),     # null output
        (INV, (T.Q4_K, p, rows, cols, null, 38, 3, T.F32, o, cols * 4, st)),    # row0 + n_ids > rows
        (INV, (T.Q4_K, p, rows, cols, null, -1, 3, T.F32, o, cols * 4, st)),
        (INV, (T.Q4_K, p, rows, cols, i, 0, -1, T.F32, o, cols * 4, st)),
    ]
    for want, args in cases:
        rc = L.lfamd_get_rows(*args)
        assert rc == want, (rc, want, args)
        assert L.lfamd_last_error()
    ucases = [
        (UNS, (99, rows, cols, p, raw.data_ptr(), raw.shape[1], st)),
        (INV, (T.Q4_K, rows, cols - 32, p, raw.data_ptr(), raw.shape[1], st)),
        (INV, (T.Q4_K, rows, cols, p, raw.data_ptr(), raw.shape[1] - 1, st)),
        (INV, (T.Q4_K, rows, cols, null, raw.data_ptr(), raw.shape[1], st)),
        (INV, (T.Q4_K, rows, cols, p, null, raw.shape[1], st)),
    ]
    for want, args in ucases:
        assert L.lfamd_unpack_weights(*args) == want, args
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (raw == SENT).all()
    with pytest.raises(_hip.LfamdError):
        gpu.get_rows(W, None, torch.bfloat16)


@pytest.mark.parametrize("dt", ["F32", "F16"])
def test_rows_of_one_expert_of_a_stack(gpu, oracle, dt):
    experts, rows, cols = 8, 64, 512
    raws = [synth.random_weights(T.Q4_K, rows, cols, 40 + e) for e in range(experts)]
    Ws = [gpu.upload_weights(T.Q4_K, r, rows, cols) for r in raws]
    size = _hip.lib().lfamd_packed_size(T.Q4_K, rows, cols)
    stack = torch.cat([w.data for w in Ws])
    assert stack.numel() == experts * size
    e5 = gpu.PackedWeights(T.Q4_K, rows, cols, stack[5 * size: 6 * size])  # expert e = base + e * lfamd_packed_size
    ids = torch.tensor([63, 1, 32, 1], dtype=torch.int32, device="cuda")
    got = bits(gpu.get_rows(e5, ids, DT[dt][0]), dt)
    assert mismatches(got, want_bits(oracle, T.Q4_K, raws[5], cols, dt)[[63, 1, 32, 1]]) == 0


@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("t,shape", QCASES + FCASES, ids=QIDS + FIDS)
def test_unpack_returns_the_gguf_bytes(gpu, t, shape, gen):
    """pack -> unpack is the identity on the file's bytes for EVERY type (no image loses a field), and unpack's output packs
    to the same image."""
    rows, cols = shape
    raw = weights(t, rows, cols, gen)
    W = gpu.upload_weights(t, raw, rows, cols)
    back = gpu.unpack_weights(W)
    got = back.cpu().numpy()
    bad = mismatches(got, raw)
    print(f"{T.NAMES[t]} {shape} {gen}: {bad} of {raw.size} bytes differ")
    assert got.shape == raw.shape and bad == 0
    W2 = gpu.upload_weights(t, back, rows, cols)
    # (Q8_0: the P80 tiles; lfamd_packed_size rounds that image up to 256 bytes and nothing writes the round-up)
    n = ((rows + 7) // 8) * ((cols // 32 + 3) // 4) * 1088 if t == T.Q8_0 else W.data.numel()
    assert W2.data.numel() == W.data.numel() and torch.equal(W2.data[:n], W.data[:n])


def test_unpack_honours_the_row_stride(gpu):
    rows, cols = 37, 512
    raw = synth.random_weights(T.Q6_K, rows, cols, 9)
    W = gpu.upload_weights(T.Q6_K, raw, rows, cols)
    rb = raw.shape[1]
    dst = torch.full((rows, rb + 22), SENT, dtype=torch.uint8, device="cuda")
    _hip.check(_hip.lib().lfamd_unpack_weights(T.Q6_K, rows, cols, W.data.data_ptr(), dst.data_ptr(), rb + 22,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lfamd_unpack_weights")
    got = dst.cpu().numpy()
    assert np.array_equal(got[:, :rb], raw) and (got[:, rb:] == SENT).all()


# n <= 8 runs the exact GEMVs: the tolerances of tests/test_gpu_parity.py (integer parts exact, f32 summation order differs);
# Q8_0 differs from the default oracle variant only in where Kahan summation is applied
MM_TOL = {T.Q4_1: 1e-5, T.Q5_1: 1e-5, T.Q8_0: 1e-5}


@pytest.mark.parametrize("t", T.QUANT_WEIGHT_TYPES, ids=lambda t: T.NAMES[t])
def test_the_image_is_only_read(gpu, oracle, t):
    m, n, k = 67, 3, 1024
    A, B, bt = make_case(t, m, n, k, seed=70 + t)
    W = gpu.upload_weights(t, A, m, k)
    before = W.data.clone()
    Bd = torch.from_numpy(B).cuda()
    c0 = gpu.mul_mat(W, Bd, bt).clone()
    gpu.dequantize(W, torch.float32)
    gpu.dequantize(W, torch.float16)
    gpu.get_rows(W, torch.tensor([66, 0, 3], dtype=torch.int32, device="cuda"), torch.float16)
    gpu.unpack_weights(W)
    c1 = gpu.mul_mat(W, Bd, bt)
    torch.cuda.synchronize()
    assert torch.equal(W.data, before)
    assert torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    ok, G = oracle.sgemm(t, A, bt, B, m, n, k, nth=2)
    assert ok == 1
    assert rel_err(c1.cpu().numpy(), G) <= MM_TOL.get(t, 2e-6)


def graph_case():
    """Body of test_get_rows_in_a_captured_graph; runs in a process of its own (see there)."""
    from llamafile_amd import sgemm as gpu
    from oracle import ora as oracle
    oracle.build()
    gpu.init(0)
    rows, cols = 67, 1024
    raw = extremes.extreme_weights(T.Q6_K, rows, cols, 4)
    W = gpu.upload_weights(T.Q6_K, raw, rows, cols)
    want = want_bits(oracle, T.Q6_K, raw, cols, "F16")
    ids = torch.tensor([1, 66, 2, 40], dtype=torch.int32, device="cuda")
    out = torch.zeros((4, cols), dtype=torch.float16, device="cuda")
    gpu.get_rows(W, ids, torch.float16, out=out)  # (loads the kernel before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: one kernel node
        gpu.get_rows(W, ids, torch.float16, out=out)
    for idx in ([65, 0, 0, 33], [7, 64, 31, 32]):
        ids.copy_(torch.tensor(idx, dtype=torch.int32))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert mismatches(bits(out, "F16"), want[idx]) == 0, idx
    print("graph case ok")


def test_get_rows_in_a_captured_graph(gpu):
    """One get_rows call captured with torch.cuda.graph and replayed twice with different index contents gives the right rows
    each time.  The capture runs in a fresh child process: what a capture leaves behind in torch and the HIP runtime (the capture
    stream lives as long as the process) was seen to break a later test of this process that needs three streams to run side by
    side on the process's few hardware queues (tests/test_gpu_tp_rehearsal.py: a rank never arrived)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_get_rows as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_full_size_token_embedding(gpu, oracle):
    """Q6_K 128256 x 4096 (token_embd.weight of a Llama-3 8B Q4_K_M file): 512 random indices to F16, and 64 sampled rows of a
    whole-matrix dequantisation, against the oracle on those rows only."""
    rows, cols = 128256, 4096
    rb = T.row_size(T.Q6_K, cols)
    rng = np.random.default_rng(12)
    base = extremes.extreme_weights(T.Q6_K, 2048, cols, 77)
    raw = torch.from_numpy(base).cuda().repeat((rows + 2047) // 2048, 1)[:rows].contiguous()
    # make the rows distinct: a row's first block gets its own d (f16 of 2^-8 * (1 + (row % 1024) / 1024))
    d = (2.0 ** -8 * (1.0 + (torch.arange(rows, device="cuda") % 1024).float() / 1024.0)).half().view(torch.uint8).view(rows, 2)
    raw[:, 208:210] = d
    assert raw.shape == (rows, rb)
    W = gpu.upload_weights(T.Q6_K, raw, rows, cols)
    idx = rng.integers(0, rows, 512).astype(np.int32)
    idx[:3] = (0, rows - 1, rows - 1)
    got = bits(gpu.get_rows(W, torch.from_numpy(idx).cuda(), torch.float16), "F16")
    sel = raw[torch.from_numpy(idx.astype(np.int64)).cuda()].cpu().numpy()
    assert mismatches(got, want_bits(oracle, T.Q6_K, sel, cols, "F16")) == 0
    full = gpu.dequantize(W, torch.float16)
    assert full.shape == (rows, cols)
    samp = np.sort(rng.choice(rows, 64, replace=False))
    samp[0], samp[-1] = 0, rows - 1
    st = torch.from_numpy(samp).cuda()
    assert mismatches(bits(full[st], "F16"), want_bits(oracle, T.Q6_K, raw[st].cpu().numpy(), cols, "F16")) == 0
    del full
    back = gpu.unpack_weights(W)
    assert torch.equal(back, raw)
