"""Decode GEMV, fused launches (n = 1): sibling matrices on one activation row whose work-groups address their FIRST item from
preloaded kernel arguments (gemv_impl.h: gemv_kq_early_kernel for one to three matrices of a type, gemv_kq_dual_early_kernel for
the Q4_K / Q5_K + Q6_K launch) and every later item from the matrix table; four matrices keep the table-only kernel.

Small launches give every work-group at most one item, so the early pick alone meets every matrix and both half-tiles of the
boundaries (rows 48 | 16 | 80 | 33 and 33 | 40 | 24: boundaries at 4, 6, 12 and 4, 8 half-tiles; m not a multiple of 32); the long
walks (518 half-tiles on at most 256 work-groups) take later items from the table across the boundaries, and Q6_K's permuted
runs of 16 items straddle them.  k = 768, 4096, 4352, 14336 and 256, 1024 run the 8 x 2, 16 x 2 and 16 x 1 forms.

Every output: <= 1e-5 of the oracle (the bound of tests/test_gpu_decode_variants.py for these kernels), <= 1e-6 of the
single-matrix mul_mat (another wave layout may move the last bit), the same bits for f32 and pre-quantised
activations and the same bits on a second call."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import ggml_types as T, synth
from helpers import rel_err

pytestmark = pytest.mark.gpu

SAME_TYPES = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q4_0]
ROWSETS = [(48, 16), (48, 16, 80), (48, 16, 80, 33), (33, 40, 24)]


def _case(gpu, oracle, spec, k, seed):
    """spec: ((type, rows), ...).  -> (fused f32 outputs, packed weights, the f32 row on the device, its numpy copy)"""
    raws = [synth.random_weights_torch(t, m, k, seed + 7 * i + t).cpu().numpy() for i, (t, m) in enumerate(spec)]
    Ws = [gpu.upload_weights(t, raw, m, k) for (t, m), raw in zip(spec, raws)]
    x = synth.random_activations(1, k, seed + 3)
    if k >= 512:
        x[0, 256:512] = 0.0  # an all-zero block
    xd = torch.from_numpy(x).cuda().view(torch.uint8).view(1, k * 4)
    bt = T.VEC_DOT[spec[0][0]]
    assert all(T.VEC_DOT[t] == bt for t, _ in spec)
    Bq = synth.quantize_activations(bt, x)
    fused = [o.cpu().numpy() for o in gpu.mul_mat_multi(Ws, xd, T.F32, n=1)]
    again = [o.cpu().numpy() for o in gpu.mul_mat_multi(Ws, xd, T.F32, n=1)]
    quant = [o.cpu().numpy() for o in gpu.mul_mat_multi(Ws, torch.from_numpy(Bq).cuda(), bt, n=1)]
    for j, ((t, m), raw, W) in enumerate(zip(spec, raws, Ws)):
        tag = (T.NAMES[t], m, k, j)
        assert fused[j].shape == (1, m)
        assert np.array_equal(fused[j].view(np.uint32), again[j].view(np.uint32)), tag
        assert np.array_equal(fused[j].view(np.uint32), quant[j].view(np.uint32)), tag
        ok, G = oracle.sgemm(t, raw, bt, Bq, m, 1, k, nth=4)
        assert ok == 1
        e_ora = rel_err(fused[j], G)
        single = gpu.mul_mat(W, xd, T.F32, n=1).cpu().numpy()
        e_one = rel_err(fused[j], single)
        print(tag, "vs oracle", e_ora, "vs single", e_one)
        assert e_ora <= 1e-5, (tag, e_ora)
        assert e_one <= 1e-6, (tag, e_one)
    return fused, Ws, xd, x


@pytest.mark.parametrize("rows", ROWSETS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("k", [768, 4096, 4352, 14336])
@pytest.mark.parametrize("t", SAME_TYPES, ids=lambda t: T.NAMES[t])
def test_same_type_fused_launch(gpu, oracle, t, k, rows):
    _case(gpu, oracle, tuple((t, m) for m in rows), k, 1100 + k % 101 + len(rows))


@pytest.mark.parametrize("k", [256, 1024])
@pytest.mark.parametrize("t", SAME_TYPES, ids=lambda t: T.NAMES[t])
def test_long_walk_crosses_the_boundaries(gpu, oracle, t, k):
    _case(gpu, oracle, ((t, 4128), (t, 2080), (t, 2064)), k, 1300 + k % 89)


TWO_TYPE_SPECS = [(((T.Q4_K, 96), (T.Q4_K, 40), (T.Q6_K, 48)), k) for k in (768, 4096, 14336)] + \
                 [(((T.Q5_K, 64), (T.Q6_K, 33)), k) for k in (768, 4096, 14336)] + \
                 [(((T.Q4_K, 4128), (T.Q4_K, 1040), (T.Q6_K, 1040)), 256)]


@pytest.mark.parametrize("spec,k", TWO_TYPE_SPECS, ids=lambda v: str(v) if isinstance(v, int) else "+".join(f"{T.NAMES[t]}.{m}" for t, m in v))
def test_two_type_fused_launch(gpu, oracle, spec, k):
    _case(gpu, oracle, spec, k, 1500 + k % 83)


@pytest.mark.parametrize("spec", [((T.Q4_K, 48), (T.Q4_K, 16), (T.Q4_K, 80)), ((T.Q6_K, 33), (T.Q6_K, 40)),
                                  ((T.Q4_K, 48), (T.Q4_K, 16), (T.Q4_K, 80), (T.Q4_K, 33)), ((T.Q4_K, 96), (T.Q4_K, 40), (T.Q6_K, 48)),
                                  ((T.Q5_K, 64), (T.Q6_K, 33))],
                         ids=lambda v: "+".join(f"{T.NAMES[t]}.{m}" for t, m in v))
def test_direct_call_with_an_offset_row_and_wide_results(gpu, oracle, spec):
    """lfamd_mul_mat_multi / _multi_types by hand: the activation row 48 bytes into a larger buffer with a row stride beyond the row,
    result buffers of ldc = m + 19 filled with a sentinel.  The results are the plain call's bits and nothing at index >= m moves."""
    from llamafile_amd import _hip
    k, pad, sentinel = 4096, 19, -7.25
    fused, Ws, xd, x = _case(gpu, oracle, spec, k, 1700 + len(spec))
    L = _hip.lib()
    big = torch.full((3 * k + 64,), 1e30, dtype=torch.float32, device="cuda")
    big[12:12 + k] = torch.from_numpy(x[0]).cuda()
    cnt = len(spec)
    outs = [torch.full((m + pad,), sentinel, dtype=torch.float32, device="cuda") for _, m in spec]
    A_arr = (C.c_void_p * cnt)(*[w.data.data_ptr() for w in Ws])
    C_arr = (C.c_void_p * cnt)(*[o.data_ptr() for o in outs])
    m_arr = (C.c_long * cnt)(*[m for _, m in spec])
    ldc_arr = (C.c_long * cnt)(*[m + pad for _, m in spec])
    need = max(L.lfamd_mul_mat_workspace(t, m, k, 1) for t, m in spec)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    b_ptr, brb, stream = C.c_void_p(big.data_ptr() + 48), 2 * k * 4 + 64, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if len({t for t, _ in spec}) > 1:
        t_arr = (C.c_int * cnt)(*[t for t, _ in spec])
        rc = L.lfamd_mul_mat_multi_types(cnt, t_arr, A_arr, m_arr, k, T.F32, b_ptr, brb, 1, C_arr, ldc_arr, C.c_void_p(ws.data_ptr()),
                                         ws.numel(), 0, stream)
    else:
        rc = L.lfamd_mul_mat_multi(spec[0][0], cnt, A_arr, m_arr, k, T.F32, b_ptr, brb, 1, C_arr, ldc_arr, C.c_void_p(ws.data_ptr()),
                                   ws.numel(), 0, stream)
    assert rc == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    for j, (_, m) in enumerate(spec):
        got = outs[j].cpu().numpy()
        assert np.array_equal(got[:m].view(np.uint32), fused[j][0].view(np.uint32)), j
        assert (got[m:] == sentinel).all(), j
