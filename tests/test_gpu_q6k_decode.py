"""Q6_K decode GEMV (gemv_impl.h q6k_traits): the code placement from the qh fields, the scale-pair offset term and the
work-group order that keeps both half-tiles of a tile on one XCD, against the oracle.  Extreme codes (all 0, all 63) and
extreme scales (-128, 127); rows of 17 and 56 super-blocks (the 16-wave walk leaves empty slots in half of the waves);
ragged m; several matrices in one launch and the Q4_K + Q6_K dual launch; f32 and pre-quantised activations, which must
agree bit for bit."""
import numpy as np
import pytest
import torch

from llamafile_amd import ggml_types as T, synth
from helpers import rel_err

pytestmark = pytest.mark.gpu

QL, QH, SC, D = 0, 128, 192, 208  # block_q6_K: ql[128], qh[64], scales[16] (int8), d (f16); 210 bytes


def q6k_weights(m, k, seed):
    """Random Q6_K rows with bands of extreme blocks: codes all 0, codes all 63, scales all -128, scales all 127, and
    scales alternating -128 / 127 over codes all 63."""
    raw = synth.random_weights(T.Q6_K, m, k, seed)
    blk = raw.reshape(m, k // 256, 210)
    band = np.arange(m) % 8
    blk[band == 1, :, QL:SC] = 0x00
    blk[band == 2, :, QL:SC] = 0xFF
    blk[band == 3, :, SC:D] = 0x80
    blk[band == 4, :, SC:D] = 0x7F
    blk[band == 5, :, QL:SC] = 0xFF
    blk[band == 5, :, SC:D] = np.tile(np.array([0x80, 0x7F], np.uint8), 8)
    blk[:, 1::5, QL:SC] ^= 0xFF  # every fifth super-block of every row mirrored as well
    return raw


def sample_rows(m):
    return np.arange(m) if m <= 256 else np.unique(np.concatenate([np.arange(0, m, 37), np.arange(48), np.arange(m - 48, m)]))


def run_both(gpu, W, x, n):
    k = x.shape[1]
    Bq = synth.quantize_activations(T.Q8_K, x)
    c_f32 = gpu.mul_mat(W, torch.from_numpy(x).cuda().view(torch.uint8).view(n, k * 4), T.F32, n=n).cpu().numpy()
    c_q = gpu.mul_mat(W, torch.from_numpy(Bq).cuda(), T.Q8_K, n=n).cpu().numpy()
    assert np.array_equal(c_f32.view(np.uint32), c_q.view(np.uint32))
    return c_q, Bq


# (m, k): one half-tile per CU at most (the 8-wave form), 64 and 256 half-tiles, 258 (a ragged last tile and two half-tiles
# past the last run of 16 items), the full ffn_down shape; k = 4352 / 14336 rows leave empty slots in the 16-wave walk
SHAPES = [(40, 4352), (1000, 4352), (1000, 14336), (4104, 14336), (4096, 14336), (4104, 4096)]


@pytest.mark.parametrize("m,k", SHAPES, ids=lambda v: str(v))
def test_q6k_extremes_vs_oracle(gpu, oracle, m, k):
    raw = q6k_weights(m, k, 900 + m % 97 + k % 89)
    x = synth.random_activations(1, k, 31 + k % 7)
    x[0, 512:768] = 0.0  # an all-zero block
    x[0, 1024:1280] = -1.0  # a block of equal values: codes of -128 (pre-quantised: the activation side's extreme)
    W = gpu.upload_weights(T.Q6_K, raw, m, k)
    c, Bq = run_both(gpu, W, x, 1)
    rows = sample_rows(m)
    ok, G = oracle.sgemm(T.Q6_K, np.ascontiguousarray(raw[rows]), T.Q8_K, Bq, len(rows), 1, k, nth=4)
    assert ok == 1
    assert rel_err(c[:, rows], G) <= 1e-5, rel_err(c[:, rows], G)


@pytest.mark.parametrize("k", [4352, 14336])
def test_q6k_multi_matrix_launch(gpu, oracle, k):
    """Two Q6_K matrices on one activation row (concatenated half-tiles, one launch) against the oracle and against their
    own launches (which may split the row over another number of waves: same integer dots, f32 sums in another order)."""
    ms = (1000, 4104)
    raws = [q6k_weights(m, k, 40 + i) for i, m in enumerate(ms)]
    Ws = [gpu.upload_weights(T.Q6_K, r, m, k) for r, m in zip(raws, ms)]
    x = synth.random_activations(1, k, 41)
    xd = torch.from_numpy(x).cuda().view(torch.uint8).view(1, k * 4)
    outs = [o.cpu().numpy() for o in gpu.mul_mat_multi(Ws, xd, T.F32, n=1)]
    Bq = synth.quantize_activations(T.Q8_K, x)
    for raw, m, W, o in zip(raws, ms, Ws, outs):
        alone = gpu.mul_mat(W, xd, T.F32, n=1).cpu().numpy()
        assert rel_err(o, alone) <= 1e-6
        rows = sample_rows(m)
        ok, G = oracle.sgemm(T.Q6_K, np.ascontiguousarray(raw[rows]), T.Q8_K, Bq, len(rows), 1, k, nth=4)
        assert ok == 1
        assert rel_err(o[:, rows], G) <= 1e-5


@pytest.mark.parametrize("k", [4096, 4352])
@pytest.mark.parametrize("act", ["f32", "q8k"])
def test_q4k_q6k_dual_launch(gpu, oracle, k, act):
    """attn_q / attn_k in Q4_K with attn_v in Q6_K: the two-type launch, f32 and pre-quantised activations."""
    specs = [(T.Q4_K, 2048), (T.Q4_K, 520), (T.Q6_K, 520)]
    raws = [q6k_weights(m, k, 60 + i) if t == T.Q6_K else synth.random_weights(t, m, k, 60 + i) for i, (t, m) in enumerate(specs)]
    Ws = [gpu.upload_weights(t, r, m, k) for r, (t, m) in zip(raws, specs)]
    x = synth.random_activations(1, k, 61)
    Bq = synth.quantize_activations(T.Q8_K, x)
    if act == "f32":
        B, bt = torch.from_numpy(x).cuda().view(torch.uint8).view(1, k * 4), T.F32
    else:
        B, bt = torch.from_numpy(Bq).cuda(), T.Q8_K
    outs = [o.cpu().numpy() for o in gpu.mul_mat_multi(Ws, B, bt, n=1)]
    for raw, (t, m), W, o in zip(raws, specs, Ws, outs):
        alone = gpu.mul_mat(W, B, bt, n=1).cpu().numpy()
        assert rel_err(o, alone) <= 1e-6
        rows = sample_rows(m)
        ok, G = oracle.sgemm(t, np.ascontiguousarray(raw[rows]), T.Q8_K, Bq, len(rows), 1, k, nth=4)
        assert ok == 1
        assert rel_err(o[:, rows], G) <= 1e-5, (T.NAMES[t], m, rel_err(o[:, rows], G))
