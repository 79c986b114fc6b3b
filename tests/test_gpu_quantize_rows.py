"""lfamd_quantize_rows (csrc/quantize.hip) against the oracle's scalar quantisers byte for byte: Q8_0 / Q8_1 / Q8_K on the extreme
activations of extremes.py plus rows whose block maximum is shared by opposite signs, row lengths with an odd count of 32-blocks
(the Q8_0 / Q8_1 kernel's second half-wave is idle on the last pair), padded strides on both sides with sentinels in the gaps,
and the shapes it must refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T
import producer_ref as R
from extremes import extreme_activations, for_vec_dot

pytestmark = pytest.mark.gpu

SENT = 0x5A
COLS = {T.Q8_0: (32, 96, 256, 1056, 4096, 14336), T.Q8_1: (32, 96, 256, 1056, 4096, 14336), T.Q8_K: (256, 4096, 14336)}
CASES = [(t, n, cols) for t in (T.Q8_0, T.Q8_1, T.Q8_K) for cols in COLS[t] for n in (1, 7, 300)]


def _inputs(t, n, cols, seed):
    x = for_vec_dot(extreme_activations(n, cols, seed), t)
    ties = R.tie_rows(cols, T.BLCK[t], seed + 1)
    return np.ascontiguousarray(np.concatenate([x, ties]))


@pytest.mark.parametrize("t,n,cols", CASES, ids=[f"{T.NAMES[t]}-{n}x{cols}" for t, n, cols in CASES])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_quantize_rows_matches_the_oracle(gpu, oracle, t, n, cols, strided):
    L = _hip.lib()
    x = _inputs(t, n, cols, cols + n + t)
    rows = x.shape[0]
    rs = T.row_size(t, cols)
    pin, pout = (20, 12) if strided else (0, 0)
    xd = torch.full((rows, cols + pin), 1e30, dtype=torch.float32, device="cuda")
    xd[:, :cols] = torch.from_numpy(x)
    y = torch.full((rows * (rs + pout) + 64,), SENT, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lfamd_quantize_rows(t, C.c_void_p(xd.data_ptr()), rows, cols, (cols + pin) * 4, C.c_void_p(y.data_ptr()), rs + pout, st)
    assert rc == 0, L.lfamd_last_error()
    torch.cuda.synchronize()
    a = y.cpu().numpy()
    body = a[:rows * (rs + pout)].reshape(rows, rs + pout)
    assert (body[:, rs:] == SENT).all() and (a[rows * (rs + pout):] == SENT).all(), "a gap or guard byte was written"
    want = oracle.quantize(t, x)
    bad = int((body[:, :rs] != want).sum())
    print(T.NAMES[t], rows, cols, "strided" if strided else "dense", f"{bad} of {want.size} bytes differ")
    assert bad == 0, np.unique(np.nonzero(body[:, :rs] != want)[0])[:8]


@pytest.mark.parametrize("t,cols", [(T.Q8_0, 32), (T.Q8_1, 32), (T.Q8_K, 256)], ids=lambda v: str(v))
def test_quantize_rows_at_the_row_limit(gpu, oracle, t, cols):
    """65,535 rows, the most one call takes (one grid row per input row)."""
    n = 65535
    rng = np.random.default_rng(t)
    x = ((rng.random((n, cols), dtype=np.float32) * 2 - 1) * rng.choice(np.float32([1e-2, 1.0, 1e3]), (n, 1))).astype(np.float32)
    got = gpu.quantize_rows(t, torch.from_numpy(x).cuda()).cpu().numpy()
    assert int((got != oracle.quantize(t, x)).sum()) == 0


def test_quantize_rows_refuses_bad_shapes(gpu):
    L = _hip.lib()
    x = torch.ones((4, 512), dtype=torch.float32, device="cuda")
    y = torch.full((4 * 1024,), SENT, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(t, n, cols, yrb):
        return L.lfamd_quantize_rows(t, C.c_void_p(x.data_ptr()), n, cols, 2048, C.c_void_p(y.data_ptr()), yrb, st)

    for t, cols in ((T.Q8_0, 48), (T.Q8_1, 500), (T.Q8_K, 384)):  # not a block multiple
        assert call(t, 4, cols, 1024) == -2
    for t in (T.Q8_0, T.Q8_1, T.Q8_K):  # output rows too short
        assert call(t, 4, 512, T.row_size(t, 512) - 1) == -2
    assert call(T.Q8_K, 65536, 512, T.row_size(T.Q8_K, 512)) == -2  # one grid row per input row
    assert call(T.F32, 4, 512, 2048) == -1
    assert call(T.Q8_K, 0, 512, T.row_size(T.Q8_K, 512)) == 0
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
