"""CPU: the NumPy order model of the relaxed Q8_0 GEMV (tests/q80r_ref.py) against the f64 sum of the same terms, on the shapes
of tests/test_gpu_q80_relaxed.py.  The GPU test holds the kernel to 2e-6 normwise and 2e-6 * sum |t| per element; a fixed order
of f32 adds over 8 * k / 32 terms has to land ten times inside that (a trial of this order at (64, 128), (64, 4096) and
(40, 14336) gave <= 1.5e-7 normwise and <= 4.6e-8 * sum |t|), or the bound would say nothing about the kernel."""
import ctypes as C

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
from helpers import rel_err
import q80r_ref


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


def plan_waves(k):
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    p = Plan()
    assert L.lfamd_gemv_plan_of(4, T.Q8_0, 1, 8, 0, k, 1, 256, C.byref(p)) == 0
    return p.nw


@pytest.mark.parametrize("m,k", [(64, 32), (64, 96), (64, 128), (64, 160), (64, 544), (64, 4096), (64, 4224), (40, 14336)])
def test_the_order_is_ten_times_inside_the_gpu_bound(m, k):
    A = synth.random_weights(T.Q8_0, m, k, 500 + k)
    B = synth.quantize_activations(T.Q8_0, synth.random_activations(2, k, 501 + k))
    G, S = q80r_ref.f64_reference(A, B)
    Cm = q80r_ref.relaxed_model(A, B, plan_waves(k))
    assert Cm.dtype == np.float32 and Cm.shape == G.shape == (2, m)
    assert rel_err(Cm, G) <= 2e-6
    assert (np.abs(Cm.astype(np.float64) - G) <= 2e-7 * S).all(), float((np.abs(Cm - G) / S).max())


def test_the_model_is_an_order_not_a_formula():
    """One block, one term per lane: the result is the lane tree of eight exact products, whatever the wave count."""
    A = synth.random_weights(T.Q8_0, 3, 32, 7)
    B = synth.quantize_activations(T.Q8_0, synth.random_activations(1, 32, 8))
    a, dot = q80r_ref.block_terms(A, B)
    v = (a[..., None].astype(np.float64) * dot).astype(np.float32)[:, :, 0, :]  # fma(a, b, 0) = f32(a * b)
    want = ((v[..., 0] + v[..., 4]) + (v[..., 2] + v[..., 6])) + ((v[..., 1] + v[..., 5]) + (v[..., 3] + v[..., 7]))
    for nw in (1, 4, 16):
        assert np.array_equal(q80r_ref.relaxed_model(A, B, nw).view(np.uint32), want.view(np.uint32))


def test_the_reference_sums_every_term_once():
    A = synth.random_weights(T.Q8_0, 5, 160, 9)
    B = synth.quantize_activations(T.Q8_0, synth.random_activations(2, 160, 10))
    G, S = q80r_ref.f64_reference(A, B)
    dA, qA = q80r_ref.decode_q8_0(A)
    dB, qB = q80r_ref.decode_q8_0(B)
    want = np.einsum("nl,ml,mlx,nlx->nm", dB.astype(np.float64), dA.astype(np.float64), qA.astype(np.float64), qB.astype(np.float64))
    assert rel_err(G, want) <= 1e-6 and (S >= np.abs(G)).all()
