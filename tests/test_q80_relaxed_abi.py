"""CPU: LFAMD_FLAG_Q80_RELAXED at the ABI — the flag's value, the new predicate lfamd_mul_mat_is_bit_exact beside
lfamd_mul_mat_is_exact, and the workspace, which the flag does not change.  No device call is made."""
import ctypes as C
import os

import pytest

from llamafile_amd import _hip, ggml_types as T

R, P, X, G, V = 128, _hip.FLAG_PRECISE, _hip.FLAG_Q80_EXACT, _hip.FLAG_FORCE_GENERIC, _hip.FLAG_Q0_VREGS32


@pytest.fixture(scope="module")
def lib():
    return _hip.lib()


def test_the_flag_and_the_export(lib):
    assert _hip.FLAG_Q80_RELAXED == 128
    assert "lfamd_mul_mat_is_bit_exact" in _hip.EXPORTS
    assert lib.lfamd_abi_version() == 1
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfamd_hip.h")) as f:
        assert "#define LFAMD_FLAG_Q80_RELAXED 128u" in f.read()


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("m,k", [(4096, 4096), (7, 32), (64, 14336)])
def test_bit_exact_follows_the_route(lib, m, k, n):
    be = lambda f: lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, m, k, n, f)  # noqa: E731
    assert (be(0), be(R), be(R | P), be(R | X)) == (1, 0, 1, 1)
    assert be(V) == 1 and be(R | V) == 0  # (FORCE_GENERIC on packed Q8_0 is refused with or without the flag: no result to speak of)
    assert be(R | G) == be(G)
    for f in (0, R, R | P, R | X, R | V):
        assert lib.lfamd_mul_mat_is_exact(T.Q8_0, m, k, n, f) == 1  # integer block dots, f32 sums: "exact" either way


def test_batches_and_other_types_ignore_the_flag(lib):
    for m, k in [(4096, 4096), (96, 160)]:
        for f in (0, P, X):
            assert lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, m, k, 9, f | R) == lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, m, k, 9, f)
            assert lib.lfamd_mul_mat_is_exact(T.Q8_0, m, k, 9, f | R) == lib.lfamd_mul_mat_is_exact(T.Q8_0, m, k, 9, f)
    assert lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, 4096, 4096, 9, X) == 1  # the bit-exact batch kernel
    assert lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, 4096, 4096, 9, 0) == 0  # the f16 MFMA body
    for t in (T.Q4_K, T.Q6_K, T.Q4_0, T.F16):
        for n in (1, 8, 9):
            assert lib.lfamd_mul_mat_is_bit_exact(t, 4096, 4096, n, 0) == 0 == lib.lfamd_mul_mat_is_bit_exact(t, 4096, 4096, n, R)
            assert lib.lfamd_mul_mat_is_exact(t, 4096, 4096, n, R) == lib.lfamd_mul_mat_is_exact(t, 4096, 4096, n, 0)
    assert lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, 0, 4096, 1, 0) == 0 and lib.lfamd_mul_mat_is_bit_exact(999, 64, 4096, 1, 0) == 0


def test_rows_the_relaxed_plan_declines_stay_bit_exact(lib):
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_q80_relaxed_cols.argtypes = [C.c_long]
    k = 262144
    assert L.lfamd_gemv_q80_relaxed_cols(k) == 0
    assert lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, 64, k, 1, R) == 1 == lib.lfamd_mul_mat_is_bit_exact(T.Q8_0, 64, k, 1, 0)


def test_the_workspace_does_not_depend_on_the_flag(lib):
    """lfamd_mul_mat_workspace takes no flags; the relaxed kernel needs none, so the sizes are what the calls without it need."""
    for n in (1, 8):
        assert lib.lfamd_mul_mat_workspace(T.Q8_0, 4096, 4096, n) == 0
    for f in (0, R):
        assert lib.lfamd_mul_mat_takes_staged_q80(T.Q8_0, 4096, 4096, 1, f) == 0
        assert lib.lfamd_mul_mat_takes_staged_q80(T.Q8_0, 4096, 4096, 64, f) == lib.lfamd_mul_mat_takes_staged_q80(T.Q8_0, 4096, 4096, 64, 0)
