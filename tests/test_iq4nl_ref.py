"""IQ4_NL without a GPU: the yardstick of tests/iq4nl_ref.py against itself, and the answers of the C ABI that need no device
(sizes, exactness, workspace, the decode plan).  The ABI answers fail on a build that does not know type 20."""
import ctypes as C
import os

import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
import iq4nl_ref as R
from test_gemv_plan import MULTI, PLAIN, EARLY, ROWS32, Plan, check_single_grid, half_tiles

P4K_TILE = 4608  # bytes of one 32-row x 256-weight tile of the P40 image (csrc/lfamd_device.h)


def test_the_codebook_is_the_references():
    # the two forms the reference's CPU kernels load: unsigned (value + 128) and signed
    u8 = np.array([1, 24, 45, 63, 79, 93, 106, 118, 129, 141, 153, 166, 181, 197, 217, 241], dtype=np.uint8)
    i8 = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.int8)
    assert np.array_equal(u8.astype(np.int32) - 128, i8.astype(np.int32))
    assert np.array_equal(R.KVALUES, i8) and R.KVALUES.dtype == np.int8
    assert (np.diff(R.KVALUES.astype(np.int32)) > 0).all() and 0 not in R.KVALUES


def test_the_block_walk():
    raw = np.zeros((1, 36), dtype=np.uint8)
    raw[0, 0:2] = np.array([0.5], dtype=np.float16).view(np.uint8)
    raw[0, 18:20] = np.array([-2.0], dtype=np.float16).view(np.uint8)
    raw[0, 2:18] = np.arange(16, dtype=np.uint8) | ((15 - np.arange(16, dtype=np.uint8)) << 4)  # low nibbles 0..15, high 15..0
    raw[0, 20:36] = 0x8F  # low nibbles 15, high nibbles 8
    w = R.dequantize(raw)
    kv = R.KVALUES.astype(np.float32)
    assert w.shape == (1, 64) and w.dtype == np.float32
    assert np.array_equal(w[0, :16], 0.5 * kv) and np.array_equal(w[0, 16:32], 0.5 * kv[::-1])
    assert np.array_equal(w[0, 32:48], np.full(16, -2.0 * 113, np.float32)) and np.array_equal(w[0, 48:], np.full(16, -2.0, np.float32))
    assert T.BLCK[T.IQ4_NL] == 32 and T.TYPE_SIZE[T.IQ4_NL] == 18 and T.VEC_DOT[T.IQ4_NL] == T.Q8_0 and T.NAMES[T.IQ4_NL] == "IQ4_NL"
    assert T.IQ4_NL == 20 and T.IQ4_NL not in T.QUANT_WEIGHT_TYPES


def test_signed_zeros_come_back_positive():
    raw = np.zeros((1, 36), dtype=np.uint8)
    raw[0, 18:20] = np.array([-0.0], dtype=np.float16).view(np.uint8)
    raw[0, 20:36] = 0xFF  # value 113 under d = -0: the product is -0, the read-back value +0
    assert (R.dequantize(raw).view(np.uint32) == 0).all()


@pytest.mark.parametrize("m,k", [(256, 256), (512, 4096), (512, 14336), (300, 28672), (67, 288)])
def test_the_two_forms_of_the_dot_agree(m, k):
    """The integer-dot form and dequantise-then-f64 differ only by the one f32 rounding of d * d8 against the two roundings of
    d * value and d8 * q8: 2e-7 relative is the oracle's own pinning rule."""
    raw = synth.random_weights(T.IQ4_NL, m, k, 5)
    B = R.activations(synth.random_activations(3, k, 6))
    a, b = R.dot_ref(raw, B), R.dot_dequant(raw, B)
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"dot_ref vs dequantised f64, {m} x {k}: {err:.3e}")
    assert err <= 2e-7


def test_extreme_weights_hold_what_they_promise():
    raw = R.extreme_weights(64, 1024, 3)
    c, d = R.codes(raw), R.scales(raw)
    assert (c[R.BAND_MIN] == 0).all() and (c[R.BAND_MAX] == 15).all() and (c[R.BAND_ALT, 0, :16] == 0).all() and (c[R.BAND_ALT, 0, 16:] == 15).all()
    assert (d[R.ZERO_ROW] == 0).all() and (d < 0).any() and (np.abs(d) == 65504.0).any() and (np.abs(d) == np.float32(2.0 ** -20)).any()
    assert (d[1] == 0).any() and np.isfinite(R.dequantize(raw)).all()


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    L = C.CDLL(_hip.HIP_SO)
    sz, l, i, u = C.c_size_t, C.c_long, C.c_int, C.c_uint
    L.lfamd_packed_size.restype, L.lfamd_packed_size.argtypes = sz, [i, l, l]
    L.lfamd_mul_mat_is_exact.restype, L.lfamd_mul_mat_is_exact.argtypes = i, [i, l, l, l, u]
    L.lfamd_mul_mat_workspace.restype, L.lfamd_mul_mat_workspace.argtypes = sz, [i, l, l, l]
    L.lfamd_gemv_plan_of.argtypes = [i, i, i, l, l, l, i, i, C.POINTER(Plan)]
    L.lfamd_gemv_has_kernel.argtypes = [i, i, C.POINTER(Plan)]
    L.lfamd_gemv_lds_bytes.restype, L.lfamd_gemv_lds_bytes.argtypes = sz, [i, i, l, i, i]
    L.lfamd_gemv_cols_per_launch.argtypes = [i, l]
    return L


def test_sizes_of_the_resident_image(lib):
    assert lib.lfamd_packed_size(T.IQ4_NL, 4096, 4096) == lib.lfamd_packed_size(T.Q4_0, 4096, 4096) == 128 * 16 * P4K_TILE
    assert lib.lfamd_packed_size(T.IQ4_NL, 67, 1024) == lib.lfamd_packed_size(T.Q4_0, 67, 1024) == 3 * 4 * P4K_TILE
    assert lib.lfamd_packed_size(T.IQ4_NL, 64, 288) == 64 * 9 * 18  # not whole 256-weight groups: the GGUF rows
    assert lib.lfamd_packed_size(T.IQ4_NL, 64, 300) == 0            # not whole blocks
    assert lib.lfamd_packed_size(99, 4096, 4096) == 0


@pytest.mark.parametrize("n", [1, 8, 9, 512])
def test_every_call_is_exact_and_takes_q40s_workspace(lib, n):
    assert lib.lfamd_mul_mat_is_exact(T.IQ4_NL, 4096, 4096, n, 0) == 1
    for m, k in [(4096, 4096), (14336, 4096), (4096, 14336), (67, 256), (64, 288), (64, 4000)]:
        assert lib.lfamd_mul_mat_is_exact(T.IQ4_NL, m, k, n, 0) == 1
        assert lib.lfamd_mul_mat_workspace(T.IQ4_NL, m, k, n) == lib.lfamd_mul_mat_workspace(T.Q4_0, m, k, n), (m, k, n)


def test_every_planned_decode_launch_has_its_kernel(lib):
    """The shape grid of test_gemv_plan.py's invariants, on devices of 256, 64 and 32 CUs."""
    checked = 0
    for cus in (256, 64, 32):
        n_hts = sorted({2, 4, 34, cus // 2 * 2, cus, cus + 2, 2 * cus, 8 * cus - 2, 8 * cus, 15 * cus, 16 * cus, 16 * cus + 2, 31 * cus,
                        32 * cus, 8016, half_tiles(128256), half_tiles(14336), half_tiles(4096)})
        for nb in (1, 3, 16, 17, 32, 33, 40, 56, 400):
            k = nb * 256
            for n_ht in n_hts:
                for count in (1, 2, 3):
                    for nc in range(1, lib.lfamd_gemv_cols_per_launch(T.IQ4_NL, k) + 1):
                        p = Plan()
                        assert lib.lfamd_gemv_plan_of(MULTI, T.IQ4_NL, nc, n_ht, 0, k, count, cus, C.byref(p)) == 0
                        assert p.variant in (PLAIN, EARLY, ROWS32) and (p.variant == ROWS32) == (p.rows == 32)
                        check_single_grid(lib, T.IQ4_NL, p, n_ht // 2 if p.variant == ROWS32 else n_ht, k, cus)
                        checked += 1
    assert checked > 5000
