"""The launch plan of the relaxed-order Q8_0 decode GEMV (csrc/gemv.hip: lfamd_gemv_plan_of, kind LFAMD_GEMV_MULTI_RELAXED = 4,
variant LFAMD_GEMV_Q80R = 7) without a GPU: waves, quads per chunk, the even-share grid and the LDS bytes on devices of 256, 64
and 32 CUs.  tests/test_gemv_plan.py pins the kinds and variants that were there before; on the commit before this kind existed
the plan answers -1 to it."""
import ctypes as C
import os

import pytest

from llamafile_amd import _hip, ggml_types as T

MULTI, MULTI_RELAXED = 0, 4
Q80, Q80R = 6, 7
KS = (32, 128, 544, 4096, 4224, 14336)
CUS = (256, 64, 32)
WORKS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 1792, 4001)
X80_QUAD, IMAGE_CAP = 144, 150 * 1024
# (waves, quads per chunk) of each k, written out: 16 waves; a wave's share of the row's quads (k / 128, rounded up)
# is ceil(quads / 16) = 1, 1, 1, 2, 3, 7, taken in chunks of that share up to 2 and of 4 beyond.  tests/q80r_ref.py restates the
# order of the sum from these two numbers, so a change of either changes every result's bits.
FORMS = {32: (16, 1), 128: (16, 1), 544: (16, 1), 4096: (16, 2), 4224: (16, 4), 14336: (16, 4)}


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_has_kernel.argtypes = [C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_q80_relaxed_cols.argtypes = [C.c_long]
    L.lfamd_gemv_q80_relaxed_lds_bytes.argtypes = [C.c_int, C.c_long]
    L.lfamd_gemv_q80_relaxed_lds_bytes.restype = C.c_size_t
    return L


def plan_of(lib, kind, t, nc, work, k, count, cus):
    p = Plan()
    return lib.lfamd_gemv_plan_of(kind, t, nc, work, 0, k, count, cus, C.byref(p)), p


def layout_bytes(nc, k, nw):
    """gemv_launch.h, q80r_lds_of: the image [nc][nquads] of 144 bytes, one quad of zeros, the reduction buffers f32 [2][nw][nc][8]."""
    nquads = (k // 32 + 3) // 4
    return nc * nquads * X80_QUAD + X80_QUAD + 2 * nw * nc * 8 * 4


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("k", KS)
def test_the_relaxed_kind_is_planned(lib, k, cus):
    step = lib.lfamd_gemv_q80_relaxed_cols(k)
    assert step == 8  # (every k of this list fits eight columns under the cap)
    forms = set()
    for nc in range(1, step + 1):
        for work in WORKS:
            for count in (1, 3):
                rc, p = plan_of(lib, MULTI_RELAXED, T.Q8_0, nc, work, k, count, cus)
                assert rc == 0, (nc, work, k, cus)
                assert (p.variant, p.nc, p.rows, p.grid_b) == (Q80R, nc, 8, 0)
                per_wg = -(-work // cus)  # every work-group the same number of items, at most one work-group per CU
                assert p.grid == -(-work // per_wg) and 1 <= p.grid <= cus and p.grid * per_wg >= work > (p.grid - 1) * per_wg
                nquads = (k // 32 + 3) // 4
                assert (p.nw, p.ch) == FORMS[k], (nc, work, k, cus)
                qpw = -(-nquads // p.nw)  # the chunk never exceeds a wave's share rounded up to the chunk sizes there are
                assert p.ch == (1 if qpw <= 1 else 2 if qpw <= 2 else 4)
                assert p.lds == layout_bytes(nc, k, p.nw) == lib.lfamd_gemv_q80_relaxed_lds_bytes(nc, k) <= IMAGE_CAP
                assert p.nw * 64 <= 1024
                assert lib.lfamd_gemv_has_kernel(T.Q8_0, 1, C.byref(p)) and lib.lfamd_gemv_has_kernel(T.Q8_0, 0, C.byref(p))
                forms.add((p.nw, p.ch))
    assert forms == {FORMS[k]}, forms  # waves and chunk depend on k alone: so does the order of an output's sum


def test_only_q8_0_has_the_kind(lib):
    for t in T.QUANT_WEIGHT_TYPES:
        if t != T.Q8_0:
            assert plan_of(lib, MULTI_RELAXED, t, 1, 64, 4096, 1, 256)[0] == -1, T.NAMES[t]
    for t in (T.F32, T.F16, T.BF16):
        assert plan_of(lib, MULTI_RELAXED, t, 1, 64, 4096, 1, 256)[0] == -1
    assert plan_of(lib, MULTI_RELAXED, T.Q8_0, 1, 0, 4096, 1, 256)[0] == -1  # no work
    assert plan_of(lib, MULTI_RELAXED, T.Q8_0, 1, 64, 4096, 1, 0)[0] == -1  # no CUs


def test_deep_rows_split_the_columns_then_decline(lib):
    """The launcher steps the columns by lfamd_gemv_q80_relaxed_cols(k); where one column does not fit, the plan answers -1 (the
    call runs gemv_q80_kernel)."""
    last = 8
    for k in (14336, 16384, 28672, 65536, 131072, 135168, 139264, 262144):
        step = lib.lfamd_gemv_q80_relaxed_cols(k)
        assert 0 <= step <= last
        last = step
        for nc in range(1, 9):
            rc, p = plan_of(lib, MULTI_RELAXED, T.Q8_0, nc, 512, k, 1, 256)
            assert (rc == 0) == (nc <= step), (k, nc, step)
            assert (layout_bytes(nc, k, 16) <= IMAGE_CAP) == (nc <= step)
            if rc == 0:
                assert p.lds <= IMAGE_CAP and lib.lfamd_gemv_has_kernel(T.Q8_0, 1, C.byref(p)) and lib.lfamd_gemv_has_kernel(T.Q8_0, 0, C.byref(p))
    assert lib.lfamd_gemv_q80_relaxed_cols(28672) < 8 and lib.lfamd_gemv_q80_relaxed_cols(262144) == 0
    assert lib.lfamd_gemv_q80_relaxed_cols(100) == 0 and lib.lfamd_gemv_q80_relaxed_cols(0) == 0  # not rows of whole blocks


def test_the_exact_kind_is_what_it_was(lib):
    rc, p = plan_of(lib, MULTI, T.Q8_0, 1, 512, 4096, 1, 256)
    assert rc == 0 and (p.variant, p.nw, p.ch, p.grid, p.rows, p.lds) == (Q80, 2, 0, 256, 8, 32 * X80_QUAD)
