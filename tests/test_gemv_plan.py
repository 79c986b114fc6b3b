"""The decode GEMVs' launch plan (csrc/gemv.hip: lfamd_gemv_plan_of) without a GPU: which kernel form, how many waves, which
grid and how much LDS a launch gets, on devices of 256, 64, 32 and other CU counts (the CU count is an argument).

tests/golden/gemv_plan_parent.csv was recorded from the commit BEFORE the plan existed: the host objects of gemv.hip and the
13 gemv_<type>.hip were linked with g++ against a stand-in for the HIP runtime that prints every hipLaunchKernel (kernel name,
grid, block, LDS bytes, arguments) and reports the CU count it is told to.  lfamd_launch_gemv_multi / _dual / _ids / _ids_pair
were then called on the CPU, and each launch's template arguments, grids and LDS bytes became one row (f32 and pre-quantised
activations gave the same row: it is kept once)."""
import csv
import ctypes as C
import os

import pytest

from llamafile_amd import _hip, ggml_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI, IDS, IDS_PAIR, DUAL = range(4)
PLAIN, EARLY, ROWS32, EXPERT, EXPERT_PAIR, TWO_TYPES, Q80 = range(7)
KQ_TYPES = (T.Q4_K, T.Q5_K, T.Q6_K, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.Q2_K, T.Q3_K, T.IQ4_XS)
ROWS32_TYPES = (T.Q6_K, T.Q2_K, T.Q3_K, T.IQ4_XS)
EXPERT_TYPES = (T.Q4_K, T.Q5_K, T.Q6_K)
# 150 KiB of activation image (the column stepping and the depth predicate enforce it) plus the reduction buffers and dummy
# slots: at most 5120 + 3072 at five columns on eight waves, or 2048 + 6144 at one column on sixteen
LDS_MAX = 150 * 1024 + 8192


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    assert "LFAMD_GEMV_PAIR_MIN" not in os.environ, "the development switch moves the 32-row bound this test pins"
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_has_kernel.argtypes = [C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_long, C.c_int, C.c_int]
    L.lfamd_gemv_lds_bytes.restype = C.c_size_t
    L.lfamd_gemv_cols_per_launch.argtypes = [C.c_int, C.c_long]
    L.lfamd_gemv_depth_ok.argtypes = [C.c_long]
    return L


def plan(lib, kind, t, nc, work, work_b, k, count, cus):
    p = Plan()
    assert lib.lfamd_gemv_plan_of(kind, t, nc, work, work_b, k, count, cus, C.byref(p)) == 0, (kind, t, nc, work, work_b, k, count, cus)
    return p


def half_tiles(m):
    return (m + 31) // 32 * 2


def test_the_recorded_launches_of_the_issue(lib):
    """Q4_K, f32 activations, one matrix, 256 CUs: (m, k, column of the launch, columns) -> NC, NW, CH, early, grid, block, LDS."""
    rows = [((4096, 4096, 0, 1), (1, 8, 2, True, 256, 512, 10240)), ((4096, 4096, 0, 8), (8, 8, 2, False, 256, 512, 60416)),
            ((14336, 4096, 0, 1), (1, 16, 1, True, 224, 1024, 14336)), ((14336, 4096, 0, 8), (8, 16, 1, False, 224, 1024, 71680)),
            ((4096, 14336, 0, 1), (1, 16, 2, True, 256, 1024, 29696)), ((4096, 14336, 0, 8), (5, 8, 4, False, 256, 512, 115712)),
            ((4096, 14336, 5, 8), (3, 8, 4, False, 256, 512, 70656)), ((128256, 4096, 0, 1), (1, 16, 1, True, 251, 1024, 14336)),
            ((1024, 8192, 0, 3), (3, 8, 4, False, 64, 512, 43008))]
    for (m, k, col0, n), want in rows:
        nc = min(n - col0, lib.lfamd_gemv_cols_per_launch(T.Q4_K, k))
        p = plan(lib, MULTI, T.Q4_K, nc, half_tiles(m), 0, k, 1, 256)
        assert p.variant in (PLAIN, EARLY) and p.grid_b == 0
        assert (p.nc, p.nw, p.ch, p.variant == EARLY, p.grid, p.nw * 64, p.lds) == want, (m, k, col0, n)
        assert lib.lfamd_gemv_has_kernel(T.Q4_K, 1, C.byref(p)) and lib.lfamd_gemv_has_kernel(T.Q4_K, 0, C.byref(p))


def test_the_plan_gives_what_the_launchers_before_it_gave(lib):
    with open(os.path.join(ROOT, "tests", "golden", "gemv_plan_parent.csv")) as f:
        rows = [{k: int(v) for k, v in r.items()} for r in csv.DictReader(f)]
    assert len(rows) > 2000
    assert {r["cus"] for r in rows} == {256, 64, 32} and {r["variant"] for r in rows} == set(range(7))
    assert {r["type"] for r in rows} == set(KQ_TYPES) | {T.Q8_0}
    for r in rows:
        p = plan(lib, r["kind"], r["type"], r["nc"], r["work"], r["work_b"], r["k"], r["count"], r["cus"])
        got = (p.variant, p.nc, p.nw, p.ch, p.grid, p.grid_b, p.rows, p.lds)
        assert got == tuple(r[c] for c in ("variant", "nc_out", "nw", "ch", "grid", "grid_b", "rows", "lds")), r
        assert lib.lfamd_gemv_has_kernel(r["type"], 0, C.byref(p)) and lib.lfamd_gemv_has_kernel(r["type"], 1, C.byref(p)), r


def test_depth_and_column_stepping(lib):
    assert lib.lfamd_gemv_depth_ok(400 * 256) == 1 and lib.lfamd_gemv_depth_ok(401 * 256) == 0  # 400 x 384 B = 150 KiB
    step = lib.lfamd_gemv_cols_per_launch
    assert [step(T.Q4_K, nb * 256) for nb in (1, 16, 32, 33, 56, 80, 81, 134, 200, 201, 400, 401)] == [8, 8, 8, 5, 5, 5, 4, 2, 2, 1, 1, 0]
    assert step(T.Q8_0, 4096) == 8 and step(T.Q8_0, 32 * 4 * 1066) == 1 and step(T.Q8_0, 32 * 4 * 1067) == 0


def ceil_div(a, b):
    return (a + b - 1) // b


def test_invariants_on_a_dense_grid(lib):
    """Conditions every planned launch meets, whatever the device.  Half-tile counts are even: a matrix of m rows brings
    2 * ceil(m / 32) of them."""
    checked = 0
    for cus in (256, 304, 64, 32, 7, 1):
        n_hts = sorted({2, 4, 34, cus // 2 * 2, cus + cus % 2, cus + cus % 2 + 2, 2 * cus, 8 * cus - 2, 8 * cus, 15 * cus + cus % 2, 16 * cus,
                        16 * cus + 2, 31 * cus + cus % 2, 32 * cus, 8016} - {0})
        for nb in (1, 3, 16, 17, 32, 33, 40, 56, 400):
            k = nb * 256
            for t in KQ_TYPES:
                for n_ht in n_hts:
                    for count in (1, 2):
                        for nc in range(1, lib.lfamd_gemv_cols_per_launch(t, k) + 1):
                            p = plan(lib, MULTI, t, nc, n_ht, 0, k, count, cus)
                            assert p.variant == (ROWS32 if p.rows == 32 else EARLY if nc == 1 and count == 1 else PLAIN)
                            long_walk = nc == 1 and (p.nw, p.ch) == (16, 1) and ceil_div(n_ht, cus) >= 16  # half-tiles per work-group
                            assert (p.variant == ROWS32) == (t in ROWS32_TYPES and long_walk)
                            items = n_ht // 2 if p.variant == ROWS32 else n_ht
                            check_single_grid(lib, t, p, items, k, cus)
                            checked += 1
                    if t in EXPERT_TYPES:
                        p = plan(lib, IDS, t, 1, n_ht, 0, k, 2, cus)
                        assert p.variant == EXPERT and ((p.nw, p.ch) == (8, 2)) == (nb <= 16 and n_ht >= 8 * cus)
                        check_single_grid(lib, t, p, n_ht, k, cus)
                        p = plan(lib, IDS_PAIR, t, 1, n_ht, 0, k, 2, cus)
                        assert p.variant == EXPERT_PAIR and p.grid == p.grid_b
                        check_pair_grid(lib, t, p, n_ht, k, cus)
                        checked += 2
                    if t in (T.Q4_K, T.Q5_K):
                        for n_ht_b in (2, 64, cus + cus % 2, 4 * cus):
                            p = plan(lib, DUAL, t, 1, n_ht, n_ht_b, k, 2, cus)
                            assert p.variant == TWO_TYPES
                            check_two_type_grid(lib, t, p, n_ht, n_ht_b, k, cus)
                            checked += 1
        for k in (32, 1024, 4096, 14336, 32 * 4 * 1066):
            for rgs in (2, 4, 1026, 16032):
                for nc in range(1, lib.lfamd_gemv_cols_per_launch(T.Q8_0, k) + 1):
                    p = plan(lib, MULTI, T.Q8_0, nc, rgs, 0, k, 1, cus)
                    assert (p.variant, p.nw, p.grid_b) == (Q80, 2, 0) and p.grid >= 1 and p.grid * p.nw >= rgs
                    assert p.lds == lib.lfamd_gemv_lds_bytes(T.Q8_0, nc, k, p.nw, p.rows) <= 150 * 1024
                    assert all(lib.lfamd_gemv_has_kernel(T.Q8_0, f, C.byref(p)) for f in (0, 1))
                    checked += 1
    assert checked > 50000


def check_lds_and_kernel(lib, t, p, k):
    assert (p.nw, p.ch) in ((8, 2), (8, 4), (16, 1), (16, 2))
    assert p.lds == lib.lfamd_gemv_lds_bytes(t, p.nc, k, p.nw, p.rows) <= LDS_MAX
    assert all(lib.lfamd_gemv_has_kernel(t, f, C.byref(p)) for f in (0, 1)), (t, p.variant, p.nc, p.nw, p.ch)


def check_single_grid(lib, t, p, items, k, cus):
    cap = (16 // p.nw) * cus  # 16 waves per CU
    assert p.grid_b == 0 and 1 <= p.grid <= cap
    assert p.grid * ceil_div(items, cap) >= items  # every work-group ceil(items / cap) items: all are covered
    check_lds_and_kernel(lib, t, p, k)


def check_pair_grid(lib, t, p, items, k, cus):
    """Two experts, each on half of the CUs' work-groups (two work-groups on a device of one CU: no cap on the sum)."""
    cap = max(cus // 2, 1)
    assert p.nw == 16 and 1 <= p.grid == p.grid_b <= cap
    assert p.grid * ceil_div(items, cap) >= items  # per half: every work-group ceil(items / cap) half-tiles
    check_lds_and_kernel(lib, t, p, k)


def check_two_type_grid(lib, t, p, items_a, items_b, k, cus):
    """At most one work-group per CU, split so that the dearer side (a Q6_K half-tile costs 135 against 100) ends first.  For gb
    work-groups on the Q6_K side the other side can do no better than all the rest, cus - gb, so the least
    max(100 * ceil(a / (cus - gb)), 135 * ceil(b / gb)) over gb is the best any split of cus work-groups reaches: the plan must
    reach it.  A device of one CU cannot split: equal shares, and the sum may exceed the CU count by one."""
    assert p.nw == 16 and 1 <= p.grid <= items_a and 1 <= p.grid_b <= items_b
    per_a, per_b = ceil_div(items_a, p.grid), ceil_div(items_b, p.grid_b)
    assert p.grid * per_a >= items_a and p.grid_b * per_b >= items_b
    if cus > 1:
        assert p.grid + p.grid_b <= cus
        best = min(max(100 * ceil_div(items_a, cus - gb), 135 * ceil_div(items_b, gb)) for gb in range(1, min(cus - 1, items_b) + 1))
        assert max(100 * per_a, 135 * per_b) == best, (items_a, items_b, cus, p.grid, p.grid_b)
    else:
        per = ceil_div(items_a + items_b, cus)
        assert (p.grid, p.grid_b) == (ceil_div(items_a, per), ceil_div(items_b, per)) and p.grid + p.grid_b <= cus + 1
    check_lds_and_kernel(lib, t, p, k)


def test_a_form_that_a_unit_does_not_hold_is_not_found(lib):
    p = plan(lib, MULTI, T.Q6_K, 1, 8016, 0, 4096, 1, 256)
    assert (p.variant, p.rows, p.grid) == (ROWS32, 32, 251)
    assert lib.lfamd_gemv_has_kernel(T.Q6_K, 1, C.byref(p)) and not lib.lfamd_gemv_has_kernel(T.Q4_K, 1, C.byref(p))
    p = plan(lib, IDS, T.Q4_K, 1, 512, 0, 4096, 2, 256)
    assert lib.lfamd_gemv_has_kernel(T.Q5_K, 0, C.byref(p)) and not lib.lfamd_gemv_has_kernel(T.Q2_K, 0, C.byref(p))
    p.nw, p.ch = 8, 1
    assert not lib.lfamd_gemv_has_kernel(T.Q4_K, 0, C.byref(p))
    q = Plan()
    assert lib.lfamd_gemv_plan_of(MULTI, T.F16, 1, 256, 0, 4096, 1, 256, C.byref(q)) == -1
    assert lib.lfamd_gemv_plan_of(IDS, T.Q8_0, 1, 256, 0, 4096, 1, 256, C.byref(q)) == -1
    assert lib.lfamd_gemv_plan_of(DUAL, T.Q6_K, 1, 256, 64, 4096, 2, 256, C.byref(q)) == -1
    # nothing to launch, or no device to launch on: an answer, not a division by zero
    assert lib.lfamd_gemv_plan_of(MULTI, T.Q4_K, 1, 0, 0, 4096, 1, 256, C.byref(q)) == -1
    assert lib.lfamd_gemv_plan_of(MULTI, T.Q4_K, 1, 256, 0, 4096, 1, 0, C.byref(q)) == -1
    assert lib.lfamd_gemv_plan_of(DUAL, T.Q4_K, 1, 256, 0, 4096, 2, 256, C.byref(q)) == -1
    assert lib.lfamd_gemv_plan_of(MULTI, T.Q8_0, 1, 0, 0, 4096, 1, 256, C.byref(q)) == -1
