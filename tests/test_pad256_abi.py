"""LFAMD_TYPE_PAD256 without a GPU: the layout modifier on the legacy 32-block weight types (include/lfamd_hip.h, DESIGN.md
section 23).  `T | PAD256` keeps rows of any whole number of 32-blocks as the tile image of kp = 256 * ceil(cols / 256) columns, so
every size and every answer of the plan must be the base type's at kp; the modifier on any other type is an unknown id."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from llamafile_amd import _hip, ggml_types as T

PAD = _hip.TYPE_PAD256
TYPES = (T.Q4_0, T.IQ4_NL, T.Q4_1, T.Q5_0, T.Q5_1)
SHAPES = ((67, 32), (67, 288), (40, 4000), (4099, 2080))
MULTI, PLAIN, EARLY, ROWS32 = 0, 0, 1, 2


def kp_of(k):
    return (k + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    return _hip.lib()


def test_the_constant_is_the_headers(lib):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfamd_hip.h")).read()
    assert "#define LFAMD_TYPE_PAD256 0x2000" in src and PAD == 0x2000
    assert all(t & PAD == 0 for t in T.NAMES)  # no ggml type id collides with the bit


@pytest.mark.parametrize("t", TYPES, ids=lambda t: T.NAMES[t])
def test_packed_size_is_the_base_types_at_whole_groups(lib, t):
    for rows, cols in SHAPES:
        want = lib.lfamd_packed_size(t, rows, kp_of(cols))
        assert lib.lfamd_packed_size(t | PAD, rows, cols) == want > 0, (rows, cols)
        assert want != lib.lfamd_packed_size(t, rows, cols)  # (the unmodified id keeps RAW rows at these lengths)
    for cols in (256, 4096):  # whole groups: the modifier changes nothing
        assert lib.lfamd_packed_size(t | PAD, 67, cols) == lib.lfamd_packed_size(t, 67, cols) > 0
    for cols in (16, 100, 257, 300):
        assert lib.lfamd_packed_size(t | PAD, 67, cols) == 0  # not whole 32-blocks
    assert lib.lfamd_packed_size(t | PAD, 0, 288) == 0 and lib.lfamd_packed_size(t | PAD, -1, 288) == 0


def test_other_base_types_are_unknown_with_the_bit(lib):
    for t in (T.Q4_K, T.Q8_0, T.F16, T.F32, T.BF16, T.Q2_K, T.Q3_K, T.Q5_K, T.Q6_K, T.IQ4_XS, 99):
        assert lib.lfamd_packed_size(t | PAD, 64, 512) == 0, t
        assert lib.lfamd_mul_mat_workspace(t | PAD, 64, 512, 40) == 0
        assert lib.lfamd_mul_mat_is_exact(t | PAD, 64, 512, 1, 0) == 0
        # every other call: LFAMD_ERR_UNSUPPORTED, before it looks at a pointer
        assert lib.lfamd_pack_weights(t | PAD, 64, 512, None, 4096, None, None) == -1
        assert lib.lfamd_unpack_weights(t | PAD, 64, 512, None, None, 4096, None) == -1
        assert lib.lfamd_get_rows(t | PAD, None, 64, 512, None, 0, 1, T.F32, None, 2048, None) == -1
        assert lib.lfamd_mul_mat(t | PAD, None, 64, 512, T.F32, None, 2048, 1, None, 64, None, 0, 0, None) == -1
        assert lib.lfamd_mul_mat_id(t | PAD, None, 64, 512, 4, T.Q8_0, None, 544, 1, 1, None, 2, None, None, 0, 0, None) == -1
        # the sibling calls plan with the modifier stripped: they must refuse the id first, alone and among known types
        m2, A2, C2 = (C.c_long * 2)(64, 64), (C.c_void_p * 2)(), (C.c_void_p * 2)()
        for n in (1, 40):
            assert lib.lfamd_mul_mat_multi(t | PAD, 2, A2, m2, 512, T.F32, None, 2048, n, C2, m2, None, 0, 0, None) == -1, (t, n)
            for types in ((t | PAD, t | PAD), (T.Q4_0, t | PAD), (t | PAD, T.Q4_0 | PAD)):
                assert lib.lfamd_mul_mat_multi_types(2, (C.c_int * 2)(*types), A2, m2, 512, T.F32, None, 2048, n, C2, m2, None, 0, 0,
                                                     None) == -1, (types, n)


@pytest.mark.parametrize("t", TYPES, ids=lambda t: T.NAMES[t])
def test_workspace_and_answers_are_the_base_types_at_kp(lib, t):
    for m, k in SHAPES + ((300, 8480),):
        for n in (1, 8, 9, 40, 512):
            assert lib.lfamd_mul_mat_workspace(t | PAD, m, k, n) == lib.lfamd_mul_mat_workspace(t, m, kp_of(k), n), (m, k, n)
            for flags in (0, _hip.FLAG_PRECISE, _hip.FLAG_GEMM_PLAIN):
                assert lib.lfamd_mul_mat_is_exact(t | PAD, m, k, n, flags) == 1
            assert lib.lfamd_mul_mat_is_bit_exact(t | PAD, m, k, n, 0) == lib.lfamd_mul_mat_is_bit_exact(t, m, kp_of(k), n, 0) == 0
            assert lib.lfamd_mul_mat_takes_staged_b32(t | PAD, m, k, n, 0) == 0  # ragged k: the producers' images are not part of this
            assert lib.lfamd_mul_mat_takes_staged(t | PAD, m, k, n, 0) == 0
            assert lib.lfamd_mul_mat_takes_staged_scaled(t | PAD, m, k, n, 0) == 0
            assert lib.lfamd_mul_mat_takes_staged_q80(t | PAD, m, k, n, 0) == 0
        assert lib.lfamd_mul_mat_workspace(t | PAD, m, k, 1) == 0  # decode stages in LDS
        assert lib.lfamd_mul_mat_workspace(t | PAD, m, k, 40) > 0
    for k in (256, 4096):  # whole groups: the unmodified answers, the staged image included
        for n in (1, 9, 512):
            assert lib.lfamd_mul_mat_workspace(t | PAD, 300, k, n) == lib.lfamd_mul_mat_workspace(t, 300, k, n)
            assert lib.lfamd_mul_mat_takes_staged_b32(t | PAD, 300, k, n, 0) == lib.lfamd_mul_mat_takes_staged_b32(t, 300, k, n, 0) == (n > 8)


def test_the_moe_inner_workspace_bound_holds_for_the_modified_ids(lib):
    """tests/test_abi_exports.py's bound (lfamd_mul_mat_workspace_upto covers every smaller batch), on the padded images."""
    upto = C.CDLL(_hip.HIP_SO).lfamd_mul_mat_workspace_upto
    upto.restype, upto.argtypes = C.c_size_t, [C.c_int, C.c_long, C.c_long, C.c_long]
    for t in TYPES:
        for m, k in ((4096, 4000), (1024, 288), (300, 8480)):
            prev = 0
            for n in list(range(1, 70)) + list(range(70, 1200, 37)):
                bound = upto(t | PAD, m, k, n)
                assert bound >= prev and bound >= lib.lfamd_mul_mat_workspace(t | PAD, m, k, n), (T.NAMES[t], m, k, n)
                assert bound == upto(t, m, kp_of(k), n)
                prev = bound
            for n in (100, 300):
                bound = upto(t | PAD, m, k, n)
                assert all(lib.lfamd_mul_mat_workspace(t | PAD, m, k, v) <= bound for v in range(1, n + 1)), (T.NAMES[t], m, k, n)
            # MUL_MAT_ID: the workspace of the base type at kp, but for the gathered activation rows, which keep their length k
            ws = lib.lfamd_mul_mat_id_workspace
            nr = 5 * 2
            d_rows = (nr * T.row_size(T.VEC_DOT[t], kp_of(k)) + 255) // 256 * 256 - (nr * T.row_size(T.VEC_DOT[t], k) + 255) // 256 * 256
            assert ws(t | PAD, m, k, 4, 5, 2) == ws(t, m, kp_of(k), 4, 5, 2) - d_rows > 0


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


def test_the_decode_plan_works_from_the_padded_super_blocks():
    """Every launch the plan makes for a row that ends inside its last super-block is the launch of the row padded to it, names a
    kernel the type's unit holds, and fits the LDS budget; the columns per launch change past 32 super-blocks as for whole rows."""
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_has_kernel.argtypes = [C.c_int, C.c_int, C.POINTER(Plan)]
    L.lfamd_gemv_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_long, C.c_int, C.c_int]
    L.lfamd_gemv_lds_bytes.restype = C.c_size_t
    L.lfamd_gemv_cols_per_launch.argtypes = [C.c_int, C.c_long]
    L.lfamd_gemv_depth_ok.argtypes = [C.c_long]
    checked = 0
    for nb in (1, 2, 9, 16, 34):
        for tail in (32, 160, 224):  # one, five and seven valid blocks in the last super-block
            k, kp = (nb - 1) * 256 + tail, nb * 256
            assert L.lfamd_gemv_depth_ok(k) == L.lfamd_gemv_depth_ok(kp) == 1
            for t in TYPES:
                step = L.lfamd_gemv_cols_per_launch(t, k)
                assert step == L.lfamd_gemv_cols_per_launch(t, kp) == (5 if nb > 32 else 8)
                for cus in (256, 64, 32):
                    for m in (16, 67, 1030, 4099, 70000):
                        n_ht = (m + 31) // 32 * 2
                        for count in (1, 3):
                            for nc in range(1, step + 1):
                                p, q = Plan(), Plan()
                                assert L.lfamd_gemv_plan_of(MULTI, t, nc, n_ht * count, 0, k, count, cus, C.byref(p)) == 0
                                assert L.lfamd_gemv_plan_of(MULTI, t, nc, n_ht * count, 0, kp, count, cus, C.byref(q)) == 0
                                assert bytes(p) == bytes(q), (T.NAMES[t], nb, tail, cus, m, count, nc)
                                assert p.variant in (PLAIN, EARLY, ROWS32) and (p.variant == ROWS32) <= (t == T.IQ4_NL)
                                assert p.lds == L.lfamd_gemv_lds_bytes(t, nc, k, p.nw, p.rows) <= 150 * 1024 + 8192
                                assert L.lfamd_gemv_has_kernel(t, 0, C.byref(p)) and L.lfamd_gemv_has_kernel(t, 1, C.byref(p))
                                checked += 1
    assert checked > 10000
    assert L.lfamd_gemv_depth_ok(400 * 256 - 32) == 1 and L.lfamd_gemv_depth_ok(400 * 256 + 32) == 0  # 400 padded super-blocks: 150 KiB


def test_the_resident_type_helper_matches_the_modules_rule():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stdio.h>\n#include "lfamd_hip.h"\nint main(void) { for (int t = 0; t < 32; t++) for (long c = 0; c <= 1024; c += 16) '
           'printf("%d %ld %d\\n", t, c, lfamd_resident_type(t, c)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "r.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", os.path.join(d, "r"), os.path.join(d, "r.c")])
        out = subprocess.run([os.path.join(d, "r")], capture_output=True, text=True, check=True).stdout
    L = _hip.lib()
    for line in out.splitlines():
        t, c, r = (int(v) for v in line.split())
        want = t | PAD if t in TYPES and c % 32 == 0 and c % 256 != 0 else t
        assert r == want, line
        if r != t:  # where the helper sets the bit the module takes it, and the image differs from the unmodified one
            assert L.lfamd_packed_size(r, 64, c) == L.lfamd_packed_size(t, 64, kp_of(c)) != L.lfamd_packed_size(t, 64, c)
