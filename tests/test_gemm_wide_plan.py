"""Which launch form a scaled-operand wide call takes (csrc/gemm_wide.hip: wide_scaled_plan, the function wide_go switches on,
exported for tests as lfamd_gemm_wide_plan_of), without a GPU.  The forms, DESIGN.md section 34:

  T = row blocks of 128 rows (all matrices of the launch) x token tiles of 128;  T >= 129 (LW_FULL_GRID):
      Q4_K                                                               kr    (256 x 128 tiles; below 257 the int8 body takes Q4_K)
      Q5_K / Q6_K, T > 256, rem = T % 256 in 1 .. 128, rem % n_ct = 0     lw128_then_lw64, rb_cut = (T - rem) / n_ct
      Q5_K / Q6_K otherwise                                              lw128
  T <= 128, on 128 x 64 tiles (T2 = row blocks x ceil(n / 64)):
      one matrix, n_pad = 128, a workspace, ksp = lw_ksplit(T2, nb) > 1  lw64_ksplit (ksp doubles while ksp < 8, T2 * 2 ksp <= 256
                                                                         and nb / (2 ksp) >= 2)
      Q4_K                                                               ks
      Q5_K / Q6_K                                                        lw64
"""
import pytest

from llamafile_amd import ggml_types as T
import wide_routes as R
from wide_routes import KR, LW128, SPLIT, LW64, KS, KSPLIT, plan_of

KQ = (T.Q4_K, T.Q5_K, T.Q6_K)
Q56 = (T.Q5_K, T.Q6_K)
BIG = 1 << 30  # a workspace that is never the limit


@pytest.fixture(scope="module")
def lib():
    return R.plan_lib()


def model(t, rbs, count, nb, n, n_pad, p_bytes):
    """The table of the module docstring, written out a second time (this is the check, not the rule the library runs)."""
    n_ct, n_ct2 = n_pad // 128, (n + 63) // 64
    tiles = rbs * n_ct
    if tiles >= 129:
        if t == T.Q4_K:
            return KR, 0, 1
        rem = tiles % 256
        if tiles > 256 and 1 <= rem <= 128 and rem % n_ct == 0:
            return SPLIT, (tiles - rem) // n_ct, 1
        return LW128, 0, 1
    ksp = 1
    if count == 1 and p_bytes and n_pad == 128:
        while ksp < 8 and rbs * n_ct2 * ksp * 2 <= 256 and nb // (ksp * 2) >= 2:
            ksp *= 2
    if ksp > 1 and p_bytes >= ksp * 128 * rbs * 128 * 4:
        return KSPLIT, 0, ksp
    return (KS if t == T.Q4_K else LW64), 0, 1


def test_full_grid_boundary_128_129_tiles(lib):
    """LW_FULL_GRID: 128 tiles of 128 x 128 still run as 128 x 64 tiles, 129 run whole."""
    for t in KQ:
        small = KS if t == T.Q4_K else LW64
        full = KR if t == T.Q4_K else LW128
        assert plan_of(t, [128 * 128], 2, 128) == (small, 0, 1)
        assert plan_of(t, [128 * 128 + 1], 2, 128) == (full, 0, 1)
        assert plan_of(t, [64 * 128], 2, 256) == (small, 0, 1)          # 64 x 2 = 128
        assert plan_of(t, [64 * 128, 1], 2, 256) == (full, 0, 1)        # 65 x 2 = 130
        assert plan_of(t, [43 * 128], 2, 384) == (full, 0, 1)           # 43 x 3 = 129
        assert plan_of(t, [42 * 128 + 127, 1], 2, 384) == (full, 0, 1)  # the blocks of every matrix count: 43 + 1
        assert plan_of(t, [42 * 128], 2, 384) == (small, 0, 1)          # 126


def test_one_round_boundary_256_257_tiles_and_the_remainders(lib):
    """The tail split needs MORE than one round and a last round of at most half the chip: rem = 0, 1, 128, 129."""
    for t in Q56:
        assert plan_of(t, [256 * 128], 1, 100) == (LW128, 0, 1)           # 256: one round, rem 0
        assert plan_of(t, [256 * 128 + 1], 1, 100) == (SPLIT, 256, 1)     # 257: rem 1
        assert plan_of(t, [384 * 128], 1, 100) == (SPLIT, 256, 1)         # rem 128
        assert plan_of(t, [384 * 128 + 1], 1, 100) == (LW128, 0, 1)       # rem 129
        assert plan_of(t, [512 * 128], 1, 100) == (LW128, 0, 1)           # two rounds, rem 0
        assert plan_of(t, [513 * 128], 1, 100) == (SPLIT, 512, 1)
        assert plan_of(t, [128 * 128 + 1], 1, 100) == (LW128, 0, 1)       # 129 tiles, rem 129 of a grid below one round
        assert plan_of(t, [129 * 128], 1, 100) == (LW128, 0, 1)
        # rem % n_ct: 150 blocks x 2 = 300, rem 44 splits at (300 - 44) / 2; 100 blocks x 3 = 300, 44 % 3 = 2 does not
        assert plan_of(t, [150 * 128], 1, 200) == (SPLIT, 128, 1)
        assert plan_of(t, [100 * 128], 1, 300) == (LW128, 0, 1)
        # three token tiles: 3 rb - 256 is never a multiple of 3, 3 rb - 768 always is
        assert plan_of(t, [102 * 128], 1, 300) == (LW128, 0, 1)           # 306 tiles, rem 50, 50 % 3 = 2
        assert plan_of(t, [260 * 128], 1, 300) == (SPLIT, 256, 1)         # 780 tiles, rem 12: the cut after 768 / 3 row blocks
        assert plan_of(t, [299 * 128], 1, 300) == (LW128, 0, 1)           # 897 tiles, rem 129


def test_no_q4k_shape_has_a_ks_tail_and_every_answer_matches_the_table(lib):
    """Every (type, row blocks, token count, depth, workspace) of a sweep: the export answers what the table says; Q4_K never
    splits (at 129 tiles and more it is `kr`, below that there is no tail); rb_cut * n_ct is a multiple of 256 and rb_cut < n_rb."""
    seen = set()
    for t in KQ:
        for rbs in list(range(1, 140)) + list(range(250, 262)) + [299, 300, 313, 316, 383, 384, 385, 511, 512, 513, 640, 896, 1002]:
            for n in (9, 33, 64, 65, 100, 128, 129, 200, 256, 300, 512, 513):
                for nb in (1, 2, 3, 4, 8, 16):
                    for count, p_bytes in ((1, 0), (1, BIG), (2, 0), (2, BIG)):
                        if count > rbs:
                            continue
                        ms = [rbs * 128 - 5] if count == 1 else [128, (rbs - 1) * 128 - 5]
                        got = plan_of(t, ms, nb, n, p_bytes)
                        assert got == model(t, rbs, count, nb, n, R.n_pad_of(n), p_bytes), (T.NAMES[t], rbs, n, nb, count, p_bytes)
                        form, rb_cut, ksp = got
                        seen.add((t, form))
                        n_ct = R.n_pad_of(n) // 128
                        if t == T.Q4_K:
                            assert form in (KR, KS, KSPLIT) and rb_cut == 0
                            assert (form == KR) == (rbs * n_ct >= 129)
                        if form == SPLIT:
                            assert 0 < rb_cut < rbs and (rb_cut * n_ct) % 256 == 0
                            assert 1 <= (rbs - rb_cut) * n_ct <= 128  # the tail is at most half a round of 128 x 128 tiles
                        else:
                            assert rb_cut == 0
                        assert ksp == 1 or form == KSPLIT
    assert seen == {(T.Q4_K, KR), (T.Q4_K, KS), (T.Q4_K, KSPLIT)} | {(t, f) for t in Q56 for f in (LW128, SPLIT, LW64, KSPLIT)}


def test_k_split_needs_one_matrix_one_token_tile_and_its_workspace(lib):
    """4096 x 4096 at 32 tokens: 32 tiles of 128 x 64, 16 super-blocks -> K in 8 parts (32 * 4 * 2 = 256 <= 256 lets 4 double, and
    2 super-blocks per part remain): 256 work-groups of 2 super-blocks."""
    for t in KQ:
        small = KS if t == T.Q4_K else LW64
        need = lib.lfamd_gemm_lw_ksplit_bytes(4096, 32)
        assert need == 8 * 128 * 32 * 128 * 4
        assert plan_of(t, [4096], 16, 32, need) == (KSPLIT, 0, 8)
        assert plan_of(t, [4096], 16, 32, 0) == (small, 0, 1)                          # no workspace
        assert plan_of(t, [4096], 16, 32, need - 1) == (small, 0, 1)                   # one byte short
        assert plan_of(t, [4096], 8, 32, need // 2) == (KSPLIT, 0, 4)                  # exactly ksp = 4 parts
        assert plan_of(t, [4096], 8, 32, need // 2 - 1) == (small, 0, 1)
        assert plan_of(t, [2048, 2048], 16, 32, need) == (small, 0, 1)                 # count > 1
        assert plan_of(t, [4096], 16, 32, need, n_pad=256) == (small, 0, 1)            # n_pad != 128
        assert plan_of(t, [4096], 3, 32, need) == (small, 0, 1)                        # nb / 2 < 2
        assert plan_of(t, [4096], 4, 32, need) == (KSPLIT, 0, 2)
        assert plan_of(t, [1024], 64, 100, BIG) == (KSPLIT, 0, 8)                      # 16 tiles
        assert plan_of(t, [4096], 64, 100, BIG) == (KSPLIT, 0, 4)                      # 64 tiles: 64 * 2 * 2 = 256, 64 * 4 * 2 > 256
        assert plan_of(t, [4096 + 128], 64, 100, BIG) == (KSPLIT, 0, 2)                # 66 tiles
        assert plan_of(t, [8192], 64, 100, BIG) == (KSPLIT, 0, 2)                      # 128 tiles
        assert plan_of(t, [8192 + 1], 64, 100, BIG) == (small, 0, 1)                   # 130 tiles of 128 x 64: 130 * 2 > 256
    assert lib.lfamd_gemm_lw_ksplit_bytes(4096, 129) == 0 and lib.lfamd_gemm_lw_ksplit_bytes(4096, 8) == 0


def test_bad_arguments_are_refused(lib):
    import ctypes as C
    p, one = R.Plan(), (C.c_long * 1)(4096)
    f = lib.lfamd_gemm_wide_plan_of
    assert f(T.Q4_K, 1, one, 4, 100, 128, 0, C.byref(p), None) == 0
    assert f(T.Q8_0, 1, one, 4, 100, 128, 0, C.byref(p), None) == -1   # no scaled body
    assert f(T.Q4_K, 0, one, 4, 100, 128, 0, C.byref(p), None) == -1
    assert f(T.Q4_K, 5, one, 4, 100, 128, 0, C.byref(p), None) == -1   # GEMM_MAX_MATS = 4
    assert f(T.Q4_K, 1, one, 0, 100, 128, 0, C.byref(p), None) == -1
    assert f(T.Q4_K, 1, one, 4, 0, 128, 0, C.byref(p), None) == -1
    assert f(T.Q4_K, 1, one, 4, 100, 100, 0, C.byref(p), None) == -1   # n_pad: whole 128-token tiles
    assert f(T.Q4_K, 1, one, 4, 200, 128, 0, C.byref(p), None) == -1   # n_pad < n
    assert f(T.Q4_K, 1, (C.c_long * 1)(0), 4, 100, 128, 0, C.byref(p), None) == -1  # an empty launch


def expected_parts(ms, rb_cut):
    """(lo, hi) of split_mats from rb_cut alone: per matrix (index, first row, rows)."""
    lo, hi, start = [], [], 0
    for j, m in enumerate(ms):
        end = start + (m + 127) // 128
        below = max(0, min(end, rb_cut) - start) * 128  # rows of matrix j in row blocks below the cut
        below = min(below, m)
        if below:
            lo.append((j, 0, below))
        if m - below:
            hi.append((j, below, m - below))
        start = end
    return lo, hi


SPLIT_SHAPES = [
    (T.Q6_K, (38350,), 100, 1, "inside the one matrix"),
    (T.Q5_K, (19199,), 200, 2, "two token tiles"),
    (T.Q6_K, (20000, 77, 18000), 100, 1, "inside the last matrix"),
    (T.Q5_K, (32768, 5000), 100, 1, "on a boundary"),
    (T.Q6_K, (40000, 300), 100, 2, "inside matrix 0"),
    (T.Q5_K, (100, 32768, 128, 5555), 100, 4, "four matrices, the cut inside the second"),
    (T.Q6_K, (16384, 16384, 100), 100, 1, "on the second boundary: hi is the last matrix alone"),
]


@pytest.mark.parametrize("t,ms,n,nb,what", SPLIT_SHAPES, ids=[s[4] for s in SPLIT_SHAPES])
def test_split_mats_covers_every_row_once(lib, t, ms, n, nb, what):
    """split_mats itself, run on stand-in addresses by the export: the two launches' (matrix, first row, rows) are re-derived from
    rb_cut here, cover every row of every matrix exactly once, `lo` ends on a row block, and the weight pointer of a part is
    advanced by four 32-row tiles per skipped row block (the C pointer by 128 rows)."""
    (form, rb_cut, ksp), lo, hi = plan_of(t, list(ms), nb, n, 0, parts=True)
    assert (form, ksp) == (SPLIT, 1)
    n_ct = R.n_pad_of(n) // 128
    assert 0 < rb_cut < R.row_blocks(ms) and (rb_cut * n_ct) % 256 == 0
    want_lo, want_hi = expected_parts(ms, rb_cut)
    assert [p[:3] for p in lo] == want_lo and [p[:3] for p in hi] == want_hi, (lo, hi)
    tile = nb * {T.Q4_K: 144, T.Q5_K: 176, T.Q6_K: 210}[t] * 32  # bytes of 32 rows of one image (the GGUF size: test_abi_exports)
    for j, row0, rows, a_off in lo + hi:
        assert row0 % 128 == 0 and a_off == row0 // 32 * tile, (j, row0, a_off)
    assert all(p[1] == 0 for p in lo) and sum((p[2] + 127) // 128 for p in lo) == rb_cut
    assert all(p[2] % 128 == 0 for p in lo[:-1] if p[2] != ms[p[0]])
    cover = [[0] * m for m in ms]
    for j, row0, rows, _ in lo + hi:
        for r in range(row0, row0 + rows):
            cover[j][r] += 1
    assert all(c == 1 for m in cover for c in m)
    if what == "on a boundary":
        assert lo == [(0, 0, 32768, 0)] and hi == [(1, 0, 5000, 0)]
    if what == "inside the last matrix":
        assert [p[0] for p in lo] == [0, 1, 2] and hi == [(2, 98 * 128, 18000 - 98 * 128, 98 * 4 * tile)]
    if what == "inside matrix 0":
        assert lo == [(0, 0, 32768, 0)] and hi == [(0, 32768, 7232, 256 * 4 * tile), (1, 0, 300, 0)]


def test_forms_other_than_the_split_report_no_parts(lib):
    plan, lo, hi = plan_of(T.Q6_K, [12800], 1, 300, 0, parts=True)
    assert plan == (LW128, 0, 1) and lo == [] and hi == []


@pytest.mark.parametrize("name,t", R.case_list(), ids=R.case_ids())
def test_every_gpu_case_takes_the_form_it_is_named_for(lib, name, t):
    """The shapes of tests/test_gpu_wide_routes.py, here so that a moved threshold fails on a machine without a GPU too."""
    form, types, ms, n, nb, _ = R.CASES[name]
    got = R.call_form(t, list(ms), nb * 256, n)
    assert got[0] == form, (name, R.FORMS[got[0]])
    if form == SPLIT:  # the two halves, called alone, take the two forms whose bits the GPU test compares with
        _, lo, hi = plan_of(t, list(ms), nb, n, 0, parts=True)
        assert R.call_form(t, [p[2] for p in lo], nb * 256, n) == (LW128, 0, 1), name  # the rows below the cut, as one call
        for j, row0, rows, _ in hi:  # (at most 128 tiles: a fused call of these would be one call per matrix, api.hip wide_group_ok)
            assert R.call_form(t, [rows], nb * 256, n)[0] == LW64, (name, j)


def test_the_edges_the_kr_cases_are_named_for(lib):
    assert 11036 % 256 == 28 and 300 % 128 == 44 and R.row_blocks([11036]) * 3 == 261
    assert 16641 % 256 == 1 and 129 % 128 == 1 and R.row_blocks([16641]) * 2 == 262
    assert 5000 % 256 == 136 and R.row_blocks([5000, 129, 12000]) * 2 == 272
    # the same calls padded to whole 256-row blocks / 128-token tiles, which the GPU test compares bits with, are `kr` too
    for ms, n, nb in (((11036,), 300, 1), ((16641,), 129, 3)):
        padded = [(m + 255) // 256 * 256 for m in ms]
        assert R.call_form(T.Q4_K, padded, nb * 256, n)[0] == KR
        assert R.call_form(T.Q4_K, list(ms), nb * 256, R.n_pad_of(n))[0] == KR


def test_kr_on_the_staged_image_and_the_two_type_launch(lib):
    """The two launches the plan export does not decide: they are pinned through the predicates the library asks."""
    form, t, ms, n, nb = R.KR_STAGED
    tiles = R.row_blocks(ms) * (R.n_pad_of(n) // 128)
    assert 129 <= tiles <= 256 and lib.lfamd_gemm_i8_ok(t, R.row_blocks(ms), n) == 1  # (the int8 body would take it: hence the flag)
    assert R.call_form(t, list(ms), nb * 256, n, flags=R.FLAG_GEMM_WIDE)[0] == KR
    pairs, (ma, mb), n, nb = R.DUAL
    ra, rb = R.row_blocks([ma]), R.row_blocks([mb])
    assert (ra + rb) * 1 == 134 and ma % 128 and mb % 128
    assert lib.lfamd_gemm_wide_dual_ok(ra, rb, 128) == 1
    assert lib.lfamd_gemm_wide_dual_ok(128, 1, 128) == 1 and lib.lfamd_gemm_wide_dual_ok(127, 1, 128) == 0  # 129 / 128 tiles
    assert lib.lfamd_gemm_wide_dual_ok(255, 1, 128) == 1 and lib.lfamd_gemm_wide_dual_ok(256, 1, 128) == 0  # 256 / 257
    assert lib.lfamd_gemm_wide_dual_ok(0, 200, 128) == 0
    for ta, tb in pairs:  # the separate calls the Q5_K / Q6_K bits are compared with run 128 x 64 loader-wave tiles
        assert R.call_form(tb, [mb], nb * 256, n)[0] == LW64
        if ta == T.Q5_K:
            assert R.call_form(ta, [ma], nb * 256, n)[0] == LW64


def test_the_int8_rule_next_to_kr(lib):
    """Q4_K: the int8 body takes 128 x 64-tile counts >= 128 up to 256 tiles of 128 x 128; `kr` begins at 257."""
    ok = lib.lfamd_gemm_i8_ok
    assert ok(T.Q4_K, 128, 128) == 1 and ok(T.Q4_K, 256, 128) == 1 and ok(T.Q4_K, 257, 128) == 0
    assert ok(T.Q4_K, 64, 128) == 1 and ok(T.Q4_K, 63, 128) == 0  # 126 tiles of 128 x 64
    assert ok(T.Q4_K, 128, 256) == 1 and ok(T.Q4_K, 129, 256) == 0  # 256 / 258 tiles of 128 x 128
    assert ok(T.Q5_K, 128, 128) == 0 and ok(T.Q6_K, 128, 128) == 0
    assert lib.lfamd_mul_mat_is_exact(T.Q4_K, 256 * 128, 256, 100, 0) == 1  # 256 tiles: int8, exact
    assert lib.lfamd_mul_mat_is_exact(T.Q4_K, 256 * 128 + 1, 256, 100, 0) == 0  # 257: kr, f16-rounded
    for t in Q56:
        assert lib.lfamd_mul_mat_is_exact(t, 256 * 128, 256, 100, 0) == 0
