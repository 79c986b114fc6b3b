// gemm_wide.hip — launchers of the 128 x 128 MFMA body (kernel: gemm_wide_impl.h; instantiations: gemm_wide_*.hip)
#include "gemm_wide_impl.h"
#include "lfamd_internal.h"

hipError_t lfamd_wide_go_q4k(WIDE_ARGS);
hipError_t lfamd_wide_go_q5k(WIDE_ARGS);
hipError_t lfamd_wide_go_q6k(WIDE_ARGS);
hipError_t lfamd_wide_go_q40(WIDE_ARGS);
hipError_t lfamd_wide_go_q41(WIDE_ARGS);
hipError_t lfamd_wide_go_q50(WIDE_ARGS);
hipError_t lfamd_wide_go_q51(WIDE_ARGS);
hipError_t lfamd_wide_go_q2k(WIDE_ARGS);
hipError_t lfamd_wide_go_q3k(WIDE_ARGS);
hipError_t lfamd_wide_go_iq4xs(WIDE_ARGS);
hipError_t lfamd_wide_go_iq4nl(WIDE_ARGS);
hipError_t lfamd_wide_go_f16(WIDE_ARGS);
hipError_t lfamd_wide_go_bf16(WIDE_ARGS);

hipError_t lfamd_lw_go(int Atype, const gemm_mats &mats, int nb, const void *Xh, const void *d8T, const void *Xm, long n, long n_pad,
                       int n_rb, int n_ct, unsigned n_wg, int moe, int fast, int nt, int ks, float *P, hipStream_t s);
hipError_t lfamd_kr_go(int Atype, const gemm_mats &mats128, int nb, const void *Xh, const void *d8T, const void *Xm, long n, long n_pad,
                       int n_ct, hipStream_t s);
hipError_t lfamd_kr_moe_go(int Atype, const gemm_mats &mats, int nb, const void *Xh, const void *d8T, const void *Xm, long n_pad, int experts,
                           int ct_max, hipStream_t s);
hipError_t lfamd_ks_go(int Atype, const gemm_mats &mats, int nb, const void *Xh, const void *d8T, const void *Xm, long n, long n_pad,
                       int n_rb, int n_ct, hipStream_t s);
hipError_t lfamd_lw_ksplit_reduce(const float *P, int ks, long n, long n_pad, long ldp, long m, float *C, long ldc,
                                  const float *tok_scale, hipStream_t s);

// Few-token batches (n <= 128) of one matrix whose 128 x 64 tiles leave most CUs idle: K is cut into up to 8 parts, the
// partial tiles go to a workspace and are summed by a second kernel (4096 x 4096 x 32: 32 work-groups of 16 serial
// super-blocks become 256 of 2).
extern "C" size_t lfamd_gemm_lw_ksplit_bytes(long m, long n) {
    if (m <= 0 || n <= 8 || n > 128)
        return 0;
    const long n_rb = (m + 127) / 128, tiles2 = n_rb * ((n + 63) / 64);
    return tiles2 > 128 ? 0 : (size_t)8 * 128 * (size_t)n_rb * 128 * sizeof(float);
}
static int lw_ksplit(int tiles2, int nb) {
    int ks = 1;
    while (ks < 8 && tiles2 * ks * 2 <= 256 && nb / (ks * 2) >= 2)
        ks *= 2;
    return ks;
}

// Q4_K / Q5_K without K split run the loader-wave body (gemm_lw.hip) unless the caller asks for the plain one.
// `mode` (an argument of every launcher here) bit 0: plain body; bit 1: the activations were staged SCALED (prep.hip, prep mode 2) for the scaled-operand
// loader-wave body — only set when lfamd_gemm_wide_scaled_ok() said that body will run.
// 128 x 128 tiles from which the scaled-operand body uses them instead of 128 x 64: a 128 x 64 work-group takes ~0.73 of a
// 128 x 128 one (2720 vs 3680 cycles per super-block), so two rounds of the small tile (129 .. 256 big tiles = 258 .. 512
// small ones on 256 CUs) lose against one partial round of the big tile; up to 128 big tiles the small tile's single round wins.
#define LW_FULL_GRID 129
static bool lw_allowed(int mode) {
    return !(mode & 1);
}

// The first rb_cut row blocks of `mats` / the rest (a matrix straddling the cut is split: weights by row tiles, C by rows).
static void split_mats(const gemm_mats &mats, int rb_cut, size_t row_tile_bytes, gemm_mats &lo, gemm_mats &hi) {
    lo = mats, hi = mats;
    lo.count = hi.count = 0;
    int lo_end = 0, hi_end = 0;
    for (int j = 0; j < mats.count; j++) {
        const int start = j ? mats.rb_end[j - 1] : 0, end = mats.rb_end[j];
        if (start < rb_cut) { // rows [0, (min(end, rb_cut) - start) * 128) of matrix j
            const int i = lo.count++;
            const int rbs = (end < rb_cut ? end : rb_cut) - start;
            lo.A[i] = mats.A[j], lo.C[i] = mats.C[j], lo.ldc[i] = mats.ldc[j];
            lo.m[i] = end <= rb_cut ? mats.m[j] : (long)rbs * 128;
            lo_end += rbs;
            lo.rb_end[i] = lo_end;
        }
        if (end > rb_cut) {
            const int i = hi.count++;
            const int skip = start < rb_cut ? rb_cut - start : 0; // row blocks of matrix j that went to `lo`
            hi.A[i] = mats.A[j] + (size_t)skip * 4 * row_tile_bytes;
            hi.C[i] = mats.C[j] + (size_t)skip * 128, hi.ldc[i] = mats.ldc[j];
            hi.m[i] = mats.m[j] - (long)skip * 128;
            hi_end += end - start - skip;
            hi.rb_end[i] = hi_end;
        }
    }
    for (int i = lo.count; i < GEMM_MAX_MATS; i++)
        lo.A[i] = lo.A[0], lo.C[i] = lo.C[0], lo.m[i] = 0, lo.ldc[i] = 0, lo.rb_end[i] = lo_end;
    for (int i = hi.count; i < GEMM_MAX_MATS; i++)
        hi.A[i] = hi.A[0], hi.C[i] = hi.C[0], hi.m[i] = 0, hi.ldc[i] = 0, hi.rb_end[i] = hi_end;
}

// Which launch form a scaled-operand call that is not MUL_MAT_ID takes, from the grid alone (count matrices of n_rb row blocks of 128
// together, nb super-blocks, n tokens staged as n_pad rows, P_bytes of K-split workspace or 0).  wide_go switches on the answer and
// lfamd_gemm_wide_plan_of hands it to the tests: there is no second copy of this rule.
static lfamd_wide_plan wide_scaled_plan(int Atype, int count, int n_rb, int nb, long n, long n_pad, size_t P_bytes) {
    const int n_ct = (int)(n_pad / WD_COLS), tiles = n_rb * n_ct;
    // 128 x 128 tiles when they fill the chip, else 128 x 64 (twice the work-groups, no K split)
    if (tiles >= LW_FULL_GRID) {
        if (Atype == LFAMD_TYPE_Q4_K) // 256 x 128 tiles on the row-split body (gemm_kr.hip)
            return {LFAMD_WIDE_KR, 0, 1};
        // full rounds of 128 x 128 tiles; a last round of at most 128 of them (half the CUs idle) runs as one round of
        // 128 x 64 tiles instead (0.73 of the time): ffn_gate + ffn_up at 512 tokens = 896 tiles = 3 rounds + 128
        const int rem = tiles % 256;
        if (tiles > 256 && rem > 0 && rem <= 128 && rem % n_ct == 0)
            return {LFAMD_WIDE_LW128_THEN_LW64, (tiles - rem) / n_ct, 1};
        return {LFAMD_WIDE_LW128, 0, 1};
    }
    const int n_ct2 = (int)((n + 63) / 64);
    const int ksp = (count == 1 && P_bytes && n_pad == 128) ? lw_ksplit(n_rb * n_ct2, nb) : 1;
    if (ksp > 1 && P_bytes >= (size_t)ksp * 128 * (size_t)n_rb * 128 * sizeof(float))
        return {LFAMD_WIDE_LW64_KSPLIT, 0, ksp};
    // 128 x 64 tiles: Q4_K on the K-split-waves body (gemm_ks.hip)
    return {Atype == LFAMD_TYPE_Q4_K ? LFAMD_WIDE_KS : LFAMD_WIDE_LW64, 0, 1};
}

static size_t row_tile_bytes_of(int Atype, int nb) { // one 32-row tile of a K-quant image
    return (size_t)nb * (Atype == LFAMD_TYPE_Q5_K ? P5K_TILE : Atype == LFAMD_TYPE_Q6_K ? P6K_TILE : P4K_TILE);
}

static hipError_t wide_go(int Atype, int mode, float *P, size_t P_bytes, WIDE_ARGS) {
    const int g_scaled = (mode >> 1) & 1;
    const bool q45 = Atype == LFAMD_TYPE_Q4_K || Atype == LFAMD_TYPE_Q5_K;
    if ((q45 || (Atype == LFAMD_TYPE_Q6_K && g_scaled)) && lw_allowed(mode)) {
        if (g_scaled && !moe) {
            const lfamd_wide_plan p = wide_scaled_plan(Atype, mats.count, n_rb, nb, n, n_pad, P ? P_bytes : 0);
            const int n_ct2 = (int)((n + 63) / 64);
            switch (p.form) {
            case LFAMD_WIDE_KR:
                return lfamd_kr_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_ct, s);
            case LFAMD_WIDE_LW128:
                return lfamd_lw_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, (unsigned)(n_rb * n_ct), 0, 1, 4, 1, nullptr, s);
            case LFAMD_WIDE_LW128_THEN_LW64: {
                gemm_mats lo, hi;
                split_mats(mats, p.rb_cut, row_tile_bytes_of(Atype, nb), lo, hi);
                hipError_t e = lfamd_lw_go(Atype, lo, nb, Xh, d8T, Xm, n, n_pad, p.rb_cut, n_ct, (unsigned)(p.rb_cut * n_ct), 0, 1, 4, 1,
                                           nullptr, s);
                if (e != hipSuccess)
                    return e;
                const int rb_hi = n_rb - p.rb_cut;
                return lfamd_lw_go(Atype, hi, nb, Xh, d8T, Xm, n, n_pad, rb_hi, n_ct2, (unsigned)(rb_hi * n_ct2), 0, 1, 2, 1, nullptr, s);
            }
            case LFAMD_WIDE_LW64_KSPLIT: {
                hipError_t e = lfamd_lw_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct2, (unsigned)(n_rb * n_ct2 * p.ksp), 0, 1, 2,
                                           p.ksp, P, s);
                if (e != hipSuccess)
                    return e;
                return lfamd_lw_ksplit_reduce(P, p.ksp, n, n_pad, (long)n_rb * 128, mats.m[0], mats.C[0], mats.ldc[0],
                                              (const float *)d8T, s);
            }
            case LFAMD_WIDE_KS:
                return lfamd_ks_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct2, s);
            default: // LFAMD_WIDE_LW64
                return lfamd_lw_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct2, (unsigned)(n_rb * n_ct2), 0, 1, 2, 1, nullptr, s);
            }
        }
        if (ks == 1 && (q45 || (moe && g_scaled))) // exact codes; the grouped MUL_MAT_ID launch also on scaled operands (Q6_K: only)
            return lfamd_lw_go(Atype, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, n_wg, moe, moe ? g_scaled : 0, 4, 1, nullptr, s);
    }
    if (g_scaled)
        return hipErrorInvalidValue; // scaled activations reached a body that expects integer codes
    switch (Atype) {
    case LFAMD_TYPE_Q4_K:
        return lfamd_wide_go_q4k(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q5_K:
        return lfamd_wide_go_q5k(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q6_K:
        return lfamd_wide_go_q6k(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q4_0:
        return lfamd_wide_go_q40(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q4_1:
        return lfamd_wide_go_q41(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q5_0:
        return lfamd_wide_go_q50(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q5_1:
        return lfamd_wide_go_q51(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q2_K:
        return lfamd_wide_go_q2k(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_Q3_K:
        return lfamd_wide_go_q3k(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_IQ4_XS:
        return lfamd_wide_go_iq4xs(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_IQ4_NL:
        return lfamd_wide_go_iq4nl(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_F16:
        return lfamd_wide_go_f16(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    case LFAMD_TYPE_BF16:
        return lfamd_wide_go_bf16(mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, n_wg, moe, s);
    default:
        return hipErrorInvalidValue;
    }
}

// C = 0 for the K-split accumulation (rows [0,n) x [0,m) of a matrix with leading dimension ldc)
__global__ void zero_c_kernel(float *__restrict__ C, long ldc, long m, long n) {
    const long total = m * n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long j = idx / m;
        C[j * ldc + (idx - j * m)] = 0.0f;
    }
}

// How the wide body splits K: enough work-groups for 256 CUs, at least 2 super-blocks per split.
static int wide_ksplit(int n_tiles, int nb) {
    int ks = 1;
    while (n_tiles * ks < 192 && nb / (ks * 2) >= 2 && ks < 2) // ks <= 2 keeps the sum order-independent
        ks *= 2;
    return ks;
}

extern "C" int lfamd_gemm_wide_ksplit(long m, long k, long n_pad) {
    const int n_rb = (int)((m + 127) / 128), n_ct = (int)(n_pad / WD_COLS);
    return wide_ksplit(n_rb * n_ct, (int)(k / 256));
}

// Will a wide launch of these (fused) matrices run the loader-wave body, i.e. may the caller stage scaled activations?
extern "C" int lfamd_gemm_wide_scaled_ok(int Atype, int plain) {
    return !plain && (Atype == LFAMD_TYPE_Q4_K || Atype == LFAMD_TYPE_Q5_K || Atype == LFAMD_TYPE_Q6_K);
}

// The form wide_go gives a scaled-operand call (not MUL_MAT_ID) of `count` matrices of m[] rows, nb super-blocks, n tokens staged
// as n_pad rows, with P_bytes of K-split workspace (0: none), for the tests (tests/test_gemm_wide_plan.py); no device is touched.
// parts, when given: 2 * GEMM_MAX_MATS entries of {matrix, first row, rows, weight byte offset}, what split_mats hands the two
// launches of LFAMD_WIDE_LW128_THEN_LW64 (the 128 x 128 launch's matrices first; matrix = -1 ends a launch's list early); any
// other form leaves every entry at -1.  Returns 0, or -1 for arguments no such call has.
extern "C" int lfamd_gemm_wide_plan_of(int Atype, int count, const long *m, int nb, long n, long n_pad, size_t P_bytes,
                                       lfamd_wide_plan *p, long *parts) {
    if (!lfamd_gemm_wide_scaled_ok(Atype, 0) || count <= 0 || count > GEMM_MAX_MATS || !m || !p || nb <= 0 || n <= 0 || n_pad < n ||
        n_pad % WD_COLS)
        return -1;
    // stand-in addresses 2^40 apart, so that a part's pointers say which matrix and which offset split_mats gave it
    const uintptr_t step = (uintptr_t)1 << 40;
    const void *A[GEMM_MAX_MATS];
    float *C[GEMM_MAX_MATS];
    for (int j = 0; j < count; j++)
        A[j] = (const void *)((j + 1) * step), C[j] = (float *)((j + 1) * step);
    gemm_mats mats;
    const int n_rb = fill_gemm_mats(mats, count, A, m, C, m);
    if (mats.count == 0)
        return -1;
    *p = wide_scaled_plan(Atype, mats.count, n_rb, nb, n, n_pad, P_bytes);
    if (!parts)
        return 0;
    for (int i = 0; i < 2 * GEMM_MAX_MATS * 4; i++)
        parts[i] = -1;
    if (p->form != LFAMD_WIDE_LW128_THEN_LW64)
        return 0;
    gemm_mats half[2];
    split_mats(mats, p->rb_cut, row_tile_bytes_of(Atype, nb), half[0], half[1]);
    for (int h = 0; h < 2; h++)
        for (int i = 0; i < half[h].count; i++) {
            long *e = parts + (h * GEMM_MAX_MATS + i) * 4;
            const uintptr_t c = (uintptr_t)half[h].C[i], a = (uintptr_t)half[h].A[i];
            e[0] = (long)(c / step) - 1, e[1] = (long)((c % step) / sizeof(float)), e[2] = half[h].m[i], e[3] = (long)(a % step);
        }
    return 0;
}

extern "C" hipError_t lfamd_launch_gemm_wide_multi(int Atype, int count, const void *const *A, const long *m, long k,
                                                   const void *Xh, const void *d8T, const void *Xm, long n, long n_pad,
                                                   float *const *C, const long *ldc, int mode, void *P, size_t P_bytes,
                                                   hipStream_t s) {
    if (n <= 0 || count <= 0)
        return hipSuccess;
    if (n_pad % WD_COLS || count > GEMM_MAX_MATS)
        return hipErrorInvalidValue;
    const int nb = (int)(k / 256);
    gemm_mats mats;
    const int n_rb = fill_gemm_mats(mats, count, A, m, C, ldc);
    if (mats.count == 0)
        return hipSuccess;
    const int n_ct = (int)(n_pad / WD_COLS);
    const bool scaled_lw = (mode & 2) && lw_allowed(mode) &&
                           (Atype == LFAMD_TYPE_Q4_K || Atype == LFAMD_TYPE_Q5_K || Atype == LFAMD_TYPE_Q6_K);
    const int ks = scaled_lw ? 1 : wide_ksplit(n_rb * n_ct, nb); // the scaled-operand body never splits K
    const int nbs = (nb + ks - 1) / ks;
    const int n_wg = n_rb * n_ct * ks;
    if (ks > 1) {
        for (int i = 0; i < mats.count; i++) {
            long total = mats.m[i] * n;
            int blocks = (int)((total + 256 * 8 - 1) / (256 * 8));
            zero_c_kernel<<<blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks), 256, 0, s>>>(mats.C[i], mats.ldc[i], mats.m[i], n);
        }
    }
    return wide_go(Atype, mode, (float *)P, P_bytes, mats, nb, Xh, d8T, Xm, n, n_pad, n_rb, n_ct, ks, nbs, (unsigned)n_wg, 0, s);
}

hipError_t lfamd_lw_dual_go(int type_a, const gemm_mats &ma, int n_rb_a, int type_b, const gemm_mats &mb, int n_rb_b, int nb,
                            const void *Xh, const void *d8T, const void *Xm, long n, long n_pad, int n_ct, hipStream_t s);

// Does ONE launch of the 128 x 128 loader-wave body take two groups of matrices (row blocks of 128 rows each; n_pad staged token
// rows)?  When the combined grid fills more than half the chip in one round; beyond one round the separate launches with their tail
// handling do as well.
extern "C" int lfamd_gemm_wide_dual_ok(long row_blocks_a, long row_blocks_b, long n_pad) {
    const long tiles = (row_blocks_a + row_blocks_b) * (n_pad / WD_COLS);
    return row_blocks_a > 0 && row_blocks_b > 0 && tiles >= LW_FULL_GRID && tiles <= 256;
}

// Scaled staged activations, two groups of matrices of two K-quant types (type_b = Q6_K, type_a = Q4_K | Q5_K) in that one launch.
// Precondition: lfamd_gemm_wide_dual_ok (else hipErrorInvalidValue).
extern "C" hipError_t lfamd_launch_gemm_wide_dual(int type_a, int count_a, const void *const *A_a, const long *m_a,
                                                  float *const *C_a, const long *ldc_a, int type_b, int count_b,
                                                  const void *const *A_b, const long *m_b, float *const *C_b, const long *ldc_b,
                                                  long k, const void *Xh, const void *d8T, const void *Xm, long n, long n_pad,
                                                  int mode, hipStream_t s) {
    if (!(mode & 2) || !lw_allowed(mode) || type_b != LFAMD_TYPE_Q6_K || (type_a != LFAMD_TYPE_Q4_K && type_a != LFAMD_TYPE_Q5_K) ||
        count_a <= 0 || count_b <= 0 || count_a > GEMM_MAX_MATS || count_b > GEMM_MAX_MATS || n_pad % WD_COLS)
        return hipErrorInvalidValue;
    gemm_mats ma, mb;
    const int n_rb_a = fill_gemm_mats(ma, count_a, A_a, m_a, C_a, ldc_a), n_rb_b = fill_gemm_mats(mb, count_b, A_b, m_b, C_b, ldc_b);
    if (!lfamd_gemm_wide_dual_ok(n_rb_a, n_rb_b, n_pad))
        return hipErrorInvalidValue;
    return lfamd_lw_dual_go(type_a, ma, n_rb_a, type_b, mb, n_rb_b, (int)(k / 256), Xh, d8T, Xm, n, n_pad, (int)(n_pad / WD_COLS), s);
}

extern "C" hipError_t lfamd_launch_gemm_wide(int Atype, const void *A, long m, long k, const void *Xh, const void *d8T,
                                             const void *Xm, long n, long n_pad, float *C, long ldc, int mode, void *P, size_t P_bytes,
                                             hipStream_t s) {
    return lfamd_launch_gemm_wide_multi(Atype, 1, &A, &m, k, Xh, d8T, Xm, n, n_pad, &C, &ldc, mode, P, P_bytes, s);
}

// GGML_OP_MUL_MAT_ID batches: one launch over (expert, row block, token tile); see gemm_mats.  n_pad = slots staged by the
// activation prep (>= poff[experts-1] + cnt, multiple of 128); ct_max = token tiles of the worst case (all rows to one expert).
extern "C" hipError_t lfamd_launch_gemm_wide_moe(int Atype, const void *W, long expert_bytes, int experts, long m, long k,
                                                 const void *Xh, const void *d8T, const void *Xm, long n_pad, const int *cnt,
                                                 const int *poff, const int *slot_row, int ct_max, float *C, long ldc,
                                                 int mode, hipStream_t s) {
    if (m <= 0 || experts <= 0 || ct_max <= 0)
        return hipSuccess;
    const int nb = (int)(k / 256);
    gemm_mats mats;
    for (int i = 0; i < GEMM_MAX_MATS; i++)
        mats.A[i] = (const uint8_t *)W, mats.C[i] = C, mats.m[i] = m, mats.ldc[i] = ldc, mats.rb_end[i] = 0;
    mats.count = 1;
    mats.moe_cnt = cnt, mats.moe_poff = poff, mats.moe_slot_row = slot_row, mats.expert_bytes = expert_bytes, mats.moe_ct_max = ct_max;
    const int n_rb = (int)((m + 127) / 128);
    const unsigned n_wg = (unsigned)experts * n_rb * ct_max;
    if (Atype != LFAMD_TYPE_Q4_K && Atype != LFAMD_TYPE_Q5_K && Atype != LFAMD_TYPE_Q6_K)
        return hipErrorInvalidValue;
    // scaled operands, Q4_K experts: the 256 x 128 row-split body (gemm_kr.hip)
    if ((mode & 2) && lw_allowed(mode) && Atype == LFAMD_TYPE_Q4_K)
        return lfamd_kr_moe_go(Atype, mats, nb, Xh, d8T, Xm, n_pad, experts, ct_max, s);
    return wide_go(Atype, mode, nullptr, 0, mats, nb, Xh, d8T, Xm, n_pad, n_pad, n_rb, ct_max, 1, nb, n_wg, 1, s);
}
