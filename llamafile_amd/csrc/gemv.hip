// gemv.hip — the decode GEMVs' host side: the launch plan (which kernel form, how many waves, which grid, how much LDS), the
// matrix tables and the launches.  No kernel is compiled here: the units gemv_q4k / q5k / q6k / q40 / q41 / q50 / q51 / q2k /
// q3k / iq4xs / iq4nl / dual / q80 / q80b / q80r / q80rb.hip instantiate them (gemv_impl.h, gemv_q80_impl.h, gemv_q80r_impl.h) and hand out
// their addresses.
#include "gemv_launch.h"
#include <stdlib.h>

extern "C" int lfamd_num_cus(void) {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess)
            cus = p.multiProcessorCount;
        if (cus <= 0)
            cus = 256;
    }
    return cus;
}

// ---- the units: one table
struct kq_unit {
    int type;
    gemv_kernel_fn *kernel;
    // which types take 32-row items on long walks (LFAMD_GEMV_ROWS32): the ones whose dot is long enough for a second,
    // independent one to fill its gaps.  128256 x 4096, 16-row -> 32-row items: Q6_K 82.0 -> 73.7 us, Q2_K 44.6 -> 40.8, Q3_K
    // 50.3 -> 44.9, IQ4_XS 58.1 -> 55.4; the light dots lose a little: Q4_K 47.4 -> 47.7, Q5_K 58.1 -> 58.5, Q4_0 46.0 -> 47.6
    // (65536 rows: 27.0 -> 28.2).  IQ4_NL carries IQ4_XS's look-up on Q4_0's image (816 VALU per kernel against Q4_0's 564) and
    // sides with IQ4_XS: 128256 x 4096 66.1 / 66.8 -> 63.5 / 62.8 us (two processes each, alternated), 65536 rows 29.1 / 30.7 ->
    // 30.1 / 29.4 (a tie); 14336 x 4096 walks 4 half-tiles per work-group and never takes the form (9.4 us either way)
    bool rows32;
    gemv_kernel_fn *with_q6k; // the two-type unit that pairs this type with Q6_K
};
static const kq_unit kq_units[] = {
    {LFAMD_TYPE_Q4_K, lfamd_gemv_kernel_q4k, false, lfamd_gemv_kernel_q4k_q6k},
    {LFAMD_TYPE_Q5_K, lfamd_gemv_kernel_q5k, false, lfamd_gemv_kernel_q5k_q6k},
    {LFAMD_TYPE_Q6_K, lfamd_gemv_kernel_q6k, true, nullptr},
    {LFAMD_TYPE_Q4_0, lfamd_gemv_kernel_q40, false, nullptr},
    {LFAMD_TYPE_Q4_1, lfamd_gemv_kernel_q41, false, nullptr},
    {LFAMD_TYPE_Q5_0, lfamd_gemv_kernel_q50, false, nullptr},
    {LFAMD_TYPE_Q5_1, lfamd_gemv_kernel_q51, false, nullptr},
    {LFAMD_TYPE_Q2_K, lfamd_gemv_kernel_q2k, true, nullptr},
    {LFAMD_TYPE_Q3_K, lfamd_gemv_kernel_q3k, true, nullptr},
    {LFAMD_TYPE_IQ4_XS, lfamd_gemv_kernel_iq4xs, true, nullptr},
    {LFAMD_TYPE_IQ4_NL, lfamd_gemv_kernel_iq4nl, true, nullptr},
};
static const kq_unit *kq_unit_of(int Atype) {
    for (const kq_unit &u : kq_units)
        if (u.type == Atype)
            return &u;
    return nullptr;
}

// early: the launch fits the preloaded arguments (early_fits), so a PLAIN plan runs on the unit's EARLY kernels and a TWO_TYPES
// plan on the two-type unit's early ones.  Same forms, so a unit that holds the planned kernel holds this one too.
static const void *kernel_of(int Atype, int f32in, const lfamd_gemv_plan &p, int q80_mode, bool early = false) {
    if (p.variant == LFAMD_GEMV_Q80)
        return Atype != LFAMD_TYPE_Q8_0 ? nullptr : f32in ? lfamd_gemv_kernel_q80_f32(p.nc, q80_mode) : lfamd_gemv_kernel_q80_q80(p.nc, q80_mode);
    if (p.variant == LFAMD_GEMV_Q80R)
        return Atype != LFAMD_TYPE_Q8_0 ? nullptr : f32in ? lfamd_gemv_kernel_q80r_f32(p.nc, p.nw, p.ch) : lfamd_gemv_kernel_q80r_q80(p.nc, p.nw, p.ch);
    const kq_unit *u = kq_unit_of(Atype);
    gemv_kernel_fn *fn = !u ? nullptr : p.variant == LFAMD_GEMV_TWO_TYPES ? u->with_q6k : u->kernel;
    int variant = p.variant;
    if (early && p.variant == LFAMD_GEMV_PLAIN)
        variant = LFAMD_GEMV_EARLY;
    if (early && p.variant == LFAMD_GEMV_TWO_TYPES)
        variant = KQ_TWO_TYPES_EARLY;
    return fn ? fn(variant, p.nc, f32in, p.nw, p.ch) : nullptr;
}

extern "C" int lfamd_gemv_has_kernel(int Atype, int f32in, const lfamd_gemv_plan *p) {
    return kernel_of(Atype, f32in, *p, 0) != nullptr;
}

// ---- the plan

// Super-blocks of a row of k weights.  The 32-block types may come with rows that end inside the last one (LFAMD_TYPE_PAD256: the
// image is padded with zero blocks); every other caller passes whole 256-weight groups.
static int sb_of(long k) {
    return (int)((k + 255) / 256);
}
// The kernels' `nb` argument (gemv_impl.h, kq_nb_of): the row's 32-blocks for the types on 32-block activations, else its super-blocks
static int nb_arg(int Atype, long k) {
    return lfamd_image_of(Atype, k).block32() ? (int)(k / 32) : sb_of(k);
}

// LDS budget: keep one launch's activation image under 160 KiB; otherwise split the columns.
static const size_t IMAGE_CAP = 150 * 1024;

extern "C" int lfamd_gemv_depth_ok(long k) {
    return (size_t)sb_of(k) * XBLK <= IMAGE_CAP;
}

extern "C" size_t lfamd_gemv_lds_bytes(int Atype, int nc, long k, int nw, int rows) {
    return Atype == LFAMD_TYPE_Q8_0 ? q80_lds_bytes(nc, q80_quads(k)) : kq_lds_of(nc, sb_of(k), nw, rows).bytes;
}

extern "C" int lfamd_gemv_cols_per_launch(int Atype, long k) {
    const size_t per_col = Atype == LFAMD_TYPE_Q8_0 ? q80_lds_bytes(1, q80_quads(k)) : (size_t)sb_of(k) * XBLK;
    const int nc = (int)(IMAGE_CAP / (per_col ? per_col : 1));
    int step = nc < 1 ? 0 : (nc > 8 ? 8 : nc);
    // deep rows on the 8-wave x 4-block kernels: six and more columns per launch spill registers (256 VGPRs + 29..53
    // spilled).  Past 32 super-blocks two passes of at most five columns are faster (4096 x 14336, n = 8: Q4_K 47.9 -> 45.8
    // us, Q6_K 79.9 -> 67.0); at 32 the second pass costs more than the spills (4096 x 8192: 24.5 vs 29.7 us)
    if (Atype != LFAMD_TYPE_Q8_0 && sb_of(k) > 32 && step > 5)
        step = 5;
    return step;
}

// Columns one launch of the relaxed-order Q8_0 kernel takes (LFAMD_GEMV_MULTI_RELAXED): as many of eight as keep its LDS under the
// cap; 0 = one column does not fit (or k is no row of whole blocks) and the call runs gemv_q80_kernel.
extern "C" int lfamd_gemv_q80_relaxed_cols(long k) {
    if (k <= 0 || k % 32 || k / 32 > (1 << 20))
        return 0;
    int nc = 8;
    while (nc > 0 && q80r_lds_of(nc, q80_quads(k), Q80R_WAVES).bytes > IMAGE_CAP)
        nc--;
    return nc;
}

// the relaxed-order kernel's LDS for nc columns of a k-long row (the layout: gemv_launch.h, q80r_lds_of)
extern "C" size_t lfamd_gemv_q80_relaxed_lds_bytes(int nc, long k) {
    return q80r_lds_of(nc, q80_quads(k), Q80R_WAVES).bytes;
}

// every work-group the same number of items: the grid that covers `items` with at most max_wg work-groups
static int even_grid(int items, int max_wg, int *per_wg = nullptr) {
    const int per = (items + max_wg - 1) / max_wg;
    if (per_wg)
        *per_wg = per;
    return (items + per - 1) / per;
}

// What one launch of `nc` columns looks like on a device of `cus` CUs.  work: the launch's half-tiles (16 weight rows; Q8_0:
// its 8-row groups), work_b: the Q6_K side's half-tiles of LFAMD_GEMV_DUAL; count: matrices in the launch.  f32 and pre-
// quantised activations take the same form (the two launches stay bit-identical), so the plan does not ask.  Touches no
// device.  Returns 0, or -1 for a type or kind without a decode GEMV and for a launch without work or a device without CUs.
extern "C" int lfamd_gemv_plan_of(int kind, int Atype, int nc, long work, long work_b, long k, int count, int cus, lfamd_gemv_plan *p) {
    *p = lfamd_gemv_plan{};
    p->nc = nc;
    if (work <= 0 || cus <= 0 || (kind == LFAMD_GEMV_DUAL && work_b <= 0))
        return -1;
    if (kind == LFAMD_GEMV_MULTI_RELAXED) {
        // Q8_0 with K split over the waves of one persistent work-group per CU; work: the launch's 8-row groups, one item each.
        // NW and the chunk depend on k alone, so the order in which an output's terms are added does too.
        if (Atype != LFAMD_TYPE_Q8_0 || nc > lfamd_gemv_q80_relaxed_cols(k))
            return -1;
        const int nquads = q80_quads(k);
        p->variant = LFAMD_GEMV_Q80R, p->nw = Q80R_WAVES, p->ch = q80r_chunk_quads(nquads), p->rows = 8;
        p->grid = even_grid((int)work, cus);
        p->lds = (int)q80r_lds_of(nc, nquads, Q80R_WAVES).bytes;
        return 0;
    }
    if (Atype == LFAMD_TYPE_Q8_0) {
        if (kind != LFAMD_GEMV_MULTI)
            return -1;
        p->variant = LFAMD_GEMV_Q80, p->nw = Q80_WAVES, p->rows = 8;
        p->grid = (int)(unsigned)((work + Q80_WAVES - 1) / Q80_WAVES);
        p->lds = (int)q80_lds_bytes(nc, q80_quads(k));
        return 0;
    }
    const kq_unit *u = kq_unit_of(Atype);
    if (!u)
        return -1;
    const int nb = sb_of(k), n_ht = (int)work;
    p->rows = 16;
    switch (kind) {
    case LFAMD_GEMV_MULTI: {
        if (nc == 1) {
            // a launch of at most one half-tile per CU (attn_output, attn_k/v alone: the whole kernel is one prologue + one
            // item) runs 8 waves of two super-blocks each: half as many waves contend for a SIMD while the row is quantised
            // (two blocks per pass cost 140 VALU against 2 x 120) — 4096 x 4096: 4.35 -> 3.88 us, 1024 x 4096: 3.65 -> 3.27,
            // 4096 x 8192: 6.83 -> 6.49.  With more tiles per work-group the 16-wave form streams better (14336 x 4096:
            // 8.4 vs 9.1 us), and rows of 56 super-blocks lose too (9.4 vs 10.3).
            // (round 3, 8 waves for launches of MANY items too: 14336 x 4096 8.30 vs 9.10 us, 28672 13.3 vs 14.2, 32000 (Q6_K) 23.5 vs
            // 24.3, 128256 83.7 vs 84.2 — the 16-wave form keeps them; only at 57344 rows, 14 half-tiles per work-group, does
            // the 8-wave form win (24.4 -> 23.5), which is the expert launch below)
            if (n_ht <= cus && nb <= 32)
                p->nw = 8, p->ch = 2;
            else
                p->nw = 16, p->ch = nb <= 16 ? 1 : 2;
        } else {
            // several columns (n = 2..8): 16 waves when a work-group walks several half-tiles (14336 x 4096, n = 4: 24.0 ->
            // 17.5 us), 8 waves of two blocks for single-tile launches (4096 x 4096: the same either way) and for deep rows
            // (4096 x 14336, n = 4: 22.6 vs 23.7 us with 16)
            if (nb <= 16 && n_ht > cus)
                p->nw = 16, p->ch = 1;
            else
                p->nw = 8, p->ch = nb <= 16 ? 2 : 4;
        }
        // persistent grid: 16 waves per CU, every work-group the same number of half-tiles
        const int max_wg = (16 / p->nw) * cus;
        int per_wg;
        p->grid = even_grid(n_ht, max_wg, &per_wg);
        // one matrix: the variant that issues its first weight loads from the preloaded arguments
        p->variant = nc == 1 && count == 1 ? LFAMD_GEMV_EARLY : LFAMD_GEMV_PLAIN;
        // Long walks (output.weight: 63 half-tiles per work-group) take items of a full 32-row tile — both half-tiles in
        // flight together, ONE barrier + reduce + store per 74 KB instead of per 37 KB; same arithmetic per row, same bits.
        // 128256 x 4096 Q6_K: 82.8 -> 73.6 us (5.2 -> 5.9 TB/s); 32000 x 4096: 23.6 -> 22.8 (types: kq_unit::rows32).  Short walks
        // lose to the coarser division of the tiles over the work-groups (28672 x 4096, 3.5 tiles each: 13.1 -> 14.3 us), hence
        // the bound.  LFAMD_GEMV_PAIR_MIN=<half-tiles per work-group> moves it (0 = never).
        static const int pair_min = getenv("LFAMD_GEMV_PAIR_MIN") ? atoi(getenv("LFAMD_GEMV_PAIR_MIN")) : 16;
        if (nc == 1 && p->nw == 16 && p->ch == 1 && u->rows32 && pair_min > 0 && per_wg >= pair_min)
            p->variant = LFAMD_GEMV_ROWS32, p->rows = 32, p->grid = even_grid(n_ht / 2, max_wg);
        break;
    }
    case LFAMD_GEMV_IDS:
        // gate + up experts in one launch (4 x 896 half-tiles of 16 super-blocks, 14 per 16-wave work-group): every item ends in a
        // work-group barrier, and two independent 8-wave work-groups per CU hide each other's — Mixtral decode pass 1.823 ->
        // 1.706 ms (548 -> 586 tokens/s).  Shorter walks keep the 16-wave form (see LFAMD_GEMV_MULTI).
        // (the 16-wave form with 32-row items, seven per work-group, was measured too: 1.748 ms per pass against 1.702 for this one)
        if (nb <= 16 && n_ht >= 8 * cus)
            p->nw = 8, p->ch = 2;
        else
            p->nw = 16, p->ch = nb <= 16 ? 1 : 2;
        p->variant = LFAMD_GEMV_EXPERT, p->grid = even_grid(n_ht, (16 / p->nw) * cus);
        break;
    case LFAMD_GEMV_IDS_PAIR:
        // both launches' half-tiles (n_ht each) on one grid: half of the CUs' work-groups per expert
        // (round 3, 8 waves x two work-groups per CU for this launch: Mixtral decode pass 1.712 -> 1.919 ms; 16 waves stay)
        p->variant = LFAMD_GEMV_EXPERT_PAIR, p->nw = 16, p->ch = nb <= 16 ? 1 : 2;
        p->grid = p->grid_b = even_grid(n_ht, cus / 2 > 0 ? cus / 2 : 1);
        break;
    case LFAMD_GEMV_DUAL: {
        if (!u->with_q6k)
            return -1;
        p->variant = LFAMD_GEMV_TWO_TYPES, p->nw = 16, p->ch = nb <= 16 ? 1 : 2;
        // one persistent grid of at most one work-group per CU, split between the types so that the slower side finishes
        // first: a Q6_K half-tile costs about 1.35 Q4_K / Q5_K ones (dot instructions and bytes), and with equal tiles per
        // work-group the few Q6_K work-groups of attn_v set the launch's length (7.06 -> see DESIGN §4)
        const int n_ht_b = (int)work_b, max_wg = cus;
        long best = -1;
        for (int pb = 1; pb <= n_ht_b; pb++) {
            const int gb = (n_ht_b + pb - 1) / pb;
            if (gb >= max_wg)
                continue;
            const int pa = (n_ht + (max_wg - gb) - 1) / (max_wg - gb);
            const long cost = (long)pa * 100 > (long)pb * 135 ? (long)pa * 100 : (long)pb * 135;
            if (best < 0 || cost < best)
                best = cost, p->grid_b = gb, p->grid = (n_ht + pa - 1) / pa;
        }
        if (best < 0) { // (more Q6_K half-tiles than CUs can never be one per work-group: equal shares)
            const int per_wg = (n_ht + n_ht_b + max_wg - 1) / max_wg;
            p->grid = (n_ht + per_wg - 1) / per_wg, p->grid_b = (n_ht_b + per_wg - 1) / per_wg;
        }
        break;
    }
    default:
        return -1;
    }
    p->lds = (int)kq_lds_of(nc, nb, p->nw, p->rows).bytes;
    return 0;
}

// ---- the launches: one per kernel signature

static hipError_t launch(const void *kernel, const lfamd_gemv_plan &p, void **args, hipStream_t s) {
    if (!kernel) // (a planned form that its unit does not instantiate: lfamd_gemv_has_kernel, tests/test_gemv_plan.py)
        return hipErrorInvalidDeviceFunction;
    if (p.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
        if (e != hipSuccess)
            return e;
    }
    (void)hipLaunchKernel(kernel, dim3(p.grid + p.grid_b), dim3(p.nw * 64), args, p.lds, s);
    return hipGetLastError();
}

// gemv_kq_kernel
static hipError_t launch_kq(const void *kernel, const lfamd_gemv_plan &p, const void *B, size_t brb, long col0, int nbk, int n_ht,
                            gemv_mats &mats, hipStream_t s) {
    void *args[] = {&B, &brb, &col0, &nbk, &n_ht, (void *)&p.grid, &mats};
    return launch(kernel, p, args, s);
}

// A one-column launch of one to three matrices fits the preloaded arguments of the early kernels (a PLAIN plan of four keeps
// gemv_kq_kernel; ROWS32 and the expert launches have kernels of their own).
static bool early_fits(const lfamd_gemv_plan &p, const gemv_mats &mats) {
    return p.nc == 1 && mats.count <= 3 && (p.variant == LFAMD_GEMV_EARLY || p.variant == LFAMD_GEMV_PLAIN);
}
// the boundary behind matrix i, for the pick without a count
static int pre_boundary(const gemv_mats &mats, int i) {
    return i + 1 < mats.count ? mats.ht_end[i] : KQ_NO_BOUNDARY;
}

// gemv_kq_early_kernel: the column is folded into the row pointer and into a copy of the table's result pointers
static hipError_t launch_kq_early(const void *kernel, const lfamd_gemv_plan &p, const void *B, size_t brb, long col0, int nbk, int n_ht,
                                  const gemv_mats &mats, hipStream_t s) {
    gemv_mats mc = mats;
    for (int i = 0; i < GEMV_MAX_MATS; i++)
        if (mc.C[i])
            mc.C[i] += col0 * mc.ldc[i];
    const uint8_t *xrow = (const uint8_t *)B + col0 * (long)brb;
    int e0 = pre_boundary(mats, 0), e1 = pre_boundary(mats, 1);
    void *args[] = {&xrow, &mc.A[0], &mc.A[1], &mc.A[2], &nbk, &n_ht, (void *)&p.grid, &e0, &e1, &mc};
    return launch(kernel, p, args, s);
}

// gemv_kq_dual_kernel
static hipError_t launch_kq_dual(const void *kernel, const lfamd_gemv_plan &p, const void *B, size_t brb, int nbk, int n_ht_a, int n_ht_b,
                                 gemv_mats &ma, gemv_mats &mb, hipStream_t s) {
    void *args[] = {&B, &brb, &nbk, &n_ht_a, &n_ht_b, (void *)&p.grid, (void *)&p.grid_b, &ma, &mb};
    return launch(kernel, p, args, s);
}

// gemv_kq_dual_early_kernel (B: the one activation row)
static hipError_t launch_kq_dual_early(const void *kernel, const lfamd_gemv_plan &p, const void *B, int nbk, int n_ht_a, int n_ht_b,
                                       gemv_mats &ma, gemv_mats &mb, hipStream_t s) {
    int ea0 = pre_boundary(ma, 0);
    void *args[] = {&B, &ma.A[0], &ma.A[1], &mb.A[0], &nbk, &n_ht_a, &n_ht_b, (void *)&p.grid, &ea0, (void *)&p.grid_b, &ma, &mb};
    return launch(kernel, p, args, s);
}

// gemv_kq_ids_pair_kernel
static hipError_t launch_kq_ids_pair(const void *kernel, const lfamd_gemv_plan &p, const void *Ba, const void *Bb, size_t brb, int nbk, int n_ht,
                                     gemv_mats &ma, gemv_mats &mb, hipStream_t s) {
    void *args[] = {&Ba, &Bb, &brb, &nbk, &n_ht, &n_ht, (void *)&p.grid, (void *)&p.grid_b, &ma, &mb};
    return launch(kernel, p, args, s);
}

// gemv_q80_kernel
static hipError_t launch_q80(const void *kernel, const lfamd_gemv_plan &p, const void *B, size_t brb, long col0, long k, long n_total,
                             int vregs32, int precise, q80_mats &mats, hipStream_t s) {
    int nblocks = (int)(k / 32), nquads = q80_quads(k);
    void *args[] = {&B, &brb, &col0, &nblocks, &nquads, &n_total, &vregs32, &precise, &mats};
    return launch(kernel, p, args, s);
}

// gemv_q80r_kernel
static hipError_t launch_q80r(const void *kernel, const lfamd_gemv_plan &p, const void *B, size_t brb, long col0, long k, int n_items,
                              q80_mats &mats, hipStream_t s) {
    int nblocks = (int)(k / 32), nquads = q80_quads(k);
    void *args[] = {&B, &brb, &col0, &nblocks, &nquads, &n_items, (void *)&p.grid, &mats};
    return launch(kernel, p, args, s);
}

// ---- the matrix tables

// The K-quant kernels' table of `count` matrices, rows m[j] <= 0 left out; returns its half-tiles.  ids != nullptr: matrix j is
// expert ids[id_idx[j]] of the stack at A[j].  The unused entries repeat entry 0 with no rows.
static int fill_mats(gemv_mats &mats, int count, const void *const *A, const long *m, float *const *C, const long *ldc,
                     const int32_t *ids = nullptr, long expert_bytes = 0, int experts = 0, const int *id_idx = nullptr) {
    int n_ht = 0;
    mats.count = 0;
    mats.ids = ids, mats.expert_bytes = expert_bytes, mats.experts = experts;
    mats.A[0] = nullptr, mats.C[0] = nullptr, mats.ldc[0] = 0, mats.id_idx[0] = 0; // (what the unused entries repeat when no matrix has rows)
    for (int j = 0; j < count; j++) {
        if (m[j] <= 0)
            continue;
        const int i = mats.count++;
        mats.A[i] = (const uint8_t *)A[j], mats.C[i] = C[j], mats.m[i] = m[j], mats.ldc[i] = ldc[j];
        mats.id_idx[i] = id_idx ? id_idx[j] : 0;
        n_ht += (int)(((m[j] + 31) / 32) * 2);
        mats.ht_end[i] = n_ht;
    }
    for (int i = mats.count; i < GEMV_MAX_MATS; i++) {
        mats.A[i] = mats.A[0], mats.C[i] = mats.C[0], mats.m[i] = 0, mats.ldc[i] = ids ? mats.ldc[0] : 0, mats.ht_end[i] = n_ht;
        mats.id_idx[i] = mats.id_idx[0];
    }
    return n_ht;
}

// ---- the entry points

// Btype: the weight type's vec_dot type (pre-quantised rows) or LFAMD_TYPE_F32 (quantise in-kernel).
// `count` matrices (<= GEMV_MAX_MATS for the K-quants, any number for Q8_0) of the same type and k share B.
extern "C" hipError_t lfamd_launch_gemv_multi(int Atype, int count, const void *const *A, const long *m, long k, int Btype,
                                              const void *B, size_t b_row_bytes, long n, float *const *C, const long *ldc,
                                              int vregs32, int precise, int relaxed, hipStream_t s) {
    if (count <= 0 || n <= 0)
        return hipSuccess;
    if (relaxed && Atype == LFAMD_TYPE_Q8_0 && lfamd_gemv_q80_relaxed_cols(k) > 0) {
        // relaxed order: the 8-row groups of up to four matrices concatenated, one item each (no padding between matrices)
        const int rstep = lfamd_gemv_q80_relaxed_cols(k), f32in = Btype == LFAMD_TYPE_F32, cus = lfamd_num_cus();
        hipError_t e = hipSuccess;
        for (int j0 = 0; j0 < count && e == hipSuccess; j0 += GEMV_MAX_MATS) {
            q80_mats qm;
            long rgs = 0;
            qm.count = 0;
            for (int j = j0; j < count && j < j0 + GEMV_MAX_MATS; j++) {
                if (m[j] <= 0)
                    continue;
                const int i = qm.count++;
                qm.A[i] = (const uint8_t *)A[j], qm.C[i] = C[j], qm.m[i] = m[j], qm.ldc[i] = ldc[j];
                rgs += (m[j] + 7) / 8;
                qm.rg_end[i] = rgs;
            }
            if (qm.count == 0)
                continue;
            if (rgs > 0x7fffffffL)
                return hipErrorInvalidValue;
            for (int i = qm.count; i < GEMV_MAX_MATS; i++)
                qm.A[i] = qm.A[0], qm.C[i] = qm.C[0], qm.m[i] = 0, qm.ldc[i] = 0, qm.rg_end[i] = rgs;
            for (long col0 = 0; col0 < n && e == hipSuccess; col0 += rstep) {
                const int nc = (int)((n - col0) < rstep ? (n - col0) : rstep);
                lfamd_gemv_plan p;
                if (lfamd_gemv_plan_of(LFAMD_GEMV_MULTI_RELAXED, Atype, nc, rgs, 0, k, qm.count, cus, &p) != 0)
                    return hipErrorInvalidValue;
                e = launch_q80r(kernel_of(Atype, f32in, p, 0), p, B, b_row_bytes, col0, k, (int)rgs, qm, s);
            }
        }
        return e;
    }
    const int step = lfamd_gemv_cols_per_launch(Atype, k);
    if (step == 0)
        return hipErrorInvalidValue;
    const int f32in = Btype == LFAMD_TYPE_F32, cus = lfamd_num_cus();
    lfamd_gemv_plan p;
    hipError_t e = hipSuccess;
    if (Atype == LFAMD_TYPE_Q8_0) {
        // n = 1: the whole problem is one column of 2x1 / 1x1 tiles, so the summation mode is uniform
        const int mode = n == 1 ? ((vregs32 || precise) ? 1 : 0) : 2;
        for (int j0 = 0; j0 < count && e == hipSuccess; j0 += GEMV_MAX_MATS) { // groups of up to four matrices per launch
            q80_mats qm;
            long rgs = 0;
            qm.count = 0;
            for (int j = j0; j < count && j < j0 + GEMV_MAX_MATS; j++) {
                if (m[j] <= 0)
                    continue;
                const int i = qm.count++;
                qm.A[i] = (const uint8_t *)A[j], qm.C[i] = C[j], qm.m[i] = m[j], qm.ldc[i] = ldc[j];
                rgs += (m[j] + 7) / 8;
                rgs = (rgs + Q80_WAVES - 1) / Q80_WAVES * Q80_WAVES; // a work-group never straddles two matrices
                qm.rg_end[i] = rgs;
            }
            if (qm.count == 0)
                continue;
            for (int i = qm.count; i < GEMV_MAX_MATS; i++)
                qm.A[i] = qm.A[0], qm.C[i] = qm.C[0], qm.m[i] = 0, qm.ldc[i] = 0, qm.rg_end[i] = rgs;
            for (long col0 = 0; col0 < n && e == hipSuccess; col0 += step) {
                const int nc = (int)((n - col0) < step ? (n - col0) : step);
                lfamd_gemv_plan_of(LFAMD_GEMV_MULTI, Atype, nc, rgs, 0, k, qm.count, cus, &p);
                e = launch_q80(kernel_of(Atype, f32in, p, mode), p, B, b_row_bytes, col0, k, n, vregs32, precise, qm, s);
            }
        }
        return e;
    }
    if (count > GEMV_MAX_MATS || !kq_unit_of(Atype))
        return hipErrorInvalidValue;
    gemv_mats mats;
    const int n_ht = fill_mats(mats, count, A, m, C, ldc);
    if (mats.count == 0)
        return hipSuccess;
    for (long col0 = 0; col0 < n && e == hipSuccess; col0 += step) {
        const int nc = (int)((n - col0) < step ? (n - col0) : step);
        lfamd_gemv_plan_of(LFAMD_GEMV_MULTI, Atype, nc, n_ht, 0, k, mats.count, cus, &p);
        if (early_fits(p, mats))
            e = launch_kq_early(kernel_of(Atype, f32in, p, 0, true), p, B, b_row_bytes, col0, nb_arg(Atype, k), n_ht, mats, s);
        else
            e = launch_kq(kernel_of(Atype, f32in, p, 0), p, B, b_row_bytes, col0, nb_arg(Atype, k), n_ht, mats, s);
    }
    return e;
}

// ONE activation row, two groups of matrices of two K-quant types (type_b = Q6_K, type_a = Q4_K or Q5_K): one launch.
extern "C" hipError_t lfamd_launch_gemv_dual(int type_a, int count_a, const void *const *A_a, const long *m_a, float *const *C_a,
                                             const long *ldc_a, int type_b, int count_b, const void *const *A_b, const long *m_b,
                                             float *const *C_b, const long *ldc_b, long k, int Btype, const void *B,
                                             size_t b_row_bytes, hipStream_t s) {
    if (type_b != LFAMD_TYPE_Q6_K || count_a <= 0 || count_b <= 0 || count_a > GEMV_MAX_MATS || count_b > GEMV_MAX_MATS ||
        !lfamd_gemv_depth_ok(k))
        return hipErrorInvalidValue;
    gemv_mats ma, mb;
    const int n_ht_a = fill_mats(ma, count_a, A_a, m_a, C_a, ldc_a), n_ht_b = fill_mats(mb, count_b, A_b, m_b, C_b, ldc_b);
    lfamd_gemv_plan p;
    if (ma.count == 0 || mb.count == 0 || // (the caller sends an empty group through the one-type path)
        lfamd_gemv_plan_of(LFAMD_GEMV_DUAL, type_a, 1, n_ht_a, n_ht_b, k, ma.count + mb.count, lfamd_num_cus(), &p) != 0)
        return hipErrorInvalidValue;
    const int f32in = Btype == LFAMD_TYPE_F32;
    if (ma.count <= 2 && mb.count == 1) // (every Q4_K_M / Q5_K_M layer: attn_q/k + attn_v)
        return launch_kq_dual_early(kernel_of(type_a, f32in, p, 0, true), p, B, nb_arg(type_a, k), n_ht_a, n_ht_b, ma, mb, s);
    return launch_kq_dual(kernel_of(type_a, f32in, p, 0), p, B, b_row_bytes, nb_arg(type_a, k), n_ht_a, n_ht_b, ma, mb, s);
}

// GGML_OP_MUL_MAT_ID for ONE activation row: `count` (<= GEMV_MAX_MATS) outputs C[j] = W[ids[id_idx[j]]] x B, the expert
// index read on the device.  Q4_K / Q5_K / Q6_K stacks; Btype F32 or Q8_K.
// W[j]: the expert tensor matrix j picks from (ffn_gate_exps and ffn_up_exps may share one launch: same activations)
extern "C" hipError_t lfamd_launch_gemv_ids(int Atype, int count, const void *const *W, long expert_bytes, int experts,
                                            const int32_t *ids, const int *id_idx, long m, long k, int Btype, const void *B,
                                            size_t b_row_bytes, float *const *C, hipStream_t s) {
    lfamd_gemv_plan p;
    if (count <= 0 || count > GEMV_MAX_MATS || m <= 0 || !lfamd_gemv_depth_ok(k))
        return hipErrorInvalidValue;
    const long ms[GEMV_MAX_MATS] = {m, m, m, m};
    gemv_mats mats;
    const int n_ht = fill_mats(mats, count, W, ms, C, ms, ids, expert_bytes, experts, id_idx);
    if (lfamd_gemv_plan_of(LFAMD_GEMV_IDS, Atype, 1, n_ht, 0, k, count, lfamd_num_cus(), &p) != 0)
        return hipErrorInvalidValue;
    const void *kernel = kernel_of(Atype, Btype == LFAMD_TYPE_F32, p, 0);
    if (!kernel) // (a K-quant type whose unit holds no expert kernels)
        return hipErrorInvalidValue;
    return launch_kq(kernel, p, B, b_row_bytes, 0, nb_arg(Atype, k), n_ht, mats, s);
}

// two experts of one tensor, each against its own activation row (ffn_down_exps at decode): one launch
extern "C" hipError_t lfamd_launch_gemv_ids_pair(int Atype, const void *W, long expert_bytes, int experts, const int32_t *ids, int idx_a,
                                                 int idx_b, long m, long k, int Btype, const void *Ba, const void *Bb, size_t b_row_bytes,
                                                 float *Ca, float *Cb, hipStream_t s) {
    lfamd_gemv_plan p;
    if (m <= 0 || !lfamd_gemv_depth_ok(k))
        return hipErrorInvalidValue;
    gemv_mats ma, mb;
    const int n_ht = fill_mats(ma, 1, &W, &m, &Ca, &m, ids, expert_bytes, experts, &idx_a);
    fill_mats(mb, 1, &W, &m, &Cb, &m, ids, expert_bytes, experts, &idx_b);
    if (lfamd_gemv_plan_of(LFAMD_GEMV_IDS_PAIR, Atype, 1, n_ht, 0, k, 2, lfamd_num_cus(), &p) != 0)
        return hipErrorInvalidValue;
    const void *kernel = kernel_of(Atype, Btype == LFAMD_TYPE_F32, p, 0);
    if (!kernel)
        return hipErrorInvalidValue;
    return launch_kq_ids_pair(kernel, p, Ba, Bb, b_row_bytes, nb_arg(Atype, k), n_ht, ma, mb, s);
}

extern "C" hipError_t lfamd_launch_gemv(int Atype, const void *A, long m, long k, int Btype, const void *B,
                                        size_t b_row_bytes, long n, float *C, long ldc, int vregs32, int precise, int relaxed,
                                        hipStream_t s) {
    return lfamd_launch_gemv_multi(Atype, 1, &A, &m, k, Btype, B, b_row_bytes, n, &C, &ldc, vregs32, precise, relaxed, s);
}
