// lfamd_internal.h — what the module's translation units share on the host side: the table of the resident weight images (which
// layout a weight type id has at a row length), every extern "C" function that one csrc unit defines and another calls (declared once
// here, so that the defining unit's compiler checks each prototype against its definition; the definitions name the parameters), and
// the byte layouts of the staged activation images.  Public functions: include/lfamd_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/lfamd_hip.h"
#include "lfamd_device.h"

// ---- the resident weight images (DESIGN.md sections 3 and 24).  pack.hip writes them, dequant.hip reads them back, the mat-mul
// bodies read them; which one a (type id, row length) has is answered here and nowhere else.
enum lfamd_layout {
    LY_P4K, LY_P5K, LY_P6K, LY_P40, LY_PK2, LY_PK3, LY_PX4, // PX4: the compact IQ4_XS image
    LY_PCL41, LY_PCL50, LY_PCL51, LY_P80, LY_P4N, // P4N: the P40 image of IQ4_NL (nibbles = codebook indices)
    LY_RAW40, LY_RAW41, LY_RAW50, LY_RAW51, LY_RAW4N, LY_F32, LY_F16, LY_BF16, // GGUF rows
    LY_NONE
};
__host__ __device__ static constexpr int lfamd_ly_tile(int ly) { // bytes of a tile; 0: GGUF rows
    return ly == LY_P4K || ly == LY_P40 || ly == LY_PX4 || ly == LY_P4N ? P4K_TILE
           : ly == LY_P5K                                ? P5K_TILE
           : ly == LY_P6K                                ? P6K_TILE
           : ly == LY_PK2                                ? PK2_TILE
           : ly == LY_PK3                                ? PK3_TILE
           : ly == LY_PCL41 || ly == LY_PCL50 || ly == LY_PCL51 ? PCL_TILE
           : ly == LY_P80                                ? P80_TILE
                                                         : 0;
}
struct lfamd_image {
    int ly;   // LY_NONE: an unknown id, or LFAMD_TYPE_PAD256 on a type that has no tile image to pad
    int type; // the id without the modifier
    long cols; // columns of the image: 256 * ceil(cols / 256) under LFAMD_TYPE_PAD256, else the row's
    int tile; // bytes of a tile (32 rows x 256 weights; P80: 8 rows x 4 blocks); 0: GGUF rows at lfamd_row_size(type, cols)
    bool tuned() const { // a layout only the tuned kernels read: the decode GEMVs take it, the generic kernels do not
        return tile != 0;
    }
    bool p40() const {
        return ly == LY_P40 || ly == LY_P4N;
    }
    bool pcl() const {
        return ly == LY_PCL41 || ly == LY_PCL50 || ly == LY_PCL51;
    }
    bool block32() const { // a legacy 32-block type (Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL), tiles or GGUF rows: activations in 32-blocks
        return p40() || pcl() || (ly >= LY_RAW40 && ly <= LY_RAW4N);
    }
    size_t tiles(long rows) const {
        return ly == LY_P80 ? (size_t)((rows + 7) / 8) * (size_t)((cols / 32 + 3) / 4) : (size_t)((rows + 31) / 32) * (size_t)(cols / 256);
    }
};
static inline int lfamd_base_type(int id) { // the id without the layout modifier
    return id & ~LFAMD_TYPE_PAD256;
}
// id: a public weight type id, with or without LFAMD_TYPE_PAD256.  The legacy 32-block types keep rows of whole 256-weight groups,
// and any row under the modifier, as tiles (the last super-block continued with zero blocks); their other rows stay GGUF rows.
static inline lfamd_image lfamd_image_of(int id, long cols) {
    static const struct {
        int type, ly, raw_ly; // raw_ly: the layout of rows that are not whole groups, LY_NONE = the type has whole groups only
    } tab[] = {
        {LFAMD_TYPE_Q4_K, LY_P4K, LY_NONE},    {LFAMD_TYPE_Q5_K, LY_P5K, LY_NONE},     {LFAMD_TYPE_Q6_K, LY_P6K, LY_NONE},
        {LFAMD_TYPE_Q2_K, LY_PK2, LY_NONE},    {LFAMD_TYPE_Q3_K, LY_PK3, LY_NONE},     {LFAMD_TYPE_IQ4_XS, LY_PX4, LY_NONE},
        {LFAMD_TYPE_Q8_0, LY_P80, LY_NONE},    {LFAMD_TYPE_Q4_0, LY_P40, LY_RAW40},    {LFAMD_TYPE_IQ4_NL, LY_P4N, LY_RAW4N},
        {LFAMD_TYPE_Q4_1, LY_PCL41, LY_RAW41}, {LFAMD_TYPE_Q5_0, LY_PCL50, LY_RAW50},  {LFAMD_TYPE_Q5_1, LY_PCL51, LY_RAW51},
        {LFAMD_TYPE_F32, LY_F32, LY_NONE},     {LFAMD_TYPE_F16, LY_F16, LY_NONE},      {LFAMD_TYPE_BF16, LY_BF16, LY_NONE},
    };
    const int type = lfamd_base_type(id);
    const bool pad = id != type;
    for (const auto &e : tab)
        if (e.type == type) {
            const bool whole = e.raw_ly == LY_NONE; // (no tile image to pad: the modifier makes an unknown id)
            const int ly = whole ? (pad ? (int)LY_NONE : e.ly) : (pad || cols % 256 == 0) ? e.ly : e.raw_ly;
            return {ly, type, whole || ly == e.raw_ly ? cols : (cols + 255) / 256 * 256, lfamd_ly_tile(ly)};
        }
    return {LY_NONE, type, cols, 0};
}
static inline bool lfamd_type_known(int id) { // (at every row length: cols only picks between a type's layouts)
    return lfamd_image_of(id, 0).ly != LY_NONE;
}
// the K cache types: what lfamd_mul_mat_batched_q reads as raw GGUF rows and lfamd_cpy writes (the 32-block types; an id with
// LFAMD_TYPE_PAD256 is not one).  The one definition of the list: cpy.hip and the ggml backend ask it too.
static inline bool lfamd_block_k_type(int id) {
    return id == LFAMD_TYPE_Q8_0 || id == LFAMD_TYPE_Q4_0 || id == LFAMD_TYPE_Q4_1 || id == LFAMD_TYPE_Q5_0 || id == LFAMD_TYPE_Q5_1 ||
           id == LFAMD_TYPE_IQ4_NL;
}

// A planned decode GEMV launch.  kind = the entry point that asks, variant = the kernel form it gets.
enum { LFAMD_GEMV_MULTI, LFAMD_GEMV_IDS, LFAMD_GEMV_IDS_PAIR, LFAMD_GEMV_DUAL, LFAMD_GEMV_MULTI_RELAXED }; // (_RELAXED: Q8_0 under LFAMD_FLAG_Q80_RELAXED)
enum {
    LFAMD_GEMV_PLAIN,       // gemv_kq_kernel
    LFAMD_GEMV_EARLY,       // ... one matrix, one column: first weight loads from the preloaded arguments
    LFAMD_GEMV_ROWS32,      // ... items of a whole 32-row tile (long walks of the types with a long dot)
    LFAMD_GEMV_EXPERT,      // ... expert picked on the device (MUL_MAT_ID)
    LFAMD_GEMV_EXPERT_PAIR, // gemv_kq_ids_pair_kernel: two experts, two activation rows, two sub-grids
    LFAMD_GEMV_TWO_TYPES,   // gemv_kq_dual_kernel: {Q4_K | Q5_K} and Q6_K matrices, two sub-grids
    LFAMD_GEMV_Q80,         // gemv_q80_kernel
    LFAMD_GEMV_Q80R         // gemv_q80r_kernel: Q8_0 with K split over the waves, this module's own summation order
};
struct lfamd_gemv_plan {
    int variant, nc, nw, ch; // columns, waves per work-group, super-blocks per chunk (Q8_0: ch = 0; Q80R: quads per chunk)
    int grid, grid_b;        // work-groups; grid_b: the second sub-grid of the two split launches, else 0
    int rows;                // result rows per item (16, ROWS32: 32; Q8_0: 8 per wave; Q80R: 8)
    int lds;                 // dynamic LDS bytes
};

// The launch form of a scaled-operand wide call that is not MUL_MAT_ID (gemm_wide.hip: wide_go switches on it).
enum {
    LFAMD_WIDE_KR,              // 256 x 128 tiles, the row-split body (gemm_kr.hip)
    LFAMD_WIDE_LW128,           // 128 x 128 tiles, the loader-wave body (gemm_lw.hip)
    LFAMD_WIDE_LW128_THEN_LW64, // the tail split: row blocks [0, rb_cut) as LW128, the rest as one round of 128 x 64 tiles
    LFAMD_WIDE_LW64,            // 128 x 64 tiles, the loader-wave body
    LFAMD_WIDE_KS,              // 128 x 64 tiles, the K-split-waves body (gemm_ks.hip)
    LFAMD_WIDE_LW64_KSPLIT      // 128 x 64 tiles with K cut into ksp parts over work-groups, then the reduce
};
struct lfamd_wide_plan {
    int form;
    int rb_cut; // LW128_THEN_LW64: the first row block of the 128 x 64 launch, else 0
    int ksp;    // LW64_KSPLIT: the parts of K (2, 4, 8), else 1
};

extern "C" {
void lfamd_set_error(const char *); // (api.hip: sets lfamd_last_error)
size_t lfamd_mul_mat_workspace_upto(int, long, long, long);
// weight images (pack.hip: every packer, expander and image size; dequant.hip: the read-back; blaslt.hip)
// (lfamd_launch_pack: the image of `im` from GGUF rows of `cols` weights; wprep16 / wprep8: the canonical per-call images, from GGUF
// rows, pk_expand / pk4x_expand: from the resident compact image)
hipError_t lfamd_launch_pack(const lfamd_image &, const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_scaled_ok(int, long, long, const void *, int *, hipStream_t);
size_t lfamd_wprep16_bytes(long, long);
hipError_t lfamd_launch_wprep16(int, const void *, size_t, long, long, void *, hipStream_t);
size_t lfamd_wprep8_bytes(long, long);
hipError_t lfamd_launch_wprep8(int, const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pk_expand(int, const void *, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pk4x_expand(const void *, long, long, void *, hipStream_t);
hipError_t lfamd_launch_q80_image(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_get_rows(const lfamd_image &, const void *, long, long, const int32_t *, long, long, int, void *, size_t, hipStream_t);
hipError_t lfamd_launch_unpack(const lfamd_image &, const void *, long, long, void *, size_t, hipStream_t);
// activation staging (prep.hip, quantize.hip, blaslt.hip)
hipError_t lfamd_launch_quantize(int, const float *, long, long, size_t, void *, size_t, hipStream_t);
hipError_t lfamd_launch_prep_q8k(const void *, size_t, long, long, long, void *, void *, void *, int, const int32_t *, hipStream_t);
hipError_t lfamd_launch_prep_f32(const void *, size_t, long, long, long, void *, void *, void *, int, const int32_t *, hipStream_t);
hipError_t lfamd_launch_prep80(int, const void *, size_t, long, long, long, void *, void *, void *, hipStream_t);
hipError_t lfamd_launch_prep_float(int, int, const void *, size_t, long, long, long, void *, hipStream_t);
hipError_t lfamd_launch_rows_to_16(int, const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_q80_rows_to_f16(int, const void *, size_t, long, long, void *, hipStream_t);
// decode GEMVs (gemv.hip, gemv_float.hip)
// (the three ints before the stream: Q0_VREGS32, PRECISE, and `relaxed` = Q8_0 may run the relaxed-order kernel where its plan accepts)
hipError_t lfamd_launch_gemv(int, const void *, long, long, int, const void *, size_t, long, float *, long, int, int, int, hipStream_t);
hipError_t lfamd_launch_gemv_multi(int, int, const void *const *, const long *, long, int, const void *, size_t, long, float *const *, const long *,
                                   int, int, int, hipStream_t);
hipError_t lfamd_launch_gemv_dual(int, int, const void *const *, const long *, float *const *, const long *, int, int, const void *const *,
                                  const long *, float *const *, const long *, long, int, const void *, size_t, hipStream_t);
hipError_t lfamd_launch_gemv_ids(int, int, const void *const *, long, int, const int32_t *, const int *, long, long, int, const void *, size_t,
                                 float *const *, hipStream_t);
hipError_t lfamd_launch_gemv_ids_pair(int, const void *, long, int, const int32_t *, int, int, long, long, int, const void *, const void *, size_t,
                                      float *, float *, hipStream_t);
// the decode GEMVs' launch plan (gemv.hip): pure host arithmetic, the CU count is an argument
int lfamd_num_cus(void); // of the current device, read once per process; 256 when no device answers
int lfamd_gemv_depth_ok(long);                    // one row's K-quant LDS image (k / 256 blocks of 384 bytes) fits in 150 KiB
int lfamd_gemv_cols_per_launch(int, long);        // (Atype, k): activation columns one launch takes, 0 = the row is too deep
size_t lfamd_gemv_lds_bytes(int, int, long, int, int); // (Atype, nc, k, nw, rows per item): the LDS layout's total
int lfamd_gemv_plan_of(int, int, int, long, long, long, int, int, struct lfamd_gemv_plan *);
int lfamd_gemv_has_kernel(int, int, const struct lfamd_gemv_plan *); // (Atype, f32in, plan): the type's unit instantiates it
int lfamd_gemv_q80_relaxed_cols(long); // (k): columns one launch of the relaxed-order Q8_0 kernel takes, 0 = it declines the row
size_t lfamd_gemv_q80_relaxed_lds_bytes(int, long); // (nc, k): that kernel's LDS layout's total
int lfamd_gemv_float_ok(int, long, long);
hipError_t lfamd_launch_gemv_float(int, const void *, long, long, int, const void *, size_t, long, float *, long, hipStream_t);
// batch bodies (gemm_*.hip, generic.hip)
bool lfamd_gemm_sb_ok(int, long, long);
size_t lfamd_gemm_sb_workspace(long);
hipError_t lfamd_launch_gemm_sb(int, const void *, long, long, int, const void *, size_t, long, float *, long, void *, int, hipStream_t);
int lfamd_gemm_i8_ok(int, long, long);
size_t lfamd_gemm_i8_workspace(long, long);
hipError_t lfamd_launch_gemm_i8(int, const void *const *, const long *, long, int, const void *, size_t, long, float *const *, const long *, void *,
                                const int32_t *, hipStream_t);
hipError_t lfamd_launch_gemm_i8_staged(int, const void *const *, const long *, long, const void *, long, float *const *, const long *, hipStream_t);
hipError_t lfamd_launch_gemm_kq(int, const void *, long, long, const void *, const void *, const void *, long, long, float *, long, hipStream_t);
// (the wide launchers take `mode`: bit 0 plain body, bit 1 activations staged scaled — gemm_wide.hip)
int lfamd_gemm_wide_scaled_ok(int, int);
int lfamd_gemm_wide_dual_ok(long, long, long);
// (Atype, count, m[], nb, n, n_pad, K-split workspace bytes or 0, plan out, parts out or NULL): pure host arithmetic, no device
int lfamd_gemm_wide_plan_of(int, int, const long *, int, long, long, size_t, struct lfamd_wide_plan *, long *);
size_t lfamd_gemm_lw_ksplit_bytes(long, long);
hipError_t lfamd_launch_gemm_wide(int, const void *, long, long, const void *, const void *, const void *, long, long, float *, long, int, void *,
                                  size_t, hipStream_t);
hipError_t lfamd_launch_gemm_wide_multi(int, int, const void *const *, const long *, long, const void *, const void *, const void *, long, long,
                                        float *const *, const long *, int, void *, size_t, hipStream_t);
hipError_t lfamd_launch_gemm_wide_dual(int, int, const void *const *, const long *, float *const *, const long *, int, int, const void *const *,
                                       const long *, float *const *, const long *, long, const void *, const void *, const void *, long, long, int,
                                       hipStream_t);
hipError_t lfamd_launch_gemm_wide_moe(int, const void *, long, int, long, long, const void *, const void *, const void *, long, const int *,
                                      const int *, const int *, int, float *, long, int, hipStream_t);
size_t lfamd_gemm_lf_workspace(long, long);
hipError_t lfamd_launch_gemm_lf_q80(int, const void *const *, const long *, long, int, const void *, size_t, long, float *const *, const long *,
                                    void *, hipStream_t);
hipError_t lfamd_launch_gemm_lf_q80_staged(int, const void *const *, const long *, long, const void *, long, float *const *, const long *, hipStream_t);
int lfamd_gemm_lf_q80_fits(long, long); // (m, k): the P80 image is below the 4 GiB the loaders address
hipError_t lfamd_launch_gemm_lf_float(int, const void *, size_t, long, long, const void *, long, long, float *, long, hipStream_t);
size_t lfamd_gemm_q80_workspace(long, long);
hipError_t lfamd_launch_gemm_q80(const void *, long, long, int, const void *, size_t, long, float *, long, void *, int, int, hipStream_t);
hipError_t lfamd_launch_generic(int, const void *, long, long, int, const void *, size_t, long, float *, long, hipStream_t);
// the vendor GEMM (blaslt.hip; LFAMD_USE_BLASLT=1)
bool lfamd_blaslt_ok();
size_t lfamd_blaslt_workspace();
hipError_t lfamd_blaslt_gemm(int, const void *, long, const void *, long, long, long, long, float *, long, void *, size_t, hipStream_t);
// MUL_MAT_ID (moe.hip)
size_t lfamd_moe_workspace(int, long, long, int, long, int);
bool lfamd_moe_decode_multi_ok(int, long, int, int, long, unsigned);
hipError_t lfamd_launch_moe(int, const void *, long, long, int, size_t, int, const void *, size_t, int, long, const int32_t *, int, float *, void *,
                            size_t, unsigned, hipStream_t);
hipError_t lfamd_launch_moe_decode_multi(int, int, const void *const *, long, long, int, size_t, int, const void *, size_t, long, const int32_t *,
                                         int, float *const *, hipStream_t);
}

// ---- staged activation images for k weights per row and n token rows (n_pad: n rounded up to 128): byte offsets and the total.
// Fused producers (norm_quant.hip) and the activation preps write them, the batch bodies read them: all take the offsets from here.
static inline size_t lfamd_up256(size_t v) {
    return (v + 255) / 256 * 256;
}

// The K-quant image (LFAMD_TYPE_STAGED_SCALED, and the staging of every K-quant batch body): Xh f16 [nb][n_pad][256], then d8T
// f32 [nb][n_pad], then Xm f16 [nb][n_pad][16], each starting on 256 bytes; a K-split launch keeps its partial tiles at `parts`.
struct lfamd_kq_image {
    size_t n_pad, d8T, Xm, parts;
};
static inline lfamd_kq_image lfamd_kq_image_of(long k, long n) {
    const size_t n_pad = ((size_t)n + 127) / 128 * 128, nb = (size_t)(k / 256), d8T = lfamd_up256(n_pad * (size_t)k * 2);
    const size_t Xm = d8T + lfamd_up256(nb * n_pad * 4);
    return {n_pad, d8T, Xm, Xm + lfamd_up256(n_pad * nb * 32)};
}

// The int8 body's image (LFAMD_TYPE_STAGED_Q8K): Xq int8 [nb][n_pad][256], then d8T f32 [nb][n_pad], then Xs f16 [nb][n_pad][16],
// packed without padding.
struct lfamd_i8_image {
    size_t n_pad, d8T, Xs, bytes;
};
static inline lfamd_i8_image lfamd_i8_image_of(long k, long n) {
    const size_t n_pad = ((size_t)n + 127) / 128 * 128, nb = (size_t)(k / 256), d8T = n_pad * nb * 256, Xs = d8T + n_pad * nb * 4;
    return {n_pad, d8T, Xs, Xs + n_pad * nb * 32};
}

// The 32-block image (Q8_0 / Q8_1-quantised activations of the PCL bodies): Xh f16 [nb][n_pad][256], then d8T f32 [nb * 8][n_pad],
// then sT f32 [nb * 8][n_pad], each starting on 256 bytes.
struct lfamd_b32_image {
    size_t n_pad, d8T, sT, bytes;
};
static inline lfamd_b32_image lfamd_b32_image_of(long k, long n) {
    const size_t n_pad = ((size_t)n + 127) / 128 * 128, nb = (size_t)(k / 256), d8T = lfamd_up256(n_pad * (size_t)k * 2);
    const size_t sT = d8T + lfamd_up256(nb * 8 * n_pad * 4);
    return {n_pad, d8T, sT, sT + lfamd_up256(nb * 8 * n_pad * 4)};
}

// The image of the Q8_0-weight loader-wave body (LFAMD_TYPE_STAGED_Q80, and what lfamd_launch_gemm_lf_q80 stages per call; gemm_lf.hip):
// Xh f16 [k / 128][n_pad][128], 256 bytes per token and quad in the chunk permutation of prep_lf_kernel, then stage f32 [n_pad], then
// tok_scale f32 [n_pad], packed without padding.
struct lfamd_q80_image {
    size_t n_pad, stage, tok_scale, bytes;
};
static inline lfamd_q80_image lfamd_q80_image_of(long k, long n) {
    const size_t n_pad = ((size_t)n + 127) / 128 * 128, stage = n_pad * (size_t)k * 2;
    return {n_pad, stage, stage + n_pad * 4, stage + n_pad * 8};
}
