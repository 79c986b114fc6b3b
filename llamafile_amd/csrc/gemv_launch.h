// gemv_launch.h — what the decode GEMV's dispatcher (gemv.hip) and its kernel units (gemv_<type>.hip) share: the by-value
// matrix tables of the kernels' arguments, the byte layout of their LDS, and the prototype of each unit's kernel lookup.
// No kernel text (gemv_common.h, gemv_impl.h, gemv_q80_impl.h, gemv_q80r_impl.h) and no launch policy (gemv.hip: lfamd_gemv_plan_of).
#pragma once
#include "../../include/lfamd_blocks.h"
#include "lfamd_internal.h"

// LDS image of one Q8_K activation block for the K-quant GEMVs.  A lane = (gsel, h) reads its 64 code
// bytes (two groups g = 2gsel+gi, four K-steps dd each) with four ds_read_b128, its 8 half-sums with
// one more, its 4 sub-block sums with a ds_read_b64.
//   [0,256)    codes: 8-byte groups at position pos = 16 gsel + 8 h + 4 gi + dd
//   [256,320)  hb  : int16 sum of each 8-byte group, same position order
//   [320,352)  ps  : int16 sum of K-step pairs (dd = 2e, 2e+1): position 8 gsel + 4 h + 2 gi + e
//   [352,384)  d   : f32 block scale (Q8_K: one; Q8_0-quantised activations for the legacy 32-block types: eight;
//                    Q8_1: eight dwords {f16 d, f16 s = d * sum(q)} like the block_q8_1 header)
#define XBLK 384
#define XBLK_HB 256
#define XBLK_PS 320
#define XBLK_D 352

// The K-quant GEMV's dynamic LDS for nc columns of nb super-blocks, nw waves and `rows` result rows per item: the activation
// image [nc][nb] XBLK, the two reduction buffers f32 [2][nw][nc][rows] at `red`, one dummy image block per wave at `dummy`
// (where a wave stages a block past the row's end).  The plan sizes the launch with it and both device bodies take their
// offsets from it.
struct kq_lds {
    size_t red, dummy, bytes;
};
constexpr kq_lds kq_lds_of(int nc, int nb, int nw, int rows) {
    const size_t red = (size_t)nc * nb * XBLK, dummy = red + 2 * (size_t)nw * nc * rows * sizeof(float);
    return {red, dummy, dummy + (size_t)nw * XBLK};
}

// LDS image of the Q8_0 activations, per QUAD of four 32-blocks (the unit a weight tile covers): for each of the
// eight dword positions j the four blocks' dwords side by side (a lane = (row r, position j) takes its four
// activation dwords with ONE ds_read_b128; the eight rows of a wave read the same 128 bytes: broadcast), then the
// four block scales as f32 (one more ds_read_b128, uniform).  8 ds_read_b32 per quad became 2 ds_read_b128.
#define X80_QUAD 144
#define X80_QD 128
#define Q80_WAVES 2 // waves per work-group (8 rows each) sharing one staged activation image
constexpr int q80_quads(long k) {
    return (int)((k / 32 + 3) / 4);
}
constexpr size_t q80_lds_bytes(int nc, int nquads) {
    return (size_t)nc * nquads * X80_QUAD;
}

// The relaxed-order Q8_0 GEMV (gemv_q80r_impl.h; LFAMD_FLAG_Q80_RELAXED): the same image [nc][nquads] X80_QUAD, then one quad of
// zeros at `dummy` (what a wave reads for a quad past the row's last), then the two reduction buffers f32 [2][nw][nc][8] at `red`.
// The plan sizes the launch with it and the kernel takes its offsets from it.
#define Q80R_WAVES 16 // waves per work-group: K is split over them
struct q80r_lds {
    size_t dummy, red, bytes;
};
constexpr q80r_lds q80r_lds_of(int nc, int nquads, int nw) {
    const size_t dummy = (size_t)nc * nquads * X80_QUAD, red = dummy + X80_QUAD;
    return {dummy, red, red + 2 * (size_t)nw * nc * 8 * sizeof(float)};
}
// quads of one wave that are in flight together (a chunk): the wave's share of the row up to 4, deeper rows in chunks of 4
constexpr int q80r_chunk_quads(int nquads) {
    const int qpw = (nquads + Q80R_WAVES - 1) / Q80R_WAVES;
    return qpw <= 1 ? 1 : qpw <= 2 ? 2 : 4;
}

// Up to GEMV_MAX_MATS weight matrices of one type and row length that consume the SAME activations
// (attn_q/k/v, ffn_gate/up) are served by one launch: their half-tiles are concatenated.
#define GEMV_MAX_MATS 4
struct gemv_mats {
    const uint8_t *A[GEMV_MAX_MATS];
    float *C[GEMV_MAX_MATS];
    long m[GEMV_MAX_MATS];
    long ldc[GEMV_MAX_MATS];
    int ht_end[GEMV_MAX_MATS]; // exclusive prefix of half-tile counts
    int count;
    // GGML_OP_MUL_MAT_ID at decode (IDS kernels only): matrix j is expert ids[id_idx[j]] of the stack at A[j]
    const int32_t *ids;
    long expert_bytes;
    int id_idx[GEMV_MAX_MATS];
    int experts;
};

// Q8_0: sibling matrices that share the activations (attn_q/k/v, ffn_gate/up) run as ONE launch over their concatenated
// 8-row groups: a 1024-row matrix alone is 128 waves, each a serial k-long chain — three such launches cost three times
// the chain latency, one launch costs it once.  The mnpack geometry (Kahan choice) stays per matrix.
struct q80_mats {
    const uint8_t *A[GEMV_MAX_MATS];
    float *C[GEMV_MAX_MATS];
    long m[GEMV_MAX_MATS];
    long ldc[GEMV_MAX_MATS];
    long rg_end[GEMV_MAX_MATS]; // exclusive prefix of row-group counts
    int count;
};

// The n = 1 launches of one to three matrices address their first item from preloaded kernel arguments (gemv_impl.h: kq_pre).
// The boundary in front of an absent matrix: a value no half-tile index reaches.
#define KQ_NO_BOUNDARY 0x7fffffff
// What the launcher asks a two-type unit for when the launch fits those arguments (<= 2 matrices of type A, one of type B): not a
// plan variant — the plan says LFAMD_GEMV_TWO_TYPES either way.  (One type: the unit's LFAMD_GEMV_EARLY kernels, which a PLAIN
// plan of two or three matrices runs on as well.)
#define KQ_TWO_TYPES_EARLY 0x100

// Each unit maps a planned launch to one of the kernels it instantiates: the kernel's address for hipLaunchKernel, nullptr
// for a form the unit does not hold.  (variant, nc, f32in, nw, ch); the two-type units: type A of the pair, Q6_K as type B.
typedef const void *gemv_kernel_fn(int variant, int nc, int f32in, int nw, int ch);
gemv_kernel_fn lfamd_gemv_kernel_q4k, lfamd_gemv_kernel_q5k, lfamd_gemv_kernel_q6k, lfamd_gemv_kernel_q40, lfamd_gemv_kernel_q41,
    lfamd_gemv_kernel_q50, lfamd_gemv_kernel_q51, lfamd_gemv_kernel_q2k, lfamd_gemv_kernel_q3k, lfamd_gemv_kernel_iq4xs, lfamd_gemv_kernel_iq4nl,
    lfamd_gemv_kernel_q4k_q6k, lfamd_gemv_kernel_q5k_q6k;
// Q8_0 (gemv_q80.hip: f32 activations, gemv_q80b.hip: Q8_0 blocks); mode = the summation form, see gemv_q80_kernel
const void *lfamd_gemv_kernel_q80_f32(int nc, int mode);
const void *lfamd_gemv_kernel_q80_q80(int nc, int mode);
// Q8_0, relaxed order (gemv_q80r.hip: f32 activations, gemv_q80rb.hip: Q8_0 blocks); (nc, nw, ch) of the plan
const void *lfamd_gemv_kernel_q80r_f32(int nc, int nw, int ch);
const void *lfamd_gemv_kernel_q80r_q80(int nc, int nw, int ch);
