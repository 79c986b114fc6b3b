// gemv_impl.h — wave-reduction GEMV kernels of the K-quant and 32-block types for the batch-1 (decode) case and small batches
// n <= 8: activation staging, per-type traits, kernels.  Launched from gemv.hip (the plan); the Q8_0 kernel: gemv_q80_impl.h.
//
// Replaces the reference's mul_mat_vec_q + quantize_q8_1 pair (ggml-cuda.cu.patch:14428-14575,
// 15259-15293: 32-wide warps, dp4a with a scalar fallback on gfx950) and follows the CPU
// path's arithmetic:
//   Q4_K / Q6_K x Q8_K : mul_mat_qX_K_q8_K_T (iqk_mul_mat.inc:601-643) — exact int8 block dots,
//                        f32 scales; the -32 offset of Q6_K is folded into a sums term like
//                        DequantizerQ6K does (iqk_mul_mat.inc:570-599).
//   Q8_0 x Q8_0        : tinyBLAS_Q0_AVX2::gemm (tinyblas_cpu.h:934-971) BIT-EXACT: 8 f32 lanes per
//                        output, blocks accumulated sequentially with fma (or Kahan), same hsum tree.
//
// Activations may arrive already quantised (the llamafile_sgemm boundary: Btype = Q8_K / Q8_0) or as
// f32 (the GGML_OP_MUL_MAT boundary): then every work-group quantises the (tiny) activation vector
// itself in its prologue, bit-identically to quantize_row_q8_K / q8_0, which removes one launch and
// one HBM round trip per mat-mul.
//
// These are HBM-bandwidth kernels: weights stream once from the packed layout with one
// global_load_dwordx4 per lane (1 KiB per wave instruction) straight into VGPRs — no LDS round
// trip for the weights (cdna_hip_programming.md §5 "GEMV / M <= 16" row).  The first chunk of
// weight loads is issued BEFORE the activation staging so HBM latency overlaps it, and the next
// chunk is always in flight while the current one is consumed.
#pragma once
#include "gemv_common.h"

// (the LDS image of one Q8_K activation block, XBLK, and the launch's LDS layout kq_lds_of: gemv_launch.h)

// Within every 8-byte group the codes (y0..y7) are stored as (y0,y4,y1,y5 | y2,y6,y3,y7): the order
// in which (x & 0x0F0F0F0F) and ((x>>4) & 0x0F0F0F0F) expose the nibbles of a packed K-step dword.
// grp = (k offset)/8 = 16 gsel + 8 gi + 2 dd + h.  Returns the group's code sum.
__device__ static inline int put_group(uint8_t *dst, int grp, uint32_t y0, uint32_t y1) {
    const uint32_t p0 = __builtin_amdgcn_perm(y1, y0, 0x05010400);
    const uint32_t p1 = __builtin_amdgcn_perm(y1, y0, 0x07030602);
    const int pos = (grp & 16) | ((grp & 1) << 3) | ((grp & 8) >> 1) | ((grp >> 1) & 3);
    *(uint2 *)(dst + 8 * pos) = make_uint2(p0, p1);
    int hs = sdot4(y0, 0x01010101u, 0);
    hs = sdot4(y1, 0x01010101u, hs);
    *(int16_t *)(dst + XBLK_HB + 2 * pos) = (int16_t)hs;
    return hs;
}

// pair sum of groups grp (dd even) and grp+2 (dd odd), written by the even one
__device__ static inline void put_pair(uint8_t *dst, int grp, int hs_even_plus_odd) {
    const int pp = ((grp & 16) >> 1) | ((grp & 1) << 2) | ((grp & 8) >> 2) | ((grp >> 2) & 1);
    *(int16_t *)(dst + XBLK_PS + 2 * pp) = (int16_t)hs_even_plus_odd;
}

// a group and, written by the lane of its even K-step, the pair sum with group grp ^ 2, which the lane two on holds (DPP: all
// lanes of the quad active).  Returns the pair sum.
__device__ static inline int put_group_pair(uint8_t *dst, int grp, uint32_t y0, uint32_t y1) {
    const int hs = put_group(dst, grp, y0, y1);
    const int pair = hs + (int)dpp_u32<DPP_XOR2>((uint32_t)hs);
    if ((grp & 2) == 0)
        put_pair(dst, grp, pair);
    return pair;
}

// already-quantised Q8_K rows (llamafile field order {d, bsums[16], qs[256]}); blockDim % 32 == 0
__device__ static inline void stage_q8k(uint8_t *lds, const uint8_t *B, size_t b_row_bytes, long col0, int nc, int nb) {
    const int groups = nc * nb * 32; // 8-byte groups; a block's 32 groups sit in 32 consecutive lanes
    for (int gidx = threadIdx.x; gidx < groups; gidx += blockDim.x) {
        int c = gidx / (nb * 32), r = gidx % (nb * 32);
        int b = r >> 5, grp = r & 31;
        const uint8_t *y = B + (col0 + c) * b_row_bytes + (size_t)b * 292;
        const uint32_t *src = (const uint32_t *)(y + 36 + 8 * grp);
        uint8_t *dst = lds + (size_t)(c * nb + b) * XBLK;
        const int hs = put_group(dst, grp, src[0], src[1]);
        const int other = __shfl_xor(hs, 2, 64); // group grp ^ 2: the other K-step of the pair
        if ((grp & 2) == 0)
            put_pair(dst, grp, hs + other);
        if (grp == 0)
            *(float *)(dst + XBLK_D) = *(const float *)y;
    }
}

// (pack_codes, the rounding and packing of the quantisers below: gemv_common.h)
// f32 rows, quantised here exactly like quantize_row_q8_K (upstream ggml-quants.c; restated in
// quantize.hip): first index of the largest |x| fixes the sign of iscale = -128/max, codes are
// nearest_int (round-half-even) clamped at 127, d = 1/iscale.  One "piece" = 16 consecutive floats;
// 16 consecutive lanes share one 256-block.
__device__ static inline void quantise_piece_q8k(uint8_t *dst, const float (&v)[16], int l16) {
    float amax = 0.0f, val = 0.0f;
    int idx = l16 * 16;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        float ax = fabsf(v[e]);
        if (ax > amax) {
            amax = ax;
            val = v[e];
            idx = l16 * 16 + e;
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        float oa = __shfl_xor(amax, off, 64);
        int oi = __shfl_xor(idx, off, 64);
        float ov = __shfl_xor(val, off, 64);
        if (oa > amax || (oa == amax && oi < idx)) {
            amax = oa;
            idx = oi;
            val = ov;
        }
    }
    uint32_t y[4] = {0, 0, 0, 0};
    float d = 0.0f;
    if (amax != 0.0f) {
        const float iscale = -128.0f / val;
        pack_codes<true>(y, v, iscale);
        d = 1.0f / iscale;
    }
    // this lane's 16 codes = groups 2*l16 (h = 0) and 2*l16+1 (h = 1) of K-step dd = l16 & 3
    const int hs0 = put_group(dst, 2 * l16 + 0, y[0], y[1]);
    const int hs1 = put_group(dst, 2 * l16 + 1, y[2], y[3]);
    const int o0 = __shfl_xor(hs0, 1, 64), o1 = __shfl_xor(hs1, 1, 64); // K-step dd ^ 1
    if ((l16 & 1) == 0) {
        put_pair(dst, 2 * l16 + 0, hs0 + o0);
        put_pair(dst, 2 * l16 + 1, hs1 + o1);
    }
    if (l16 == 0)
        *(float *)(dst + XBLK_D) = d;
}

__device__ static inline void stage_f32_as_q8k(uint8_t *lds, const uint8_t *X, size_t x_row_bytes, long col0, int nc,
                                               int nb) {
    const int pieces = nb * 16;
    const int l16 = threadIdx.x & 15;
    for (int c = 0; c < nc; c++) {
        const float *x = (const float *)(X + (col0 + c) * x_row_bytes);
        for (int p = threadIdx.x; p < pieces; p += blockDim.x) {
            float v[16];
            load_piece(v, x, p);
            quantise_piece_q8k(lds + (size_t)(c * nb + (p >> 4)) * XBLK, v, l16);
        }
    }
}

// scale slot `blk` (0..7) of a Q8_0 / Q8_1 activation image: Q8_0 keeps the f16-rounded d as f32; Q8_1 keeps {d, s} as
// the two f16 of block_q8_1, s = f16(d * sum) from the UNROUNDED d like upstream quantize_row_q8_1
template <bool S1>
__device__ static inline void put_scale_q80(uint8_t *dst, int blk, float d, int sum) {
    if constexpr (S1)
        *(uint32_t *)(dst + XBLK_D + 4 * blk) = (uint32_t)f2h_bits(d) | ((uint32_t)f2h_bits((float)sum * d) << 16);
    else
        *(float *)(dst + XBLK_D + 4 * blk) = h2f(f2h_bits(d));
}

// ---- activations of the legacy 32-block weight types (Q4_0 ...): Q8_0 quantisation (d = amax/127 per 32 values,
// stored as f16; q = roundf(x/d): upstream quantize_row_q8_0), same code / group-sum / pair-sum image, eight scales.
template <bool S1 = false>
__device__ static inline void quantise_piece_q80(uint8_t *dst, const float (&v)[16], int l16) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; e++)
        amax = fmaxf(amax, fabsf(v[e]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64)); // lanes 2b, 2b+1 hold the two halves of 32-block b
    const float d = amax / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t y[4] = {0, 0, 0, 0};
    pack_codes<false>(y, v, id);
    const int hs0 = put_group(dst, 2 * l16 + 0, y[0], y[1]);
    const int hs1 = put_group(dst, 2 * l16 + 1, y[2], y[3]);
    const int o0 = __shfl_xor(hs0, 1, 64), o1 = __shfl_xor(hs1, 1, 64);
    if ((l16 & 1) == 0) {
        put_pair(dst, 2 * l16 + 0, hs0 + o0);
        put_pair(dst, 2 * l16 + 1, hs1 + o1);
        put_scale_q80<S1>(dst, l16 >> 1, d, hs0 + o0 + hs1 + o1);
    }
}

// The rows of the 32-block types may end inside the last super-block (LFAMD_TYPE_PAD256: the weight image continues with all-zero
// blocks to a whole 256-weight group).  kb = the row's 32-blocks, nb = ceil(kb / 8).  TAIL (kb != 8 nb): nothing behind block kb is
// read — what lies there may be NaN, and NaN * 0 is not 0 — and the image's blocks from kb on are written as what a row of zeros
// gives: codes, group and pair sums, d and s all 0.  Whole rows run the TAIL = false code, which is the code from before the layout.
template <bool S1, bool TAIL>
__device__ static inline void stage_f32_as_q80_rows(uint8_t *lds, const uint8_t *X, size_t x_row_bytes, long col0, int nc, int nb, int kb) {
    const int pieces = nb * 16;
    const int l16 = threadIdx.x & 15;
    for (int c = 0; c < nc; c++) {
        const float *x = (const float *)(X + (col0 + c) * x_row_bytes);
        for (int p = threadIdx.x; p < pieces; p += blockDim.x) {
            float v[16];
            if (!TAIL || p < 2 * kb) { // (both pieces of a 32-block take the same side)
                load_piece(v, x, p);
            } else {
#pragma unroll
                for (int e = 0; e < 16; e++)
                    v[e] = 0.0f;
            }
            quantise_piece_q80<S1>(lds + (size_t)(c * nb + (p >> 4)) * XBLK, v, l16);
        }
    }
}

template <bool S1>
__device__ static inline void stage_f32_as_q80(uint8_t *lds, const uint8_t *X, size_t x_row_bytes, long col0, int nc, int nb, int kb) {
    if (kb == 8 * nb) // (uniform over the launch)
        stage_f32_as_q80_rows<S1, false>(lds, X, x_row_bytes, col0, nc, nb, kb);
    else
        stage_f32_as_q80_rows<S1, true>(lds, X, x_row_bytes, col0, nc, nb, kb);
}

// already-quantised Q8_0 (34-byte blocks) / Q8_1 (36-byte blocks {d, s, qs}) rows: one 8-byte group per lane, 32
// consecutive lanes per 256 codes
template <bool S1, bool TAIL>
__device__ static inline void stage_q80_blocks_rows(uint8_t *lds, const uint8_t *B, size_t b_row_bytes, long col0, int nc, int nb, int kb) {
    constexpr int BS = S1 ? 36 : 34, QS = S1 ? 4 : 2;
    const int groups = nc * nb * 32;
    for (int gidx = threadIdx.x; gidx < groups; gidx += blockDim.x) {
        int c = gidx / (nb * 32), r = gidx % (nb * 32);
        int b = r >> 5, grp = r & 31;
        const uint8_t *blk = B + (col0 + c) * b_row_bytes + (size_t)(b * 8 + (grp >> 2)) * BS;
        const bool in = !TAIL || b * 8 + (grp >> 2) < kb; // (the four groups of a 32-block take the same side)
        uint32_t y0 = 0, y1 = 0;
        if (in) {
            const uint16_t *src = (const uint16_t *)(blk + QS + 8 * (grp & 3));
            y0 = (uint32_t)src[0] | ((uint32_t)src[1] << 16), y1 = (uint32_t)src[2] | ((uint32_t)src[3] << 16);
        }
        uint8_t *dst = lds + (size_t)(c * nb + b) * XBLK;
        const int hs = put_group(dst, grp, y0, y1);
        const int other = __shfl_xor(hs, 2, 64);
        if ((grp & 2) == 0)
            put_pair(dst, grp, hs + other);
        if ((grp & 3) == 0) {
            if constexpr (S1)
                *(uint32_t *)(dst + XBLK_D + 4 * (grp >> 2)) = in ? (uint32_t)((const uint16_t *)blk)[0] | ((uint32_t)((const uint16_t *)blk)[1] << 16) : 0u;
            else
                *(float *)(dst + XBLK_D + 4 * (grp >> 2)) = in ? h2f(*(const uint16_t *)blk) : 0.0f;
        }
    }
}

template <bool S1>
__device__ static inline void stage_q80_blocks(uint8_t *lds, const uint8_t *B, size_t b_row_bytes, long col0, int nc, int nb, int kb) {
    if (kb == 8 * nb)
        stage_q80_blocks_rows<S1, false>(lds, B, b_row_bytes, col0, nc, nb, kb);
    else
        stage_q80_blocks_rows<S1, true>(lds, B, b_row_bytes, col0, nc, nb, kb);
}

// (kb: the row's 32-blocks, read by the 32-block formats only)
template <int BT, int ACT>
__device__ static inline void stage_x(uint8_t *lds, const uint8_t *B, size_t b_row_bytes, long col0, int nc, int nb, int kb) {
    if constexpr (ACT == LFAMD_TYPE_Q8_K) {
        if constexpr (BT == LFAMD_TYPE_F32)
            stage_f32_as_q8k(lds, B, b_row_bytes, col0, nc, nb);
        else
            stage_q8k(lds, B, b_row_bytes, col0, nc, nb);
    } else {
        if constexpr (BT == LFAMD_TYPE_F32)
            stage_f32_as_q80<ACT == LFAMD_TYPE_Q8_1>(lds, B, b_row_bytes, col0, nc, nb, kb);
        else
            stage_q80_blocks<ACT == LFAMD_TYPE_Q8_1>(lds, B, b_row_bytes, col0, nc, nb, kb);
    }
}

// ---------------------------------------------------------------------------------------------
// K-quant GEMV skeleton.  PERSISTENT work-groups: the grid is sized to about two work-groups per CU and
// each work-group walks half-tiles (16 weight rows) ht = blockIdx.x, +gridDim.x, ...  The activation
// vector is quantised / staged ONCE per work-group and reused for all its tiles, and the weight
// stream is software-pipelined across tiles: the loads of work item f+1 are issued before item f is
// consumed, so every wave keeps 12+ KiB of HBM reads in flight for its whole life.
//   work item = (tile, chunk of GEMV_CH super-blocks of this wave); wave w owns super-blocks w, w+NW, ...
//   NW = 16 waves for a single activation row: a k = 4096 row (16 super-blocks) then costs each wave ONE
//   super-block per tile, so the integer-dot phase that follows the arrival of the data is as short as it
//   can be; unused chunk slots are never touched, so the register allocator drops them.
//   lane = (i16 = lane&15, h = (lane>>4)&1, gsel = lane>>5) covers groups g = 2*gsel + gi (gi = 0,1).

#define GEMV_CH_MAX 4

// ---- What the traits' dots share (which sites use it, which kept their text and why).  The readers return small
// structs by value: the arrays are indexed with constants after unrolling and stay in registers.
// The reading side of a staged activation block (XBLK, XBLK_HB, XBLK_PS, XBLK_D: gemv_launch.h) for lane (gsel, h):
// its 16 code dwords: K-step t8 = 4 gi + dd of the lane is w[2 t8] (low nibbles' codes) and w[2 t8 + 1] (high nibbles')
struct kq_codes {
    uint32_t w[16];
};
__device__ static inline kq_codes kq_codes_of(const uint8_t *xb, int gsel, int h) {
    const uint4 *yq = (const uint4 *)(xb + 128 * gsel + 64 * h);
    const uint4 ya = yq[0], yb = yq[1], yc = yq[2], yd = yq[3];
    return {{ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w, yc.x, yc.y, yc.z, yc.w, yd.x, yd.y, yd.z, yd.w}};
}
// its four int16 pair sums: v[jj] = code sum of K-steps 2 jj, 2 jj + 1 (a 32-wide sub-block's half)
struct kq_sums4 {
    int v[4];
};
__device__ static inline kq_sums4 kq_pair_sums_of(const uint8_t *xb, int gsel, int h) {
    const uint2 psw = *(const uint2 *)(xb + XBLK_PS + 16 * gsel + 8 * h);
    return {{(int)(int16_t)(psw.x & 0xffff), (int)(int16_t)(psw.x >> 16), (int)(int16_t)(psw.y & 0xffff), (int)(int16_t)(psw.y >> 16)}};
}
// its eight int16 group sums as four dwords: w[p] = K-steps (2p, 2p + 1)
struct kq_words4 {
    uint32_t w[4];
};
__device__ static inline kq_words4 kq_group_sums_of(const uint8_t *xb, int gsel, int h) {
    const uint4 hbw = *(const uint4 *)(xb + XBLK_HB + 32 * gsel + 16 * h);
    return {{hbw.x, hbw.y, hbw.z, hbw.w}};
}

// the lane's eight code dwords of the nibble lattice, w[t8]: groups 2 gsel (q0) and 2 gsel + 1 (q1)
struct kq_words8 {
    uint32_t w[8];
};
__device__ static inline kq_words8 kq_words_of(const uint4 q0, const uint4 q1) {
    return {{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}};
}
// K-step t8 of a nibble dword against the staged codes, added to isum; LUT: the nibbles are kvalues_iq4nl indices (lfamd_device.h)
template <bool LUT = false>
__device__ static inline int kq_nib_dot(uint32_t x, const kq_codes &y, int t8, int isum) {
    if constexpr (LUT) {
        isum = sdot4(kvalues_lut4(x & 0x0F0F0F0Fu), y.w[2 * t8], isum);
        return sdot4(kvalues_lut4((x >> 4) & 0x0F0F0F0Fu), y.w[2 * t8 + 1], isum);
    } else {
        isum = sdot4(x & 0x0F0F0F0F, y.w[2 * t8], isum);
        return sdot4((x >> 4) & 0x0F0F0F0F, y.w[2 * t8 + 1], isum);
    }
}
// ... with a fifth bit per weight: Hd = the K-step's fifth-bit dword (P5K lattice) shifted down by dd = t8 & 3
__device__ static inline int kq_nib5_dot(uint32_t x, uint32_t Hd, const kq_codes &y, int t8, int isum) {
    const uint32_t c0 = (x & 0x0F0F0F0F) | (Hd & 0x10101010);
    const uint32_t c1 = ((x >> 4) & 0x0F0F0F0F) | ((Hd >> 4) & 0x00100010) | ((Hd << 12) & 0x10001000);
    isum = sdot4(c0, y.w[2 * t8], isum);
    return sdot4(c1, y.w[2 * t8 + 1], isum);
}
// f16 number jj of a uint2 of four (a row's block scales 4 gsel .. 4 gsel + 3); by reference: by value, the Q4_1 kernels change
__device__ static inline float kq_h4(const uint2 &hd, int jj) {
    const uint32_t dw = jj < 2 ? hd.x : hd.y;
    return h2f((uint16_t)((jj & 1) ? (dw >> 16) : (dw & 0xffff)));
}

struct q4k_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_K; // activation quantisation the reference uses for this type
    static constexpr int TILE = P4K_TILE;
    struct chunk {
        uint4 q0[GEMV_CH_MAX], q1[GEMV_CH_MAX], hd[GEMV_CH_MAX];
    };
    // `off` = byte offset of the super-block's tile inside the row-tile the descriptor covers
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.q0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
        ch.q1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
        ch.hd[s] = buf_ld16_nt(r, off + P4K_HDR + hrow * 16);
    }
    // one super-block of this lane against one staged activation block; returns the f32 contribution
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 q0 = ch.q0[s], q1 = ch.q1[s], hd = ch.hd[s];
        const float d = h2f((uint16_t)(hd.x & 0xffff)), dmin = h2f((uint16_t)(hd.x >> 16));
        uint32_t sc03, sc47, mn03, mn47;
        q4k_scales_bytes(hd.y, hd.z, hd.w, sc03, sc47, mn03, mn47);
        // this lane's four sub-blocks: j = 2g + e, g = 2*gsel + gi  ->  j = 4*gsel + 2*gi + e
        const uint32_t scw = gsel ? sc47 : sc03, mnw = gsel ? mn47 : mn03;
        const kq_words8 qw = kq_words_of(q0, q1);
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const kq_sums4 ps = kq_pair_sums_of(xb, gsel, h);
        int sumi = 0, summ = 0;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) { // jj = 2 gi + e
            int isum = 0;
#pragma unroll
            for (int d2 = 0; d2 < 2; d2++) {
                const int t8 = 2 * jj + d2; // = 4 gi + dd
                isum = kq_nib_dot(qw.w[t8], y, t8, isum);
            }
            sumi += (int)((scw >> (8 * jj)) & 0xff) * isum;
            summ += (int)((mnw >> (8 * jj)) & 0xff) * ps.v[jj];
        }
        const float d8 = *(const float *)(xb + XBLK_D);
        // d*d8*sumi - dmin*d8*summ  (iqk_mul_mat.inc:284-291, 632)
        return fmaf(d * d8, (float)sumi, -(dmin * d8) * (float)summ);
    }
};

// Q4_0 and IQ4_NL (legacy 32-blocks {f16 d, 16 nibble bytes}, activations Q8_0) on ONE resident image (P40): the P4K nibble
// image with eight f16 block scales per row as header.
//   Q4_0 (mul_mat_qX_0_q8_0_T, iqk_mul_mat.inc:998-1349): w = d*(q - 8).  Per 32-block: d*d8*(<q, q8> - 8*sum(q8)), the sum
//        taken from the staged pair sums like the Q4_K mins.
//   IQ4_NL (CODEBOOK): the nibbles are codebook indices (the lookup kvalues_lut4: lfamd_device.h).  Per 32-block:
//        (d * d8) * <kvalue[q], q8>; no offset, so the staged pair sums are not read.
struct p40_chunk {
    uint4 q0[GEMV_CH_MAX], q1[GEMV_CH_MAX];
    uint2 hd[GEMV_CH_MAX];
};
template <bool CODEBOOK>
struct p40_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_0;
    static constexpr int TILE = P4K_TILE;
    using chunk = p40_chunk;
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        if constexpr (CODEBOOK) { // (one inlining level more, as IQ4_NL always had: without it its address arithmetic comes out differently)
            p40_traits<false>::load(ch, s, r, off, gsel, slot, hrow);
        } else {
            ch.q0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
            ch.q1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
            ch.hd[s] = buf_ld8(r, off + P4K_HDR + hrow * 16 + gsel * 8); // scales of blocks 4 gsel .. 4 gsel + 3
        }
    }
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 q0 = ch.q0[s], q1 = ch.q1[s];
        const uint2 hd = ch.hd[s];
        const kq_words8 qw = kq_words_of(q0, q1);
        const kq_codes y = kq_codes_of(xb, gsel, h);
        kq_sums4 ps = {};
        if constexpr (!CODEBOOK)
            ps = kq_pair_sums_of(xb, gsel, h);
        const float4 d8 = *(const float4 *)(xb + XBLK_D + 16 * gsel);
        const float d8v[4] = {d8.x, d8.y, d8.z, d8.w};
        float acc = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) { // block 4 gsel + jj
            int isum = 0;
#pragma unroll
            for (int d2 = 0; d2 < 2; d2++) {
                const int t8 = 2 * jj + d2;
                isum = kq_nib_dot<CODEBOOK>(qw.w[t8], y, t8, isum);
            }
            acc = fmaf(kq_h4(hd, jj) * d8v[jj], (float)(isum - (CODEBOOK ? 0 : 8) * ps.v[jj]), acc);
        }
        return acc;
    }
};
// (derived, not aliases: the kernels' symbols keep the names q40_traits / iq4nl_traits)
struct q40_traits : p40_traits<false> {};
struct iq4nl_traits : p40_traits<true> {};

// Q5_K: Q4_K with a fifth bit per weight (DequantizerQ5K, iqk_mul_mat.inc:496-511): codes 0..31, same scales / mins.
struct q5k_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_K; // activation quantisation the reference uses for this type
    static constexpr int TILE = P5K_TILE;
    struct chunk {
        uint4 q0[GEMV_CH_MAX], q1[GEMV_CH_MAX], hd[GEMV_CH_MAX];
        uint2 hq[GEMV_CH_MAX];
    };
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.q0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
        ch.q1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
        ch.hd[s] = buf_ld16_nt(r, off + P5K_HDR + hrow * 16);
        ch.hq[s] = buf_ld8(r, off + P5K_QH + slot * 16 + gsel * 8); // fifth bits of groups 2 gsel, 2 gsel + 1
    }
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 q0 = ch.q0[s], q1 = ch.q1[s], hd = ch.hd[s];
        const uint32_t hw[2] = {ch.hq[s].x, ch.hq[s].y};
        const float d = h2f((uint16_t)(hd.x & 0xffff)), dmin = h2f((uint16_t)(hd.x >> 16));
        uint32_t sc03, sc47, mn03, mn47;
        q4k_scales_bytes(hd.y, hd.z, hd.w, sc03, sc47, mn03, mn47);
        const uint32_t scw = gsel ? sc47 : sc03, mnw = gsel ? mn47 : mn03;
        const kq_words8 qw = kq_words_of(q0, q1);
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const kq_sums4 ps = kq_pair_sums_of(xb, gsel, h);
        int sumi = 0, summ = 0;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) { // jj = 2 gi + e
            int isum = 0;
#pragma unroll
            for (int d2 = 0; d2 < 2; d2++) {
                const int t8 = 2 * jj + d2; // = 4 gi + dd
                isum = kq_nib5_dot(qw.w[t8], hw[t8 >> 2] >> (t8 & 3), y, t8, isum);
            }
            sumi += (int)((scw >> (8 * jj)) & 0xff) * isum;
            summ += (int)((mnw >> (8 * jj)) & 0xff) * ps.v[jj];
        }
        const float d8 = *(const float *)(xb + XBLK_D);
        return fmaf(d * d8, (float)sumi, -(dmin * d8) * (float)summ);
    }
};

// Q6_K: sub-blocks are 16 wide (one per K-step), codes are 6 bit, offset -32 handled as
// sum sc*(dot(code,q8) - 32*sum(q8)) like DequantizerQ6K (iqk_mul_mat.inc:570-599).
typedef short short2_t __attribute__((ext_vector_type(2)));
struct q6k_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_K; // activation quantisation the reference uses for this type
    static constexpr int TILE = P6K_TILE;
    struct chunk {
        uint4 l0[GEMV_CH_MAX], l1[GEMV_CH_MAX], hq[GEMV_CH_MAX];
        uint2 sc[GEMV_CH_MAX];
        uint32_t d[GEMV_CH_MAX];
    };
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.l0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
        ch.l1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
        ch.hq[s] = buf_ld16_nt(r, off + P6K_QH + gsel * 1024 + slot * 16);
        ch.sc[s] = buf_ld8(r, off + P6K_SC + hrow * 16 + gsel * 8); // scales of K-steps 8*gsel..+7
        ch.d[s] = buf_ld2(r, off + P6K_D + hrow * 2);
    }
    // Per lane: sumi = sum_t sc_t * <c_t, y_t> - 32 * sum_t sc_t * hs_t over its eight K-steps t (exact integers).
    //   codes: the two K-steps of a qh dword H share its bytes.  The fields of the lo bytes (j0,j4,j1,j5) sit at bits 4-5 /
    //   6-7 of H's bytes (even / odd K-step); those of the hi bytes (j2,j6,j3,j7) at bits 0-1 / 2-3 of H's bytes 1,0,3,2 —
    //   one v_perm per pair puts them in byte order, after which both halves are a shift and a mask away.
    //   offset term: once per super-block as four v_dot2_i32_i16 of the sign-extended scale pairs (two v_perm per four
    //   scales) against the staged int16 group sums, which already sit in pairs of K-steps.
    //   |<c_t, y_t>| <= 16 * 63 * 128 < 2^23, so sc_t * <c_t, y_t> is a 24-bit multiply.
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 l0 = ch.l0[s], l1 = ch.l1[s], hq = ch.hq[s];
        const uint2 scb = ch.sc[s];
        const float d = h2f((uint16_t)ch.d[s]);
        const kq_words8 lw = kq_words_of(l0, l1);
        const uint32_t hw[4] = {hq.x, hq.y, hq.z, hq.w}; // [gi*2 + e]
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const kq_words4 hbv = kq_group_sums_of(xb, gsel, h); // int16 group sums of K-steps (2p, 2p + 1)
        // int16 pairs (sc_2p, sc_2p+1): bytes (s, sign s, s', sign s') — v_perm selectors 8-11 copy the sign of bytes 1, 3,
        // 5, 7 of {a, b}, so b = scales << 8 puts s0 / s2 there and a = scales s1 / s3
        const uint32_t scw[2] = {scb.x, scb.y};
        int sums = 0;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t sh = scw[u] << 8;
            const uint32_t p01 = __builtin_amdgcn_perm(scw[u], sh, 0x0A050801), p23 = __builtin_amdgcn_perm(scw[u], sh, 0x0B070903);
            sums = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, p01), __builtin_bit_cast(short2_t, hbv.w[2 * u]), sums, false);
            sums = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, p23), __builtin_bit_cast(short2_t, hbv.w[2 * u + 1]), sums, false);
        }
        int sumi = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) { // K-steps t8 = 2p (even dd), 2p + 1 (odd dd)
            const uint32_t H = hw[p];
            const uint32_t P = __builtin_amdgcn_perm(H, H, 0x02030001); // bytes 1,0,3,2: hi-byte fields at bits 0-3
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int t8 = 2 * p + e;
                const uint32_t x = lw.w[t8];
                const uint32_t clo = (x & 0x0F0F0F0F) | ((e ? H >> 2 : H) & 0x30303030);
                const uint32_t chi = ((x >> 4) & 0x0F0F0F0F) | ((e ? P << 2 : P << 4) & 0x30303030);
                int isum = sdot4(clo, y.w[2 * t8], 0);
                isum = sdot4(chi, y.w[2 * t8 + 1], isum);
                const int sc = (int)(int8_t)((scw[t8 >> 2] >> (8 * (t8 & 3))) & 0xff);
                sumi += sc * ((int)((uint32_t)isum << 8) >> 8); // (an i24 operand: v_mul_i32_i24, the shifts fold away)
            }
        }
        sumi -= 32 * sums;
        const float d8 = *(const float *)(xb + XBLK_D);
        return (d * d8) * (float)sumi;
    }
};

// Q4_1 / Q5_0 / Q5_1 on the PCL image (rows of whole 256-weight groups): the P4K nibble lattice, eight f16 d and eight
// f16 m per row, fifth bits on the P5K lattice.  Per 32-block (iqk_mul_mat.inc:1241-1349, ggml_vec_dot_q5_0_q8_0):
//   Q5_0: d*d8*(<q5, q8> - 16*sum(q8))          Q4_1 / Q5_1: d*d8*<q, q8> + m*s,  s = the activation block's d8*sum(q8)
// A lane holds half of a block's weights (K-half h): the m*s term is added by the h = 0 lane.
template <int TYPE>
struct pcl_traits {
    static constexpr bool HAS_M = TYPE == LFAMD_TYPE_Q4_1 || TYPE == LFAMD_TYPE_Q5_1;
    static constexpr bool HAS_H = TYPE == LFAMD_TYPE_Q5_0 || TYPE == LFAMD_TYPE_Q5_1;
    static constexpr int ACT = HAS_M ? LFAMD_TYPE_Q8_1 : LFAMD_TYPE_Q8_0;
    static constexpr int TILE = PCL_TILE;
    struct chunk {
        uint4 q0[GEMV_CH_MAX], q1[GEMV_CH_MAX];
        uint2 hd[GEMV_CH_MAX], hm[GEMV_CH_MAX], hq[GEMV_CH_MAX];
    };
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.q0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
        ch.q1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
        ch.hd[s] = buf_ld8(r, off + PCL_D + hrow * 16 + gsel * 8); // scales of blocks 4 gsel .. 4 gsel + 3
        if constexpr (HAS_M)
            ch.hm[s] = buf_ld8(r, off + PCL_M + hrow * 16 + gsel * 8);
        if constexpr (HAS_H)
            ch.hq[s] = buf_ld8(r, off + PCL_QH + slot * 16 + gsel * 8); // fifth bits of groups 2 gsel, 2 gsel + 1
    }
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 q0 = ch.q0[s], q1 = ch.q1[s];
        const uint2 hd = ch.hd[s];
        const kq_words8 qw = kq_words_of(q0, q1);
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const uint4 dsw = *(const uint4 *)(xb + XBLK_D + 16 * gsel); // Q8_0: four f32 d8; Q8_1: four {f16 d8, f16 s}
        const uint32_t dsv[4] = {dsw.x, dsw.y, dsw.z, dsw.w};
        kq_sums4 ps = {};
        if constexpr (!HAS_M)
            ps = kq_pair_sums_of(xb, gsel, h);
        float acc = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) { // block 4 gsel + jj
            int isum = 0;
#pragma unroll
            for (int d2 = 0; d2 < 2; d2++) {
                const int t8 = 2 * jj + d2;
                // (written out: both codes before the fifth bits and the dots.  Through kq_nib_dot / kq_nib5_dot the same
                // operations reach the scheduler in another order and the Q4_1 / Q5_0 / Q5_1 kernels come out renamed)
                const uint32_t x = qw.w[t8];
                uint32_t c0 = x & 0x0F0F0F0F, c1 = (x >> 4) & 0x0F0F0F0F;
                if constexpr (HAS_H) {
                    const uint32_t Hd = (t8 < 4 ? ch.hq[s].x : ch.hq[s].y) >> (t8 & 3);
                    c0 |= Hd & 0x10101010;
                    c1 |= ((Hd >> 4) & 0x00100010) | ((Hd << 12) & 0x10001000);
                }
                isum = sdot4(c0, y.w[2 * t8], isum);
                isum = sdot4(c1, y.w[2 * t8 + 1], isum);
            }
            const float d = kq_h4(hd, jj);
            if constexpr (HAS_M) {
                const float m = kq_h4(ch.hm[s], jj);
                const float d8 = h2f((uint16_t)(dsv[jj] & 0xffff)), s8 = h2f((uint16_t)(dsv[jj] >> 16));
                acc = fmaf(d * d8, (float)isum, acc);
                acc = fmaf(m, h ? 0.0f : s8, acc);
            } else {
                acc = fmaf(d * __builtin_bit_cast(float, dsv[jj]), (float)(isum - 16 * ps.v[jj]), acc);
            }
        }
        return acc;
    }
};

// Q2_K / Q3_K on the RESIDENT compact images (lfamd_device.h: PK2 / PK3): half the bytes of the canonical image per row; two
// K-steps come out of one code dword with an AND and a shift-AND, Q3_K's third bit with a shift, an AND and a shift-OR.
// Per 16-wide sub-block: sc * (<q + OFF, y> - OFF * sum(y)) with the staged group sums; Q2_K's mins against the same sums
// (iqk_mul_mat.inc:432-470, 533-568).
template <int TYPE>
struct pk_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_K;
    static constexpr bool Q3 = TYPE == LFAMD_TYPE_Q3_K;
    static constexpr int TILE = Q3 ? PK3_TILE : PK2_TILE;
    static constexpr bool MINS = !Q3;
    static constexpr int OFF = Q3 ? 4 : 0;
    struct chunk {
        uint4 q[GEMV_CH_MAX];
        uint2 hb[GEMV_CH_MAX], sc[GEMV_CH_MAX];
        uint32_t dd[GEMV_CH_MAX];
    };
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.q[s] = buf_ld16_nt(r, off + gsel * 1024 + slot * 16);
        if constexpr (Q3)
            ch.hb[s] = buf_ld8(r, off + PK3_HB + gsel * 512 + slot * 8);
        ch.sc[s] = buf_ld8(r, off + (Q3 ? PK3_SC : PK2_SC) + hrow * 16 + gsel * 8); // scale bytes of K-steps 8*gsel..+7
        ch.dd[s] = __builtin_amdgcn_raw_buffer_load_b32(r, off + (Q3 ? PK3_D : PK2_D) + hrow * 4, 0, 0); // {d, dmin}
    }
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 qc = ch.q[s];
        const uint2 scb = ch.sc[s];
        const uint32_t dw = ch.dd[s];
        const float d = h2f((uint16_t)(dw & 0xffff));
        const uint32_t cw[4] = {qc.x, qc.y, qc.z, qc.w};
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const kq_words4 hbv = kq_group_sums_of(xb, gsel, h);
        int sumi = 0, summ = 0;
#pragma unroll
        for (int t8 = 0; t8 < 8; t8++) { // t8 = 4 gi + dd
            uint32_t x = ((t8 & 1) ? (cw[t8 >> 1] >> 2) : cw[t8 >> 1]) & 0x33333333u;
            if constexpr (Q3) {
                const uint32_t H = (t8 < 4 ? ch.hb[s].x : ch.hb[s].y) >> (t8 & 3);
                x |= (H & 0x11111111u) << 2;
            }
            const int isum = kq_nib_dot(x, y, t8, 0);
            const int hs = (int)(int16_t)((hbv.w[t8 >> 1] >> (16 * (t8 & 1))) & 0xffff);
            const uint32_t sbyte = ((t8 < 4 ? scb.x : scb.y) >> (8 * (t8 & 3))) & 0xff;
            if constexpr (Q3) {
                sumi += (int)(int8_t)sbyte * (isum - OFF * hs);
            } else {
                sumi += (int)(sbyte & 15) * isum;
                summ += (int)(sbyte >> 4) * hs;
            }
        }
        const float d8 = *(const float *)(xb + XBLK_D);
        if constexpr (MINS)
            return fmaf(d * d8, (float)sumi, -(h2f((uint16_t)(dw >> 16)) * d8) * (float)summ);
        return (d * d8) * (float)sumi;
    }
};

// IQ4_XS on the RESIDENT compact image (pack.hip: pack_tiles_kernel<LY_PX4>): codebook indices on the P4K nibble lattice, so a dword's
// nibbles already sit in the order of the staged activation codes; the 16-entry int8 codebook (kvalues_iq4nl,
// iqk_mul_mat.inc:601-628 looks it up with a byte shuffle too) is looked up by kvalues_lut4 (above, shared with IQ4_NL).
struct iq4c_traits {
    static constexpr int ACT = LFAMD_TYPE_Q8_K;
    static constexpr int TILE = P4K_TILE;
    struct chunk {
        uint4 q0[GEMV_CH_MAX], q1[GEMV_CH_MAX], hd[GEMV_CH_MAX];
    };
    __device__ static inline void load(chunk &ch, int s, lfamd_rsrc r, uint32_t off, int gsel, int slot, int hrow) {
        ch.q0[s] = buf_ld16_nt(r, off + (2 * gsel + 0) * 1024 + slot * 16);
        ch.q1[s] = buf_ld16_nt(r, off + (2 * gsel + 1) * 1024 + slot * 16);
        ch.hd[s] = buf_ld16(r, off + P4K_HDR + hrow * 16);
    }
    __device__ static inline float dot(const chunk &ch, int s, const uint8_t *xb, int gsel, int h) {
        const uint4 q0 = ch.q0[s], q1 = ch.q1[s], hd = ch.hd[s];
        const kq_words8 qw = kq_words_of(q0, q1);
        const kq_codes y = kq_codes_of(xb, gsel, h);
        const uint32_t scw = gsel ? hd.y : hd.x; // scales of sub-blocks 4 gsel .. 4 gsel + 3
        int sumi = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) { // sub-block 4 gsel + u = K-steps t8 = 2u, 2u + 1 of this lane
            int isum = 0;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                isum = kq_nib_dot<true>(qw.w[2 * u + e], y, 2 * u + e, isum);
            }
            sumi += (int)(int8_t)((scw >> (8 * u)) & 0xff) * isum;
        }
        const float d8 = *(const float *)(xb + XBLK_D);
        return (h2f((uint16_t)(hd.z & 0xffff)) * d8) * (float)sumi;
    }
};

// (gemv_mats, the by-value table of a launch's matrices: gemv_launch.h; the GEMV_DIAG stamps: gemv_common.h)

// ---------------------------------------------------------------------------------------------
// Decode body (ONE activation row).  What the stamps of the body above showed on 4096 x 4096 (tools/gemv_stamps.py):
// 0.8 us of dependent kernel-argument rounds before the first load, then 1.4 us in which four of the sixteen waves
// fetch the row as 64-byte-strided pieces (32 cache-line lookups per wave instruction — more L1 work than the whole
// weight stream of the CU), quantise it for everybody and release a work-group barrier.  Here instead:
//   * every kernel argument is read with static indices (one round of s_load, selects instead of indexed reads);
//   * wave w quantises exactly the super-blocks it will consume (w, w + NW, ...): one coalesced float4 per lane and
//     block (1 KiB per wave instruction), the block maximum by DPP, the LDS image written with one dword per lane;
//     a wave only ever reads image blocks it wrote itself (LDS operations of one wave execute in order), so there
//     is NO work-group barrier before the dots;
//   * the activation loads go out first and the weight loads right behind them (vmcnt retires in order);
//   * no integer division: tiles and chunks are walked with cursors.
// Arithmetic (per-lane dot, wave reduction, fixed-order sum over the waves) is the body above's: results are
// bit-identical.

// lane l holds codes y = (c[4l] .. c[4l+3]) of one 256-code block: write the code image, the group sums and the pair
// sums (layout: XBLK above).  Two lanes form an 8-code group.
__device__ static inline void put_codes_wave(uint8_t *dst, uint32_t y, int lane) {
    const int hf = lane & 1, grp = lane >> 1;
    const uint32_t other = dpp_u32<DPP_XOR1>(y);
    const uint32_t lo = hf ? other : y, hi = hf ? y : other;
    const uint32_t word = hf ? __builtin_amdgcn_perm(hi, lo, 0x07030602) : __builtin_amdgcn_perm(hi, lo, 0x05010400);
    const int pos = (grp & 16) | ((grp & 1) << 3) | ((grp & 8) >> 1) | ((grp >> 1) & 3);
    *(uint32_t *)(dst + 8 * pos + 4 * hf) = word;
    const int s4 = sdot4(y, 0x01010101u, 0);
    const int hs = s4 + (int)dpp_u32<DPP_XOR1>((uint32_t)s4);
    if (hf == 0)
        *(int16_t *)(dst + XBLK_HB + 2 * pos) = (int16_t)hs;
    const int hs2 = hs + (int)dpp_u32<DPP_ROW_SHL4>((uint32_t)hs); // group grp + 2 = lane + 4 (the pair's odd K-step)
    if ((lane & 5) == 0)
        put_pair(dst, grp, hs2);
}

// quantize_row_q8_K on one block held as a float4 per lane (element 4 lane + e): first index of the largest |x| gives
// the sign of iscale = -128/max; codes nearest_int (half-even) clamped at 127; d = 1/iscale.
__device__ static inline void stage_f32_q8k_wave(uint8_t *dst, const float4 v, int lane) {
    const float a0 = fabsf(v.x), a1 = fabsf(v.y), a2 = fabsf(v.z), a3 = fabsf(v.w);
    float am = fmaxf(fmaxf(a0, a1), fmaxf(a2, a3));
    am = fmaxf(am, dpp_f32<DPP_XOR1>(am));
    am = fmaxf(am, dpp_f32<DPP_XOR2>(am));
    am = fmaxf(am, dpp_f32<DPP_HALF_MIRROR>(am));
    am = fmaxf(am, dpp_f32<DPP_MIRROR>(am));
    const float amax = fmaxf(fmaxf(readlane_f32(am, 0), readlane_f32(am, 16)), fmaxf(readlane_f32(am, 32), readlane_f32(am, 48)));
    // (branch-free: an all-zero block goes through the same arithmetic with a harmless divisor and is zeroed by selects)
    const bool m0 = a0 == amax, m1 = a1 == amax, m2 = a2 == amax, m3 = a3 == amax;
    const unsigned long long ball = __builtin_amdgcn_ballot_w64(m0 || m1 || m2 || m3);
    const float cand = m0 ? v.x : (m1 ? v.y : (m2 ? v.z : v.w));
    const int first = ball ? __builtin_ctzll(ball) : 0;
    const bool nz = amax != 0.0f;
    const float val = nz ? readlane_f32(cand, first) : 1.0f;
    const float iscale = -128.0f / val;
    int q0 = (int)rintf(iscale * v.x), q1 = (int)rintf(iscale * v.y), q2 = (int)rintf(iscale * v.z), q3 = (int)rintf(iscale * v.w);
    q0 = q0 > 127 ? 127 : q0, q1 = q1 > 127 ? 127 : q1, q2 = q2 > 127 ? 127 : q2, q3 = q3 > 127 ? 127 : q3;
    uint32_t y = (uint32_t)(q0 & 0xff) | ((uint32_t)(q1 & 0xff) << 8) | ((uint32_t)(q2 & 0xff) << 16) | ((uint32_t)(q3 & 0xff) << 24);
    y = nz ? y : 0u;
    const float d = nz ? 1.0f / iscale : 0.0f;
    put_codes_wave(dst, y, lane);
    if (lane == 0)
        *(float *)(dst + XBLK_D) = d;
}

// quantize_row_q8_0 on eight 32-blocks held as a float4 per lane (8 lanes per block): d = amax/127 (stored as f16),
// q = roundf(x / d).
template <bool S1>
__device__ static inline void stage_f32_q80_wave(uint8_t *dst, const float4 v, int lane) {
    float am = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    am = fmaxf(am, dpp_f32<DPP_XOR1>(am));
    am = fmaxf(am, dpp_f32<DPP_XOR2>(am));
    am = fmaxf(am, dpp_f32<DPP_HALF_MIRROR>(am));
    const float d = am / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    const int q0 = (int)roundf(v.x * id), q1 = (int)roundf(v.y * id), q2 = (int)roundf(v.z * id), q3 = (int)roundf(v.w * id);
    const uint32_t y = (uint32_t)(q0 & 0xff) | ((uint32_t)(q1 & 0xff) << 8) | ((uint32_t)(q2 & 0xff) << 16) | ((uint32_t)(q3 & 0xff) << 24);
    put_codes_wave(dst, y, lane);
    int sum = 0;
    if constexpr (S1) { // the block's code sum over its eight lanes
        sum = sdot4(y, 0x01010101u, 0);
        sum += (int)dpp_u32<DPP_XOR1>((uint32_t)sum);
        sum += (int)dpp_u32<DPP_XOR2>((uint32_t)sum);
        sum += (int)dpp_u32<DPP_HALF_MIRROR>((uint32_t)sum);
    }
    if ((lane & 7) == 0)
        put_scale_q80<S1>(dst, lane >> 3, d, sum);
}

// Two blocks per pass (deep rows: a wave owns several super-blocks): lane l holds the EIGHT values 8 (l & 31) + e of
// block (l >> 5) — one whole 8-code group — so the fixed part of the quantiser (DPP maximum, the two IEEE divisions, the
// image addressing) is paid once per two blocks: ~70 VALU per block instead of ~120.  `dst` is this lane's block image.
__device__ static inline void stage_f32_q8k_wave2(uint8_t *dst, const float4 va, const float4 vb, int lane) {
    const float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; e++)
        a[e] = fabsf(v[e]);
    float am = fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7])));
    am = fmaxf(am, dpp_f32<DPP_XOR1>(am));
    am = fmaxf(am, dpp_f32<DPP_XOR2>(am));
    am = fmaxf(am, dpp_f32<DPP_HALF_MIRROR>(am));
    am = fmaxf(am, dpp_f32<DPP_MIRROR>(am));
    const bool hi = lane >= 32;
    const float amax_lo = fmaxf(readlane_f32(am, 0), readlane_f32(am, 16)), amax_hi = fmaxf(readlane_f32(am, 32), readlane_f32(am, 48));
    const float amax = hi ? amax_hi : amax_lo;
    bool any = false;
    float cand = v[7];
#pragma unroll
    for (int e = 7; e >= 0; e--) { // the FIRST element that reaches the maximum wins
        const bool me = a[e] == amax;
        cand = me ? v[e] : cand;
        any = any || me;
    }
    const unsigned long long ball = __builtin_amdgcn_ballot_w64(any);
    const uint32_t blo = (uint32_t)ball, bhi = (uint32_t)(ball >> 32);
    const int first_lo = blo ? __builtin_ctz(blo) : 0, first_hi = 32 + (bhi ? __builtin_ctz(bhi) : 0);
    const float val_lo = readlane_f32(cand, first_lo), val_hi = readlane_f32(cand, first_hi);
    const bool nz = amax != 0.0f;
    const float val = nz ? (hi ? val_hi : val_lo) : 1.0f;
    const float iscale = -128.0f / val;
    uint32_t y[2] = {0, 0};
    pack_codes<true>(y, v, iscale);
    const uint32_t y0 = nz ? y[0] : 0u, y1 = nz ? y[1] : 0u;
    const float d = nz ? 1.0f / iscale : 0.0f;
    const int grp = lane & 31;
    put_group_pair(dst, grp, y0, y1);
    if (grp == 0)
        *(float *)(dst + XBLK_D) = d;
}

template <bool S1>
__device__ static inline void stage_f32_q80_wave2(uint8_t *dst, const float4 va, const float4 vb, int lane) {
    const float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
    float am = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++)
        am = fmaxf(am, fabsf(v[e]));
    am = fmaxf(am, dpp_f32<DPP_XOR1>(am)); // four lanes per 32-block
    am = fmaxf(am, dpp_f32<DPP_XOR2>(am));
    const float d = am / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t y[2] = {0, 0};
    pack_codes<false>(y, v, id);
    const int grp = lane & 31;
    const int pair = put_group_pair(dst, grp, y[0], y[1]); // groups grp, grp ^ 2; with the neighbour pair: the four groups of the 32-block
    const int sum = pair + (int)dpp_u32<DPP_XOR1>((uint32_t)pair); // (all lanes active: a DPP source lane must be)
    if ((grp & 3) == 0)
        put_scale_q80<S1>(dst, grp >> 2, d, sum);
}

// one block of already-quantised activations, staged by one wave (lanes 0..31: one 8-code group each)
// TAIL (32-block formats, the row ends inside this super-block after kb 32-blocks): the blocks from kb on are not read and staged
// as zeros (stage_f32_as_q80_rows has the rule)
template <int ACT, bool TAIL = false>
__device__ static inline void stage_quantised_wave(uint8_t *dst, const uint8_t *row_generic, int b, int lane, int kb = 0) {
    // (explicitly GLOBAL: the pointer went through an SGPR pin and would otherwise be read with FLAT loads, which make
    // hipcc's wait counts conservative for the whole kernel — tests/test_isa_hazards.py)
    typedef const __attribute__((address_space(1))) uint8_t *gptr;
    const gptr row = (gptr)row_generic;
    if (lane < 32) {
        const int grp = lane;
        uint32_t y0, y1;
        if constexpr (ACT == LFAMD_TYPE_Q8_K) {
            const gptr y = row + (size_t)b * 292;
            const __attribute__((address_space(1))) uint32_t *src = (const __attribute__((address_space(1))) uint32_t *)(y + 36 + 8 * grp);
            y0 = src[0], y1 = src[1];
            if (grp == 0)
                *(float *)(dst + XBLK_D) = *(const __attribute__((address_space(1))) float *)y;
        } else {
            constexpr bool S1 = ACT == LFAMD_TYPE_Q8_1;
            const gptr blk = row + (size_t)(b * 8 + (grp >> 2)) * (S1 ? 36 : 34);
            const bool in = !TAIL || b * 8 + (grp >> 2) < kb;
            y0 = y1 = 0;
            if (in) {
                const __attribute__((address_space(1))) uint16_t *src = (const __attribute__((address_space(1))) uint16_t *)(blk + (S1 ? 4 : 2) + 8 * (grp & 3));
                y0 = (uint32_t)src[0] | ((uint32_t)src[1] << 16), y1 = (uint32_t)src[2] | ((uint32_t)src[3] << 16);
            }
            if ((grp & 3) == 0) {
                const __attribute__((address_space(1))) uint16_t *hdr = (const __attribute__((address_space(1))) uint16_t *)blk;
                if constexpr (S1)
                    *(uint32_t *)(dst + XBLK_D + 4 * (grp >> 2)) = in ? (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 16) : 0u;
                else
                    *(float *)(dst + XBLK_D + 4 * (grp >> 2)) = in ? h2f(hdr[0]) : 0.0f;
            }
        }
        put_group_pair(dst, grp, y0, y1);
    }
}

// a loaded uint4 as the four floats it holds
#define KQ_F4(u) make_float4(__builtin_bit_cast(float, (u).x), __builtin_bit_cast(float, (u).y), __builtin_bit_cast(float, (u).z), \
                           __builtin_bit_cast(float, (u).w))

// The kernels' `nb` argument.  Types on Q8_K activations: the row's super-blocks.  Types on 32-block activations (Q8_0 / Q8_1), whose
// rows may end inside the last super-block of a padded image (LFAMD_TYPE_PAD256): the row's 32-blocks kb, so nb = ceil(kb / 8) and
// a row of f32 activations is kb * 128 bytes long.  One argument either way: the early kernels' preloaded dwords stay 13.
template <typename TR>
__device__ __forceinline__ int kq_nb_of(int nbk) {
    if constexpr (TR::ACT == LFAMD_TYPE_Q8_K)
        return nbk;
    else
        return (nbk + 7) >> 3;
}
template <typename TR>
__device__ __forceinline__ uint32_t kq_row_bytes_f32(int nbk) {
    return (uint32_t)nbk * (TR::ACT == LFAMD_TYPE_Q8_K ? 1024u : 128u);
}

// The body of a GEMV work-group: work-group `bid` of `gdim` over the half-tiles of `mats` (the plain kernel passes its
// block index and grid size; the two-type kernel gives each type its own sub-grid).
template <typename TR, int NC, int BT, int NW, int GEMV_CH, bool IDS>
__device__ __forceinline__ void gemv_kq_body(const gemv_mats &mats, const int nbk, const uint8_t *__restrict__ B, size_t b_row_bytes,
                                             long col0, int n_ht, const int bid, const int gdim, uint8_t *lds) {
    const int nb = kq_nb_of<TR>(nbk), kb = nbk; // (kb: read by the 32-block types only)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, h = (lane >> 4) & 1, gsel = lane >> 5;
    const kq_lds lay = kq_lds_of(NC, nb, NW, 16);
    float *red = (float *)(lds + lay.red); // [2][NW][NC][16]
#if GEMV_DIAG
    int stamp_n = 0;
#endif
    GSTAMP();

    const int sb_per_wave = (nb + NW - 1) / NW;
    const int cpt = (sb_per_wave + GEMV_CH - 1) / GEMV_CH; // chunks per tile
    const int ntile = (n_ht - bid + gdim - 1) / gdim;
    const int total = ntile * cpt;

    // Loads are issued UNCONDITIONALLY through a bounds-checked buffer descriptor: a branch around a load
    // makes hipcc fall back to s_waitcnt vmcnt(0) (the prefetch of the next item is lost), whereas a
    // descriptor with zero records ("no item f") or an offset past the row-tile ("no super-block b")
    // returns zeros without touching memory and keeps the counted waits exact.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t rt_bytes = (uint32_t)nb * TR::TILE;
    // the matrix that half-tile `ht` of the launch belongs to
    auto mat_of = [&](long ht) __attribute__((always_inline)) {
        int j = 0;
#pragma unroll
        for (int jj = 1; jj < GEMV_MAX_MATS; jj++)
            if (jj < mats.count && ht >= mats.ht_end[jj - 1])
                j = jj;
        return j;
    };
    auto issue = [&](typename TR::chunk &ch, int f) {
        const int tile_i = f / cpt, chunk_i = f - tile_i * cpt;
        long ht = (long)bid + (long)tile_i * gdim;
        const int j = mat_of(ht);
        const uint8_t *A = mats.A[j];
        bool have = f < total;
        if constexpr (IDS) { // expert picked on the device: no routing-table read-back, graph-capturable
            const int ex = mats.ids[mats.id_idx[j]];
            const bool ok = ex >= 0 && ex < mats.experts;
            A += (size_t)(ok ? ex : 0) * mats.expert_bytes;
            have = have && ok;
        }
        if (j > 0)
            ht -= mats.ht_end[j - 1];
        const int hh = (int)(ht & 1);
        const lfamd_rsrc r = make_rsrc(A + (size_t)(ht >> 1) * rt_bytes, have ? rt_bytes : 0u);
        const int slot = h * 32 + hh * 16 + i16, hrow = hh * 16 + i16;
#pragma unroll
        for (int s = 0; s < GEMV_CH; s++) {
            const int b = wave_u + NW * (chunk_i * GEMV_CH + s); // b >= nb lands past the descriptor: zeros
            TR::load(ch, s, r, (uint32_t)b * TR::TILE, gsel, slot, hrow);
        }
    };

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[c] = 0.0f;

    auto consume = [&](const typename TR::chunk &ch, int f) {
        const int tile_i = f / cpt, chunk_i = f - tile_i * cpt;
#pragma unroll
        for (int s = 0; s < GEMV_CH; s++) {
            const int b = wave + NW * (chunk_i * GEMV_CH + s);
            const int bc = b < nb ? b : nb - 1;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                // a super-block beyond the row was loaded as zeros (d = 0): contributes exactly 0
                acc[c] += TR::dot(ch, s, lds + (size_t)(c * nb + bc) * XBLK, gsel, h);
            }
        }
        if (chunk_i == cpt - 1) { // tile finished: 4 lanes per row (h, gsel), then the waves through LDS
            float *rb = red + (tile_i & 1) * (NW * NC * 16);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float v = acc[c];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (lane < 16)
                    rb[(wave * NC + c) * 16 + lane] = v;
                acc[c] = 0.0f;
            }
            GSTAMP();
            __syncthreads();
            GSTAMP();
            if (threadIdx.x < 16 * NC) {
                const int c = threadIdx.x >> 4, i = threadIdx.x & 15;
                float v = 0.0f;
#pragma unroll
                for (int w = 0; w < NW; w++)
                    v += rb[(w * NC + c) * 16 + i];
                long ht = (long)bid + (long)tile_i * gdim;
                const int j = mat_of(ht);
                if (j > 0)
                    ht -= mats.ht_end[j - 1];
                const long row = (ht >> 1) * 32 + (ht & 1) * 16 + i;
                bool ok = true;
                if constexpr (IDS) { // an out-of-range expert id leaves its result row untouched (the host path skips it)
                    const int ex = mats.ids[mats.id_idx[j]];
                    ok = ex >= 0 && ex < mats.experts;
                }
                if (row < mats.m[j] && ok)
                    mats.C[j][(col0 + c) * mats.ldc[j] + row] = v;
            }
        }
    };

    typename TR::chunk bufA, bufB;
    if (total <= 0)
        return; // (whole work-group: total is uniform)
    // vmcnt retires in order: whatever is loaded first is waited for first.  In the decode case (one f32
    // row, at most one piece per thread) fetch the activations BEFORE the first weight chunk, so the
    // quantisation below only waits for them and the weights keep flying.
    if (BT == LFAMD_TYPE_F32 && NC == 1 && nb * 16 <= NW * 64) {
        float v[16];
        const bool mine = (int)threadIdx.x < nb * 16;
        if (mine)
            load_piece(v, (const float *)(B + col0 * b_row_bytes), threadIdx.x);
        issue(bufA, 0);
        GSTAMP();
        if (mine) {
            if constexpr (TR::ACT == LFAMD_TYPE_Q8_K)
                quantise_piece_q8k(lds + (size_t)(threadIdx.x >> 4) * XBLK, v, threadIdx.x & 15);
            else
                quantise_piece_q80<TR::ACT == LFAMD_TYPE_Q8_1>(lds + (size_t)(threadIdx.x >> 4) * XBLK, v, threadIdx.x & 15);
        }
        GSTAMP();
    } else if (BT == LFAMD_TYPE_F32 && GEMV_CH <= 2 && nb <= GEMV_CH * NW) {
        // several f32 rows, shallow: wave w quantises the blocks it consumes (w, w + NW) of every column from one
        // coalesced float4 per lane and block (the per-thread 64-byte pieces of stage_x cost 32 cache-line lookups per
        // wave instruction); the loads go out before the weights, blocks past the row arrive as zeros and land in the
        // wave's dummy slot
        uint4 xv[NC][GEMV_CH];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const lfamd_rsrc rx = make_rsrc(B + (col0 + c) * b_row_bytes, kq_row_bytes_f32<TR>(nbk)); // (past the row: zeros)
#pragma unroll
            for (int u = 0; u < GEMV_CH; u++)
                xv[c][u] = buf_ld16(rx, (uint32_t)(wave_u + NW * u) * 1024u + (uint32_t)lane * 16u);
        }
        __builtin_amdgcn_sched_barrier(0);
        issue(bufA, 0);
        __builtin_amdgcn_sched_barrier(0);
        // (= lds + lay.dummy + wave * XBLK, stepped from `red` in floats here and in gemv_kq_body1: with the byte form hipcc moves
        // the LDS base add of the f32 16 x 2 kernels across a scheduling barrier; this form keeps their code as it was)
        uint8_t *dummy = (uint8_t *)(red + (lay.dummy - lay.red) / sizeof(float)) + (size_t)wave * XBLK;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int u = 0; u < GEMV_CH; u++) {
                const int b = wave + NW * u;
                uint8_t *dst = b < nb ? lds + (size_t)(c * nb + b) * XBLK : dummy;
                const float4 v = KQ_F4(xv[c][u]);
                if constexpr (TR::ACT == LFAMD_TYPE_Q8_K)
                    stage_f32_q8k_wave(dst, v, lane);
                else
                    stage_f32_q80_wave<TR::ACT == LFAMD_TYPE_Q8_1>(dst, v, lane);
            }
    } else {
        issue(bufA, 0); // in flight during the staging below
        stage_x<BT, TR::ACT>(lds, B, b_row_bytes, col0, NC, nb, kb);
    }
    __syncthreads();
    GSTAMP();

    // (issuing bufB before the staging as well, and re-issuing each buffer right after its consume, measured
    // 10-25 % SLOWER on every decode shape: the counted waits degrade and the activation loads queue behind more
    // weight traffic)
    for (int f = 0; f < total; f += 2) {
        issue(bufB, f + 1);
        consume(bufA, f);
        GSTAMP();
        issue(bufA, f + 2);
        if (f + 1 < total)
            consume(bufB, f + 1);
    }
}


// the matrices of a launch as SSA values: every kernel argument is fetched in ONE round of scalar loads at the top of
// the kernel (the empty asm pins each value in SGPRs there: left alone, hipcc turns a select of two kernel arguments
// into a load from a selected ADDRESS — a second, dependent round trip of ~0.4 us before the first weight load and
// another one before the stores)
struct kq_tab {
    const uint8_t *A[GEMV_MAX_MATS];
    float *C[GEMV_MAX_MATS];
    long m[GEMV_MAX_MATS], ldc[GEMV_MAX_MATS];
    int e[GEMV_MAX_MATS];
    int idx[GEMV_MAX_MATS];
    int cnt;
};

__device__ __forceinline__ kq_tab kq_table(const gemv_mats &mats) {
    kq_tab t;
#pragma unroll
    for (int i = 0; i < GEMV_MAX_MATS; i++) {
        t.A[i] = mats.A[i], t.C[i] = mats.C[i], t.m[i] = mats.m[i], t.ldc[i] = mats.ldc[i], t.e[i] = mats.ht_end[i];
        t.idx[i] = mats.id_idx[i];
        asm volatile("" : "+s"(t.A[i]), "+s"(t.C[i]), "+s"(t.m[i]), "+s"(t.ldc[i]), "+s"(t.e[i]), "+s"(t.idx[i]));
    }
    t.cnt = mats.count;
    asm volatile("" : "+s"(t.cnt));
    return t;
}

struct kq_sel {
    const uint8_t *A;
    float *C;
    long m, ldc;
    int ht; // half-tile inside the matrix
    int idx; // id_idx of the matrix (IDS)
};

__device__ __forceinline__ kq_sel kq_pick(const kq_tab t, int ht) {
    const bool s1 = t.cnt > 1 && ht >= t.e[0], s2 = t.cnt > 2 && ht >= t.e[1], s3 = t.cnt > 3 && ht >= t.e[2];
    kq_sel r;
    r.A = s3 ? t.A[3] : (s2 ? t.A[2] : (s1 ? t.A[1] : t.A[0]));
    r.C = s3 ? t.C[3] : (s2 ? t.C[2] : (s1 ? t.C[1] : t.C[0]));
    r.m = s3 ? t.m[3] : (s2 ? t.m[2] : (s1 ? t.m[1] : t.m[0]));
    r.ldc = s3 ? t.ldc[3] : (s2 ? t.ldc[2] : (s1 ? t.ldc[1] : t.ldc[0]));
    r.idx = s3 ? t.idx[3] : (s2 ? t.idx[2] : (s1 ? t.idx[1] : t.idx[0]));
    r.ht = ht - (s3 ? t.e[2] : (s2 ? t.e[1] : (s1 ? t.e[0] : 0)));
    return r;
}

struct kq_cursor {
    int ht, chunk;
};

// loads are issued UNCONDITIONALLY through bounds-checked descriptors (zero records = nothing to fetch), see above
template <typename TR, int NW, int GEMV_CH, bool IDS>
__device__ __forceinline__ void kq_issue(typename TR::chunk &ch, const gemv_mats &mats, const kq_tab tab, const kq_cursor c, const int n_ht,
                                         const uint32_t rt_bytes, const int wave, const int i16, const int h, const int gsel) {
    const kq_sel p = kq_pick(tab, c.ht);
    const uint8_t *A = p.A;
    bool have = c.ht < n_ht;
    if constexpr (IDS) { // expert picked on the device: no routing-table read-back, graph-capturable
        const int ex = mats.ids[p.idx];
        const bool ok = ex >= 0 && ex < mats.experts;
        A += (size_t)(ok ? ex : 0) * mats.expert_bytes;
        have = have && ok;
    }
    const int hh = p.ht & 1;
    const lfamd_rsrc r = make_rsrc(A + (size_t)(p.ht >> 1) * rt_bytes, have ? rt_bytes : 0u);
    const int slot = h * 32 + hh * 16 + i16, hrow = hh * 16 + i16;
#pragma unroll
    for (int s = 0; s < GEMV_CH; s++) {
        const int b = wave + NW * (c.chunk * GEMV_CH + s); // b >= nb lands past the descriptor: zeros
        TR::load(ch, s, r, (uint32_t)b * TR::TILE, gsel, slot, hrow);
    }
}

// v[l] + v[l ^ 16] + v[l ^ 32] + v[l ^ 48] in every lane, with gfx950's row / half-wave swaps (two VALU instead of two
// ds_bpermute round trips through the LDS at the end of every tile)
__device__ static inline float kq_sum_rows(float v) {
    // (inline asm: with __builtin_amdgcn_permlane16_swap hipcc 7.2 loses the instruction's SECOND result in this kernel
    // and adds the first to itself — tests/test_golden.py caught it; s_nop 1 = the VALU-write -> permlane-read hazard)
    float x = v, y = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y)); // rows (r0,r0,r2,r2) and (r1,r1,r3,r3)
    float p = x + y, q;
    q = p;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(p), "+v"(q)); // halves (lo,lo) and (hi,hi)
    return p + q;
}

// What the EARLY kernels know of their first item without the table, all of it in PRELOADED arguments: the weights of up to
// three matrices and the two half-tile boundaries between them.  The host sets the boundary in front of an absent matrix to
// KQ_NO_BOUNDARY, which no half-tile reaches, so the pick needs no count (gemv.hip: launch_kq_early).
struct kq_pre {
    const uint8_t *A0, *A1, *A2;
    int e0, e1;
};

template <typename TR, int BT, int NW, int GEMV_CH, bool IDS, bool EARLY = false, bool PAIR = false>
__device__ __forceinline__ void gemv_kq_body1(const gemv_mats &mats, int nbk, const uint8_t *__restrict__ B,
                                              size_t b_row_bytes, long col0, int n_ht, const int bid, int gdim,
                                              uint8_t *lds, const kq_pre pre) {
    // (EARLY: B is the activation row itself, b_row_bytes and col0 are the literal 0 and fold away)
    if constexpr (EARLY)
        asm volatile("" : "+s"(nbk), "+s"(B), "+s"(n_ht), "+s"(gdim));
    else
        asm volatile("" : "+s"(nbk), "+s"(B), "+s"(b_row_bytes), "+s"(col0), "+s"(n_ht), "+s"(gdim)); // (one s_load round)
    const int nb = kq_nb_of<TR>(nbk), kb = nbk; // (kb: read by the 32-block types only)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i16 = lane & 15, h = (lane >> 4) & 1, gsel = lane >> 5;
    constexpr int RW = PAIR ? 32 : 16; // result rows per item: a half-tile, or (PAIR) both half-tiles of a 32-row tile
    const kq_lds lay = kq_lds_of(1, nb, NW, RW);
    float *red = (float *)(lds + lay.red); // [2][NW][RW]
#if GEMV_DIAG
    int stamp_n = 0;
    unsigned long long gwg_clk0 = 0;
#endif
    GWG(0);
    GSTAMP();
    // the activation loads need only the leading (preloaded) kernel arguments: they go out before the rest of the
    // arguments has even arrived (-amdgpu-kernarg-preload-count, Makefile)
    // GEMV_CH == 1 (launched for nb <= NW only): ONE block per wave, a float4 per lane.  Deeper rows: FOUR blocks per
    // group as two passes of two (lane l: eight values of block (l >> 5) of the pass), four loads per lane.
    constexpr int JX = GEMV_CH == 1 ? 1 : (NW == 8 ? 2 : 4);
    const uint8_t *xrow = B + col0 * b_row_bytes;
    const lfamd_rsrc rx = make_rsrc(xrow, kq_row_bytes_f32<TR>(nbk)); // (a load past the row returns zeros: a padded tail stages as zeros)
    uint4 xv[JX];
    auto x_off = [&](int j0, int j) __attribute__((always_inline)) { // byte offset of load j of the group starting at block slot j0
        if constexpr (JX == 1)
            return (uint32_t)(wave + NW * j0) * 1024u + (uint32_t)lane * 16u;
        else
            return (uint32_t)(wave + NW * (j0 + 2 * (j >> 1) + (lane >> 5))) * 1024u + (uint32_t)(lane & 31) * 32u + 16u * (j & 1);
    };
    if constexpr (BT == LFAMD_TYPE_F32) {
#pragma unroll
        for (int j = 0; j < JX; j++)
            xv[j] = buf_ld16(rx, x_off(0, j));
        __builtin_amdgcn_sched_barrier(0); // (the scheduler would put the weight loads first)
    }
    // pre-quantised Q8_K rows, one block per wave: the block's codes (8 bytes per lane of the lower half-wave) and its scale
    // are fetched here too, ahead of the weights
    // (two blocks per wave in the 8-wave form: the upper half-wave fetches block wave + NW)
    constexpr bool PRE1 = BT == LFAMD_TYPE_Q8_K && TR::ACT == LFAMD_TYPE_Q8_K && JX <= 2;
    uint2 pq = make_uint2(0, 0);
    uint32_t pd = 0;
    const int pre_b = JX == 1 ? wave : wave + NW * (lane >> 5);
    if constexpr (PRE1) {
        const lfamd_rsrc rq = make_rsrc(xrow, (uint32_t)nb * 292u);
        pq = buf_ld8(rq, (uint32_t)pre_b * 292u + 36u + (uint32_t)(lane & 31) * 8u);
        pd = __builtin_amdgcn_raw_buffer_load_b32(rq, (uint32_t)pre_b * 292u, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    // a launch of up to three matrices (attn_output, ffn_down; attn_q/k/v, ffn_gate + ffn_up) knows its weights and the
    // boundaries between them from the preloaded arguments: its first item goes out BEFORE the argument table's scalar
    // loads have returned (~0.4 us earlier); both branches issue the same loads
    typename TR::chunk bufA, bufB;
    typename TR::chunk bufA2, bufB2; // (PAIR: the second half-tile of the item; dead otherwise)
    static_assert(!(PAIR && (EARLY || IDS)), "the paired item is a variant of the plain launch");
    constexpr bool early = EARLY && !IDS; // (a kernel variant, not a run-time branch: hipcc merges its wait counts at a join)
    // Tiles whose size is not a multiple of the 128-byte cache line (P6K: 6720 B) start 64 B into a line every other
    // super-block: then every 256-byte run of a half-tile has its edge lines in common with the other half-tile of the
    // tile, and both halves' d sit in one line.  Fetched by two work-groups on two XCDs, such a line crosses the fabric
    // twice (Q6_K 4096 x 14336: 61.3 MB fetched for a 48.2 MB matrix).  Work-groups b and b + 8 share an XCD (blocks are
    // dealt round-robin over the eight), so in every run of 16 items, items q and q + 8 take the two halves of one tile and
    // the shared lines are fetched into one L2.  A bijection of [0, n_ht): the items past the last full run keep their
    // order.  Which rows a work-group computes changes, not how: same bits.
    constexpr bool XPAIR = !PAIR && TR::TILE % 128 != 0;
    auto ht_of = [&](int q) __attribute__((always_inline)) {
        return (XPAIR && q < (n_ht & ~15)) ? ((q & ~15) | ((q & 7) << 1) | ((q >> 3) & 1)) : q;
    };
    if constexpr (early) {
        const int hb = ht_of(bid);
        const bool s1 = hb >= pre.e0, s2 = hb >= pre.e1; // (kq_pick's choice, from SGPRs the hardware filled)
        const uint8_t *Ap = s2 ? pre.A2 : (s1 ? pre.A1 : pre.A0);
        const int hl = hb - (s2 ? pre.e1 : (s1 ? pre.e0 : 0)); // half-tile inside the matrix
        const int hh = hl & 1;
        const uint32_t rtb = (uint32_t)nb * TR::TILE;
        const lfamd_rsrc r = make_rsrc(Ap + (size_t)(hl >> 1) * rtb, hb < n_ht ? rtb : 0u);
#pragma unroll
        for (int s = 0; s < GEMV_CH; s++)
            TR::load(bufA, s, r, (uint32_t)(wave + NW * s) * TR::TILE, gsel, h * 32 + hh * 16 + i16, hh * 16 + i16);
        // (left alone, the scheduler lets the table's s_waitcnt lgkmcnt(0) in between these loads: the 16 x 1 form's header load,
        // which the dot needs first, then waited for the table after all)
        __builtin_amdgcn_sched_barrier(0);
        GSTAMP(); // (the second stamp of a wave = its first weight loads are out, here as behind KQ_ISSUE below: tools/gemv_stamps.py --fused)
    }
    const kq_tab tab = kq_table(mats);

    const int sb_per_wave = (nb + NW - 1) / NW;
    const int cpt = (sb_per_wave + GEMV_CH - 1) / GEMV_CH; // chunks per tile
    const uint32_t rt_bytes = (uint32_t)nb * TR::TILE;

    float acc = 0.0f, acc2 = 0.0f;
    int par = 0;
    constexpr int HT_STEP = PAIR ? 2 : 1; // (PAIR: a cursor points at the even half-tile of its tile)
    kq_cursor ci{HT_STEP * bid, 0}, cc{HT_STEP * bid, 0};
#define KQ_ADVANCE(c)                                                                                                  \
    do {                                                                                                               \
        if (++(c).chunk == cpt)                                                                                        \
            (c).chunk = 0, (c).ht += HT_STEP * gdim;                                                                   \
    } while (0)
    // (measured and rejected: s_setprio 3 around the load issue, and a work-group barrier between every wave's activation
    // loads and the first weight loads — the youngest waves of a k = 14336 row still issue 1.5-3 us after the oldest, the
    // CU's vector-memory queue is simply full — both 2-7 % slower on every decode shape)
#define KQ_ISSUE(buf)                                                                                                  \
    do {                                                                                                               \
        kq_issue<TR, NW, GEMV_CH, IDS>(buf, mats, tab, kq_cursor{ht_of(ci.ht), ci.chunk}, n_ht, rt_bytes, wave, i16, h, gsel); \
        if constexpr (PAIR) {                                                                                          \
            const kq_cursor c2{ci.ht + 1, ci.chunk};                                                                   \
            kq_issue<TR, NW, GEMV_CH, IDS>(buf##2, mats, tab, c2, n_ht, rt_bytes, wave, i16, h, gsel);                 \
        }                                                                                                              \
        KQ_ADVANCE(ci);                                                                                                \
    } while (0)
    // one chunk of this wave against its own image blocks; at the end of a tile: 4 lanes per row (h, gsel), then the
    // waves through LDS in a fixed order
#define KQ_CONSUME(buf)                                                                                                \
    do {                                                                                                               \
        GSTAMP_ARRIVAL();                                                                                              \
        _Pragma("unroll") for (int s = 0; s < GEMV_CH; s++) {                                                          \
            const int b = wave + NW * (cc.chunk * GEMV_CH + s);                                                        \
            /* a super-block beyond the row was loaded as zeros and its image slot belongs to nobody: no dot (b is   \
               wave-uniform, a scalar branch; the loads stay unconditional, see kq_issue).  acc is never -0, so       \
               skipping an addend of zero changes no bit */                                                            \
            if (b < nb) {                                                                                              \
                acc += TR::dot(buf, s, lds + (size_t)b * XBLK, gsel, h);                                               \
                if constexpr (PAIR)                                                                                    \
                    acc2 += TR::dot(buf##2, s, lds + (size_t)b * XBLK, gsel, h);                                       \
            }                                                                                                          \
        }                                                                                                              \
        if (cc.chunk == cpt - 1) {                                                                                     \
            float *rb = red + par * (NW * RW);                                                                         \
            par ^= 1;                                                                                                  \
            float v = kq_sum_rows(acc); /* lanes i16, i16 + 16, i16 + 32, i16 + 48 */                                  \
            if (lane < 16)                                                                                             \
                rb[wave * RW + lane] = v;                                                                              \
            acc = 0.0f;                                                                                                \
            if constexpr (PAIR) {                                                                                      \
                float v2 = kq_sum_rows(acc2);                                                                          \
                if (lane < 16)                                                                                         \
                    rb[wave * RW + 16 + lane] = v2;                                                                    \
                acc2 = 0.0f;                                                                                           \
            }                                                                                                          \
            GSTAMP();                                                                                                  \
            __syncthreads();                                                                                           \
            GSTAMP();                                                                                                  \
            if (threadIdx.x < RW) {                                                                                    \
                const int i = threadIdx.x;                                                                             \
                float t = 0.0f;                                                                                        \
                _Pragma("unroll") for (int w = 0; w < NW; w++) t += rb[w * RW + i];                                    \
                const kq_sel p = kq_pick(tab, ht_of(cc.ht));                                                           \
                const long row = (long)(p.ht >> 1) * 32 + (p.ht & 1) * 16 + i; /* (PAIR: p.ht even, i < 32) */         \
                bool ok = true;                                                                                        \
                if constexpr (IDS) { /* an out-of-range expert id leaves its result row untouched */                   \
                    const int ex = mats.ids[p.idx];                                                                    \
                    ok = ex >= 0 && ex < mats.experts;                                                                 \
                }                                                                                                      \
                if (row < p.m && ok)                                                                                   \
                    ((__attribute__((address_space(1))) float *)p.C)[col0 * p.ldc + row] = t; /* (not FLAT) */                                                                     \
            }                                                                                                          \
        }                                                                                                              \
        KQ_ADVANCE(cc);                                                                                                \
    } while (0)

    if constexpr (BT == LFAMD_TYPE_F32) {
        // this wave's blocks, JX at a time; the first JX went out BEFORE the first weight chunk (in-order vmcnt).  The
        // staging is straight-line code (a block past the row is loaded as zeros through the descriptor and staged
        // into the wave's dummy slot): with a branch per block hipcc merges its vmcnt bookkeeping at the joins and
        // makes the second block wait for the WEIGHTS.
        uint8_t *dummy = (uint8_t *)(red + (lay.dummy - lay.red) / sizeof(float)) + (size_t)wave * XBLK;
        if constexpr (early)
            KQ_ADVANCE(ci);
        else
            KQ_ISSUE(bufA);
        __builtin_amdgcn_sched_barrier(0);
        GSTAMP();
#define KQ_STAGE_GROUP(j0)                                                                                             \
    if constexpr (JX == 1) {                                                                                           \
        const int b = wave + NW * (j0);                                                                                \
        uint8_t *dst = b < nb ? lds + (size_t)b * XBLK : dummy;                                                        \
        if constexpr (TR::ACT == LFAMD_TYPE_Q8_K)                                                                      \
            stage_f32_q8k_wave(dst, KQ_F4(xv[0]), lane);                                                               \
        else                                                                                                           \
            stage_f32_q80_wave<TR::ACT == LFAMD_TYPE_Q8_1>(dst, KQ_F4(xv[0]), lane);                                   \
    } else {                                                                                                           \
        _Pragma("unroll") for (int ps = 0; ps < JX / 2; ps++) {                                                        \
            const int b = wave + NW * ((j0) + 2 * ps + (lane >> 5));                                                   \
            uint8_t *dst = b < nb ? lds + (size_t)b * XBLK : dummy;                                                    \
            if constexpr (TR::ACT == LFAMD_TYPE_Q8_K)                                                                  \
                stage_f32_q8k_wave2(dst, KQ_F4(xv[2 * ps]), KQ_F4(xv[2 * ps + 1]), lane);                              \
            else                                                                                                       \
                stage_f32_q80_wave2<TR::ACT == LFAMD_TYPE_Q8_1>(dst, KQ_F4(xv[2 * ps]), KQ_F4(xv[2 * ps + 1]), lane);  \
        }                                                                                                              \
    }
        KQ_STAGE_GROUP(0) // (peeled: inside the loop below the back edge would hide the weight loads from the wait counts)
        for (int j0 = JX; j0 < sb_per_wave; j0 += JX) { // rows longer than JX * NW super-blocks
#pragma unroll
            for (int j = 0; j < JX; j++)
                xv[j] = buf_ld16(rx, x_off(j0, j));
            KQ_STAGE_GROUP(j0)
        }
#undef KQ_STAGE_GROUP
    } else {
        if constexpr (early)
            KQ_ADVANCE(ci);
        else
            KQ_ISSUE(bufA);
        GSTAMP();
        if constexpr (PRE1 && JX == 1) {
            if (wave < nb && lane < 32) {
                uint8_t *dst = lds + (size_t)wave * XBLK;
                put_group_pair(dst, lane, pq.x, pq.y);
                if (lane == 0)
                    *(uint32_t *)(dst + XBLK_D) = pd;
            }
        } else if constexpr (PRE1) {
            { // both half-waves, straight-line (a block past the row was fetched as zeros and lands in the dummy slot)
                uint8_t *dummy = (uint8_t *)(red + (lay.dummy - lay.red) / sizeof(float)) + (size_t)wave * XBLK;
                uint8_t *dst = pre_b < nb ? lds + (size_t)pre_b * XBLK : dummy;
                const int grp = lane & 31;
                put_group_pair(dst, grp, pq.x, pq.y);
                if (grp == 0)
                    *(uint32_t *)(dst + XBLK_D) = pd;
            }
            for (int b = wave + 2 * NW; b < nb; b += NW)
                stage_quantised_wave<TR::ACT>(lds + (size_t)b * XBLK, xrow, b, lane);
        } else {
            if (TR::ACT != LFAMD_TYPE_Q8_K && kb != 8 * nb) { // a padded row (uniform over the launch): its last block stages the tail
                for (int b = wave; b < nb; b += NW) {
                    if (b * 8 + 8 > kb) // (b is wave-uniform: a scalar branch)
                        stage_quantised_wave<TR::ACT, true>(lds + (size_t)b * XBLK, xrow, b, lane, kb);
                    else
                        stage_quantised_wave<TR::ACT>(lds + (size_t)b * XBLK, xrow, b, lane);
                }
            } else { // whole rows: the loop as it was before the layout
                for (int b = wave; b < nb; b += NW)
                    stage_quantised_wave<TR::ACT>(lds + (size_t)b * XBLK, xrow, b, lane);
            }
        }
    }
    // the image blocks this wave reads are the ones it has just written: program order in the LDS queue is enough;
    // only the compiler must not move the reads above the (differently typed) writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    GSTAMP();

    // (measured and rejected, round 2, twice: TWO items ahead for deep rows — the second buffer issued before the staging, or
    // right after this wave's activations have landed and before the quantisation arithmetic; pre-quantised rows with both
    // up front: 9.5 -> 10.5 us Q4_K, 14.9 -> 16.4 Q6_K, 11.0 / 17.6 pre-quantised.  A CU's loads return in issue order and
    // the 256 CUs together already take what HBM gives (33 MB in ~5.2 us of a ~6.8 us kernel body): putting wave w's second
    // item ahead of wave w+1's first only delays the moment the LAST wave can start its first dot, and both its dots
    // then run after the stream has ended)
    // pairs of items without a branch inside (a conditionally skipped consume leaves its buffer's loads "pending" at
    // the loop header for hipcc's wait-count pass, which then drains vmcnt(0) before every issue), then the odd one
    // (measured and rejected, round 3: FOUR items in flight per wave for launches whose work-groups walk many small items — the
    // Mixtral gate + up experts, 14 half-tiles of 37 KB per work-group: decode pass 1.820 -> 1.883 ms)
    for (;;) {
        kq_cursor cn = cc;
        KQ_ADVANCE(cn);
        if (cn.ht >= n_ht)
            break;
        KQ_ISSUE(bufB);
        KQ_CONSUME(bufA);
        GSTAMP();
        KQ_ISSUE(bufA);
        KQ_CONSUME(bufB);
    }
    if (cc.ht < n_ht)
        KQ_CONSUME(bufA);
    GWG(1);
#undef KQ_ADVANCE
#undef KQ_ISSUE
#undef KQ_CONSUME
}

template <typename TR, int NC, int BT, int NW, int GEMV_CH, bool IDS = false, bool PAIR = false>
__global__ __launch_bounds__(NW * 64) void gemv_kq_kernel(const uint8_t *__restrict__ B, size_t b_row_bytes, long col0, int nbk,
                                                          int n_ht, int gdim, const gemv_mats mats) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if constexpr (NC == 1)
        gemv_kq_body1<TR, BT, NW, GEMV_CH, IDS, false, PAIR>(mats, nbk, B, b_row_bytes, col0, n_ht, (int)blockIdx.x, gdim, lds, kq_pre{});
    else
        gemv_kq_body<TR, NC, BT, NW, GEMV_CH, IDS>(mats, nbk, B, b_row_bytes, col0, n_ht, (int)blockIdx.x, gdim, lds);
}

// ONE activation row, one to three matrices: the 13 dwords the hardware preloads are exactly what work-group `bid` needs to
// address its first item — the row (column offset and row stride folded in on the host, which folds the column into mats.C as
// well), the three weight pointers, nbk (kq_nb_of: the row's super-blocks, or its 32-blocks), n_ht, gdim and the two boundaries.  mats (and so the store path and every later item) is
// what gemv_kq_kernel gets.
template <typename TR, int NC, int BT, int NW, int GEMV_CH>
__global__ __launch_bounds__(NW * 64) void gemv_kq_early_kernel(const uint8_t *__restrict__ xrow, const uint8_t *__restrict__ A0,
                                                                const uint8_t *__restrict__ A1, const uint8_t *__restrict__ A2, int nbk,
                                                                int n_ht, int gdim, int e0, int e1, const gemv_mats mats) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    static_assert(NC == 1, "one activation row (the parameter keeps the kernel's name in line with gemv_kq_kernel's)");
    asm volatile("" : "+s"(A0), "+s"(A1), "+s"(A2), "+s"(e0), "+s"(e1));
    gemv_kq_body1<TR, BT, NW, GEMV_CH, false, true>(mats, nbk, xrow, 0, 0, n_ht, (int)blockIdx.x, gdim, lds, kq_pre{A0, A1, A2, e0, e1});
}

// Two expert GEMVs on DIFFERENT activation rows in ONE decode launch (GGML_OP_MUL_MAT_ID ffn_down_exps: every chosen expert
// multiplies its own row): work-groups [0, grid_a) run mats_a against row Ba, the rest mats_b against row Bb.  A work-group
// serves one of the two, so it stages one row, as in a single launch.
template <typename TR, int BT, int NW, int GEMV_CH>
__global__ __launch_bounds__(NW * 64) void gemv_kq_ids_pair_kernel(const uint8_t *__restrict__ Ba, const uint8_t *__restrict__ Bb,
                                                                   size_t b_row_bytes, int nbk, int n_ht_a, int n_ht_b, int grid_a, int grid_b,
                                                                   const gemv_mats mats_a, const gemv_mats mats_b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if ((int)blockIdx.x < grid_a)
        gemv_kq_body1<TR, BT, NW, GEMV_CH, true>(mats_a, nbk, Ba, b_row_bytes, 0, n_ht_a, (int)blockIdx.x, grid_a, lds, kq_pre{});
    else
        gemv_kq_body1<TR, BT, NW, GEMV_CH, true>(mats_b, nbk, Bb, b_row_bytes, 0, n_ht_b, (int)blockIdx.x - grid_a, grid_b, lds, kq_pre{});
}

// Two weight types in ONE decode launch (sibling mat-muls on the same activations whose types differ: attn_q/k in Q4_K
// with attn_v in Q6_K in a Q4_K_M file): work-groups [0, grid_a) run type A's body over mats_a, the rest type B's over
// mats_b.  A work-group is of one type, so it stages the activations once, in the (shared) Q8_K image.
template <typename TRA, typename TRB, int BT, int NW, int GEMV_CH>
__global__ __launch_bounds__(NW * 64) void gemv_kq_dual_kernel(const uint8_t *__restrict__ B, size_t b_row_bytes, int nbk, int n_ht_a,
                                                               int n_ht_b, int grid_a, int grid_b, const gemv_mats mats_a,
                                                               const gemv_mats mats_b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    static_assert(TRA::ACT == TRB::ACT, "both types must share the activation image, and so the meaning of nbk (kq_nb_of)");
    if ((int)blockIdx.x < grid_a)
        gemv_kq_body1<TRA, BT, NW, GEMV_CH, false>(mats_a, nbk, B, b_row_bytes, 0, n_ht_a, (int)blockIdx.x, grid_a, lds, kq_pre{});
    else
        gemv_kq_body1<TRB, BT, NW, GEMV_CH, false>(mats_b, nbk, B, b_row_bytes, 0, n_ht_b, (int)blockIdx.x - grid_a, grid_b, lds, kq_pre{});
}

// ... with the first item of BOTH sub-grids from preloaded arguments, for the launch every Q4_K_M / Q5_K_M layer makes: one or
// two matrices of type A (one boundary) and ONE of type B.  13 dwords again; grid_b, which only later items need, comes last
// (a fourteenth dword is all the hardware grants beside the kernel-argument pointer).
template <typename TRA, typename TRB, int BT, int NW, int GEMV_CH>
__global__ __launch_bounds__(NW * 64) void gemv_kq_dual_early_kernel(const uint8_t *__restrict__ xrow, const uint8_t *__restrict__ Aa0,
                                                                     const uint8_t *__restrict__ Aa1, const uint8_t *__restrict__ Ab0, int nbk,
                                                                     int n_ht_a, int n_ht_b, int grid_a, int ea0, int grid_b,
                                                                     const gemv_mats mats_a, const gemv_mats mats_b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    static_assert(TRA::ACT == TRB::ACT, "both types must share the activation image, and so the meaning of nbk (kq_nb_of)");
    asm volatile("" : "+s"(Aa0), "+s"(Aa1), "+s"(Ab0), "+s"(ea0), "+s"(grid_a));
    if ((int)blockIdx.x < grid_a)
        gemv_kq_body1<TRA, BT, NW, GEMV_CH, false, true>(mats_a, nbk, xrow, 0, 0, n_ht_a, (int)blockIdx.x, grid_a, lds,
                                                         kq_pre{Aa0, Aa1, Aa1, ea0, KQ_NO_BOUNDARY});
    else
        gemv_kq_body1<TRB, BT, NW, GEMV_CH, false, true>(mats_b, nbk, xrow, 0, 0, n_ht_b, (int)blockIdx.x - grid_a, grid_b, lds,
                                                         kq_pre{Ab0, Ab0, Ab0, KQ_NO_BOUNDARY, KQ_NO_BOUNDARY});
}

// ---------------------------------------------------------------------------------------------
// One translation unit per weight type (gemv_*.hip) instantiates its kernels by naming them here and exports the lookup that
// gemv.hip launches through (the 8 column counts x 2 activation types x chunk variants of every type used to compile serially
// in one 140-second file).  Which (waves, chunk) pairs exist is the plan's range (gemv.hip: lfamd_gemv_plan_of); anything
// else answers nullptr.

// n = 1: {8 x 2, 16 x 1, 16 x 2} plain (four matrices) and with the early first issue (one to three); 32-row items (16 x 1 only) where the type takes them
template <typename TR, int BT, bool ROWS32>
static const void *kq_kernel_1(int variant, int nw, int ch) {
    const int form = nw * 10 + ch;
    if (variant == LFAMD_GEMV_PLAIN)
        return form == 82    ? (const void *)gemv_kq_kernel<TR, 1, BT, 8, 2>
               : form == 161 ? (const void *)gemv_kq_kernel<TR, 1, BT, 16, 1>
               : form == 162 ? (const void *)gemv_kq_kernel<TR, 1, BT, 16, 2>
                             : nullptr;
    if (variant == LFAMD_GEMV_EARLY)
        return form == 82    ? (const void *)gemv_kq_early_kernel<TR, 1, BT, 8, 2>
               : form == 161 ? (const void *)gemv_kq_early_kernel<TR, 1, BT, 16, 1>
               : form == 162 ? (const void *)gemv_kq_early_kernel<TR, 1, BT, 16, 2>
                             : nullptr;
    if constexpr (ROWS32)
        if (variant == LFAMD_GEMV_ROWS32 && form == 161)
            return (const void *)gemv_kq_kernel<TR, 1, BT, 16, 1, false, true>;
    return nullptr;
}

// n = 2..8: {16 x 1, 8 x 2, 8 x 4}, plain
template <typename TR, int BT, int NC>
static const void *kq_kernel_n(int nw, int ch) {
    const int form = nw * 10 + ch;
    return form == 161  ? (const void *)gemv_kq_kernel<TR, NC, BT, 16, 1>
           : form == 82 ? (const void *)gemv_kq_kernel<TR, NC, BT, 8, 2>
           : form == 84 ? (const void *)gemv_kq_kernel<TR, NC, BT, 8, 4>
                        : nullptr;
}

template <typename TR, int BT, bool ROWS32>
static const void *kq_kernel(int variant, int nc, int nw, int ch) {
    static const void *(*const cols[])(int, int) = {kq_kernel_n<TR, BT, 2>, kq_kernel_n<TR, BT, 3>, kq_kernel_n<TR, BT, 4>, kq_kernel_n<TR, BT, 5>,
                                                    kq_kernel_n<TR, BT, 6>, kq_kernel_n<TR, BT, 7>, kq_kernel_n<TR, BT, 8>};
    if (nc == 1)
        return kq_kernel_1<TR, BT, ROWS32>(variant, nw, ch);
    return nc >= 2 && nc <= 8 && variant == LFAMD_GEMV_PLAIN ? cols[nc - 2](nw, ch) : nullptr;
}

// the expert forms (MUL_MAT_ID at decode): {8 x 2, 16 x 1, 16 x 2} for one row, {16 x 1, 16 x 2} for the pair of rows
template <typename TR, int BT>
static const void *kq_kernel_ids(int variant, int nw, int ch) {
    const int form = nw * 10 + ch;
    if (variant == LFAMD_GEMV_EXPERT)
        return form == 82    ? (const void *)gemv_kq_kernel<TR, 1, BT, 8, 2, true>
               : form == 161 ? (const void *)gemv_kq_kernel<TR, 1, BT, 16, 1, true>
               : form == 162 ? (const void *)gemv_kq_kernel<TR, 1, BT, 16, 2, true>
                             : nullptr;
    if (variant == LFAMD_GEMV_EXPERT_PAIR)
        return form == 161   ? (const void *)gemv_kq_ids_pair_kernel<TR, BT, 16, 1>
               : form == 162 ? (const void *)gemv_kq_ids_pair_kernel<TR, BT, 16, 2>
                             : nullptr;
    return nullptr;
}

// What a type's unit exports.  QTYPE: the type's pre-quantised activation format.  ROWS32: the unit holds the 32-row-item
// kernel (the plan asks for it by kq_unit::rows32 in gemv.hip).  IDS: it holds the expert forms (Q4_K, Q5_K, Q6_K).
template <typename TR, int QTYPE, bool ROWS32, bool IDS>
static const void *kq_unit_kernel(int variant, int nc, int f32in, int nw, int ch) {
    if constexpr (IDS)
        if (nc == 1 && (variant == LFAMD_GEMV_EXPERT || variant == LFAMD_GEMV_EXPERT_PAIR))
            return f32in ? kq_kernel_ids<TR, LFAMD_TYPE_F32>(variant, nw, ch) : kq_kernel_ids<TR, QTYPE>(variant, nw, ch);
    return f32in ? kq_kernel<TR, LFAMD_TYPE_F32, ROWS32>(variant, nc, nw, ch) : kq_kernel<TR, QTYPE, ROWS32>(variant, nc, nw, ch);
}

// ... and a two-type unit (16 x 1, 16 x 2; the shared activation image is Q8_K)
template <typename TRA, typename TRB>
static const void *kq_dual_unit_kernel(int variant, int nc, int f32in, int nw, int ch) {
    if (variant == KQ_TWO_TYPES_EARLY && nc == 1 && nw == 16 && (ch == 1 || ch == 2)) {
        if (f32in)
            return ch == 1 ? (const void *)gemv_kq_dual_early_kernel<TRA, TRB, LFAMD_TYPE_F32, 16, 1>
                           : (const void *)gemv_kq_dual_early_kernel<TRA, TRB, LFAMD_TYPE_F32, 16, 2>;
        return ch == 1 ? (const void *)gemv_kq_dual_early_kernel<TRA, TRB, LFAMD_TYPE_Q8_K, 16, 1>
                       : (const void *)gemv_kq_dual_early_kernel<TRA, TRB, LFAMD_TYPE_Q8_K, 16, 2>;
    }
    if (variant != LFAMD_GEMV_TWO_TYPES || nc != 1 || nw != 16 || (ch != 1 && ch != 2))
        return nullptr;
    if (f32in)
        return ch == 1 ? (const void *)gemv_kq_dual_kernel<TRA, TRB, LFAMD_TYPE_F32, 16, 1>
                       : (const void *)gemv_kq_dual_kernel<TRA, TRB, LFAMD_TYPE_F32, 16, 2>;
    return ch == 1 ? (const void *)gemv_kq_dual_kernel<TRA, TRB, LFAMD_TYPE_Q8_K, 16, 1>
                   : (const void *)gemv_kq_dual_kernel<TRA, TRB, LFAMD_TYPE_Q8_K, 16, 2>;
}
