// gemm_common.h — what the MFMA batch bodies share (gemm_mfma, gemm_wide_*, gemm_lw, gemm_ks, gemm_kr, gemm_i8, gemm_lf, gemm_sb):
//   * exact-integer dequantisation of packed K-quant dwords into f16 MFMA fragments;
//   * the XCD-aware tile order and the work-group tile prologues built on it (XCD_ORDER, WG_TILE_AT, MOE_TILE_OR_RETURN);
//   * gemm_mats, the by-value table of a fused launch, and its host filler fill_gemm_mats;
//   * the inline-asm issue forms: loads with their own wait states (gload*, glds*), the lean ones (dma16, dma4, ld16, dsr16).
// A new body starts from these and writes its own K loop and epilogue.
#pragma once
#include "lfamd_device.h"
#ifndef GEMM_DIAG
#define GEMM_DIAG 0 // development builds of one unit: 1, 2 ablations (gemm_mfma, gemm_wide); 3, 4, 6, 7 stamps (diag_stamps.h)
#endif

#define XT_ROW_BYTES 512 // 256 f16 codes of one token for one super-block

__device__ static inline half2_t as_half2(uint32_t u) {
    return __builtin_bit_cast(half2_t, u);
}

__device__ static inline half2_t pk_fma(half2_t a, half2_t b, half2_t c) {
    return __builtin_elementwise_fma(a, b, c);
}

__device__ static inline half2_t bcast_h2(float v) {
    _Float16 h = (_Float16)v;
    half2_t r = {h, h};
    return r;
}

union frag_u {
    half8_t v;
    half2_t p[4];
    uint4 u;
};

// One K-step (8 nibbles of this lane) of a Q4_K-family dword -> f16x8 of sc*q.
// S = (sc,sc), O = (-1024 sc), S16 = sc/16, O16 = -64 sc.
// `magic` = 0x64006400 held in a VGPR: gfx9 VOP3 encodes one literal/SGPR only, so with both constants as
// literals hipcc splits (x & m) | magic into v_and + v_or; with the magic in a register it is one v_and_or_b32.
__device__ static inline half8_t dequant_q4(uint32_t x, half2_t S, half2_t O, half2_t S16, half2_t O16, uint32_t magic) {
    frag_u f;
    const uint32_t y = x >> 8;
    f.p[0] = pk_fma(as_half2((x & 0x000F000Fu) | magic), S, O);
    f.p[1] = pk_fma(as_half2((x & 0x00F000F0u) | magic), S16, O16);
    f.p[2] = pk_fma(as_half2((y & 0x000F000Fu) | magic), S, O);
    f.p[3] = pk_fma(as_half2((y & 0x00F000F0u) | magic), S16, O16);
    return f.v;
}

// Q5_K: the fifth bits of the K-step, already shifted onto their lattice (Hd = H >> dd, see q5hpos), join the
// nibbles before the same fused multiply-add: sc*q <= 63*31 = 1953 stays exact in f16.
__device__ static inline half8_t dequant_q5(uint32_t x, uint32_t Hd, half2_t S, half2_t O, half2_t S16, half2_t O16,
                                            uint32_t magic) {
    frag_u f;
    const uint32_t y = x >> 8;
    f.p[0] = pk_fma(as_half2((Hd & 0x00100010u) | ((x & 0x000F000Fu) | magic)), S, O);
    f.p[1] = pk_fma(as_half2((Hd & 0x01000100u) | ((x & 0x00F000F0u) | magic)), S16, O16);
    f.p[2] = pk_fma(as_half2(((Hd >> 8) & 0x00100010u) | ((y & 0x000F000Fu) | magic)), S, O);
    f.p[3] = pk_fma(as_half2(((Hd << 8) & 0x01000100u) | ((y & 0x00F000F0u) | magic)), S16, O16);
    return f.v;
}

// codes with an offset (Q3_K: q = code - 4): -(1024 + off) * sc is not an f16 number in general (1028 * 31 needs 13
// mantissa bits), so the offset is removed first (exact) and the scale applied by a second packed op.
__device__ static inline half8_t dequant_q4_off(uint32_t x, half2_t S, float off, uint32_t magic) {
    frag_u f;
    const uint32_t y = x >> 8;
    const half2_t o1 = bcast_h2(-(1024.0f + off)), o16 = bcast_h2(-(64.0f + off));
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    f.p[0] = (as_half2((x & 0x000F000Fu) | magic) + o1) * S;
    f.p[1] = pk_fma(as_half2((x & 0x00F000F0u) | magic), r16, o16) * S;
    f.p[2] = (as_half2((y & 0x000F000Fu) | magic) + o1) * S;
    f.p[3] = pk_fma(as_half2((y & 0x00F000F0u) | magic), r16, o16) * S;
    return f.v;
}

// Q4_0: the code minus 8, no integer scale (the f16 block scale is applied in f32 per 32-block).
__device__ static inline half8_t dequant_q40(uint32_t x, uint32_t magic) {
    frag_u f;
    const uint32_t y = x >> 8;
    const half2_t m1032 = {(_Float16)-1032.0f, (_Float16)-1032.0f};
    const half2_t m72 = {(_Float16)-72.0f, (_Float16)-72.0f};
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    f.p[0] = as_half2((x & 0x000F000Fu) | magic) + m1032;
    f.p[1] = pk_fma(as_half2((x & 0x00F000F0u) | magic), r16, m72);
    f.p[2] = as_half2((y & 0x000F000Fu) | magic) + m1032;
    f.p[3] = pk_fma(as_half2((y & 0x00F000F0u) | magic), r16, m72);
    return f.v;
}

// IQ4_NL: the dword's eight nibbles are indices into the 16-entry codebook (kvalues_iq4nl, |value| <= 127: exact in f16).  The
// look-up is three v_perm per four indices on a table of value + 128 (lower / upper eight entries by the index's low three bits,
// then byte i of one or the other by its bit 3); v_perm then builds the f16 pairs 1024 + u (bytes [u, 0x64, u', 0x64]) and one
// packed add removes the 1152, as dequant_bytes does.  Element order: dequant_q40's (nibbles 0, 4, 1, 5, 2, 6, 3, 7).
__device__ static inline half8_t dequant_iq4nl(uint32_t x) {
    constexpr uint32_t T0 = 0x3F2D1801u, T1 = 0x766A5D4Fu, T2 = 0xA6998D81u, T3 = 0xF1D9C5B5u; // kvalues_iq4nl + 128, 4 entries each
    const half2_t m1152 = {(_Float16)-1152.0f, (_Float16)-1152.0f};
    const uint32_t n0 = x & 0x0F0F0F0Fu, n1 = (x >> 4) & 0x0F0F0F0Fu; // nibbles 0, 2, 4, 6 / 1, 3, 5, 7, one per byte
    const uint32_t s0 = n0 & 0x07070707u, s1 = n1 & 0x07070707u;
    const uint32_t u0 = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T3, T2, s0), __builtin_amdgcn_perm(T1, T0, s0),
                                              ((n0 >> 1) & 0x04040404u) | 0x03020100u);
    const uint32_t u1 = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T3, T2, s1), __builtin_amdgcn_perm(T1, T0, s1),
                                              ((n1 >> 1) & 0x04040404u) | 0x03020100u);
    frag_u f;
    f.p[0] = as_half2(__builtin_amdgcn_perm(0x64646464u, u0, 0x04020400u)) + m1152; // nibbles 0, 4
    f.p[1] = as_half2(__builtin_amdgcn_perm(0x64646464u, u1, 0x04020400u)) + m1152; // 1, 5
    f.p[2] = as_half2(__builtin_amdgcn_perm(0x64646464u, u0, 0x04030401u)) + m1152; // 2, 6
    f.p[3] = as_half2(__builtin_amdgcn_perm(0x64646464u, u1, 0x04030401u)) + m1152; // 3, 7
    return f.v;
}

// legacy 32-block types on a per-call image: code (4 or 5 bits, fifth bits Hd on the P5K lattice) minus `off`, no scale
template <bool H5>
__device__ static inline half8_t dequant_legacy(uint32_t x, uint32_t Hd, float off, uint32_t magic) {
    frag_u f;
    const uint32_t y = x >> 8;
    const half2_t o1 = bcast_h2(-(1024.0f + off)), o16 = bcast_h2(-(64.0f + off));
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    uint32_t c0 = (x & 0x000F000Fu) | magic, c1 = (x & 0x00F000F0u) | magic, c2 = (y & 0x000F000Fu) | magic,
             c3 = (y & 0x00F000F0u) | magic;
    if constexpr (H5) {
        c0 |= Hd & 0x00100010u;
        c1 |= Hd & 0x01000100u;
        c2 |= (Hd >> 8) & 0x00100010u;
        c3 |= (Hd << 8) & 0x01000100u;
    }
    f.p[0] = as_half2(c0) + o1;
    f.p[1] = pk_fma(as_half2(c1), r16, o16);
    f.p[2] = as_half2(c2) + o1;
    f.p[3] = pk_fma(as_half2(c3), r16, o16);
    return f.v;
}

// IQ4_XS byte image: two dwords = the K-step's eight values + 128; v_perm builds the f16 pairs 1024 + u directly
// (bytes [u0, 0x64, u1, 0x64]), then sc * value = (1024 + u) * sc - 1152 * sc (1152 * sc = 9 * sc * 2^7 is exact in f16;
// |sc * value| reaches 4064, so products above 2048 round like Q6_K's).
__device__ static inline half8_t dequant_bytes(uint32_t d0, uint32_t d1, half2_t S, half2_t O) {
    frag_u f;
    f.p[0] = pk_fma(as_half2(__builtin_amdgcn_perm(0x64646464u, d0, 0x04010400u)), S, O);
    f.p[1] = pk_fma(as_half2(__builtin_amdgcn_perm(0x64646464u, d0, 0x04030402u)), S, O);
    f.p[2] = pk_fma(as_half2(__builtin_amdgcn_perm(0x64646464u, d1, 0x04010400u)), S, O);
    f.p[3] = pk_fma(as_half2(__builtin_amdgcn_perm(0x64646464u, d1, 0x04030402u)), S, O);
    return f.v;
}

// The four dequantisation constants (S, O = -1024 S, S16 = S/16, O16 = -64 S) of TWO sub-blocks at once, lane-packed:
// v_perm puts the two scale bytes into f16 slots as 1024 + sc, one packed add removes the 1024, three packed multiplies
// give the rest: 5 VALU per sub-block pair instead of 12 (the K loop is VALU-issue bound: PMC shows VALU and MFMA
// cycles adding up rather than overlapping).  Users pick a half with a broadcast shuffle (folded into op_sel).
struct q4_consts2 {
    half2_t S, O, S16, O16;
};
__device__ static inline q4_consts2 q4_consts_pair(uint32_t word, int byte_lo) { // scales = bytes byte_lo, byte_lo + 1 of word
    q4_consts2 c;
    const uint32_t sel = byte_lo == 0 ? 0x04010400u : 0x04030402u; // [b, 0x64, b', 0x64]
    const half2_t m1024 = {(_Float16)-1024.0f, (_Float16)-1024.0f}, m64 = {(_Float16)-64.0f, (_Float16)-64.0f};
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    c.S = as_half2(__builtin_amdgcn_perm(0x64646464u, word, sel)) + m1024;
    c.O = c.S * m1024;
    c.S16 = c.S * r16;
    c.O16 = c.S * m64;
    return c;
}

// the same with the row's f16 super-block scale folded in (scaled-operand GEMM: S = d * sc rounded to f16; the three
// derived constants are exact multiples of it)
__device__ static inline q4_consts2 q4_consts_pair_scaled(uint32_t word, int byte_lo, half2_t d2) {
    q4_consts2 c;
    const uint32_t sel = byte_lo == 0 ? 0x04010400u : 0x04030402u;
    const half2_t m1024 = {(_Float16)-1024.0f, (_Float16)-1024.0f}, m64 = {(_Float16)-64.0f, (_Float16)-64.0f};
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    c.S = (as_half2(__builtin_amdgcn_perm(0x64646464u, word, sel)) + m1024) * d2;
    c.O = c.S * m1024;
    c.S16 = c.S * r16;
    c.O16 = c.S * m64;
    return c;
}

__device__ static inline uint32_t opaque_magic() {
    uint32_t magic = 0x64006400u;
    asm volatile("" : "+v"(magic)); // keep it a register value (see dequant_q4)
    return magic;
}

// Q6_K: codes are 6 bit (ql nibble | qh field), value sc*(code-32).  (code-32) is formed exactly,
// the product with the int8 scale is rounded to f16 (exact up to 2048; RNE to even above).
__device__ static inline half8_t dequant_q6(uint32_t x, uint32_t H, half2_t S) {
    frag_u f;
    const uint32_t y = x >> 8;
    const half2_t m1056 = {(_Float16)-1056.0f, (_Float16)-1056.0f};
    const half2_t m96 = {(_Float16)-96.0f, (_Float16)-96.0f};
    const half2_t r16 = {(_Float16)0.0625f, (_Float16)0.0625f};
    half2_t c0 = as_half2((x & 0x000F000Fu) | (H & 0x00300030u) | 0x64006400u) + m1056;
    half2_t c1 = pk_fma(as_half2((x & 0x00F000F0u) | (H & 0x03000300u) | 0x64006400u), r16, m96);
    half2_t c2 = as_half2((y & 0x000F000Fu) | ((H >> 8) & 0x00300030u) | 0x64006400u) + m1056;
    half2_t c3 = pk_fma(as_half2((y & 0x00F000F0u) | ((H << 8) & 0x03000300u) | 0x64006400u), r16, m96);
    f.p[0] = c0 * S;
    f.p[1] = c1 * S;
    f.p[2] = c2 * S;
    f.p[3] = c3 * S;
    return f.v;
}

// Linear tile order -> (row-block, token tile).  Tiles are walked in SUPER-TILES of 8 row-blocks x 4 token tiles
// (ragged at the edges): an XCD's 32 resident work-groups then share 8 x 128 weight rows (8 x 72 B/row/256k) and
// 4 x 64 activation rows in its L2, instead of each XCD streaming every weight row (measured: 6x the algorithmic
// HBM bytes with the row-blocks-fastest order).  72a + 128b bytes per K element is minimal at a x b = 8 x 4.
__device__ static inline void tile_of(int L, int n_rb, int n_tt, int &rb, int &tt) {
    constexpr int SA = 8, SB = 4;
    const int grp = n_rb * SB;                    // tiles in one group of SB token tiles
    const int g = L / grp;
    const int idx = L - g * grp;
    const int w = min(SB, n_tt - g * SB);         // token tiles in this group (last group may be narrower)
    const int run = idx / (SA * w);
    const int rem = idx - run * SA * w;
    const int hgt = min(SA, n_rb - run * SA);     // row-blocks in this run (last run may be shorter)
    const int tl = rem / hgt;
    rb = run * SA + (rem - tl * hgt);
    tt = g * SB + tl;
}

// Up to GEMM_MAX_MATS weight matrices of one type and row length that consume the SAME activations (attn_q/k/v,
// ffn_gate/up) share one prep and one launch: their 128-row blocks are concatenated (rb_end = exclusive prefix).
#define GEMM_MAX_MATS 4
struct gemm_mats {
    const uint8_t *A[GEMM_MAX_MATS];
    float *C[GEMM_MAX_MATS];
    long m[GEMM_MAX_MATS];
    long ldc[GEMM_MAX_MATS];
    int rb_end[GEMM_MAX_MATS];
    int count;
    // GGML_OP_MUL_MAT_ID batches (MOE kernels only): A[0] = the expert stack, C[0] = result rows; token slots are grouped
    // by expert on the device (moe.hip, moe_route_kernel): expert e owns slots [poff[e], poff[e] + cnt[e]), slot -> result
    // row through slot_row.  The grid covers the worst case; work-groups beyond an expert's count exit at once.
    const int *moe_cnt, *moe_poff, *moe_slot_row;
    long expert_bytes;
    int moe_ct_max;
};

// The matrices of a launch with m > 0, padded to GEMM_MAX_MATS with empty ones; returns their row blocks of 128
// (mats.count == 0: an empty launch, nothing else is set).
static inline int fill_gemm_mats(gemm_mats &mats, int count, const void *const *A, const long *m, float *const *C, const long *ldc) {
    int n_rb = 0;
    mats.count = 0;
    mats.moe_cnt = mats.moe_poff = mats.moe_slot_row = nullptr, mats.expert_bytes = 0, mats.moe_ct_max = 0;
    for (int j = 0; j < count; j++) {
        if (m[j] <= 0)
            continue;
        const int i = mats.count++;
        mats.A[i] = (const uint8_t *)A[j], mats.C[i] = C[j], mats.m[i] = m[j], mats.ldc[i] = ldc[j];
        n_rb += (int)((m[j] + 127) / 128);
        mats.rb_end[i] = n_rb;
    }
    for (int i = mats.count; i < GEMM_MAX_MATS && mats.count > 0; i++)
        mats.A[i] = mats.A[0], mats.C[i] = mats.C[0], mats.m[i] = 0, mats.ldc[i] = 0, mats.rb_end[i] = n_rb;
    return n_rb;
}

// ---- the work-group tile prologues
// Block ids go round-robin over the 8 XCDs.  XCD_ORDER gives every XCD one contiguous run of the linear order of the n_wg
// work-groups (q8 = n_wg >> 3, r8 = n_wg & 7, xcd = id & 7: XCD xcd starts at xcd * q8 + min(xcd, r8) and takes its (id >> 3)-th):
// an XCD's resident work-groups then walk neighbouring tiles of tile_of's super-tiles and share weight rows and activation rows
// in that XCD's L2 (row blocks fastest, the first order tried, had every XCD stream every weight row).
//
// The three pieces below are macros, not functions: a helper that returns {rb, ct, mj} leaves the instruction mix of a body as
// it is but renames registers and reorders its first instructions, even the permutation alone as an inline function commuted the
// operands of one s_mul in gemm_lw's two-type kernel, and a body whose ISA moved owes a timing.  A macro
// expands to the statements the bodies held and moves nothing.
#define XCD_ORDER(block_id, wgs)                                                                                       \
    ({                                                                                                                 \
        const int n_wg_ = (wgs); /* (trailing underscores: the arguments may be called n_wg and id) */                 \
        const int id_ = (block_id), q8_ = n_wg_ >> 3, r8_ = n_wg_ & 7, xcd_ = id_ & 7;                                 \
        (xcd_ < r8_ ? xcd_ * (q8_ + 1) : r8_ * (q8_ + 1) + (xcd_ - r8_) * q8_) + (id_ >> 3);                           \
    })

// WG_TILE_AT: position L of the linear order over n_rb x n_ct tiles -> (row block rb, token tile ct) and the matrix mj of a fused
// launch that the row block belongs to, with rb rebased onto that matrix.  L = XCD_ORDER(block id, n_rb * n_ct); a launch whose K
// is split over ks work-groups per tile orders n_rb * n_ct * ks of them, K part slowest (L / tiles), and passes L % tiles.
#define WG_TILE_AT(mats, L, n_rb, n_ct, rb, ct, mj)                                                                    \
    do {                                                                                                               \
        tile_of(L, n_rb, n_ct, rb, ct);                                                                                \
        mj = 0;                                                                                                        \
        _Pragma("unroll") for (int jj = 1; jj < GEMM_MAX_MATS; jj++)                                                   \
            if (jj < (mats).count && rb >= (mats).rb_end[jj - 1])                                                      \
                mj = jj;                                                                                               \
        if (mj > 0)                                                                                                    \
            rb -= (mats).rb_end[mj - 1];                                                                               \
    } while (0)

// GGML_OP_MUL_MAT_ID: work-group `bid` of `gdim` = (token tile of `cols` slots, expert, row block), row blocks fastest and the
// token tile slowest: consecutive ids go round-robin over the XCDs, so the live tiles (low token-tile index) spread over all
// eight instead of piling onto XCD 0 and 1, and they are dispatched before the tiles that only exit.  The routing kernel ran
// earlier on this stream.  Yields rb, ct, moe_left = the token slots of this tile that carry a row, A = the expert's weights and
// n0 = the tile's first slot — and RETURNS from the kernel when the tile carries none (uniform over the work-group).  It declares
// per_ct, rem and e, so it stands first in the MUL_MAT_ID block of a kernel.  bid, gdim: ints, or the built-in unsigned block index
// and grid size as they are (the wide kernel divides them unsigned).
#define MOE_TILE_OR_RETURN(mats, bid, gdim, n_rb, cols, rb, ct, moe_left, A, n0)                                       \
    const int per_ct = (int)((gdim) / (mats).moe_ct_max); /* experts * n_rb */                                         \
    ct = (bid) / per_ct;                                                                                               \
    const int rem = (bid)-ct * per_ct;                                                                                 \
    const int e = rem / n_rb;                                                                                          \
    rb = rem - e * n_rb;                                                                                               \
    moe_left = (mats).moe_cnt[e] - ct * (cols);                                                                        \
    if (moe_left <= 0)                                                                                                 \
        return;                                                                                                        \
    A = (mats).A[0] + (size_t)e * (mats).expert_bytes;                                                                 \
    n0 = (long)(mats).moe_poff[e] + (long)ct * (cols)

// ---- issue forms
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// make a wave-uniform pointer provably so (an "s" operand must be), via two v_readfirstlane
__device__ static inline const uint8_t *uniform_ptr(const void *p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const uint8_t *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

__device__ static inline uint32_t lds_addr(const void *p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint8_t *)(const uint8_t *)p);
}

// Forms that carry their own wait states: a VALU write of an SGPR — v_readfirstlane, so uniform_ptr() — needs five wait states
// before a vector-memory instruction reads that SGPR, and hipcc's hazard recogniser does not see inside an asm statement.  These
// lead with `s_nop 4`, and the glds* save and restore M0.
template <int IMM>
__device__ static inline void gload16(u32x4 &dst, const void *base, uint32_t voff) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
template <int IMM>
__device__ static inline void gload4(uint32_t &dst, const void *base, uint32_t voff) {
    asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
template <int IMM>
__device__ static inline void gload2(uint32_t &dst, const void *base, uint32_t voff) {
    asm volatile("s_nop 4\n\tglobal_load_ushort %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}

// four LDS-DMA pieces (1 KiB each) to consecutive LDS slots from one SGPR base + per-lane offsets
__device__ static inline void glds4(const void *base, uint32_t lds_dst, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3) {
    uint32_t keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(base), "s"(lds_dst)
                 : "memory", "scc");
}
__device__ static inline void glds1x16(const void *base, uint32_t lds_dst, uint32_t o0) {
    uint32_t keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(o0), "s"(base), "s"(lds_dst)
                 : "memory");
}
__device__ static inline void glds1x4(const void *base, uint32_t lds_dst, uint32_t o0) {
    uint32_t keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(o0), "s"(base), "s"(lds_dst)
                 : "memory");
}

// LEAN forms, one instruction each (plus the M0 write of an LDS-DMA piece: 64 lanes x 16 B, or x 4 B, from base + voff to LDS at
// lds_dst + 16, or 4, * lane).  Their asm carries no wait states: the bodies that use them keep their addresses in SGPRs by
// scalar adds and follow uniform_ptr() with an `s_nop 4` fence that consumes the pointers; tools/isa_hazards.py checks the rule
// on the final ISA.  M0 is written and never restored (nothing else in those kernels reads it).
// dma16<IMM>: LDS address lds_dst + IMM (one s_add; a plain offset field would move the global address too)
template <int IMM>
__device__ static inline void dma16(const void *base, uint32_t lds_dst, uint32_t voff) {
    asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds_dst), "n"(IMM) : "memory", "scc");
}
__device__ static inline void dma16(const void *base, uint32_t lds_dst, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds_dst) : "memory");
}
__device__ static inline void dma4(const void *base, uint32_t lds_dst, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(base), "s"(lds_dst) : "memory");
}
template <int IMM>
__device__ static inline void ld16(u32x4 &dst, const void *base, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
// LDS fragment read hipcc neither counts nor moves: the K loops keep the next K-step's fragments in flight under the current
// step's MFMAs and wait with a counted lgkmcnt (left to itself hipcc reuses ONE fragment register and waits lgkmcnt(0) in front
// of every MFMA — the whole LDS latency, 64 times per super-block).  V: half8_t or u32x4.
template <int IMM, class V>
__device__ static inline void dsr16(V &dst, uint32_t addr) {
    static_assert(sizeof(V) == 16, "ds_read_b128 fills four registers");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(IMM));
}
template <int N>
__device__ static inline void ds_wait(half8_t &a, half8_t &b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}

