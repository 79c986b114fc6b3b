// pack.hip — the WRITE side of the weight images (lfamd_device.h; DESIGN.md section 24 has the dword ranges of every tile): every
// packer, expander and image size.  dequant.hip is the read side, lfamd_internal.h says which image a type has.
//
// Counterpart of the reference's weight upload, ggml_backend_cuda_buffer_set_tensor
// (ggml-cuda.cu.patch:16971-16977): the backend owns the device copy, so it may choose its layout.
//
// Every image of 32 rows x 256 weights but P6K (pack_q6k_kernel, kept for its speed) is written by ONE kernel, pack_tiles_kernel<IMG>,
// the mirror of dequant.hip's tile_code<LY>: one thread per output dword; a tile is a list of sections (sections_of), and each kind of section is written once for all the
// images that have it.  What differs per type is where weight k of a super-block sits in the GGUF block (gguf_code) and what the
// header holds (hdr_word, row_word).
#include "lfamd_device.h"
#include "lfamd_internal.h"

__device__ static const int8_t kvalues_iq4nl_dev[16] = {-127, -104, -83, -65, -49, -35, -22, -10,
                                                        1,    13,   25,  38,  53,  69,  89,  113};

// ---------------------------------------------------------------------------------------------
// Sources: the integer code of weight k (0..255) of super-block b of a GGUF row, as the file stores it.

// Q2_K / Q3_K in units of 16 consecutive weights (unit s of a super-block): w = d*sc*q - dmin*mn.
// Formulas: ggml-cuda.cu.patch:3217-3471, 3684-3699.
template <int TYPE>
__device__ static inline int code16(const uint8_t *blk, int s, int l) { // q of weight l of unit s
    const int n = s >> 3, j = (s >> 1) & 3, l0 = (s & 1) * 16;
    if constexpr (TYPE == LFAMD_TYPE_Q2_K) {
        const uint8_t *qs = blk + 16;
        return (qs[32 * n + l0 + l] >> (2 * j)) & 3;
    } else {
        const uint8_t *hmask = blk, *qs = blk + 32;
        const uint8_t m = (uint8_t)(1 << (4 * n + j));
        const int v = (qs[32 * n + l0 + l] >> (2 * j)) & 3;
        return v - ((hmask[l0 + l] & m) ? 0 : 4);
    }
}
template <int TYPE>
__device__ static inline void scale16(const uint8_t *blk, int s, int &sc, int &mn, float &d, float &dmin) {
    if constexpr (TYPE == LFAMD_TYPE_Q2_K) {
        const uint8_t *scales = blk;
        d = h2f(*(const uint16_t *)(blk + 80));
        dmin = h2f(*(const uint16_t *)(blk + 82));
        sc = scales[s] & 0xF;
        mn = scales[s] >> 4;
    } else {
        const uint8_t *scales = blk + 96;
        d = h2f(*(const uint16_t *)(blk + 108));
        dmin = 0.0f;
        int is = s;
        int us = is < 4    ? (scales[is] & 0xF) | (((scales[is + 8] >> 0) & 3) << 4)
                 : is < 8  ? (scales[is] & 0xF) | (((scales[is + 4] >> 2) & 3) << 4)
                 : is < 12 ? (scales[is - 8] >> 4) | (((scales[is] >> 4) & 3) << 4)
                           : (scales[is - 8] >> 4) | (((scales[is - 4] >> 6) & 3) << 4);
        sc = us - 32;
        mn = 0;
    }
}

__device__ static inline int q6k_code(const lfamd_block_q6_K *blk, int k) { // 0..63
    int p = k >> 7, wi = k & 127, l = wi & 31, quarter = wi >> 5;
    uint8_t qlb = blk->ql[64 * p + (quarter & 1) * 32 + l];
    int nib = quarter < 2 ? (qlb & 15) : (qlb >> 4);
    int hi = (blk->qh[32 * p + l] >> (2 * quarter)) & 3;
    return nib | (hi << 4);
}

// bytes of a block; the legacy 32-blocks: {d, [m], [qh[4]], qs[16]}
__host__ __device__ static constexpr int gguf_block(int type) {
    return type == LFAMD_TYPE_Q4_K     ? 144
           : type == LFAMD_TYPE_Q5_K   ? 176
           : type == LFAMD_TYPE_Q6_K   ? 210
           : type == LFAMD_TYPE_Q2_K   ? 84
           : type == LFAMD_TYPE_Q3_K   ? 110
           : type == LFAMD_TYPE_IQ4_XS ? 136
           : type == LFAMD_TYPE_Q4_1   ? 20
           : type == LFAMD_TYPE_Q5_0   ? 22
           : type == LFAMD_TYPE_Q5_1   ? 24
                                       : 18; // Q4_0, IQ4_NL
}
__host__ __device__ static constexpr bool gguf_has_m(int type) {
    return type == LFAMD_TYPE_Q4_1 || type == LFAMD_TYPE_Q5_1;
}
__host__ __device__ static constexpr bool gguf_has_h(int type) {
    return type == LFAMD_TYPE_Q5_0 || type == LFAMD_TYPE_Q5_1;
}

// kb: 32-blocks of a raw row of the legacy types.  kb < 8 nb (LFAMD_TYPE_PAD256): the blocks from kb on are not read and count as zero
// bytes (d = +0, m = +0, nibbles and fifth bits 0), for every row of the tile.  The other types have whole super-blocks.
template <int TYPE>
__device__ static inline int gguf_code(const uint8_t *row, int b, int k, int kb) {
    if constexpr (TYPE == LFAMD_TYPE_Q4_K) {
        const lfamd_block_q4_K *blk = (const lfamd_block_q4_K *)row + b;
        const uint8_t byte = blk->qs[32 * (k >> 6) + (k & 31)];
        return (k & 32) ? byte >> 4 : byte & 15;
    } else if constexpr (TYPE == LFAMD_TYPE_Q5_K) { // weight l of sub-block j has its fifth bit at bit j of qh[l]
        const lfamd_block_q5_K *blk = (const lfamd_block_q5_K *)row + b;
        const uint8_t byte = blk->qs[32 * (k >> 6) + (k & 31)];
        return ((k & 32) ? byte >> 4 : byte & 15) | (((blk->qh[k & 31] >> (k >> 5)) & 1) << 4);
    } else if constexpr (TYPE == LFAMD_TYPE_Q2_K) {
        return code16<TYPE>(row + (size_t)b * gguf_block(TYPE), k >> 4, k & 15);
    } else if constexpr (TYPE == LFAMD_TYPE_Q3_K) { // q + 4 in 0..7
        return code16<TYPE>(row + (size_t)b * gguf_block(TYPE), k >> 4, k & 15) + 4;
    } else if constexpr (TYPE == LFAMD_TYPE_IQ4_XS) { // the codebook index
        const lfamd_block_iq4_xs *blk = (const lfamd_block_iq4_xs *)row + b;
        const uint8_t byte = blk->qs[16 * (k >> 5) + (k & 15)];
        return (k & 16) ? byte >> 4 : byte & 15;
    } else { // weight l of a 32-block: low nibble of qs[l] (l < 16) or high nibble of qs[l - 16], fifth bit = bit l of qh
        constexpr int BS = gguf_block(TYPE), QH_OFF = gguf_has_m(TYPE) ? 4 : 2, QS_OFF = QH_OFF + (gguf_has_h(TYPE) ? 4 : 0);
        const int bl = b * 8 + (k >> 5), l = k & 31;
        const uint8_t *blk = row + (size_t)bl * BS;
        const uint8_t byte = bl < kb ? blk[QS_OFF + (l & 15)] : (uint8_t)0; // (a guarded load, not an early return: the eight loads
        int c = l < 16 ? byte & 15 : byte >> 4;                             // of a dword stay in flight together)
        if constexpr (gguf_has_h(TYPE)) {
            const uint8_t hb = bl < kb ? blk[QH_OFF + (l >> 3)] : (uint8_t)0;
            c |= ((hb >> (l & 7)) & 1) << 4;
        }
        return c;
    }
}

// ---------------------------------------------------------------------------------------------
// Images: the sections of a tile, in dwords.  IMG is the layout id of lfamd_internal.h, or one of the canonical per-call images.
enum { IMG_PCK2 = LY_NONE + 1, IMG_PCK3, IMG_PC8 }; // PCK from Q2_K / Q3_K rows, PC8 from IQ4_XS rows
enum {
    S_NIB,   // 1024: the nibble lattice, 4 groups g x 64 lanes x 4 dwords dd: K-step t = 4 g + dd of lane (i, h), low four bits
    S_HDR,   // 128 per part: 32 rows x 4 header words (hdr_word)
    S_FIFTH, // 256: 64 lanes x 4 groups: the fifth bits of the group's four K-steps
    S_BIT2,  // 512: PK2 / PK3, the low two bits of two K-steps per dword
    S_BIT3,  // 256: PK3's third bits of four K-steps per dword
    S_ROW,   // 32: one word per row (row_word)
    S_BYTE   // 2048: PC8, one byte per weight
};
struct tile_sections {
    int type;     // the GGUF type the tile is made from
    int n;        // sections
    int kind[4];
    int first[5]; // first dword of each section; first[n]: dwords of the tile
};
__host__ __device__ static constexpr tile_sections sections_of(int img) {
    switch (img) {
    case LY_P4K:
        return {LFAMD_TYPE_Q4_K, 2, {S_NIB, S_HDR}, {0, P4K_HDR / 4, P4K_TILE / 4}};
    case LY_P40: // (IQ4_NL, LY_P4N: the same image)
        return {LFAMD_TYPE_Q4_0, 2, {S_NIB, S_HDR}, {0, P4K_HDR / 4, P4K_TILE / 4}};
    case LY_PX4:
        return {LFAMD_TYPE_IQ4_XS, 2, {S_NIB, S_HDR}, {0, P4K_HDR / 4, P4K_TILE / 4}};
    case LY_P5K:
        return {LFAMD_TYPE_Q5_K, 3, {S_NIB, S_HDR, S_FIFTH}, {0, P5K_HDR / 4, P5K_QH / 4, P5K_TILE / 4}};
    case LY_PCL41: // (two header parts: d, m)
        return {LFAMD_TYPE_Q4_1, 3, {S_NIB, S_HDR, S_FIFTH}, {0, PCL_D / 4, PCL_QH / 4, PCL_TILE / 4}};
    case LY_PCL50:
        return {LFAMD_TYPE_Q5_0, 3, {S_NIB, S_HDR, S_FIFTH}, {0, PCL_D / 4, PCL_QH / 4, PCL_TILE / 4}};
    case LY_PCL51:
        return {LFAMD_TYPE_Q5_1, 3, {S_NIB, S_HDR, S_FIFTH}, {0, PCL_D / 4, PCL_QH / 4, PCL_TILE / 4}};
    case LY_PK2:
        return {LFAMD_TYPE_Q2_K, 3, {S_BIT2, S_HDR, S_ROW}, {0, PK2_SC / 4, PK2_D / 4, PK2_TILE / 4}};
    case LY_PK3:
        return {LFAMD_TYPE_Q3_K, 4, {S_BIT2, S_BIT3, S_HDR, S_ROW}, {0, PK3_HB / 4, PK3_SC / 4, PK3_D / 4, PK3_TILE / 4}};
    case IMG_PCK2: // (two header parts: scales, mins)
        return {LFAMD_TYPE_Q2_K, 3, {S_NIB, S_HDR, S_ROW}, {0, PCK_SC / 4, PCK_D / 4, PCK_TILE / 4}};
    case IMG_PCK3:
        return {LFAMD_TYPE_Q3_K, 3, {S_NIB, S_HDR, S_ROW}, {0, PCK_SC / 4, PCK_D / 4, PCK_TILE / 4}};
    case IMG_PC8:
        return {LFAMD_TYPE_IQ4_XS, 2, {S_BYTE, S_HDR}, {0, PC8_HDR / 4, PC8_TILE / 4}};
    default:
        return {0, 0, {}, {}};
    }
}

// Header word q of a row: q = 0..3, and 4..7 where the image has a second part.
//   P4K / P5K    the block's first 16 bytes {d, dmin, scales[12]}
//   P40 / PCL    d of the 32-blocks 2q, 2q + 1; second part (PCL): their m, zeros for the types without
//   PX4 / PC8    {8 int8 sub-block scales (ls - 32), f16 d, pad}
//   PK2          the block's scale bytes sc | mn << 4;  PK3: int8 6-bit scale - 32;  PCK: int8 scales, second part uint8 mins
template <int IMG>
__device__ static inline uint32_t hdr_word(const uint8_t *row, int b, int q, int kb) {
    constexpr int TYPE = sections_of(IMG).type, BS = gguf_block(TYPE);
    uint32_t v = 0;
    if constexpr (IMG == LY_P4K || IMG == LY_P5K) {
        // raw blocks are only 2-byte aligned in general (row strides are multiples of 144, so 4-byte here, but stay safe)
        const uint16_t *p = (const uint16_t *)(row + (size_t)b * BS + 4 * q);
        v = (uint32_t)p[0] | ((uint32_t)p[1] << 16);
    } else if constexpr (IMG == LY_P40 || IMG == LY_PCL41 || IMG == LY_PCL50 || IMG == LY_PCL51) {
        const int is_m = q >> 2, bl = b * 8 + 2 * (q & 3);
        if (!is_m || gguf_has_m(TYPE)) {
            const uint8_t *blk = row + (size_t)bl * BS + (is_m ? 2 : 0);
            const uint32_t lo = bl < kb ? *(const uint16_t *)blk : 0u, hi = bl + 1 < kb ? *(const uint16_t *)(blk + BS) : 0u;
            v = lo | (hi << 16);
        }
    } else if constexpr (IMG == LY_PX4 || IMG == IMG_PC8) {
        const lfamd_block_iq4_xs *blk = (const lfamd_block_iq4_xs *)row + b;
        if (q < 2) {
            for (int e = 0; e < 4; e++) {
                const int ib = 4 * q + e;
                const int ls = ((blk->scales_l[ib / 2] >> (4 * (ib % 2))) & 0xf) | (((blk->scales_h >> (2 * ib)) & 3) << 4);
                v |= (uint32_t)((ls - 32) & 0xff) << (8 * e);
            }
        } else if (q == 2) {
            v = blk->d;
        }
    } else {
        for (int e = 0; e < 4; e++) {
            int sc, mn;
            float d, dmin;
            scale16<TYPE>(row + (size_t)b * BS, 4 * (q & 3) + e, sc, mn, d, dmin);
            v |= (uint32_t)((IMG == LY_PK2 ? sc | (mn << 4) : q >= 4 ? mn : sc) & 0xff) << (8 * e);
        }
    }
    return v;
}
// PK2 / PK3 / PCK: {d, dmin} of the row's block (both were f16 in the block: exact round trip)
template <int IMG>
__device__ static inline uint32_t row_word(const uint8_t *row, int b) {
    constexpr int TYPE = sections_of(IMG).type;
    int sc, mn;
    float d, dmin;
    scale16<TYPE>(row + (size_t)b * gguf_block(TYPE), 0, sc, mn, d, dmin);
    return (uint32_t)f2h_bits(d) | ((uint32_t)f2h_bits(dmin) << 16);
}

// The lattice walk: the eight weights k = 16 t + 8 h + j of K-step t of lane half h; place(j, code) gives weight j's bits in the dword.
// (j stays a compile-time index: a position table indexed by a runtime j would go through scratch memory.)
template <int TYPE, class PLACE>
__device__ static inline uint32_t lat_walk(const uint8_t *row, int b, int kb, int t, int h, PLACE place) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
        v |= place(j, (uint32_t)gguf_code<TYPE>(row, b, 16 * t + 8 * h + j, kb));
    return v;
}
// bits (code >> lo) & mask of weight j at bit 4 NIBPOS(j) + at: the nibble section, PK2 / PK3's two- and third-bit sections
template <int TYPE>
__device__ static inline uint32_t lat_bits(const uint8_t *row, int b, int kb, int t, int h, int lo, uint32_t mask, int at) {
    return lat_walk<TYPE>(row, b, kb, t, h, [=](int j, uint32_t c) { return ((c >> lo) & mask) << (4 * NIBPOS(j) + at); });
}

// the rows of a tile: row i at base + i * stride, rows from n on lie past the matrix (zeros are written)
struct tile_rows {
    const uint8_t *base;
    size_t stride;
    int n;
    __device__ const uint8_t *operator()(int i) const {
        return base + (size_t)i * stride;
    }
};

// dword w of the tile, from section E on
template <int IMG, int E>
__device__ static inline uint32_t tile_dword(int w, const tile_rows &row, int b, int kb) {
    constexpr tile_sections S = sections_of(IMG);
    constexpr int TYPE = S.type;
    if constexpr (E == S.n) {
        return 0;
    } else {
        if (w >= S.first[E + 1])
            return tile_dword<IMG, E + 1>(w, row, b, kb);
        constexpr int KIND = S.kind[E];
        const int s = w - S.first[E];
        const int lane = (s >> 2) & 63, i = lane & 31, h = lane >> 5; // (all but S_BIT3, S_ROW)
        uint32_t v = 0;
        if constexpr (KIND == S_NIB) {
            if (const uint8_t *r = row(i); i < row.n)
                v = lat_bits<TYPE>(r, b, kb, 4 * (s >> 8) + (s & 3), h, 0, 15, 0);
        } else if constexpr (KIND == S_HDR) {
            if (const uint8_t *r = row(i); i < row.n)
                v = hdr_word<IMG>(r, b, 4 * (s >> 7) + (s & 3), kb);
        } else if constexpr (KIND == S_FIFTH) { // element j of K-step dd of group g = s & 3 at bit 4 q5hpos(j) + dd
            if (const uint8_t *r = row(i); i < row.n) {
#pragma unroll
                for (int dd = 0; dd < 4; dd++)
                    v |= lat_walk<TYPE>(r, b, kb, 4 * (s & 3) + dd, h, [=](int j, uint32_t c) { return (c >> 4) << (4 * q5hpos(j) + dd); });
            }
        } else if constexpr (KIND == S_BIT2) { // dword u of [gsel][lane]: K-steps 8 gsel + 2 u (bits 0-1 of a nibble) and + 1 (bits 2-3)
            if (const uint8_t *r = row(i); i < row.n)
                for (int e = 0; e < 2; e++)
                    v |= lat_bits<TYPE>(r, b, kb, 8 * (s >> 8) + 2 * (s & 3) + e, h, 0, 3, 2 * e);
        } else if constexpr (KIND == S_BIT3) { // dword x of [gsel][lane]: K-steps 8 gsel + 4 x + e at bit 4 NIBPOS(j) + e
            const int ln = (s >> 1) & 63;
            if (const uint8_t *r = row(ln & 31); (ln & 31) < row.n)
                for (int e = 0; e < 4; e++)
                    v |= lat_bits<TYPE>(r, b, kb, 8 * (s >> 7) + 4 * (s & 1) + e, ln >> 5, 2, 1, e);
        } else if constexpr (KIND == S_ROW) {
            if (const uint8_t *r = row(s); s < row.n)
                v = row_word<IMG>(r, b);
        } else { // S_BYTE: K-steps 2 g', 2 g' + 1 of the lane in 16 bytes; kvalues_iq4nl applied here, so the GEMM sees plain integers
            const int e = s & 3, t = 2 * (s >> 8) + (e >> 1);
            if (const uint8_t *r = row(i); i < row.n)
                for (int jj = 0; jj < 4; jj++) {
                    const int val = kvalues_iq4nl_dev[gguf_code<TYPE>(r, b, 16 * t + 8 * h + 4 * (e & 1) + jj, kb)];
                    v |= (uint32_t)((val + 128) & 0xff) << (8 * jj);
                }
        }
        return v;
    }
}

// One thread per output dword; every dword of every tile is written, zeros included.  nb: super-blocks of an image row.
template <int IMG>
__global__ void pack_tiles_kernel(const uint8_t *__restrict__ raw, size_t raw_row_bytes, long rows, int nb, int kb,
                                  uint8_t *__restrict__ out, long n_tiles) {
    constexpr int NDW = sections_of(IMG).first[sections_of(IMG).n];
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tile = tid / NDW;
    const int w = (int)(tid % NDW);
    if (tile >= n_tiles)
        return;
    const long rt = tile / nb;
    const int b = (int)(tile % nb);
    const long left = rows - rt * 32;
    const tile_rows row = {raw + rt * 32 * raw_row_bytes, raw_row_bytes, left < 32 ? (int)left : 32};
    ((uint32_t *)(out + tile * (NDW * 4)))[w] = tile_dword<IMG, 0>(w, row, b, kb);
}

// ---------------------------------------------------------------------------------------------
// Q6_K -> P6K: a kernel of its own.  As an instantiation of pack_tiles_kernel (sections: nibbles, upper two bits, scales, d) the
// image was the same, and the largest tensor of a model, 128256 x 4096, packed 0.9 % slower (473.8 us against 469.4:
// profiles/pack_images_q6k_writers.txt).  The nibble section is the lattice of lat_bits; the upper two bits sit at qhbit.
__global__ void pack_q6k_kernel(const uint8_t *__restrict__ raw, size_t raw_row_bytes, long rows, int nb,
                                uint8_t *__restrict__ out, long n_tiles) {
    long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // per tile: 1024 ql dwords + 512 qh dwords + 128 scale dwords + 16 d dwords = 1680 dwords
    long tile = tid / 1680;
    int w = (int)(tid % 1680);
    if (tile >= n_tiles)
        return;
    long rt = tile / nb;
    int b = (int)(tile % nb);
    uint32_t *dst = (uint32_t *)(out + tile * P6K_TILE);
    if (w < 1024) {
        int g = w >> 8, lane = (w >> 2) & 63, dd = w & 3;
        int i = lane & 31, h = lane >> 5;
        long row = rt * 32 + i;
        uint32_t v = 0;
        if (row < rows) {
            const lfamd_block_q6_K *blk = (const lfamd_block_q6_K *)(raw + row * raw_row_bytes) + b;
            int t = 4 * g + dd;
            for (int j = 0; j < 8; j++)
                v |= (uint32_t)(q6k_code(blk, 16 * t + 8 * h + j) & 15) << (4 * NIBPOS(j));
        }
        dst[w] = v;
    } else if (w < 1536) {
        int s = w - 1024;
        int gg = s >> 8, lane = (s >> 2) & 63, q = s & 3; // dword q of the lane's 16 B: group 2gg+(q>>1), pair e=q&1
        int i = lane & 31, h = lane >> 5;
        int g = 2 * gg + (q >> 1), e = q & 1;
        long row = rt * 32 + i;
        uint32_t v = 0;
        if (row < rows) {
            const lfamd_block_q6_K *blk = (const lfamd_block_q6_K *)(raw + row * raw_row_bytes) + b;
            for (int ab = 0; ab < 2; ab++) {
                int dd = 2 * e + ab, t = 4 * g + dd;
                for (int j = 0; j < 8; j++)
                    v |= (uint32_t)(q6k_code(blk, 16 * t + 8 * h + j) >> 4) << qhbit(dd, j);
            }
        }
        dst[w] = v;
    } else if (w < 1664) {
        int s = w - 1536;
        int i = s >> 2, q = s & 3;
        long row = rt * 32 + i;
        uint32_t v = 0;
        if (row < rows) {
            const lfamd_block_q6_K *blk = (const lfamd_block_q6_K *)(raw + row * raw_row_bytes) + b;
            const uint8_t *sc = (const uint8_t *)blk->scales + 4 * q;
            v = sc[0] | (sc[1] << 8) | (sc[2] << 16) | ((uint32_t)sc[3] << 24);
        }
        dst[w] = v;
    } else {
        int s = w - 1664; // 16 dwords = 32 f16
        uint32_t v = 0;
        for (int e = 0; e < 2; e++) {
            long row = rt * 32 + 2 * s + e;
            if (row < rows) {
                const lfamd_block_q6_K *blk = (const lfamd_block_q6_K *)(raw + row * raw_row_bytes) + b;
                v |= (uint32_t)blk->d << (16 * e);
            }
        }
        dst[w] = v;
    }
}
// ---------------------------------------------------------------------------------------------
// Q8_0 -> P80

__global__ void pack_q80_kernel(const uint8_t *__restrict__ raw, size_t raw_row_bytes, long rows, int nblocks,
                                int nquads, uint8_t *__restrict__ out, long n_tiles) {
    long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // per tile: 256 qs dwords + 16 scale dwords = 272 dwords
    long tile = tid / 272;
    int w = (int)(tid % 272);
    if (tile >= n_tiles)
        return;
    long rg = tile / nquads;
    int L = (int)(tile % nquads);
    uint32_t *dst = (uint32_t *)(out + tile * P80_TILE);
    if (w < 256) {
        int r = w >> 5, j = (w >> 2) & 7, dd = w & 3;
        long row = rg * 8 + r;
        int blk = 4 * L + dd;
        uint32_t v = 0;
        if (row < rows && blk < nblocks) {
            const lfamd_block_q8_0 *bp = (const lfamd_block_q8_0 *)(raw + row * raw_row_bytes) + blk;
            const uint8_t *q = (const uint8_t *)bp->qs + 4 * j;
            v = q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24);
        }
        dst[w] = v;
    } else {
        int s = w - 256; // 16 dwords = 32 f16 = d[r][dd]
        uint32_t v = 0;
        for (int e = 0; e < 2; e++) {
            int idx = 2 * s + e;
            int r = idx >> 2, dd = idx & 3;
            long row = rg * 8 + r;
            int blk = 4 * L + dd;
            if (row < rows && blk < nblocks) {
                const lfamd_block_q8_0 *bp = (const lfamd_block_q8_0 *)(raw + row * raw_row_bytes) + blk;
                v |= (uint32_t)bp->d << (16 * e);
            }
        }
        dst[w] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// RAW passthrough (row compaction): bytes copied row by row to stride = row_bytes.

__global__ void pack_raw_kernel(const uint8_t *__restrict__ raw, size_t raw_row_bytes, long rows, size_t row_bytes,
                                uint8_t *__restrict__ out) {
    size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)rows * row_bytes;
    for (; tid < total; tid += (size_t)gridDim.x * blockDim.x) {
        size_t r = tid / row_bytes, c = tid % row_bytes;
        out[tid] = raw[r * raw_row_bytes + c];
    }
}

// ---------------------------------------------------------------------------------------------
// Batches of Q2_K / Q3_K / IQ4_XS: the resident compact image -> the canonical image the MFMA body reads, into the caller's
// workspace (per call).

template <int TYPE>
__global__ void pk_expand_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long n_tiles) {
    constexpr bool Q3 = TYPE == LFAMD_TYPE_Q3_K;
    constexpr int TILE = Q3 ? PK3_TILE : PK2_TILE, SC0 = Q3 ? PK3_SC : PK2_SC, D0 = Q3 ? PK3_D : PK2_D;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tile = tid / (PCK_TILE / 4); // (the PCK sections of sections_of)
    const int w = (int)(tid % (PCK_TILE / 4));
    if (tile >= n_tiles)
        return;
    const uint8_t *src = in + tile * TILE;
    uint32_t *dst = (uint32_t *)(out + tile * PCK_TILE);
    uint32_t v;
    if (w < PCK_SC / 4) {
        const int g = w >> 8, lane = (w >> 2) & 63, dd = w & 3;
        const int t = 4 * g + dd, gsel = t >> 3, t8 = t & 7;
        const uint32_t c = *(const uint32_t *)(src + gsel * 1024 + lane * 16 + (t8 >> 1) * 4);
        v = ((t8 & 1) ? (c >> 2) : c) & 0x33333333u;
        if constexpr (Q3) {
            const uint32_t hb = *(const uint32_t *)(src + PK3_HB + gsel * 512 + lane * 8 + (t8 >> 2) * 4);
            v |= ((hb >> (t8 & 3)) & 0x11111111u) << 2;
        }
    } else if (w < PCK_D / 4) {
        const int s4 = w - PCK_SC / 4, mins = s4 >= 128;
        const int i = (s4 & 127) >> 2, u = s4 & 3;
        const uint32_t sb = *(const uint32_t *)(src + SC0 + i * 16 + u * 4);
        v = Q3 ? (mins ? 0u : sb) : (mins ? (sb >> 4) & 0x0F0F0F0Fu : sb & 0x0F0F0F0Fu);
    } else {
        v = *(const uint32_t *)(src + D0 + (w - PCK_D / 4) * 4);
    }
    dst[w] = v;
}

// batches: compact image -> the PC8 byte image (codebook value + 128) the MFMA body reads, per call, into the workspace
__global__ void pk4x_expand_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long n_tiles, long rows, int nb) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long tile = tid / (PC8_TILE / 4); // (the PC8 sections of sections_of)
    const int w = (int)(tid % (PC8_TILE / 4));
    if (tile >= n_tiles)
        return;
    const uint8_t *src = in + tile * P4K_TILE;
    uint32_t *dst = (uint32_t *)(out + tile * PC8_TILE);
    uint32_t v = 0;
    if (w < PC8_HDR / 4) {
        const int g2 = w >> 8, lane = (w >> 2) & 63, e = w & 3;
        const int t = 2 * g2 + (e >> 1);
        const uint32_t x = *(const uint32_t *)(src + (t >> 2) * 1024 + lane * 16 + (t & 3) * 4);
        if ((tile / nb) * 32 + (lane & 31) < rows) // (rows past the matrix: zero bytes, like the builder from GGUF rows)
        for (int jj = 0; jj < 4; jj++) {
            const int j = 4 * (e & 1) + jj;
            const int val = kvalues_iq4nl_dev[(x >> (4 * NIBPOS(j))) & 15];
            v |= (uint32_t)((val + 128) & 0xff) << (8 * jj);
        }
    } else {
        v = *(const uint32_t *)(src + P4K_HDR + (w - PC8_HDR / 4) * 4);
    }
    dst[w] = v;
}

// ---------------------------------------------------------------------------------------------
// Range check for the scaled-operand GEMM (gemm_lw.hip FAST): every row header of a P4K / P5K / P6K image; for Q8_0 every block
// scale of the P80 image that the f16 batch body (gemm_lf.hip) turns into f16(d * q).

__global__ void scaled_ok_kernel(const uint8_t *__restrict__ img, long tiles, int tile_bytes, int mode, int *__restrict__ bad) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; // (tile, row in tile) / P80: (tile, row r * 4 + block)
    if (idx >= tiles * 32)
        return;
    union {
        uint16_t u;
        _Float16 h;
    } d, dm;
    const uint8_t *tile = img + (size_t)(idx >> 5) * tile_bytes;
    if (mode == 2) { // f16(d * q), |q| <= 127 (padding scales are 0)
        d.u = *(const uint16_t *)(tile + P80_D + (idx & 31) * 2);
        if (!(fabsf((float)d.h) * 127.0f <= 65504.0f))
            atomicOr(bad, 1);
        return;
    }
    if (mode == 1) { // f16(d * sc) * (code - 32): |d| * 127 * 32 must stay inside f16
        d.u = *(const uint16_t *)(tile + P6K_D + (idx & 31) * 2);
        if (!(fabsf((float)d.h) * (127.0f * 32.0f) <= 65504.0f))
            atomicOr(bad, 1);
        return;
    }
    const uint32_t dd = *(const uint32_t *)(tile + P4K_HDR + (idx & 31) * 16);
    d.u = (uint16_t)(dd & 0xffff), dm.u = (uint16_t)(dd >> 16);
    const float fd = fabsf((float)d.h), fm = fabsf((float)dm.h);
    // the body forms S = f16(d * sc) and O = S * -1024 in f16 (q4_consts_pair_scaled): f16(|d| * 63) * 1024 must stay inside f16
    if (!((float)(_Float16)(fd * 63.0f) * 1024.0f <= 65504.0f) || !(fm * 63.0f <= 65504.0f)) // also catches NaN / inf
        atomicOr(bad, 1);
}

// ---------------------------------------------------------------------------------------------
// host-callable launchers and the sizes of the canonical images

// cols: of a GGUF row (the legacy types: whole 32-blocks; the image has ceil(cols / 256) super-blocks per row)
template <int IMG>
static hipError_t launch_tiles(const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s) {
    constexpr int NDW = sections_of(IMG).first[sections_of(IMG).n];
    const int nb = (int)((cols + 255) / 256), kb = (int)(cols / 32);
    const long n_tiles = ((rows + 31) / 32) * nb;
    if (n_tiles == 0)
        return hipSuccess;
    const long threads = n_tiles * NDW;
    pack_tiles_kernel<IMG><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>((const uint8_t *)raw, raw_row_bytes, rows, nb, kb, (uint8_t *)out,
                                                                            n_tiles);
    return hipGetLastError();
}

extern "C" {

hipError_t lfamd_launch_pack(const lfamd_image &im, const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s) {
    switch (im.ly) {
#define TILES(LY)                                                                                                                          \
    case LY:                                                                                                                               \
        return launch_tiles<LY>(raw, raw_row_bytes, rows, cols, out, s);
        TILES(LY_P4K)
        TILES(LY_P5K)
    case LY_P6K: {
        int nb = (int)(cols / 256);
        long n_tiles = ((rows + 31) / 32) * nb;
        long threads = n_tiles * 1680;
        pack_q6k_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>((const uint8_t *)raw, raw_row_bytes, rows, nb, (uint8_t *)out, n_tiles);
        return hipGetLastError();
    }
        TILES(LY_PK2)
        TILES(LY_PK3)
        TILES(LY_PX4)
        TILES(LY_PCL41)
        TILES(LY_PCL50)
        TILES(LY_PCL51)
    case LY_P4N:
        TILES(LY_P40)
#undef TILES
    case LY_P80: {
        int nblocks = (int)(cols / 32);
        int nquads = (nblocks + 3) / 4;
        long n_tiles = ((rows + 7) / 8) * nquads;
        long threads = n_tiles * 272;
        pack_q80_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>((const uint8_t *)raw, raw_row_bytes, rows, nblocks,
                                                                            nquads, (uint8_t *)out, n_tiles);
        return hipGetLastError();
    }
    case LY_NONE:
        return hipErrorInvalidValue;
    default: { // GGUF rows
        const size_t row_bytes = lfamd_row_size(im.type, cols);
        size_t total = (size_t)rows * row_bytes;
        size_t blocks = (total + 255) / 256;
        if (blocks > 65536)
            blocks = 65536;
        if (blocks == 0)
            return hipSuccess;
        pack_raw_kernel<<<(unsigned)blocks, 256, 0, s>>>((const uint8_t *)raw, raw_row_bytes, rows, row_bytes, (uint8_t *)out);
        return hipGetLastError();
    }
    }
}

// the canonical images from GGUF rows: what the expanders below give from the resident compact images (tests/test_gpu_pack.py)
size_t lfamd_wprep16_bytes(long rows, long cols) {
    return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * PCK_TILE;
}
hipError_t lfamd_launch_wprep16(int type, const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s) {
    if (type == LFAMD_TYPE_Q2_K)
        return launch_tiles<IMG_PCK2>(raw, raw_row_bytes, rows, cols, out, s);
    if (type == LFAMD_TYPE_Q3_K)
        return launch_tiles<IMG_PCK3>(raw, raw_row_bytes, rows, cols, out, s);
    return hipErrorInvalidValue;
}
size_t lfamd_wprep8_bytes(long rows, long cols) {
    return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * PC8_TILE;
}
hipError_t lfamd_launch_wprep8(int type, const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s) {
    if (type != LFAMD_TYPE_IQ4_XS)
        return hipErrorInvalidValue;
    return launch_tiles<IMG_PC8>(raw, raw_row_bytes, rows, cols, out, s);
}

hipError_t lfamd_launch_pk4x_expand(const void *packed, long rows, long cols, void *out, hipStream_t s) {
    const long n_tiles = ((rows + 31) / 32) * (cols / 256);
    if (n_tiles == 0)
        return hipSuccess;
    const long threads = n_tiles * (PC8_TILE / 4);
    pk4x_expand_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>((const uint8_t *)packed, (uint8_t *)out, n_tiles, rows, (int)(cols / 256));
    return hipGetLastError();
}

hipError_t lfamd_launch_pk_expand(int type, const void *packed, long rows, long cols, void *out, hipStream_t s) {
    const long n_tiles = ((rows + 31) / 32) * (cols / 256);
    if (n_tiles == 0)
        return hipSuccess;
    const long threads = n_tiles * (PCK_TILE / 4);
    const unsigned grid = (unsigned)((threads + 255) / 256);
    if (type == LFAMD_TYPE_Q2_K)
        pk_expand_kernel<LFAMD_TYPE_Q2_K><<<grid, 256, 0, s>>>((const uint8_t *)packed, (uint8_t *)out, n_tiles);
    else if (type == LFAMD_TYPE_Q3_K)
        pk_expand_kernel<LFAMD_TYPE_Q3_K><<<grid, 256, 0, s>>>((const uint8_t *)packed, (uint8_t *)out, n_tiles);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t lfamd_launch_scaled_ok(int type, long rows, long cols, const void *packed, int *d_flag, hipStream_t s) {
    const lfamd_image im = lfamd_image_of(type, cols); // (Q4_K, Q5_K, Q6_K or Q8_0: api.hip)
    const long tiles = (long)im.tiles(rows);
    const long threads = tiles * 32;
    scaled_ok_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>((const uint8_t *)packed, tiles, im.tile,
                                                                       im.ly == LY_P80 ? 2 : im.ly == LY_P6K ? 1 : 0, d_flag);
    return hipGetLastError();
}
}
