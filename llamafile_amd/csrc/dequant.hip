// dequant.hip — the READ side of the resident weight images: rows of a packed matrix as F32 / F16 (GGML_OP_GET_ROWS and the
// to_fp16 / to_fp32 converters of the reference's GPU module, ggml-cuda.cu.patch:10687-10860, 3929-4040), and the image back to
// GGUF rows byte for byte (its buffer_get_tensor, :16890-17027).  Nothing here writes an image: pack.hip does; which image a type has: lfamd_internal.h.
//
// ARITHMETIC.  Exactly oracle/oracle.c: ora_dequantize_row, in f32, in this order and with no contraction:
//   K-quants, IQ4_XS   ((d * (float)sc) * (float)q) - (dmin * (float)mn)        (dmin = +0, mn = 0 where the type has no mins)
//   32-blocks          (d * (float)q) + m                                        (m = +0 where the type has none; IQ4_NL: q = kvalue[index])
// The "+ m" with m = +0 is NOT dropped: it turns a -0 product (q = 0 under a negative d) into the +0 the reference gives.  A fused
// multiply-add would skip the rounding of the product, so this file must be built with -ffp-contract=off (the Makefile's HIPFLAGS);
// the pragma below states it here too, so that the file does not depend on the flag silently.
// Values come from the CODES and the file's own d / dmin / m / integer scales.  Fields an image keeps only for the mat-mul bodies
// are read where they are the file's integers unchanged (PK3's and IQ4_XS's int8 scales ARE the oracle's sc = 6-bit value - 32) and
// ignored where they are not part of the file (PCL's m slot of Q5_0, which that type does not have).
// F16 output: the f32 value rounded to nearest-even by v_cvt_f16_f32 (subnormals kept, overflow to inf).
//
// MAPPING.  One wave per (row, 256 weights); lane L owns weights 4L .. 4L+3, so a wave writes one contiguous
// run of 1 KiB (F32) or 512 B (F16) with one 16 / 8-byte store per lane.  On the nibble lattice shared by P4K / P5K / P6K / P40 /
// PK2 / PK3 / IQ4_XS / PCL those four weights sit in ONE dword of the lane-order fragment of lane (i = row % 32, h): K-step
// t = L / 4, h = (L / 2) % 2, nibbles j = 4 (L % 2) .. + 3.  A row's share of a 32-row tile is eight 16-byte fragments; the four
// lanes that share a fragment read its four dwords, so the wave's load touches exactly those 128 bytes.  A work-group takes `rpb`
// consecutive row slots of one super-block column: 32 for ranges of rows, so that the tile's every byte is fetched from HBM once
// and the 31 later rows hit the caches; 4 (one per wave) for index lists, so that a handful of indices still spreads over the chip.
#include "lfamd_device.h"
#include "../../include/lfamd_hip.h"
#include "lfamd_internal.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// layout traits (tile bytes: lfamd_ly_tile, lfamd_internal.h): the arithmetic forms of lfamd_device.h's position tables (NIBPOS, q5hpos, qhbit) — the tables
// themselves are arrays, and an array indexed by a lane-dependent j would go through scratch memory.

__host__ __device__ static constexpr int ly_raw_block(int ly) { // bytes of one 32-block of the RAW legacy layouts
    return ly == LY_RAW40 || ly == LY_RAW4N ? 18 : ly == LY_RAW41 ? 20 : ly == LY_RAW50 ? 22 : ly == LY_RAW51 ? 24 : 0;
}

__device__ static inline int nibpos(int j) {
    return (j >> 1) + 4 * (j & 1);
}
__device__ static inline int q5pos(int j) { // q5hpos: {1, 5, 2, 6, 3, 7, 0, 4}
    return (int)(0x40736251u >> (4 * j)) & 7;
}
__device__ static inline int qhbit_a(int dd, int j) { // qhbit: field {2, 4, 6, 0}[j >> 1] + (dd & 1)
    return 16 * (j & 1) + 2 * (((2 * (j >> 1) + 2) & 7) + (dd & 1));
}

__device__ static inline uint32_t ld32(const uint8_t *p) {
    return *(const uint32_t *)p;
}
__device__ static inline uint32_t ld16(const uint8_t *p) {
    return *(const uint16_t *)p;
}

__constant__ static const int8_t kvalues_iq4nl_dq[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};

// the dword of K-step t of lane (i, h) on the P4K nibble lattice; element j at bit 4 NIBPOS(j)
__device__ static inline uint32_t lat_dword(const uint8_t *tile, int i, int t, int h) {
    return ld32(tile + (t >> 2) * 1024 + (h * 32 + i) * 16 + (t & 3) * 4);
}
// Q5_K / PCL fifth bits (plane at `qh`): one dword per (lane, group g), element j of K-step dd at bit 4 q5hpos(j) + dd
__device__ static inline uint32_t fifth_dword(const uint8_t *qh, int i, int t, int h) {
    return ld32(qh + ((h * 32 + i) * 4 + (t >> 2)) * 4);
}
// P6K upper two bits: 2 x 64 lanes x 16 B; dword q of lane's 16 B = group 2 gg + (q >> 1), K-step pair q & 1
__device__ static inline uint32_t q6h_dword(const uint8_t *tile, int i, int t, int h) {
    const int g = t >> 2, dd = t & 3;
    return ld32(tile + P6K_QH + (g >> 1) * 1024 + (h * 32 + i) * 16 + ((g & 1) * 2 + (dd >> 1)) * 4);
}
// PK2 / PK3 two-bit codes: K-steps 2u, 2u+1 of an eight-step half folded into one dword (bits 0-1 / 2-3 of every nibble)
__device__ static inline uint32_t pk_dword(const uint8_t *tile, int i, int t, int h) {
    return ld32(tile + (t >> 3) * 1024 + (h * 32 + i) * 16 + ((t & 7) >> 1) * 4);
}
// PK3 third bits: dword x of [gsel][lane] = K-steps 8 gsel + 4 x + s at bit 4 NIBPOS(j) + s
__device__ static inline uint32_t pk3_dword(const uint8_t *tile, int i, int t, int h) {
    return ld32(tile + PK3_HB + (t >> 3) * 512 + (h * 32 + i) * 8 + ((t & 7) >> 2) * 4);
}

// integer code (as stored, before the type's offset) of weight k (0..255) of row i of a lattice tile
template <int LY>
__device__ static inline int tile_code(const uint8_t *tile, int i, int k) {
    const int t = k >> 4, h = (k >> 3) & 1, j = k & 7;
    if constexpr (LY == LY_PK2 || LY == LY_PK3) {
        int c = (pk_dword(tile, i, t, h) >> (4 * nibpos(j) + 2 * (t & 1))) & 3;
        if constexpr (LY == LY_PK3)
            c |= ((pk3_dword(tile, i, t, h) >> (4 * nibpos(j) + (t & 3))) & 1) << 2;
        return c;
    } else {
        int c = (lat_dword(tile, i, t, h) >> (4 * nibpos(j))) & 15;
        if constexpr (LY == LY_P5K)
            c |= ((fifth_dword(tile + P5K_QH, i, t, h) >> (4 * q5pos(j) + (t & 3))) & 1) << 4;
        if constexpr (LY == LY_PCL50 || LY == LY_PCL51)
            c |= ((fifth_dword(tile + PCL_QH, i, t, h) >> (4 * q5pos(j) + (t & 3))) & 1) << 4;
        if constexpr (LY == LY_P6K)
            c |= ((q6h_dword(tile, i, t, h) >> qhbit_a(t & 3, j)) & 3) << 4;
        return c;
    }
}

// ---------------------------------------------------------------------------------------------
// (a) four consecutive weights col .. col + 3 (col = 256 b + 4 L) of row `row`, in the oracle's arithmetic

__device__ static inline float kq_value(float d, int sc, int q, float dmin, int mn) {
    const float dl = d * (float)sc;
    const float p = dl * (float)q;
    const float ml = dmin * (float)mn;
    return p - ml;
}
__device__ static inline float lq_value(float d, int q, float m) {
    const float p = d * (float)q;
    return p + m;
}

template <int LY>
__device__ static inline void decode4(const uint8_t *__restrict__ img, long row, long cols, int nb, int b, int L, float v[4]) {
    const int t = L >> 2, h = (L >> 1) & 1, j0 = (L & 1) * 4, i = (int)(row & 31);
    if constexpr (LY == LY_P4K || LY == LY_P5K) {
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * lfamd_ly_tile(LY);
        const uint32_t x = lat_dword(tile, i, t, h);
        const uint4 H = *(const uint4 *)(tile + P4K_HDR + i * 16); // {d, dmin, scales[12]} as in the file
        uint32_t sc03, sc47, mn03, mn47;
        q4k_scales_bytes(H.y, H.z, H.w, sc03, sc47, mn03, mn47); // get_scale_min_k4 on all eight sub-blocks
        const int sub = L >> 3, sh = 8 * (sub & 3);
        const int sc = (int)(((sub < 4 ? sc03 : sc47) >> sh) & 0xff), mn = (int)(((sub < 4 ? mn03 : mn47) >> sh) & 0xff);
        const float d = h2f((uint16_t)H.x), dmin = h2f((uint16_t)(H.x >> 16));
        uint32_t f = 0;
        if constexpr (LY == LY_P5K)
            f = fifth_dword(tile + P5K_QH, i, t, h) >> (t & 3);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            int q = (int)(x >> (4 * nibpos(j0 + e))) & 15;
            if constexpr (LY == LY_P5K)
                q |= (int)((f >> (4 * q5pos(j0 + e))) & 1) << 4;
            v[e] = kq_value(d, sc, q, dmin, mn);
        }
    } else if constexpr (LY == LY_P6K) {
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * P6K_TILE;
        const uint32_t x = lat_dword(tile, i, t, h), y = q6h_dword(tile, i, t, h);
        const int sc = (int)(int8_t)tile[P6K_SC + i * 16 + t];
        const float d = h2f((uint16_t)ld16(tile + P6K_D + i * 2));
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int c = ((int)(x >> (4 * nibpos(j0 + e))) & 15) | (((int)(y >> qhbit_a(t & 3, j0 + e)) & 3) << 4);
            v[e] = kq_value(d, sc, c - 32, 0.0f, 0);
        }
    } else if constexpr (LY == LY_PK2 || LY == LY_PK3) {
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * lfamd_ly_tile(LY);
        const uint32_t x = pk_dword(tile, i, t, h) >> (2 * (t & 1));
        if constexpr (LY == LY_PK2) {
            const int sb = tile[PK2_SC + i * 16 + t]; // the block's scale byte: scale | min << 4
            const uint32_t dm = ld32(tile + PK2_D + i * 4);
            const float d = h2f((uint16_t)dm), dmin = h2f((uint16_t)(dm >> 16));
#pragma unroll
            for (int e = 0; e < 4; e++)
                v[e] = kq_value(d, sb & 15, (int)(x >> (4 * nibpos(j0 + e))) & 3, dmin, sb >> 4);
        } else {
            const uint32_t y = pk3_dword(tile, i, t, h) >> (t & 3);
            const int sc = (int)(int8_t)tile[PK3_SC + i * 16 + t]; // 6-bit scale - 32: the oracle's integer sc
            const float d = h2f((uint16_t)ld32(tile + PK3_D + i * 4));
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int c = ((int)(x >> (4 * nibpos(j0 + e))) & 3) | (((int)(y >> (4 * nibpos(j0 + e))) & 1) << 2);
                v[e] = kq_value(d, sc, c - 4, 0.0f, 0);
            }
        }
    } else if constexpr (LY == LY_PX4) {
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * P4K_TILE;
        const uint32_t x = lat_dword(tile, i, t, h);
        const uint8_t *hdr = tile + P4K_HDR + i * 16; // {8 int8 scales (ls - 32), f16 d, pad}
        const int sc = (int)(int8_t)hdr[L >> 3];
        const float d = h2f((uint16_t)ld16(hdr + 8));
#pragma unroll
        for (int e = 0; e < 4; e++)
            v[e] = kq_value(d, sc, (int)kvalues_iq4nl_dq[(x >> (4 * nibpos(j0 + e))) & 15], 0.0f, 0);
    } else if constexpr (LY == LY_P40 || LY == LY_P4N || LY == LY_PCL41 || LY == LY_PCL50 || LY == LY_PCL51) {
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * lfamd_ly_tile(LY);
        const uint32_t x = lat_dword(tile, i, t, h);
        const int bl = L >> 3; // 32-block of the 256-weight group
        const float d = h2f((uint16_t)ld16(tile + P4K_HDR + i * 16 + bl * 2)); // (PCL_D == P4K_HDR)
        float m = 0.0f;
        if constexpr (LY == LY_PCL41 || LY == LY_PCL51)
            m = h2f((uint16_t)ld16(tile + PCL_M + i * 16 + bl * 2));
        uint32_t f = 0;
        if constexpr (LY == LY_PCL50 || LY == LY_PCL51)
            f = fifth_dword(tile + PCL_QH, i, t, h) >> (t & 3);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            int q = (int)(x >> (4 * nibpos(j0 + e))) & 15;
            if constexpr (LY == LY_PCL50 || LY == LY_PCL51)
                q |= (int)((f >> (4 * q5pos(j0 + e))) & 1) << 4;
            if constexpr (LY == LY_P40)
                q -= 8;
            if constexpr (LY == LY_P4N)
                q = (int)kvalues_iq4nl_dq[q];
            if constexpr (LY == LY_PCL50)
                q -= 16;
            v[e] = lq_value(d, q, m);
        }
    } else if constexpr (LY == LY_P80) {
        const int nq = (int)((cols / 32 + 3) / 4), blk = b * 8 + (L >> 3), r = (int)(row & 7), dd = blk & 3;
        const uint8_t *tile = img + ((size_t)(row >> 3) * nq + (blk >> 2)) * P80_TILE;
        const uint32_t x = ld32(tile + r * 128 + (L & 7) * 16 + dd * 4);
        const float d = h2f((uint16_t)ld16(tile + P80_D + (r * 4 + dd) * 2));
#pragma unroll
        for (int e = 0; e < 4; e++)
            v[e] = lq_value(d, (int)(int8_t)(x >> (8 * e)), 0.0f);
    } else if constexpr (LY == LY_RAW40 || LY == LY_RAW41 || LY == LY_RAW50 || LY == LY_RAW51 || LY == LY_RAW4N) {
        constexpr int BS = ly_raw_block(LY);
        constexpr bool HAS_M = LY == LY_RAW41 || LY == LY_RAW51, HAS_H = LY == LY_RAW50 || LY == LY_RAW51;
        constexpr int QH_OFF = HAS_M ? 4 : 2, QS_OFF = QH_OFF + (HAS_H ? 4 : 0);
        const uint8_t *blk = img + (size_t)row * (size_t)(cols / 32) * BS + (size_t)(b * 8 + (L >> 3)) * BS;
        const int l = (L & 7) * 4; // weight l of a block: low nibble of qs[l] (l < 16) or high nibble of qs[l - 16], fifth bit = bit l of qh
        const float d = h2f((uint16_t)ld16(blk));
        float m = 0.0f;
        if constexpr (HAS_M)
            m = h2f((uint16_t)ld16(blk + 2));
        uint32_t f = 0;
        if constexpr (HAS_H)
            f = (ld16(blk + QH_OFF) | (ld16(blk + QH_OFF + 2) << 16)) >> l;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint8_t byte = blk[QS_OFF + (l & 15) + e];
            int q = l < 16 ? (byte & 15) : (byte >> 4);
            if constexpr (HAS_H)
                q |= (int)((f >> e) & 1) << 4;
            if constexpr (LY == LY_RAW40)
                q -= 8;
            if constexpr (LY == LY_RAW4N)
                q = (int)kvalues_iq4nl_dq[q];
            if constexpr (LY == LY_RAW50)
                q -= 16;
            v[e] = lq_value(d, q, m);
        }
    } else { // float rows: exact conversions (element guard: cols need not be a multiple of four)
        const long col = (long)b * 256 + 4 * L;
        const uint8_t *r = img + (size_t)row * (size_t)cols * (LY == LY_F32 ? 4 : 2);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            v[e] = 0.0f;
            if (col + e < cols) {
                if constexpr (LY == LY_F32)
                    v[e] = ((const float *)r)[col + e];
                else if constexpr (LY == LY_F16)
                    v[e] = h2f(((const uint16_t *)r)[col + e]);
                else
                    v[e] = __builtin_bit_cast(float, (uint32_t)((const uint16_t *)r)[col + e] << 16);
            }
        }
    }
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

// f32 -> output element.  F16: round to nearest-even with v_cvt_f16_f32.  The conversion must see the f32 VALUE: written as a plain cast
// of a product, the compiler selects v_fma_mixlo_f16 (a * b + 0, rounded to f16), and the "+ 0" turns a -0 product into +0.  The
// canonicalize (the identity on every value that is not a signalling NaN, and free after a multiply) keeps the two apart;
// tests/test_gpu_get_rows.py compares negative zeros in F16 and fails if the fused form comes back.
template <typename OutT>
__device__ static inline OutT to_out(float v) {
    if constexpr (sizeof(OutT) == 4)
        return v;
    else
        return (_Float16)__builtin_elementwise_canonicalize(v);
}

// grid: (row-slot chunk, super-block column b), flattened with b fastest: consecutive work-groups walk one row of tiles, which is
// contiguous in the image, and write neighbouring 1 KiB runs of the same output rows.
// vec: the output base and row stride are 16-byte multiples (whole 16 / 8-byte stores); otherwise element stores.
template <int LY, typename OutT>
__global__ __launch_bounds__(256) void get_rows_kernel(const uint8_t *__restrict__ img, long rows, long cols, int nb,
                                                       const int32_t *__restrict__ ids, long row0, long n_ids, int rpb,
                                                       uint8_t *__restrict__ out, size_t out_row_bytes, int vec) {
    const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
    const long chunk = blockIdx.x / nb;
    const int b = (int)(blockIdx.x % nb);
    const long col = (long)b * 256 + 4 * L;
    if (col >= cols)
        return;
    for (int s = wave; s < rpb; s += 4) {
        const long slot = chunk * rpb + s;
        if (slot >= n_ids)
            break;
        const long row = ids ? (long)ids[slot] : row0 + slot;
        if (row < 0 || row >= rows) // like an out-of-range expert id of lfamd_mul_mat_id: the output row stays untouched
            continue;
        float v[4];
        decode4<LY>(img, row, cols, nb, b, L, v);
        OutT *o = (OutT *)(out + (size_t)slot * out_row_bytes) + col;
        if (vec && col + 4 <= cols) {
            if constexpr (sizeof(OutT) == 4) {
                const f32x4_t w = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(w, (f32x4_t *)o);
            } else {
                const f16x4_t w = {to_out<OutT>(v[0]), to_out<OutT>(v[1]), to_out<OutT>(v[2]), to_out<OutT>(v[3])};
                __builtin_nontemporal_store(w, (f16x4_t *)o);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (col + e < cols)
                    o[e] = to_out<OutT>(v[e]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// (b) unpack: byte `o` of the GGUF row `row`, gathered from the image.  One thread per output byte: neighbouring threads write
// neighbouring bytes, and the 32 rows of a tile are neighbouring work-groups, so the tile is fetched once and re-read from the caches.
// Every image determines the file's bytes: codes and file headers are stored as they are or as a bijection of them —
//   PK3: the sixteen int8 (6-bit scale - 32) -> scales[12] by the inverse of the oracle's unpack_q3_K split (low nibbles of scales 0-7
//        in bytes 0-7's low halves, of scales 8-15 in their high halves, the upper two bits of scale 4u + m in bits 2u of byte 8 + m);
//   IQ4_XS: the eight int8 (ls - 32) -> scales_l nibbles and scales_h bit pairs;  PCL: d, m, nibbles and fifth bits as stored.
// (PK2 / PK3 keep d and dmin as f16(f32(f16)): identical bits for every value but a signalling NaN, which comes back quiet.)

template <int TYPE>
__device__ static inline uint8_t raw_byte(const uint8_t *__restrict__ img, long row, long cols, int nb, long o) {
    const int i = (int)(row & 31);
    if constexpr (TYPE == LFAMD_TYPE_Q4_K || TYPE == LFAMD_TYPE_Q5_K) {
        constexpr int LY = TYPE == LFAMD_TYPE_Q4_K ? LY_P4K : LY_P5K;
        constexpr int BS = TYPE == LFAMD_TYPE_Q4_K ? 144 : 176, QS = BS - 128;
        const int b = (int)(o / BS), p = (int)(o % BS);
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * lfamd_ly_tile(LY);
        if (p < 16)
            return tile[P4K_HDR + i * 16 + p];
        if (p < QS) { // Q5_K qh[l]: bit s = fifth bit of weight 32 s + l
            const int l = p - 16;
            int v = 0;
            for (int s = 0; s < 8; s++)
                v |= (tile_code<LY>(tile, i, 32 * s + l) >> 4) << s;
            return (uint8_t)v;
        }
        const int c = (p - QS) >> 5, l = (p - QS) & 31;
        return (uint8_t)((tile_code<LY>(tile, i, 64 * c + l) & 15) | ((tile_code<LY>(tile, i, 64 * c + 32 + l) & 15) << 4));
    } else if constexpr (TYPE == LFAMD_TYPE_Q6_K) {
        const int b = (int)(o / 210), p = (int)(o % 210);
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * P6K_TILE;
        if (p < 128) {
            const int n = p >> 6, q = (p >> 5) & 1, l = p & 31;
            return (uint8_t)((tile_code<LY_P6K>(tile, i, 128 * n + 32 * q + l) & 15) |
                             ((tile_code<LY_P6K>(tile, i, 128 * n + 32 * (q + 2) + l) & 15) << 4));
        }
        if (p < 192) {
            const int n = (p - 128) >> 5, l = (p - 128) & 31;
            int v = 0;
            for (int q = 0; q < 4; q++)
                v |= (tile_code<LY_P6K>(tile, i, 128 * n + 32 * q + l) >> 4) << (2 * q);
            return (uint8_t)v;
        }
        if (p < 208)
            return tile[P6K_SC + i * 16 + (p - 192)];
        return tile[P6K_D + i * 2 + (p - 208)];
    } else if constexpr (TYPE == LFAMD_TYPE_Q2_K) {
        const int b = (int)(o / 84), p = (int)(o % 84);
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * PK2_TILE;
        if (p < 16)
            return tile[PK2_SC + i * 16 + p];
        if (p < 80) {
            const int n = (p - 16) >> 5, l = (p - 16) & 31;
            int v = 0;
            for (int q = 0; q < 4; q++)
                v |= tile_code<LY_PK2>(tile, i, 128 * n + 32 * q + l) << (2 * q);
            return (uint8_t)v;
        }
        return tile[PK2_D + i * 4 + (p - 80)];
    } else if constexpr (TYPE == LFAMD_TYPE_Q3_K) {
        const int b = (int)(o / 110), p = (int)(o % 110);
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * PK3_TILE;
        if (p < 32) { // hmask[l]: bit 4 n + j = third bit of the stored code (q + 4) of weight 128 n + 32 j + l
            int v = 0;
            for (int s = 0; s < 8; s++)
                v |= (tile_code<LY_PK3>(tile, i, 32 * s + p) >> 2) << s;
            return (uint8_t)v;
        }
        if (p < 96) {
            const int n = (p - 32) >> 5, l = (p - 32) & 31;
            int v = 0;
            for (int q = 0; q < 4; q++)
                v |= (tile_code<LY_PK3>(tile, i, 128 * n + 32 * q + l) & 3) << (2 * q);
            return (uint8_t)v;
        }
        const uint8_t *sc = tile + PK3_SC + i * 16; // int8 = us - 32
        if (p < 104) {
            const int m = p - 96;
            return (uint8_t)((((int)(int8_t)sc[m] + 32) & 15) | ((((int)(int8_t)sc[m + 8] + 32) & 15) << 4));
        }
        if (p < 108) {
            const int m = p - 104;
            int v = 0;
            for (int u = 0; u < 4; u++)
                v |= ((((int)(int8_t)sc[4 * u + m] + 32) >> 4) & 3) << (2 * u);
            return (uint8_t)v;
        }
        return tile[PK3_D + i * 4 + (p - 108)];
    } else if constexpr (TYPE == LFAMD_TYPE_IQ4_XS) {
        const int b = (int)(o / 136), p = (int)(o % 136);
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * P4K_TILE;
        const uint8_t *hdr = tile + P4K_HDR + i * 16;
        if (p < 2)
            return hdr[8 + p];
        if (p < 4) { // scales_h: bits 2 ib = ls >> 4
            int v = 0;
            for (int u = 0; u < 4; u++)
                v |= ((((int)(int8_t)hdr[4 * (p - 2) + u] + 32) >> 4) & 3) << (2 * u);
            return (uint8_t)v;
        }
        if (p < 8) {
            const int m = p - 4;
            return (uint8_t)((((int)(int8_t)hdr[2 * m] + 32) & 15) | ((((int)(int8_t)hdr[2 * m + 1] + 32) & 15) << 4));
        }
        const int ib = (p - 8) >> 4, l = (p - 8) & 15;
        return (uint8_t)(tile_code<LY_PX4>(tile, i, 32 * ib + l) | (tile_code<LY_PX4>(tile, i, 32 * ib + 16 + l) << 4));
    } else if constexpr (TYPE == LFAMD_TYPE_Q4_0 || TYPE == LFAMD_TYPE_Q4_1 || TYPE == LFAMD_TYPE_Q5_0 || TYPE == LFAMD_TYPE_Q5_1) {
        constexpr int LY = TYPE == LFAMD_TYPE_Q4_0 ? LY_P40 : TYPE == LFAMD_TYPE_Q4_1 ? LY_PCL41 : TYPE == LFAMD_TYPE_Q5_0 ? LY_PCL50 : LY_PCL51;
        constexpr bool HAS_M = TYPE == LFAMD_TYPE_Q4_1 || TYPE == LFAMD_TYPE_Q5_1, HAS_H = TYPE == LFAMD_TYPE_Q5_0 || TYPE == LFAMD_TYPE_Q5_1;
        constexpr int QH_OFF = HAS_M ? 4 : 2, QS_OFF = QH_OFF + (HAS_H ? 4 : 0), BS = QS_OFF + 16;
        const int blk = (int)(o / BS), p = (int)(o % BS), b = blk >> 3, bl = blk & 7;
        const uint8_t *tile = img + ((size_t)(row >> 5) * nb + b) * lfamd_ly_tile(LY);
        if (p < 2)
            return tile[P4K_HDR + i * 16 + bl * 2 + p];
        if (HAS_M && p < 4)
            return tile[PCL_M + i * 16 + bl * 2 + (p - 2)];
        if (p < QS_OFF) { // qh byte: bit e = fifth bit of weight 8 (p - QH_OFF) + e of the block
            int v = 0;
            for (int e = 0; e < 8; e++)
                v |= (tile_code<LY>(tile, i, 32 * bl + 8 * (p - QH_OFF) + e) >> 4) << e;
            return (uint8_t)v;
        }
        const int l = p - QS_OFF;
        return (uint8_t)((tile_code<LY>(tile, i, 32 * bl + l) & 15) | ((tile_code<LY>(tile, i, 32 * bl + 16 + l) & 15) << 4));
    } else { // Q8_0
        const int blk = (int)(o / 34), p = (int)(o % 34), r = (int)(row & 7), dd = blk & 3;
        const uint8_t *tile = img + ((size_t)(row >> 3) * nb + (blk >> 2)) * P80_TILE; // (nb: quads per row here)
        if (p < 2)
            return tile[P80_D + (r * 4 + dd) * 2 + p];
        return tile[r * 128 + ((p - 2) >> 2) * 16 + dd * 4 + ((p - 2) & 3)];
    }
}

template <int TYPE>
__global__ __launch_bounds__(256) void unpack_kernel(const uint8_t *__restrict__ img, long cols, int nb, size_t row_bytes,
                                                     uint8_t *__restrict__ raw, size_t raw_row_bytes) {
    const long row = blockIdx.x;
    const size_t o = (size_t)blockIdx.y * 256 + threadIdx.x;
    if (o < row_bytes)
        raw[(size_t)row * raw_row_bytes + o] = raw_byte<TYPE>(img, row, cols, nb, (long)o);
}

// RAW images: the rows back at the caller's stride
__global__ __launch_bounds__(256) void unpack_raw_kernel(const uint8_t *__restrict__ img, size_t row_bytes, uint8_t *__restrict__ raw,
                                                         size_t raw_row_bytes) {
    const long row = blockIdx.x;
    const size_t o = (size_t)blockIdx.y * 256 + threadIdx.x;
    if (o < row_bytes)
        raw[(size_t)row * raw_row_bytes + o] = img[(size_t)row * row_bytes + o];
}

// ---------------------------------------------------------------------------------------------

// rows per work-group: a whole tile's 32 rows for a range of rows (every image byte from HBM once), one row per wave for an index
// list or a range shorter than a tile (1 index x 16 super-blocks = 16 work-groups, 512 indices = 2048)
static int rows_per_group(const int32_t *ids, long n_ids) {
    return !ids && n_ids >= 32 ? 32 : 4;
}

// im: lfamd_image_of(the call's type id, cols).  cols: the columns read back.  A 32-block type's tile image may have more (im.cols: its
// last super-block is padded with zero blocks); the kernels' column guards stop at cols, so nothing of the padding is written out.
extern "C" hipError_t lfamd_launch_get_rows(const lfamd_image &im, const void *img, long rows, long cols, const int32_t *ids, long row0, long n_ids,
                                            int out_type, void *out, size_t out_row_bytes, hipStream_t s) {
    const int ly = im.ly;
    if (ly == LY_NONE || (out_type != LFAMD_TYPE_F32 && out_type != LFAMD_TYPE_F16))
        return hipErrorInvalidValue;
    if (n_ids <= 0 || cols <= 0)
        return hipSuccess;
    const int nb = (int)((cols + 255) / 256), rpb = rows_per_group(ids, n_ids);
    const long groups = (n_ids + rpb - 1) / rpb * nb;
    if (groups > 0x7fffffffL)
        return hipErrorInvalidValue;
    const int vec = ((uintptr_t)out % 16 == 0 && out_row_bytes % 16 == 0) ? 1 : 0;
    const bool f32 = out_type == LFAMD_TYPE_F32;
#define GR(LY)                                                                                                                             \
    case LY:                                                                                                                               \
        if (f32)                                                                                                                           \
            get_rows_kernel<LY, float><<<(unsigned)groups, 256, 0, s>>>((const uint8_t *)img, rows, cols, nb, ids, row0, n_ids, rpb,       \
                                                                        (uint8_t *)out, out_row_bytes, vec);                               \
        else                                                                                                                               \
            get_rows_kernel<LY, _Float16><<<(unsigned)groups, 256, 0, s>>>((const uint8_t *)img, rows, cols, nb, ids, row0, n_ids, rpb,    \
                                                                           (uint8_t *)out, out_row_bytes, vec);                            \
        break;
    switch (ly) {
        GR(LY_P4K)
        GR(LY_P5K)
        GR(LY_P6K)
        GR(LY_P40)
        GR(LY_PK2)
        GR(LY_PK3)
        GR(LY_PX4)
        GR(LY_PCL41)
        GR(LY_PCL50)
        GR(LY_PCL51)
        GR(LY_P80)
        GR(LY_P4N)
        GR(LY_RAW40)
        GR(LY_RAW41)
        GR(LY_RAW50)
        GR(LY_RAW51)
        GR(LY_RAW4N)
        GR(LY_F32)
        GR(LY_F16)
        GR(LY_BF16)
    }
#undef GR
    return hipGetLastError();
}

extern "C" hipError_t lfamd_launch_unpack(const lfamd_image &im, const void *img, long rows, long cols, void *raw, size_t raw_row_bytes,
                                          hipStream_t s) {
    const int ly = im.ly, type = im.type;
    if (ly == LY_NONE)
        return hipErrorInvalidValue;
    const size_t row_bytes = lfamd_row_size(type, cols);
    if (rows <= 0 || row_bytes == 0)
        return hipSuccess;
    if (rows > 0x7fffffffL || (row_bytes + 255) / 256 > 65535)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)rows, (unsigned)((row_bytes + 255) / 256));
    const uint8_t *in = (const uint8_t *)img;
    uint8_t *o = (uint8_t *)raw;
    const int nb = type == LFAMD_TYPE_Q8_0 ? (int)((cols / 32 + 3) / 4) : (int)((cols + 255) / 256); // (a gather stops at row_bytes)
#define UP(T)                                                                                                                              \
    case T:                                                                                                                                \
        unpack_kernel<T><<<grid, 256, 0, s>>>(in, cols, nb, row_bytes, o, raw_row_bytes);                                                  \
        break;
    if (ly >= LY_RAW40) {
        unpack_raw_kernel<<<grid, 256, 0, s>>>(in, row_bytes, o, raw_row_bytes);
    } else {
        switch (type) {
            UP(LFAMD_TYPE_Q4_K)
            UP(LFAMD_TYPE_Q5_K)
            UP(LFAMD_TYPE_Q6_K)
            UP(LFAMD_TYPE_Q2_K)
            UP(LFAMD_TYPE_Q3_K)
            UP(LFAMD_TYPE_IQ4_XS)
        case LFAMD_TYPE_IQ4_NL: // the P40 image: Q4_0's gather
            UP(LFAMD_TYPE_Q4_0)
            UP(LFAMD_TYPE_Q4_1)
            UP(LFAMD_TYPE_Q5_0)
            UP(LFAMD_TYPE_Q5_1)
            UP(LFAMD_TYPE_Q8_0)
        }
    }
#undef UP
    return hipGetLastError();
}
