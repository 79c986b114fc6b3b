// cpy.hip — lfamd_cpy: GGML_OP_CPY on the device (include/lfamd_hip.h), the store of k_cur / v_cur into an offloaded K / V cache and the
// same-type moves of a cache defragmentation.  Reference: ggml_cuda_cpy (ggml-cuda.cu.patch:4242-4760, dispatch :5150-5260); its
// quantising copies launch one thread per 32-block, this unit gives a block to eight lanes.
//
// Arithmetic is a function of the element or the 32-block alone: ONE quantiser (quant_block) serves every route, so the bytes do not
// depend on the route, the shape description or the alignment.  Every product is rounded to f32 before the add that follows it (the
// unit is compiled without contraction), divisions are IEEE.
//
// Routes, selected by the layouts alone (the end of lfamd_cpy):
//   ROWS        both sides contiguous over runs of R elements (R = gcd of the two sides' contiguous prefixes): a work-group converts a
//               tile of 1024 elements of one run with 16-byte loads, assembles the destination image in LDS at the destination's own
//               offset inside a 16-byte line, and writes it with 16-byte stores between a narrow head and a narrow tail.
//   TRANSPOSED  F32 -> F16, source elements strided and source dim 1 contiguous, destination rows contiguous (the V store without -fa):
//               a 64 x 32 tile through padded LDS, reads coalesced along dim 1, writes along dim 0 in 16-byte lines of a row.
//   GENERAL     anything else of a served pair: one element per lane (one block per eight lanes, one whole block per lane for the
//               same-type moves), the index arithmetic of the reference.
#include "entry_checks.h"

#pragma clang fp contract(off)

namespace {

// one side of the copy in UNITS: an element of a float type, a 32-block of a block type (for the F32 source of a block destination:
// 32 floats, 128 bytes)
struct cpy_side {
    long ne[4];
    size_t nb[4];
};
struct cpy_args {
    const uint8_t *src;
    uint8_t *dst;
    cpy_side s, d;
    long n;            // units in all (< 2^31)
    uint32_t run;      // ROWS: units per run
    uint32_t tiles;    // ROWS: tiles per run; TRANSPOSED: tiles along dim 0
    uint32_t s_linear; // bytes per unit where the whole source is one contiguous run (unit i at i * s_linear), else 0
    uint32_t d_linear; // the same for the destination
    int unit;          // same-type kernels: bytes per unit
};

// (a call has at most 2^31 - 1 elements and no extent of 0: the index and every extent fit 32 bits, whose division is a fraction of
// the 64-bit one's instructions — it is on the path of every work-group before its first load)
__device__ static inline size_t unit_offset(const cpy_side &t, long i) {
    uint32_t r = (uint32_t)i;
    const uint32_t n0 = (uint32_t)t.ne[0], n1 = (uint32_t)t.ne[1], n2 = (uint32_t)t.ne[2];
    const uint32_t i0 = r % n0;
    r /= n0;
    const uint32_t i1 = r % n1;
    r /= n1;
    const uint32_t i2 = r % n2, i3 = r / n2;
    return (size_t)i0 * t.nb[0] + (size_t)i1 * t.nb[1] + (size_t)i2 * t.nb[2] + (size_t)i3 * t.nb[3];
}
// the K store's two sides are contiguous: no division stands in front of the one-token store's first load
__device__ static inline size_t src_offset(const cpy_args &A, long i) {
    return A.s_linear ? (size_t)i * A.s_linear : unit_offset(A.s, i);
}
__device__ static inline size_t dst_offset(const cpy_args &A, long i) {
    return A.d_linear ? (size_t)i * A.d_linear : unit_offset(A.d, i);
}

__device__ static const float k_iq4nl[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};

// best_index_int8 (ggml-cuda.cu.patch:4665-4674): the nearest codebook value, a tie to the upper index
__device__ static inline int iq4nl_index(float x) {
    if (x <= k_iq4nl[0])
        return 0;
    if (x >= k_iq4nl[15])
        return 15;
    int mu = 1; // the first entry above x
    for (int j = 1; j < 15; j++)
        mu += x >= k_iq4nl[j] ? 1 : 0;
    return x - k_iq4nl[mu - 1] < k_iq4nl[mu] - x ? mu - 1 : mu;
}

// the first of equal candidates wins, as the scalar loops' strict comparisons decide: (value, lane) pairs through the group of 8
template <typename Better>
__device__ static inline float first_of_group(float key, float val, int g, Better better) {
    int idx = g;
    for (int m = 1; m < 8; m <<= 1) {
        const float ok = __shfl_xor(key, m, 64), ov = __shfl_xor(val, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (better(ok, key) || (ok == key && oi < idx))
            key = ok, val = ov, idx = oi;
    }
    return val;
}

__device__ static inline uint32_t pack4(const int (&q)[4]) {
    return (uint32_t)(q[0] & 0xff) | (uint32_t)(q[1] & 0xff) << 8 | (uint32_t)(q[2] & 0xff) << 16 | (uint32_t)(q[3] & 0xff) << 24;
}

// quantize_row_<type>_reference on one 32-block held by 8 consecutive lanes: lane g of the group has elements 4 g .. 4 g + 3.  The
// block goes to `out` (LDS or global memory, 2-byte aligned) in 16-bit words, each lane its own; `live` = false computes and writes
// nothing (every lane of the wave takes part in the exchanges).
template <int DT>
__device__ static inline void quant_block(const float (&x)[4], int g, uint16_t *out, bool live) {
    int q[4];
    if constexpr (DT == LFAMD_TYPE_Q8_0) {
        float amax = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
        for (int m = 1; m < 8; m <<= 1)
            amax = fmaxf(amax, __shfl_xor(amax, m, 64));
        const float d = amax / 127.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        for (int c = 0; c < 4; c++)
            q[c] = (int)roundf(x[c] * id);
        const uint32_t w = pack4(q);
        if (live) {
            if (g == 0)
                out[0] = f2h_bits(d);
            out[1 + 2 * g] = (uint16_t)w, out[2 + 2 * g] = (uint16_t)(w >> 16);
        }
    } else if constexpr (DT == LFAMD_TYPE_Q4_0 || DT == LFAMD_TYPE_Q5_0 || DT == LFAMD_TYPE_IQ4_NL) {
        float am = 0.0f, vm = 0.0f;
        for (int c = 0; c < 4; c++)
            if (am < fabsf(x[c]))
                am = fabsf(x[c]), vm = x[c];
        const float vmax = first_of_group(am, vm, g, [](float a, float b) { return a > b; });
        float d = vmax / (DT == LFAMD_TYPE_Q4_0 ? -8.0f : DT == LFAMD_TYPE_Q5_0 ? -16.0f : k_iq4nl[0]);
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        for (int c = 0; c < 4; c++) {
            const float y = x[c] * id;
            if constexpr (DT == LFAMD_TYPE_Q4_0)
                q[c] = min(15, (int)(int8_t)(y + 8.5f));
            else if constexpr (DT == LFAMD_TYPE_Q5_0)
                q[c] = min(31, (int)(int8_t)(y + 16.5f));
            else
                q[c] = iq4nl_index(y);
        }
        if constexpr (DT == LFAMD_TYPE_IQ4_NL) {
            // the refit of d, in the reference's serial order (ggml-cuda.cu.patch:4706-4721): pairs (j, j + 16) in ascending j, every lane
            // of the group the same 16 steps on exchanged values, so that d is a function of the block alone
            float sumqx = 0.0f, sumq2 = 0.0f;
            const int base = (threadIdx.x & 63) & ~7;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int c = j & 3, l0 = base + (j >> 2), l1 = l0 + 4;
                const float x0 = __shfl(x[c], l0, 64), x1 = __shfl(x[c], l1, 64);
                const float v0 = k_iq4nl[__shfl(q[c], l0, 64)], v1 = k_iq4nl[__shfl(q[c], l1, 64)];
                const float w0 = x0 * x0, w1 = x1 * x1;
                sumqx += w0 * v0 * x0 + w1 * v1 * x1;
                sumq2 += w0 * v0 * v0 + w1 * v1 * v1;
            }
            d = sumq2 > 0.0f ? sumqx / sumq2 : d;
        }
        const uint32_t w = pack4(q), lo = w & 0x0f0f0f0fu;
        const uint32_t olo = __shfl_xor(lo, 4, 64);
        uint32_t qh = ((w >> 4) & 1u) | ((w >> 11) & 2u) | ((w >> 18) & 4u) | ((w >> 25) & 8u); // bit 4 of each code
        qh <<= 4 * g;
        if constexpr (DT == LFAMD_TYPE_Q5_0)
            for (int m = 1; m < 8; m <<= 1)
                qh |= __shfl_xor(qh, m, 64);
        if (live) {
            constexpr int QS = DT == LFAMD_TYPE_Q5_0 ? 3 : 1;
            if (g == 0) {
                out[0] = f2h_bits(d);
                if constexpr (DT == LFAMD_TYPE_Q5_0)
                    out[1] = (uint16_t)qh, out[2] = (uint16_t)(qh >> 16);
            }
            if (g < 4) {
                const uint32_t qs = lo | olo << 4;
                out[QS + 2 * g] = (uint16_t)qs, out[QS + 1 + 2 * g] = (uint16_t)(qs >> 16);
            }
        }
    } else { // Q4_1, Q5_1
        float lo_v = x[0], hi_v = x[0];
        for (int c = 1; c < 4; c++) {
            lo_v = x[c] < lo_v ? x[c] : lo_v;
            hi_v = x[c] > hi_v ? x[c] : hi_v;
        }
        const float vmin = first_of_group(lo_v, lo_v, g, [](float a, float b) { return a < b; });
        const float vmax = first_of_group(hi_v, hi_v, g, [](float a, float b) { return a > b; });
        const float d = (vmax - vmin) / (DT == LFAMD_TYPE_Q4_1 ? 15.0f : 31.0f);
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        for (int c = 0; c < 4; c++) {
            const float y = (x[c] - vmin) * id;
            if constexpr (DT == LFAMD_TYPE_Q4_1)
                q[c] = min(15, (int)(int8_t)(y + 0.5f));
            else
                q[c] = (int)(uint8_t)(y + 0.5f);
        }
        const uint32_t w = pack4(q), lo = w & 0x0f0f0f0fu;
        const uint32_t olo = __shfl_xor(lo, 4, 64);
        uint32_t qh = ((w >> 4) & 1u) | ((w >> 11) & 2u) | ((w >> 18) & 4u) | ((w >> 25) & 8u);
        qh <<= 4 * g;
        if constexpr (DT == LFAMD_TYPE_Q5_1)
            for (int m = 1; m < 8; m <<= 1)
                qh |= __shfl_xor(qh, m, 64);
        if (live) {
            constexpr int QS = DT == LFAMD_TYPE_Q5_1 ? 4 : 2;
            if (g == 0) {
                out[0] = f2h_bits(d), out[1] = f2h_bits(vmin);
                if constexpr (DT == LFAMD_TYPE_Q5_1)
                    out[2] = (uint16_t)qh, out[3] = (uint16_t)(qh >> 16);
            }
            if (g < 4) {
                const uint32_t qs = lo | olo << 4;
                out[QS + 2 * g] = (uint16_t)qs, out[QS + 1 + 2 * g] = (uint16_t)(qs >> 16);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- ROWS
constexpr int CPY_TILE = 1024;  // elements of a run per work-group (conversions)
constexpr int CPY_BYTES = 4096; // bytes of a run per work-group (same-type moves)

// The image of `bytes` bytes sits in LDS at lds + a, a = dptr % 16: a 16-byte line of the destination is a 16-byte line of LDS.
// Head (up to the first line boundary) and tail in 16-bit stores, the lines between them in 16-byte stores; nothing outside
// [dptr, dptr + bytes) is written.
__device__ static inline void flush_image(const uint8_t *lds, int a, uint8_t *dptr, int bytes) {
    __syncthreads();
    const int t = threadIdx.x;
    const int head = min(bytes, (16 - a) & 15);
    const int body = (bytes - head) & ~15;
    const int tail = bytes - head - body;
    for (int c = t; c < body / 16; c += 256)
        *(uint4 *)(dptr + head + 16 * c) = *(const uint4 *)(lds + a + head + 16 * c);
    if (t < head / 2)
        *(uint16_t *)(dptr + 2 * t) = *(const uint16_t *)(lds + a + 2 * t);
    else if (t >= 8 && t - 8 < tail / 2)
        *(uint16_t *)(dptr + head + body + 2 * (t - 8)) = *(const uint16_t *)(lds + a + head + body + 2 * (t - 8));
}

// F32 -> F16 or a block type; DT = F16: units are elements, else 32-blocks
template <int DT>
__global__ __launch_bounds__(256) void cpy_rows_kernel(const cpy_args A) {
    constexpr bool BLOCKS = DT != LFAMD_TYPE_F16;
    constexpr int UPT = BLOCKS ? CPY_TILE / 32 : CPY_TILE; // units per tile
    __shared__ __attribute__((aligned(16))) uint8_t lds[16 + (BLOCKS ? (CPY_TILE / 32) * lfamd_block32<DT>::TS : CPY_TILE * 2)];
    const uint32_t run = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
    const long u0 = (long)run * A.run + (long)tile * UPT;                  // first unit of the tile
    const int units = (int)min((long)UPT, (long)A.run - (long)tile * UPT); // units in this tile
    const int T = BLOCKS ? units * 32 : units;                             // elements
    const float *sp = (const float *)(A.src + src_offset(A, u0));
    uint8_t *dp = A.dst + dst_offset(A, u0);
    const int a = (int)((uintptr_t)dp & 15);
    const int t = threadIdx.x, e = 4 * t;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e + 3 < T && ((uintptr_t)sp & 15) == 0) {
        const float4 v = *(const float4 *)(sp + e);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
        for (int c = 0; c < 4; c++)
            if (e + c < T)
                x[c] = sp[e + c];
    }
    if constexpr (BLOCKS) {
        quant_block<DT>(x, t & 7, (uint16_t *)(lds + a + (t >> 3) * lfamd_block32<DT>::TS), e < T);
    } else {
        uint16_t *o = (uint16_t *)(lds + a) + e;
        for (int c = 0; c < 4; c++)
            if (e + c < T)
                o[c] = f2h_bits(x[c]);
    }
    flush_image(lds, a, dp, BLOCKS ? units * lfamd_block32<DT>::TS : units * 2);
}

// same-type move: the run is a run of bytes (A.unit bytes per unit).  Where source and destination sit alike in their 16-byte lines:
// 16-byte loads and stores from registers; else 16-bit loads into the LDS image and wide stores from it
__global__ __launch_bounds__(256) void cpy_rows_same_kernel(const cpy_args A) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[16 + CPY_BYTES];
    const uint32_t run = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
    const long u0 = (long)run * A.run;
    const size_t in_run = (size_t)tile * CPY_BYTES;
    const int bytes = (int)min((size_t)CPY_BYTES, (size_t)A.run * A.unit - in_run);
    const uint8_t *sp = A.src + src_offset(A, u0) + in_run;
    uint8_t *dp = A.dst + dst_offset(A, u0) + in_run;
    const int a = (int)((uintptr_t)dp & 15), t = threadIdx.x;
    if ((int)((uintptr_t)sp & 15) == a) {
        const int head = min(bytes, (16 - a) & 15);
        const int body = (bytes - head) & ~15;
        const int tail = bytes - head - body;
        for (int c = t; c < body / 16; c += 256) // (lines of the source are lines of the destination: no image to assemble)
            *(uint4 *)(dp + head + 16 * c) = *(const uint4 *)(sp + head + 16 * c);
        if (t < head / 2)
            *(uint16_t *)(dp + 2 * t) = *(const uint16_t *)(sp + 2 * t);
        else if (t >= 8 && t - 8 < tail / 2)
            *(uint16_t *)(dp + head + body + 2 * (t - 8)) = *(const uint16_t *)(sp + head + body + 2 * (t - 8));
        return;
    } else {
        for (int i = t; i < bytes / 2; i += 256)
            *(uint16_t *)(lds + a + 2 * i) = *(const uint16_t *)(sp + 2 * i);
    }
    flush_image(lds, a, dp, bytes);
}

// ------------------------------------------------------------------------------------------------------------------- TRANSPOSED
// F32 element (i0, i1) at src + i0 * s.nb[0] + 4 i1  ->  F16 at dst + i1 * d.nb[1] + 2 i0.  Tile: 64 i0 x 32 i1 (512 tokens of 1024
// rows are 256 work-groups: one per CU; at 64 x 64 half the CUs had none), a row of the tile padded to 33 words.
constexpr int CPY_TC = 64, CPY_TR = 32;

__global__ __launch_bounds__(256) void cpy_transposed_kernel(const cpy_args A) {
    __shared__ float tile[CPY_TC][CPY_TR + 1];
    const long c0 = (long)(blockIdx.x % A.tiles) * CPY_TC, r0 = (long)(blockIdx.x / A.tiles) * CPY_TR; // first i0 (column of dst), first i1 (row)
    const int nc = (int)min((long)CPY_TC, A.s.ne[0] - c0), nr = (int)min((long)CPY_TR, A.s.ne[1] - r0);
    const int t = threadIdx.x;
    const uint8_t *sp = A.src + (size_t)c0 * A.s.nb[0] + (size_t)r0 * 4;
    if ((((uintptr_t)A.src | A.s.nb[0]) & 15) == 0) {
        const int rr = (t & 7) * 4, cc = t >> 3; // eight lanes x 16 bytes along i1, 32 columns a pass
        for (int k = 0; k < CPY_TC / 32; k++) {
            const int c = cc + 32 * k;
            if (c >= nc)
                break;
            const float *p = (const float *)(sp + (size_t)c * A.s.nb[0]) + rr;
            if (rr + 3 < nr) {
                const float4 v = *(const float4 *)p;
                tile[c][rr] = v.x, tile[c][rr + 1] = v.y, tile[c][rr + 2] = v.z, tile[c][rr + 3] = v.w;
            } else {
                for (int i = 0; rr + i < nr; i++)
                    tile[c][rr + i] = p[i];
            }
        }
    } else {
        const int rr = t & 31, cc = t >> 5;
        for (int k = 0; k < CPY_TC / 8; k++) {
            const int c = cc + 8 * k;
            if (c < nc && rr < nr)
                tile[c][rr] = *((const float *)(sp + (size_t)c * A.s.nb[0]) + rr);
        }
    }
    __syncthreads();
    // eight lanes per destination row; a lane takes every eighth 16-byte line of the row's segment (at most nine lines).  A line wholly
    // inside the segment is one 16-byte store, the lines at the segment's two ends are written half by half
    const int r = t >> 3;
    if (r >= nr)
        return;
    uint8_t *row = A.dst + (size_t)(r0 + r) * A.d.nb[1] + (size_t)c0 * 2;
    const int sh = (int)((uintptr_t)row & 15) / 2; // halves between the line boundary in front of the segment and its start
    uint8_t *line0 = row - 2 * sh;
    const int lines = (sh + nc + 7) / 8;
    for (int w = t & 7; w < lines; w += 8) {
        const int e0 = 8 * w - sh;
        if (e0 >= 0 && e0 + 8 <= nc) {
            uint32_t h[4];
            for (int i = 0; i < 4; i++)
                h[i] = (uint32_t)f2h_bits(tile[e0 + 2 * i][r]) | (uint32_t)f2h_bits(tile[e0 + 2 * i + 1][r]) << 16;
            *(uint4 *)(line0 + 16 * w) = make_uint4(h[0], h[1], h[2], h[3]);
        } else {
            for (int i = 0; i < 8; i++)
                if (e0 + i >= 0 && e0 + i < nc)
                    *(uint16_t *)(line0 + 16 * w + 2 * i) = f2h_bits(tile[e0 + i][r]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- GENERAL
__global__ __launch_bounds__(256) void cpy_general_f32_f16_kernel(const cpy_args A) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n)
        return;
    *(uint16_t *)(A.dst + unit_offset(A.d, i)) = f2h_bits(*(const float *)(A.src + unit_offset(A.s, i)));
}

// same type: a unit (element or whole block) per lane, in 16-bit words (F32: both sides are 4-byte aligned, two words)
__global__ __launch_bounds__(256) void cpy_general_same_kernel(const cpy_args A) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n)
        return;
    const uint16_t *s = (const uint16_t *)(A.src + unit_offset(A.s, i));
    uint16_t *d = (uint16_t *)(A.dst + unit_offset(A.d, i));
    for (int w = 0; w < A.unit / 2; w++)
        d[w] = s[w];
}

// F32 -> block type: a block per 8 lanes, written where it belongs in 16-bit words
template <int DT>
__global__ __launch_bounds__(256) void cpy_general_quant_kernel(const cpy_args A) {
    const long i = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = i < A.n;
    const int g = threadIdx.x & 7;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint16_t *out = nullptr;
    if (live) {
        const float *sp = (const float *)(A.src + unit_offset(A.s, i)) + 4 * g;
        for (int c = 0; c < 4; c++)
            x[c] = sp[c];
        out = (uint16_t *)(A.dst + unit_offset(A.d, i));
    }
    quant_block<DT>(x, g, out, live);
}

// ------------------------------------------------------------------------------------------------------------------------- host
bool pair_served(int s, int d) {
    if (s == LFAMD_TYPE_F32)
        return d == LFAMD_TYPE_F32 || d == LFAMD_TYPE_F16 || lfamd_block_k_type(d);
    return s == d && (s == LFAMD_TYPE_F16 || lfamd_block_k_type(s));
}

constexpr long CPY_MAX_ELEMENTS = 0x7fffffffL;

// elements of the tensor, or -1 where they exceed the limit
long count_elements(const long ne[4]) {
    long n = 1;
    for (int i = 0; i < 4; i++) {
        if (ne[i] != 0 && n > CPY_MAX_ELEMENTS / ne[i])
            return -1;
        n *= ne[i];
    }
    return n;
}

// units over which the side is contiguous from its first unit on (dimensions of extent 1 have no stride to speak of)
long contiguous_units(const cpy_side &t, size_t unit_bytes) {
    long run = 1;
    size_t bytes = unit_bytes;
    for (int i = 0; i < 4; i++) {
        if (t.ne[i] == 1)
            continue;
        if (t.nb[i] != bytes)
            break;
        run *= t.ne[i], bytes *= (size_t)t.ne[i];
    }
    return run;
}

long gcd(long a, long b) {
    while (b) {
        const long r = a % b;
        a = b, b = r;
    }
    return a;
}

#define CPY_BY_TYPE(KERNEL, GRID)                                                                                                         \
    switch (dst_type) {                                                                                                                    \
    case LFAMD_TYPE_Q8_0: KERNEL<LFAMD_TYPE_Q8_0><<<GRID, 256, 0, s>>>(A); break;                                                          \
    case LFAMD_TYPE_Q4_0: KERNEL<LFAMD_TYPE_Q4_0><<<GRID, 256, 0, s>>>(A); break;                                                          \
    case LFAMD_TYPE_Q4_1: KERNEL<LFAMD_TYPE_Q4_1><<<GRID, 256, 0, s>>>(A); break;                                                          \
    case LFAMD_TYPE_Q5_0: KERNEL<LFAMD_TYPE_Q5_0><<<GRID, 256, 0, s>>>(A); break;                                                          \
    case LFAMD_TYPE_Q5_1: KERNEL<LFAMD_TYPE_Q5_1><<<GRID, 256, 0, s>>>(A); break;                                                          \
    default: KERNEL<LFAMD_TYPE_IQ4_NL><<<GRID, 256, 0, s>>>(A); break;                                                                     \
    }

} // namespace

// where nb[0] is the element size: is a stride of a dimension of extent > 1 smaller than the row?
static bool cpy_short_row(int type, const long ne[4], const size_t nb[4]) {
    if (nb[0] != lfamd_type_size(type))
        return false;
    for (int i = 1; i < 4; i++)
        if (ne[i] > 1 && nb[i] < lfamd_row_size(type, ne[0]))
            return true;
    return false;
}

// The checks of include/lfamd_hip.h in their documented order, as one table for lfamd_run_checks (entry_checks.h: evaluated whole, so
// every row guards itself — a NULL ne / nb array is read as four zeros by the rows behind the first); no device call.  `entry`: asked
// by lfamd_cpy, to which every flag is reserved; else by lfamd_cpy_check, which takes LFAMD_CHECK_UNPLACED.  true: launch.  false:
// *rc is the answer (LFAMD_OK: an empty call).
static bool cpy_check(bool entry, int src_type, const void *d_src, const long src_ne[4], const size_t src_nb[4], int dst_type,
                      const void *d_dst, const long dst_ne[4], const size_t dst_nb[4], unsigned flags, int *rc) {
    static const long no_ne[4] = {};
    static const size_t no_nb[4] = {};
    const bool arrays = src_ne && src_nb && dst_ne && dst_nb;
    const long *s_ne = arrays ? src_ne : no_ne, *d_ne = arrays ? dst_ne : no_ne;
    const size_t *s_nb = arrays ? src_nb : no_nb, *d_nb = arrays ? dst_nb : no_nb;
    const auto [unplaced, reserved] = lfamd_check_flags_of(entry, flags);
    bool negative = false, empty = false;
    for (int i = 0; i < 4; i++)
        negative |= s_ne[i] < 0 || d_ne[i] < 0, empty |= d_ne[i] == 0;
    const long n_src = negative ? -1 : count_elements(s_ne), n_dst = negative ? -1 : count_elements(d_ne);
    const bool blocks = lfamd_block_k_type(dst_type);
    const size_t s_align = src_type == LFAMD_TYPE_F32 ? 4 : 2, d_align = dst_type == LFAMD_TYPE_F32 ? 4 : 2;
    const lfamd_check_row checks[] = {
        {!arrays, LFAMD_ERR_INVALID, "null ne / nb array"},
        {negative, LFAMD_ERR_INVALID, "negative extent"},
        {empty, LFAMD_OK, nullptr},
        {!pair_served(src_type, dst_type), LFAMD_ERR_UNSUPPORTED, "type pair not served"},
        {n_src < 0 || n_dst < 0, LFAMD_ERR_UNSUPPORTED, "more than 2^31 - 1 elements"},
        {!unplaced && (!d_src || !d_dst), LFAMD_ERR_INVALID, "null pointer"},
        {n_src != n_dst, LFAMD_ERR_INVALID, "source and destination differ in their element count"},
        {blocks && (s_ne[0] % 32 != 0 || d_ne[0] % 32 != 0), LFAMD_ERR_INVALID, "ne[0] is not a multiple of 32 beside a block type"},
        {blocks && (d_nb[0] != lfamd_type_size(dst_type) || s_nb[0] != lfamd_type_size(src_type)), LFAMD_ERR_INVALID,
         "nb[0] beside a block type: the block size, and 4 for its F32 source"},
        {((uintptr_t)d_src | s_nb[0] | s_nb[1] | s_nb[2] | s_nb[3]) % s_align != 0 ||
             ((uintptr_t)d_dst | d_nb[0] | d_nb[1] | d_nb[2] | d_nb[3]) % d_align != 0,
         LFAMD_ERR_INVALID, "a base or stride is not a multiple of the element alignment"},
        {cpy_short_row(src_type, s_ne, s_nb) || cpy_short_row(dst_type, d_ne, d_nb), LFAMD_ERR_INVALID, "a row stride is smaller than the row"},
        {reserved != 0, LFAMD_ERR_INVALID, "flags are reserved (0)"},
    };
    return lfamd_run_checks("lfamd_cpy", checks, rc);
}

extern "C" int lfamd_cpy_check(int src_type, const void *d_src, const long src_ne[4], const size_t src_nb[4], int dst_type, const void *d_dst,
                               const long dst_ne[4], const size_t dst_nb[4], unsigned flags) {
    int rc = LFAMD_OK;
    (void)cpy_check(false, src_type, d_src, src_ne, src_nb, dst_type, d_dst, dst_ne, dst_nb, flags, &rc);
    return rc;
}

extern "C" int lfamd_cpy(int src_type, const void *d_src, const long src_ne[4], const size_t src_nb[4], int dst_type, void *d_dst,
                         const long dst_ne[4], const size_t dst_nb[4], unsigned flags, void *stream) {
    int rc;
    if (!cpy_check(true, src_type, d_src, src_ne, src_nb, dst_type, d_dst, dst_ne, dst_nb, flags, &rc))
        return rc;
    const long n_dst = count_elements(dst_ne);
    const bool blocks = lfamd_block_k_type(dst_type), same = src_type == dst_type;
    const size_t s_size = lfamd_type_size(src_type), d_size = lfamd_type_size(dst_type);

    // both sides in units: an element, or a 32-block (128 bytes of an F32 source)
    cpy_args A{};
    A.src = (const uint8_t *)d_src, A.dst = (uint8_t *)d_dst;
    for (int i = 0; i < 4; i++)
        A.s.ne[i] = src_ne[i], A.s.nb[i] = src_nb[i], A.d.ne[i] = dst_ne[i], A.d.nb[i] = dst_nb[i];
    size_t s_unit = s_size, d_unit = d_size;
    if (blocks) {
        A.s.ne[0] /= 32, A.d.ne[0] /= 32;
        if (!same)
            s_unit = 128, A.s.nb[0] = 128;
    }
    A.n = n_dst / (blocks ? 32 : 1);
    A.unit = (int)d_unit;
    hipStream_t s = (hipStream_t)stream;

    const bool transposed = src_type == LFAMD_TYPE_F32 && dst_type == LFAMD_TYPE_F16 && src_ne[2] == 1 && src_ne[3] == 1 && dst_ne[2] == 1 &&
                            dst_ne[3] == 1 && src_ne[0] == dst_ne[0] && src_ne[1] == dst_ne[1] && src_ne[0] >= 8 && src_ne[1] >= 2 &&
                            src_nb[1] == 4 && src_nb[0] != 4 && dst_nb[0] == 2;
    const long s_run = contiguous_units(A.s, s_unit), d_run = contiguous_units(A.d, d_unit);
    A.s_linear = s_run == A.n ? (uint32_t)s_unit : 0, A.d_linear = d_run == A.n ? (uint32_t)d_unit : 0;
    const long run = gcd(s_run, d_run);
    const bool rows = blocks && !same ? run >= 4 : run * (long)d_unit >= 64;
    if (transposed) {
        A.tiles = (uint32_t)((src_ne[0] + CPY_TC - 1) / CPY_TC);
        cpy_transposed_kernel<<<(unsigned)((long)A.tiles * ((src_ne[1] + CPY_TR - 1) / CPY_TR)), 256, 0, s>>>(A);
    } else if (rows) {
        A.run = (uint32_t)run;
        if (same) {
            A.tiles = (uint32_t)(((size_t)run * d_unit + CPY_BYTES - 1) / CPY_BYTES);
            cpy_rows_same_kernel<<<(unsigned)(A.n / run * A.tiles), 256, 0, s>>>(A);
        } else {
            const long upt = blocks ? CPY_TILE / 32 : CPY_TILE;
            A.tiles = (uint32_t)((run + upt - 1) / upt);
            const unsigned grid = (unsigned)(A.n / run * A.tiles);
            if (dst_type == LFAMD_TYPE_F16)
                cpy_rows_kernel<LFAMD_TYPE_F16><<<grid, 256, 0, s>>>(A);
            else
                CPY_BY_TYPE(cpy_rows_kernel, grid)
        }
    } else if (same) {
        cpy_general_same_kernel<<<(unsigned)((A.n + 255) / 256), 256, 0, s>>>(A);
    } else if (dst_type == LFAMD_TYPE_F16) {
        cpy_general_f32_f16_kernel<<<(unsigned)((A.n + 255) / 256), 256, 0, s>>>(A);
    } else {
        const unsigned grid = (unsigned)((A.n + 31) / 32);
        CPY_BY_TYPE(cpy_general_quant_kernel, grid)
    }
    return lfamd_launch_status(hipGetLastError());
}
