// mul_mat_batched_q.hip — lfamd_mul_mat_batched_q: the KQ product of a QUANTISED K cache (-ctk q8_0, q4_0, q4_1, q5_0, q5_1,
// iq4_nl) in ONE launch.
//
// GGML_OP_MUL_MAT where src0 is a permuted view of a 32-block K cache that is rewritten every step and src1 is F32 with ne[2] =
// query heads.  The argument list, its checks and the index rule are lfamd_mul_mat_batched's (mul_mat_batched_common.h); A is raw GGUF
// rows of k / 32 blocks, read where ggml keeps them: no resident image, no pack call, no workspace.
//
// Arithmetic (the reference's CPU path: quantize_row_q8_0 / q8_1 of src1, then the type's vec_dot):
//   - an activation row is quantised per 32-block in LDS, bit for bit as lfamd_quantize_rows does: Q8_0 (Q8_0, Q4_0, Q5_0, IQ4_NL
//     weights) or Q8_1 (Q4_1, Q5_1), d and s = f16(sum * d) stored as f16
//   - block b gives t_b = (f32(d_w) * f32(d_a)) * (float)isum_b, isum_b the exact int32 dot of the weight codes with the activation
//     codes; Q4_1 / Q5_1 also u_b = f32(m_w) * f32(s_a)
//   - one output = ((((0 + t_0) [+ u_0]) + t_1) [+ u_1]) + ... in f32, blocks in ascending order: a function of k and the type
//     alone.  BOTH bodies add in exactly this order, so the bits do not depend on n either.
// Two bodies, picked by n alone:
//   n <= 8  mmq_gemv_kernel: blockIdx.y = (i3, KV head, chunk of hg = min(r2, 8 / n) query heads) as in mmb_gemv_kernel — where
//           r2 * n <= 8 the K rows are read once for the whole group.  The work-group quantises its NC = hg * n columns into LDS,
//           then each QUAD of lanes takes one row: lane s of the quad decodes blocks s, s + 4, ... and dots them (sdot4) with all
//           NC columns; the quad's four terms are added in block order through quad_perm DPP broadcasts, in all four lanes.
//   n > 8   mmq_mfma_kernel: v_mfma_i32_32x32x32_i8, one instruction = one 32-block of a 32 x 32 tile.  256 threads own 128 rows
//           x 64 columns of a slice and quantise the 64 columns x k once into LDS; each wave walks the blocks of 64 rows x 32
//           columns: weight codes from global memory straight into one fragment (lane half h = weights 16 h .. 16 h + 15: the low or
//           the high nibbles of the same 16 bytes), activation codes from LDS into the other.  The activations are the MFMA's
//           first operand, so a lane's 16 results are 16 columns of ITS OWN row: d_w and m_w are the lane's, the 16 d_a / s_a come
//           as four 16-byte LDS reads.  Slices on blockIdx.z in i2-major order.
// Loads: a 32-block lies on a 2-byte boundary and no better (34- and 18-byte blocks), so a block's payload is read as ALIGNED
// dwords around it plus at most one 2-byte load, and shifted into place (ld_region): the same code serves every layout that passes
// the checks, and nothing outside the block is touched.  f32 activations take 16-byte loads where the address allows, element
// loads otherwise; the values are the same either way.
// Neither body holds anything across slices: a slice's bits are those of the call on that slice alone.
#include "mul_mat_batched_common.h"

namespace {

struct mmq_args : lfamd_batched_geom {
    int kb;          // 32-blocks per row
    int hg, hchunks; // GEMV: query heads per item, items per group
};

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));

template <int T>
using wt = lfamd_block32<T>; // a weight block (S1: the activations are Q8_1)

// 4 NW bytes from the EVEN address p, whose two bytes in front (p - 2, p - 1) belong to the same block: aligned dwords, plus one 2-byte
// load where p is not a multiple of 4.  Nothing outside [p - 2, p + 4 NW) is read.
template <int NW>
__device__ static inline void ld_region(const uint8_t *p, uint32_t (&W)[NW]) {
    const bool odd = ((uintptr_t)p & 2) != 0;
    const uint32_t *al = (const uint32_t *)(p - (odd ? 2 : 0));
    uint32_t w[NW + 1];
#pragma unroll
    for (int j = 0; j < NW; j++)
        w[j] = al[j];
    w[NW] = 0;
    if (odd)
        w[NW] = *(const uint16_t *)(p + 4 * NW - 2);
#pragma unroll
    for (int j = 0; j < NW; j++)
        W[j] = odd ? (w[j] >> 16) | (w[j + 1] << 16) : w[j];
}

// one accessor per type: the int8 codes of weights 16 h .. 16 h + 15 of a block with payload P, four to a dword
template <int T>
__device__ static inline void w_codes(const uint32_t (&P)[wt<T>::NW], int h, uint32_t (&c)[4]) {
    using W = wt<T>;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (W::BYTES) {
            c[j] = h ? P[4 + j] : P[j];
        } else {
            uint32_t x = (P[(W::FIVE ? 1 : 0) + j] >> (4 * h)) & 0x0F0F0F0Fu;
            if constexpr (W::FIVE) { // bits 16 h + 4 j .. + 3 of qh to bit 4 of the four bytes
                const uint32_t t = (P[0] >> (16 * h + 4 * j)) & 0xFu;
                x |= ((t * 0x00204081u) & 0x01010101u) << 4;
            }
            if constexpr (T == LFAMD_TYPE_Q4_0) // q - 8
                x = sub_per_byte<8>(x);
            else if constexpr (T == LFAMD_TYPE_Q5_0) // q - 16
                x = sub_per_byte<16>(x);
            else if constexpr (T == LFAMD_TYPE_IQ4_NL)
                x = kvalues_lut4(x);
            c[j] = x; // (Q4_1, Q5_1: the unsigned q, below 32)
        }
    }
}

// values e0 .. e0 + 7 of an f32 row (e0 a multiple of 8)
__device__ static inline void ld_x8(const uint8_t *row, long e0, float (&v)[8]) {
    const uint8_t *p = row + e0 * 4;
    if (((uintptr_t)p & 15) == 0) {
        const float4 lo = *(const float4 *)p, hi = *(const float4 *)(p + 16);
        v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++)
            v[e] = ((const float *)p)[e];
    }
}

template <int CTRL>
__device__ static inline int dpp_i32(int v) {
    return (int)dpp_u32<CTRL>((uint32_t)v);
}

// quantize_row_q8_0 / quantize_row_q8_1 of one 32-block held by the four lanes of a quad, eight values each (all four must call):
// d = amax / 127, id = 1 / d, q = roundf(x * id); d, and Q8_1's s = sum * d (from the unrounded d), stored as f16.  The arithmetic
// of stage_f32_q80_wave2 (gemv_impl.h), without that kernel's image.
template <bool S1>
__device__ static inline void quantise_quad(const float (&v)[8], uint32_t &y0, uint32_t &y1, float &d_out, float &s_out) {
    float am = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++)
        am = fmaxf(am, fabsf(v[e]));
    am = fmaxf(am, dpp_f32<DPP_XOR1>(am));
    am = fmaxf(am, dpp_f32<DPP_XOR2>(am));
    const float d = am / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t y[2] = {0, 0};
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int q = (int)roundf(v[e] * id);
        y[e >> 2] |= (uint32_t)(q & 0xff) << (8 * (e & 3));
    }
    y0 = y[0], y1 = y[1];
    d_out = h2f(f2h_bits(d));
    s_out = 0.0f;
    if constexpr (S1) {
        int sum = sdot4(y[1], 0x01010101u, sdot4(y[0], 0x01010101u, 0));
        sum += dpp_i32<DPP_XOR1>(sum);
        sum += dpp_i32<DPP_XOR2>(sum);
        s_out = h2f(f2h_bits_of_product((float)sum, d));
    }
}

// the exact int32 dot of a block's 32 weight codes (lo: 0 .. 15, hi: 16 .. 31) with 32 activation codes
__device__ static inline int dot32(const uint32_t (&lo)[4], const uint32_t (&hi)[4], const uint4 a0, const uint4 a1) {
    int s = sdot4(lo[0], a0.x, 0);
    s = sdot4(lo[1], a0.y, s);
    s = sdot4(lo[2], a0.z, s);
    s = sdot4(lo[3], a0.w, s);
    s = sdot4(hi[0], a1.x, s);
    s = sdot4(hi[1], a1.y, s);
    s = sdot4(hi[2], a1.z, s);
    return sdot4(hi[3], a1.w, s);
}

#define DPP_QUAD_BCAST(j) ((j) * 0x55) // quad_perm [j, j, j, j]

// acc + the four lanes' t (and u) in lane order: blocks b0 .. b0 + 3 in ascending order, in every lane of the quad
template <bool S1>
__device__ static inline float quad_add_in_order(float acc, float t, float u) {
    acc = acc + dpp_f32<DPP_QUAD_BCAST(0)>(t);
    if constexpr (S1)
        acc = acc + dpp_f32<DPP_QUAD_BCAST(0)>(u);
    acc = acc + dpp_f32<DPP_QUAD_BCAST(1)>(t);
    if constexpr (S1)
        acc = acc + dpp_f32<DPP_QUAD_BCAST(1)>(u);
    acc = acc + dpp_f32<DPP_QUAD_BCAST(2)>(t);
    if constexpr (S1)
        acc = acc + dpp_f32<DPP_QUAD_BCAST(2)>(u);
    acc = acc + dpp_f32<DPP_QUAD_BCAST(3)>(t);
    if constexpr (S1)
        acc = acc + dpp_f32<DPP_QUAD_BCAST(3)>(u);
    return acc;
}

// NC: columns a lane keeps (query heads of the item x n, rounded up to 1, 2, 4 or 8; the live count is uniform)
template <int T, int NC>
__global__ __launch_bounds__(256) void mmq_gemv_kernel(const mmq_args a) {
    using W = wt<T>;
    // the item's activations: codes int8 [column][k], d (and s) f32 [column][kb]
    __shared__ __attribute__((aligned(16))) uint8_t codes[NC * 1024];
    __shared__ float dsc[NC * 32];
    __shared__ float ssc[W::S1 ? NC * 32 : 1];
    const int sub = threadIdx.x & 3, quad = threadIdx.x >> 2;
    const int kb = a.kb, k = (int)a.k;
    const lfamd_batched_index it(a.a_ne2, a.r2, a.r3, a.hg, a.hchunks);
    const int n = (int)a.n, nc = it.nh * n;
    // ---- quantise: nc * kb blocks, one quad each (the trip count is uniform: every lane reaches the DPP exchanges)
    for (int g0 = 0; g0 < nc * kb; g0 += 64) {
        const int g = g0 + quad;
        const bool live = g < nc * kb;
        const int c = live ? g / kb : 0, b = live ? g % kb : 0;
        float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (live)
            ld_x8(it.column(a.B, a.b_nb3, a.b_nb2, a.b_nb1, a.r2, c, n), (long)b * 32 + 8 * sub, v);
        uint32_t y0, y1;
        float d, s;
        quantise_quad<W::S1>(v, y0, y1, d, s);
        if (live) {
            *(uint2 *)(codes + c * k + b * 32 + 8 * sub) = make_uint2(y0, y1);
            if (sub == 0) {
                dsc[c * kb + b] = d;
                if constexpr (W::S1)
                    ssc[c * kb + b] = s;
            }
        }
    }
    __syncthreads();
    // ---- a quad per row: 64 rows per work-group.  Rows past the edge are clamped for the loads and masked at the store.
    const long row = (long)blockIdx.x * 64 + quad;
    const uint8_t *wrow = it.a_slice(a.A, a.a_nb3, a.a_nb2) + (row < a.m ? row : a.m - 1) * a.a_nb1;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[c] = 0.0f;
    for (int b0 = 0; b0 < kb; b0 += 4) {
        const int b = b0 + sub;
        const bool live = b < kb; // (a lane past the row's last block reads nothing and adds zeros, which move no bit)
        const int bl = live ? b : 0;
        uint32_t P[W::NW];
#pragma unroll
        for (int j = 0; j < W::NW; j++)
            P[j] = 0;
        float dw = 0.0f, mw = 0.0f;
        if (live) {
            const uint8_t *blk = wrow + (size_t)b * W::TS;
            dw = h2f(*(const uint16_t *)blk);
            if constexpr (W::S1)
                mw = h2f(*(const uint16_t *)(blk + 2));
            ld_region<W::NW>(blk + W::PAY, P);
        }
        uint32_t lo[4], hi[4];
        w_codes<T>(P, 0, lo);
        w_codes<T>(P, 1, hi);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) { // (uniform)
                const uint8_t *xc = codes + c * k + bl * 32;
                const int isum = dot32(lo, hi, *(const uint4 *)xc, *(const uint4 *)(xc + 16));
                const float t = (dw * dsc[c * kb + bl]) * (float)isum;
                float u = 0.0f;
                if constexpr (W::S1)
                    u = mw * ssc[c * kb + bl];
                acc[c] = quad_add_in_order<W::S1>(acc[c], t, u);
            }
        }
    }
    if (sub == 0 && row < a.m) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                float *Cc = (float *)it.column(a.C, a.c_nb3, a.c_nb2, a.c_nb1, a.r2, c, n);
                Cc[row] = acc[c];
            }
        }
    }
}

// one row tile's block: the lane's row i, weights 16 h .. 16 h + 15 as an MFMA operand, and the row's d (and m)
template <int T>
__device__ static inline v4i_t mmq_frag_w(const uint8_t *blk, int h, float &dw, float &mw) {
    using W = wt<T>;
    dw = h2f(*(const uint16_t *)blk);
    mw = 0.0f;
    if constexpr (W::S1)
        mw = h2f(*(const uint16_t *)(blk + 2));
    uint32_t c[4];
    if constexpr (W::BYTES) {
        ld_region<4>(blk + 2 + 16 * h, c); // (its own 16 codes only)
    } else {
        uint32_t P[W::NW];
        ld_region<W::NW>(blk + W::PAY, P);
        w_codes<T>(P, h, c);
    }
    const v4i_t f = {(int)c[0], (int)c[1], (int)c[2], (int)c[3]};
    return f;
}

template <int T>
__global__ __launch_bounds__(256) void mmq_mfma_kernel(const mmq_args a) {
    using W = wt<T>;
    // the work-group's 64 columns: codes int8 [kb][64][32], then d f32 [kb][64], then (Q8_1) s f32 [kb][64]
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int kb = a.kb;
    uint8_t *codes = lds;
    float *dsc = (float *)(lds + (size_t)kb * 2048), *ssc = dsc + (size_t)kb * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int sub = threadIdx.x & 3, quad = threadIdx.x >> 2;
    const lfamd_batched_index sl(a.ne2, a.r2, a.r3);
    const long n0 = (long)blockIdx.y * 64;
    // ---- quantise: 64 * kb blocks, one quad each, kb passes; the columns past n are staged as rows of zeros and never loaded
    const uint8_t *Bs = sl.slice(a.B, a.b_nb3, a.b_nb2);
    for (int g = quad; g < 64 * kb; g += 64) {
        const int c = g / kb, b = g % kb;
        float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (n0 + c < a.n)
            ld_x8(Bs + (n0 + c) * a.b_nb1, (long)b * 32 + 8 * sub, v);
        uint32_t y0, y1;
        float d, s;
        quantise_quad<W::S1>(v, y0, y1, d, s);
        *(uint2 *)(codes + ((size_t)b * 64 + c) * 32 + 8 * sub) = make_uint2(y0, y1);
        if (sub == 0) {
            dsc[b * 64 + c] = d;
            if constexpr (W::S1)
                ssc[b * 64 + c] = s;
        }
    }
    __syncthreads();
    const int cw = (wave >> 1) * 32; // the wave's 32 of the 64 columns
    const long m0 = (long)blockIdx.x * 128 + (wave & 1) * 64;
    if (m0 >= a.m || n0 + cw >= a.n)
        return;
    const bool two = m0 + 32 < a.m; // (uniform: the wave's second row tile exists)
    // rows past the edge are clamped for the loads and masked at the store
    const long ar0 = m0 + i < a.m ? m0 + i : a.m - 1, ar1 = m0 + 32 + i < a.m ? m0 + 32 + i : a.m - 1;
    const uint8_t *Ab = sl.a_slice(a.A, a.a_nb3, a.a_nb2);
    const uint8_t *A0 = Ab + ar0 * a.a_nb1, *A1 = Ab + ar1 * a.a_nb1;
    const v16i_t zero16i = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc0[16], acc1[16];
#pragma unroll
    for (int r = 0; r < 16; r++)
        acc0[r] = 0.0f, acc1[r] = 0.0f;
    for (int b = 0; b < kb; b++) {
        // first operand = the result's register index: activation column cw + (r & 3) + 8 (r >> 2) + 4 h in register r;
        // second operand = the result's lane index: the lane's own weight row
        const v4i_t fx = *(const v4i_t *)(codes + ((size_t)b * 64 + cw + i) * 32 + 16 * h);
        float da[16], sa[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 d4 = *(const float4 *)(dsc + b * 64 + cw + 8 * g + 4 * h);
            da[4 * g] = d4.x, da[4 * g + 1] = d4.y, da[4 * g + 2] = d4.z, da[4 * g + 3] = d4.w;
            if constexpr (W::S1) {
                const float4 s4 = *(const float4 *)(ssc + b * 64 + cw + 8 * g + 4 * h);
                sa[4 * g] = s4.x, sa[4 * g + 1] = s4.y, sa[4 * g + 2] = s4.z, sa[4 * g + 3] = s4.w;
            }
        }
        float dw, mw;
        const v4i_t fw0 = mmq_frag_w<T>(A0 + (size_t)b * W::TS, h, dw, mw);
        const v16i_t s0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fx, fw0, zero16i, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            acc0[r] = acc0[r] + (dw * da[r]) * (float)s0[r];
            if constexpr (W::S1)
                acc0[r] = acc0[r] + mw * sa[r];
        }
        if (two) {
            const v4i_t fw1 = mmq_frag_w<T>(A1 + (size_t)b * W::TS, h, dw, mw);
            const v16i_t s1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fx, fw1, zero16i, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                acc1[r] = acc1[r] + (dw * da[r]) * (float)s1[r];
                if constexpr (W::S1)
                    acc1[r] = acc1[r] + mw * sa[r];
            }
        }
    }
    // lane (i, h) holds rows m0 + i and m0 + 32 + i; register r holds column n0 + cw + (r & 3) + 8 (r >> 2) + 4 h
    uint8_t *Cs = sl.slice(a.C, a.c_nb3, a.c_nb2);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long col = n0 + cw + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (col < a.n) {
            float *Cc = (float *)(Cs + col * a.c_nb1);
            if (m0 + i < a.m)
                Cc[m0 + i] = acc0[r];
            if (two && m0 + 32 + i < a.m)
                Cc[m0 + 32 + i] = acc1[r];
        }
    }
}

template <int T>
hipError_t launch(const mmq_args &a, long ne3, hipStream_t s) {
    using W = wt<T>;
    if (a.n <= 8) {
        const dim3 grid((unsigned)((a.m + 63) / 64), (unsigned)(ne3 * a.a_ne2 * a.hchunks), 1);
        lfamd_dispatch_nc(a.hg * (int)a.n, [&](auto nc) { mmq_gemv_kernel<T, decltype(nc)::value><<<grid, 256, 0, s>>>(a); });
    } else {
        const size_t smem = (size_t)a.kb * (2048 + 256 * (W::S1 ? 2 : 1));
        if (smem > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute((const void *)mmq_mfma_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess)
                return e;
        }
        const dim3 grid((unsigned)((a.m + 127) / 128), (unsigned)((a.n + 63) / 64), (unsigned)(a.ne2 * ne3));
        mmq_mfma_kernel<T><<<grid, 256, smem, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch(int Atype, const mmq_args &a, long ne3, hipStream_t s) {
    static const struct {
        int type;
        hipError_t (*go)(const mmq_args &, long, hipStream_t);
    } tab[] = {{LFAMD_TYPE_Q8_0, launch<LFAMD_TYPE_Q8_0>}, {LFAMD_TYPE_Q4_0, launch<LFAMD_TYPE_Q4_0>}, {LFAMD_TYPE_Q4_1, launch<LFAMD_TYPE_Q4_1>},
               {LFAMD_TYPE_Q5_0, launch<LFAMD_TYPE_Q5_0>}, {LFAMD_TYPE_Q5_1, launch<LFAMD_TYPE_Q5_1>}, {LFAMD_TYPE_IQ4_NL, launch<LFAMD_TYPE_IQ4_NL>}};
    for (const auto &e : tab)
        if (e.type == Atype)
            return e.go(a, ne3, s);
    return hipErrorInvalidValue; // (not reached: the check admits lfamd_block_k_type alone)
}

} // namespace

extern "C" int lfamd_mul_mat_batched_q(int Atype, const void *d_A, long m, long k, size_t a_nb1, size_t a_nb2, size_t a_nb3, long a_ne2,
                                       long a_ne3, const float *d_B, long n, size_t b_nb1, size_t b_nb2, size_t b_nb3, long ne2, long ne3,
                                       float *d_C, size_t c_nb1, size_t c_nb2, size_t c_nb3, unsigned flags, void *stream) {
    mmq_args a{{(const uint8_t *)d_A, (const uint8_t *)d_B, (uint8_t *)d_C, m, k, n, a_nb1, a_nb2, a_nb3, b_nb1, b_nb2, b_nb3,
                c_nb1, c_nb2, c_nb3, a_ne2, ne2}};
    const bool six = lfamd_block_k_type(Atype); // (k <= 1024: a work-group keeps its quantised activations in LDS)
    const lfamd_batched_desc d{six, 1024, 32, six ? lfamd_row_size(Atype, k) : 0, "Q8_0, Q4_0, Q4_1, Q5_0, Q5_1 or IQ4_NL rows only",
                               "k > 1024", "k is not a multiple of 32"};
    int rc;
    if (!lfamd_batched_check("lfamd_mul_mat_batched_q", d, a, a_ne3, ne3, flags, &rc))
        return rc;
    a.kb = (int)(k / 32);
    lfamd_batched_groups(a, a_ne3, ne3, a.hg, a.hchunks);
    return lfamd_launch_status(launch(Atype, a, ne3, (hipStream_t)stream));
}
