// flash_attn.hip — lfamd_flash_attn: GGML_OP_FLASH_ATTN_EXT on an F16 K / V cache in one fused launch (include/lfamd_hip.h), and
// lfamd_flash_attn_q: the same kernels on a Q8_0 / Q4_0 K and V cache (the operand types: fa_op, below).
//
// For each (i3, head h, query row j):  s_t = scale * <Q, K_t> + mask[j][t],  dst = sum_t softmax(s)_t V_t.  K and V are the -fa cache
// views (V NOT transposed), head h reads KV head h / (n_head / n_head_kv).  Reference: ggml_cuda_flash_attn_ext
// (ggml-cuda.cu.patch:8280-8400, dispatch :9987-10030).  Two routes, picked by n_q alone:
//   n_q <= 8  fa_decode_kernel: memory-bound.  One work-group per (KV chunk of FA_CHUNK keys, item, i3); an item is a KV head with all
//             n_q * group query rows of its group where those are <= 8 (K / V read once for the group), else one query head.  A key row
//             is D / 8 lanes x 16 bytes, straight to VGPRs; a wave takes 64 / (D / 8) keys per load, four loads in flight, and every
//             lane group keeps an online (m, l, o) of its own keys in f32.  Lane groups merge by lane exchange, the eight waves through
//             LDS in wave order.  n_kv <= FA_CHUNK: the work-group writes the result.  Otherwise it writes (o[D], m, l) to the
//             workspace and fa_combine_kernel merges the chunks in ascending order.
//   n_q > 8   fa_prefill_kernel: four waves, each owns 32 query rows of one head, Q as f16 MFMA fragments in registers.  KV tiles of
//             64 keys are register-staged into LDS (the next tile's loads are issued before the current tile's arithmetic), K with its
//             16-byte chunks XOR-swizzled by the row, V row-major with rows 64 bytes apart from a bank multiple and read through
//             ds_read_b64_tr_b16.  The swapped product mfma(K, Q) leaves a query row's scores in the 16 registers of two lanes, so
//             the softmax is lane-local but for one exchange with lane ^ 32, and the f32 scores become the B operand of the PV product
//             (A = V transposed by the LDS read) with no lane movement.  A tile whose mask is -inf for every row of the work-group
//             is never loaded, and a wave skips a 32-key half whose mask is -inf for all its rows: (m, l, o) of a row are the
//             same bits either way (m stays, the rescale factor is exactly 1, every p is +0).
// Scores are kept in log2 units: s2 = S * (scale * log2 e) + mask * log2 e, p = exp2(s2 - m).  A row maximum that is still -inf is
// replaced by 0 inside the exponentials only, so exp2(-inf - -inf) never occurs.
#include <math.h>

#include "entry_checks.h"

// keys per work-group of the decode route: a compile-time constant, so that a row's bits depend on D and n_kv alone
#ifndef LFAMD_FA_CHUNK
#define LFAMD_FA_CHUNK 256
#endif

namespace {

constexpr long FA_CHUNK = LFAMD_FA_CHUNK;
constexpr float FA_LOG2E = 1.44269504088896340736f;
constexpr int FA_NW = 8;    // waves of a decode work-group
constexpr int FA_SEG = 128; // KV tiles whose live flags the prefill route keeps in LDS at a time

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));

struct fa_args {
    const uint8_t *Q, *K, *V, *mask;
    uint8_t *dst;
    float *ws;
    size_t q_nb1, q_nb2, q_nb3, k_nb1, k_nb2, k_nb3, v_nb1, v_nb2, v_nb3, mask_nb1, dst_nb1, dst_nb2, dst_nb3;
    long n_q, n_kv, n_chunks;
    int n_head, n_head_kv, group;
    int shared; // decode: an item is a KV head with every query head of its group
    int mask16; // mask base and row stride are multiples of 16
    float c;    // scale * log2 e
};

__device__ static inline float fa_exp2(float x) { // v_exp_f32: exp2(-inf) = +0
    return __builtin_amdgcn_exp2f(x);
}

__device__ static inline float fa_neg_inf() {
    return -__builtin_inff();
}

// ----------------------------------------------------------------------------------------------------------- K / V operand types
// What the two routes ask of an operand type (lfamd_flash_attn: F16; lfamd_flash_attn_q: Q8_0, Q4_0 — K and V each have their own
// parameter, so a mixed pair is one more instantiation):
//   decode   piece: the 8 consecutive elements sl * 8 .. of a row that one lane keeps, raw in registers; off8(sl): where its load
//            starts in the row; ld8 / zero8; widen8: the f32 values (a block element is f32(d) * (float)code, exact)
//   prefill  stage<D>: one thread's share of a 64-key tile, raw in registers, moved in NLD steps (load: keys past n_kv are zeros,
//            never memory), and write<ROW, SWZ>: the same elements as f16 to LDS rows of ROW bytes, 16-byte chunk ch of row r at
//            chunk ch ^ (r & 7) where SWZ.  A block element is f16(d * code), rounded once to nearest even.
template <int T>
struct fa_op;

template <>
struct fa_op<LFAMD_TYPE_F16> {
    typedef uint4 piece;
    __device__ static inline int off8(int sl) { return sl * 16; }
    __device__ static inline piece ld8(const uint8_t *p) { return *(const uint4 *)p; }
    __device__ static inline piece zero8() { return make_uint4(0, 0, 0, 0); }
    __device__ static inline void widen8(const piece v, int, float (&f)[8]) {
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            f[2 * e] = h2f((uint16_t)(d[e] & 0xffff));
            f[2 * e + 1] = h2f((uint16_t)(d[e] >> 16));
        }
    }
    template <int D>
    struct stage {
        static constexpr int CH = D / 8;           // 16-byte chunks of a row
        static constexpr int NLD = 64 * CH / 256;  // 16-byte loads per thread and tile
        uint4 r[NLD];
        __device__ inline void load(int i, const uint8_t *base, size_t nb1, long t0, long n_kv, int tid) {
            const int idx = tid + 256 * i, row = idx / CH, ch = idx % CH;
            const long t = t0 + row;
            r[i] = t < n_kv ? *(const uint4 *)(base + t * nb1 + ch * 16) : make_uint4(0, 0, 0, 0);
        }
        template <int ROW, bool SWZ>
        __device__ inline void write(int i, uint8_t *lds, int tid) const {
            const int idx = tid + 256 * i, row = idx / CH, ch = idx % CH;
            *(uint4 *)(lds + row * ROW + ((SWZ ? ch ^ (row & 7) : ch) * 16)) = r[i];
        }
    };
};

// 4 NW bytes from the EVEN address p and no other byte: dword loads off their boundary, which the target allows
template <int NW>
__device__ static inline void fa_ld_even(const uint8_t *p, uint32_t (&W)[NW]) {
    struct __attribute__((packed, aligned(2))) words {
        uint32_t w[NW];
    };
    const words v = *(const words *)p;
#pragma unroll
    for (int j = 0; j < NW; j++)
        W[j] = v.w[j];
}

// A 32-block {f16 d, payload} of TS bytes (lfamd_block32<T>) on a 2-byte boundary; NIB: 16 bytes of nibbles (element j < 16 the low
// nibble of byte j, j + 16 its high nibble, value d * (nibble - 8)), else 32 int8 codes.
template <int T>
struct fa_block_op {
    static constexpr int TS = lfamd_block32<T>::TS;
    static constexpr bool NIB = !lfamd_block32<T>::BYTES;
    // A lane's 8 elements are 8 payload bytes; the four lanes of a block sit in one quad.  A lane loads those bytes and the two in
    // front of them through ONE address: in the quad's first lane the two are the block's d, which the quad takes from there.
    struct piece {
        uint32_t x[2], hs; // 10 bytes: x[0] bits 0 .. 15 the two in front
    };
    __device__ static inline int sub8(int sl) { return NIB ? sl & 1 : sl & 3; } // which 8 payload bytes hold the lane's elements
    __device__ static inline int off8(int sl) { return (sl >> 2) * TS + 8 * sub8(sl); }
    __device__ static inline piece ld8(const uint8_t *p) {
        piece r;
        fa_ld_even<2>(p, r.x);
        r.hs = *(const uint16_t *)(p + 8);
        return r;
    }
    __device__ static inline piece zero8() { return piece{{0, 0}, 0}; } // d = +0: every element a zero, whatever the code
    __device__ static inline void widen8(const piece v, int sl, float (&f)[8]) { // (every lane of the quad is here)
        const float d = h2f((uint16_t)dpp_u32<0x00>(v.x[0])); // quad_perm [0,0,0,0]
        uint32_t w[2] = {(v.x[0] >> 16) | (v.x[1] << 16), (v.x[1] >> 16) | (v.hs << 16)};
        if constexpr (NIB) { // nibble - 8
#pragma unroll
            for (int j = 0; j < 2; j++)
                w[j] = sub_per_byte<8>((w[j] >> (2 * (sl & 2))) & 0x0F0F0F0Fu);
        }
#pragma unroll
        for (int e = 0; e < 8; e++)
            f[e] = d * (float)(int8_t)(w[e >> 2] >> (8 * (e & 3)));
    }
    // Thread tid of 256: key tid >> 2 of the tile, quarter q = tid & 3 of its row: D = 128 one block, D = 64 half a block.
    template <int D>
    struct stage {
        static constexpr int HALVES = 128 / D, NE = 32 / HALVES; // threads per block; elements per thread
        static constexpr int NW = NIB ? 4 : NE / 4;              // payload dwords per thread
        static constexpr int NLD = 1;
        uint32_t w[NW], d;
        __device__ inline void load(int, const uint8_t *base, size_t nb1, long t0, long n_kv, int tid) {
            const int q = tid & 3, b = q / HALVES, hf = q % HALVES;
            const long t = t0 + (tid >> 2);
            d = 0;
#pragma unroll
            for (int j = 0; j < NW; j++)
                w[j] = NIB ? 0x88888888u : 0u; // code 0
            if (t < n_kv) {
                const uint8_t *blk = base + t * nb1 + b * TS;
                d = *(const uint16_t *)blk;
                fa_ld_even<NW>(blk + 2 + (NIB ? 0 : NE * hf), w);
            }
        }
        // f16(d * code) for every code: 0x6400 | u is the f16 1024 + u (u < 1024), so a byte permute and one exact packed subtraction
        // convert two codes, and the packed multiply by d rounds once.
        template <int ROW, bool SWZ>
        __device__ inline void write(int, uint8_t *lds, int tid) const {
            typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
            const int row = tid >> 2, q = tid & 3, hf = q % HALVES;
            const _Float16 dh = __builtin_bit_cast(_Float16, (uint16_t)d), bias = (_Float16)(NIB ? 1032.0f : 1152.0f);
            const half2_t d2 = {dh, dh}, b2 = {bias, bias};
            uint32_t u[NE / 4]; // four biased codes to a dword: code + 128, or the nibble
#pragma unroll
            for (int j = 0; j < NE / 4; j++) {
                if constexpr (!NIB)
                    u[j] = w[j] ^ 0x80808080u;
                else if constexpr (HALVES == 1)
                    u[j] = (w[j & 3] >> (4 * (j >> 2))) & 0x0F0F0F0Fu;
                else
                    u[j] = (w[j] >> (4 * hf)) & 0x0F0F0F0Fu;
            }
#pragma unroll
            for (int c = 0; c < NE / 8; c++) {
                uint32_t o[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t x = __builtin_amdgcn_perm(0x64646464u, u[2 * c + (e >> 1)], (e & 1) ? 0x04030402u : 0x04010400u);
                    o[e] = __builtin_bit_cast(uint32_t, (__builtin_bit_cast(half2_t, x) - b2) * d2);
                }
                const int ch = q * (NE / 8) + c;
                *(uint4 *)(lds + row * ROW + ((SWZ ? ch ^ (row & 7) : ch) * 16)) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    };
};

template <>
struct fa_op<LFAMD_TYPE_Q8_0> : fa_block_op<LFAMD_TYPE_Q8_0> {};
template <>
struct fa_op<LFAMD_TYPE_Q4_0> : fa_block_op<LFAMD_TYPE_Q4_0> {};

// ------------------------------------------------------------------------------------------------------------------ decode route

template <int LPK>
__device__ static inline float fa_lane_sum(float v) { // over the LPK (8 or 16) lanes of a key, in every one of them
    v += dpp_f32<DPP_XOR1>(v);
    v += dpp_f32<DPP_XOR2>(v);
    v += dpp_f32<DPP_HALF_MIRROR>(v);
    if constexpr (LPK == 16)
        v += dpp_f32<DPP_MIRROR>(v);
    return v;
}

// NC: columns (query row x head of the item) a lane keeps, the live count rounded up to 1, 2, 4 or 8
template <int KT, int VT, int D, int NC>
__global__ __launch_bounds__(64 * FA_NW) void fa_decode_kernel(const fa_args a) {
    using KO = fa_op<KT>;
    using VO = fa_op<VT>;
    constexpr int LPK = D / 8, KPW = 64 / LPK, RU = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane / LPK, sl = lane % LPK;
    const int items = a.shared ? a.n_head_kv : a.n_head;
    const long i3 = blockIdx.y / items;
    const int it = (int)(blockIdx.y % items);
    const int h0 = a.shared ? it * a.group : it, hk = a.shared ? it : it / a.group;
    const int nq = (int)a.n_q, nc = a.shared ? a.group * nq : nq;
    const float ninf = fa_neg_inf();

    float q[NC][8];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int cc = c < nc ? c : 0;
        const uint8_t *row = a.Q + i3 * a.q_nb3 + (size_t)(h0 + cc / nq) * a.q_nb2 + (size_t)(cc % nq) * a.q_nb1 + sl * 32;
        const float4 lo = *(const float4 *)row, hi = *(const float4 *)(row + 16);
        q[c][0] = lo.x, q[c][1] = lo.y, q[c][2] = lo.z, q[c][3] = lo.w, q[c][4] = hi.x, q[c][5] = hi.y, q[c][6] = hi.z, q[c][7] = hi.w;
    }
    float m[NC], l[NC], o[NC][8];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        m[c] = ninf, l[c] = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; e++)
            o[c][e] = 0.0f;
    }
    const long t_begin = (long)blockIdx.x * FA_CHUNK, t_end = t_begin + FA_CHUNK < a.n_kv ? t_begin + FA_CHUNK : a.n_kv;
    const uint8_t *Kb = a.K + i3 * a.k_nb3 + (size_t)hk * a.k_nb2 + KO::off8(sl);
    const uint8_t *Vb = a.V + i3 * a.v_nb3 + (size_t)hk * a.v_nb2 + VO::off8(sl);
    for (long tb = t_begin + wave * (KPW * RU); tb < t_end; tb += FA_NW * KPW * RU) {
        typename KO::piece kr[RU];
        typename VO::piece vr[RU];
#pragma unroll
        for (int u = 0; u < RU; u++) { // keys past the chunk: zeros, never memory
            const long t = tb + u * KPW + slot;
            kr[u] = KO::zero8(), vr[u] = VO::zero8();
            if (t < t_end)
                kr[u] = KO::ld8(Kb + t * a.k_nb1), vr[u] = VO::ld8(Vb + t * a.v_nb1);
        }
        float s[NC][RU];
#pragma unroll
        for (int u = 0; u < RU; u++) {
            float kf[8];
            KO::widen8(kr[u], sl, kf);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c < nc) {
                    float acc = 0.0f;
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        acc = fmaf(kf[e], q[c][e], acc);
                    s[c][u] = fa_lane_sum<LPK>(acc);
                }
            }
        }
        float vf[RU][8];
#pragma unroll
        for (int u = 0; u < RU; u++)
            VO::widen8(vr[u], sl, vf[u]);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                const uint8_t *mrow = a.mask + (size_t)(c % nq) * a.mask_nb1;
                float s2[RU];
#pragma unroll
                for (int u = 0; u < RU; u++) {
                    const long t = tb + u * KPW + slot;
                    float mk = ninf;
                    if (t < t_end)
                        mk = a.mask ? h2f(*(const uint16_t *)(mrow + t * 2)) * FA_LOG2E : 0.0f;
                    s2[u] = fmaf(s[c][u], a.c, mk);
                }
                const float mn = fmaxf(m[c], fmaxf(fmaxf(s2[0], s2[1]), fmaxf(s2[2], s2[3])));
                const float mu = mn == ninf ? 0.0f : mn;
                const float al = fa_exp2(m[c] - mu);
                float p[RU];
#pragma unroll
                for (int u = 0; u < RU; u++)
                    p[u] = fa_exp2(s2[u] - mu);
                l[c] = l[c] * al + ((p[0] + p[1]) + (p[2] + p[3]));
                m[c] = mn;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    float v = o[c][e] * al;
#pragma unroll
                    for (int u = 0; u < RU; u++)
                        v = fmaf(p[u], vf[u][e], v);
                    o[c][e] = v;
                }
            }
        }
    }
    // the wave's lane groups: a butterfly, the same bits in both partners (the sums commute)
#pragma unroll
    for (int x = LPK; x < 64; x <<= 1) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                const float mo = __shfl_xor(m[c], x, 64), lo = __shfl_xor(l[c], x, 64);
                const float mn = fmaxf(m[c], mo), mu = mn == ninf ? 0.0f : mn;
                const float ea = fa_exp2(m[c] - mu), eb = fa_exp2(mo - mu);
                l[c] = l[c] * ea + lo * eb;
                m[c] = mn;
#pragma unroll
                for (int e = 0; e < 8; e++)
                    o[c][e] = o[c][e] * ea + __shfl_xor(o[c][e], x, 64) * eb;
            }
        }
    }
    __shared__ float part[FA_NW][NC][D + 2]; // per wave and column: o[D], m, l
    if (slot == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
#pragma unroll
                for (int e = 0; e < 8; e++)
                    part[wave][c][sl * 8 + e] = o[c][e];
                if (sl == 0)
                    part[wave][c][D] = m[c], part[wave][c][D + 1] = l[c];
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nc * D; idx += 64 * FA_NW) { // the waves, in wave order
        const int c = idx / D, d = idx % D;
        float mn = ninf;
#pragma unroll
        for (int w = 0; w < FA_NW; w++)
            mn = fmaxf(mn, part[w][c][D]);
        const float mu = mn == ninf ? 0.0f : mn;
        float ov = 0.0f, lv = 0.0f;
#pragma unroll
        for (int w = 0; w < FA_NW; w++) {
            const float e = fa_exp2(part[w][c][D] - mu);
            ov += part[w][c][d] * e;
            lv += part[w][c][D + 1] * e;
        }
        const int head = h0 + c / nq, j = c % nq;
        if (a.n_chunks > 1) {
            float *w = a.ws + (((i3 * a.n_head + head) * nq + j) * a.n_chunks + blockIdx.x) * (D + 2);
            w[d] = ov;
            if (d == 0)
                w[D] = mn, w[D + 1] = lv;
        } else {
            *(float *)(a.dst + i3 * a.dst_nb3 + (size_t)j * a.dst_nb2 + (size_t)head * a.dst_nb1 + d * 4) = ov / lv;
        }
    }
}

// One work-group of 512 threads per (i3, head, j).  The order is a function of the chunk count alone: the maximum over all chunks;
// then, per tile of 512 chunks, thread (g, d) adds o_c[d] * exp2(m_c - m) over the tile's chunks c = g, g + G, ... (G = 512 / D) in
// ascending order and thread t keeps l_c * exp2(m_c - m) of chunk t; the G partial o in ascending g, the 512 partial l by halving.
template <int D>
__global__ __launch_bounds__(512) void fa_combine_kernel(const fa_args a) {
    constexpr int NT = 512, G = NT / D;
    __shared__ float red[NT], es[NT], og[G][D];
    const long row = blockIdx.x;
    const int tid = threadIdx.x, g = tid / D, d = tid % D, nq = (int)a.n_q;
    const float *p = a.ws + row * a.n_chunks * (D + 2);
    const float ninf = fa_neg_inf();
    float mx = ninf;
    for (long c = tid; c < a.n_chunks; c += NT)
        mx = fmaxf(mx, p[c * (D + 2) + D]);
    red[tid] = mx;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s)
            red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float mn = red[0], mu = mn == ninf ? 0.0f : mn;
    float ov = 0.0f, lv = 0.0f;
    for (long c0 = 0; c0 < a.n_chunks; c0 += NT) {
        __syncthreads(); // red[0] and the previous tile's es[] have been read
        const long c = c0 + tid;
        const float e = c < a.n_chunks ? fa_exp2(p[c * (D + 2) + D] - mu) : 0.0f;
        es[tid] = e;
        if (c < a.n_chunks)
            lv += p[c * (D + 2) + D + 1] * e;
        __syncthreads();
        const int nt = (int)(a.n_chunks - c0 < NT ? a.n_chunks - c0 : NT);
#pragma unroll 4
        for (int i = g; i < nt; i += G)
            ov += p[(c0 + i) * (D + 2) + d] * es[i];
    }
    red[tid] = lv;
    og[g][d] = ov;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s)
            red[tid] += red[tid + s];
        __syncthreads();
    }
    if (g == 0) {
        float o = og[0][d];
#pragma unroll
        for (int gg = 1; gg < G; gg++)
            o += og[gg][d];
        const long j = row % nq, head = row / nq % a.n_head, i3 = row / nq / a.n_head;
        *(float *)(a.dst + i3 * a.dst_nb3 + j * a.dst_nb2 + head * a.dst_nb1 + d * 4) = o / red[0];
    }
}

// ----------------------------------------------------------------------------------------------------------------- prefill route

// Waves per SIMD the register allocator is held to.  1 asks for nothing (the F16 code is what it was).  2 for the block tiles at
// D = 128, whose staged registers are 18 (Q8_0) or 10 (Q4_0) against the F16 tile's 32: held to 256 registers the compiler keeps the
// MFMA accumulators in ordinary registers (no second register file, no copies between the two, no scratch), and two work-groups share
// a CU.  D = 64 has not been timed and is left alone.
template <int KT, int VT, int D>
constexpr int fa_prefill_waves = KT != LFAMD_TYPE_F16 && VT != LFAMD_TYPE_F16 && D == 128 ? 2 : 1;

template <int KT, int VT, int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(fa_prefill_waves<KT, VT, D>))) void fa_prefill_kernel(const fa_args a) {
    constexpr int KROW = 2 * D;               // K tile: rows of 2 D bytes, chunk ch of row r at chunk ch ^ (r & 7)
    constexpr int VROW = 2 * D + 64;          // V tile: four consecutive rows start 16 banks apart (the transposed read takes 4 rows x 64 B per half)
    constexpr int KS = D / 16, DB = D / 32;   // MFMA k-steps of QK; 32-wide blocks of D
    __shared__ __attribute__((aligned(16))) uint8_t Ks[64 * KROW];
    __shared__ __attribute__((aligned(16))) uint8_t Vs[64 * VROW];
    __shared__ uint8_t live[FA_SEG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = lane & 31, h = lane >> 5;
    const int head = (int)(blockIdx.x % a.n_head), hk = head / a.group;
    const long i3 = blockIdx.x / a.n_head;
    const long wg_row0 = (long)blockIdx.y * 128, row0 = wg_row0 + wave * 32;
    const long wg_rows = a.n_q - wg_row0 < 128 ? a.n_q - wg_row0 : 128;
    const bool wave_on = row0 < a.n_q; // (uniform) the wave owns at least one query row
    const long jq = row0 + qi < a.n_q ? row0 + qi : a.n_q - 1; // rows past the edge repeat the last row and are not stored
    const float ninf = fa_neg_inf();

    half8_t qf[KS]; // B operand of k-step s: Q[jq][16 s + 8 h + 0..7], rounded once to f16
    {
        const uint8_t *qrow = a.Q + i3 * a.q_nb3 + (size_t)head * a.q_nb2 + jq * a.q_nb1;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const float4 lo = *(const float4 *)(qrow + (16 * s + 8 * h) * 4), hi = *(const float4 *)(qrow + (16 * s + 8 * h) * 4 + 16);
            const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int e = 0; e < 8; e++)
                qf[s][e] = (_Float16)x[e];
        }
    }
    float16_t_ acc[DB]; // acc[db][r]: d = 32 db + (r & 3) + 8 (r >> 2) + 4 h of query row qi
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
        for (int r = 0; r < 16; r++)
            acc[db][r] = 0.0f;
    float m = ninf, l = 0.0f; // m: of the whole row (both lanes); l: of this lane's keys

    const uint8_t *Kb = a.K + i3 * a.k_nb3 + (size_t)hk * a.k_nb2;
    const uint8_t *Vb = a.V + i3 * a.v_nb3 + (size_t)hk * a.v_nb2;
    const uint8_t *mrow = a.mask + jq * a.mask_nb1;
    // transposed V read: lane 16 g + i supplies row 4 h + (i >> 2), columns 16 (g & 1) + 4 (i & 3) .. + 3 of its block
    const int tr_off = (4 * h + ((lane & 15) >> 2)) * VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    const long n_tiles = (a.n_kv + 63) / 64;
    typename fa_op<KT>::template stage<D> kst; // the staged tile: raw in registers from stage_load to stage_write
    typename fa_op<VT>::template stage<D> vst;

    constexpr int KLD = decltype(kst)::NLD, VLD = decltype(vst)::NLD;
    auto stage_load = [&](long tile) {
#pragma unroll
        for (int i = 0; i < (KLD > VLD ? KLD : VLD); i++) {
            if (i < KLD)
                kst.load(i, Kb, a.k_nb1, tile * 64, a.n_kv, tid);
            if (i < VLD)
                vst.load(i, Vb, a.v_nb1, tile * 64, a.n_kv, tid);
        }
    };
    auto stage_write = [&]() {
#pragma unroll
        for (int i = 0; i < (KLD > VLD ? KLD : VLD); i++) {
            if (i < KLD)
                kst.template write<KROW, true>(i, Ks, tid);
            if (i < VLD)
                vst.template write<VROW, false>(i, Vs, tid);
        }
    };
    auto compute = [&](long tile) {
#pragma unroll 1
        for (int sub = 0; sub < 2; sub++) {
            const long kb = tile * 64 + 32 * sub;
            if (kb >= a.n_kv)
                break;
            // this lane's 16 keys: kb + (r & 3) + 8 (r >> 2) + 4 h
            float mk[16];
            bool any = false;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const long t = kb + 8 * g + 4 * h;
                uint16_t mb[4];
                if (!a.mask) {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        mb[e] = t + e < a.n_kv ? 0 : 0xfc00;
                } else if (a.mask16 && t + 4 <= a.n_kv) {
                    const uint2 v = *(const uint2 *)(mrow + t * 2);
                    mb[0] = (uint16_t)(v.x & 0xffff), mb[1] = (uint16_t)(v.x >> 16), mb[2] = (uint16_t)(v.y & 0xffff), mb[3] = (uint16_t)(v.y >> 16);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        mb[e] = t + e < a.n_kv ? *(const uint16_t *)(mrow + (t + e) * 2) : 0xfc00;
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    mk[4 * g + e] = h2f(mb[e]) * FA_LOG2E;
                    any |= mb[e] != 0xfc00;
                }
            }
            if (__ballot(any) == 0) // every key of this half is -inf for every row of the wave: (m, l, o) would not move
                continue;
            float16_t_ S;
#pragma unroll
            for (int r = 0; r < 16; r++)
                S[r] = 0.0f;
            const int kr = 32 * sub + qi;
#pragma unroll
            for (int s = 0; s < KS; s++) {
                const half8_t kf = *(const half8_t *)(Ks + kr * KROW + (((2 * s + h) ^ (kr & 7)) * 16));
                S = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], S, 0, 0, 0);
            }
            float mx = ninf;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                S[r] = fmaf(S[r], a.c, mk[r]);
                mx = fmaxf(mx, S[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx), mu = mn == ninf ? 0.0f : mn;
            const float al = fa_exp2(m - mu);
            m = mn;
            float ps = 0.0f;
            half8_t pf[2]; // B operand of PV k-step s: registers 8 s .. 8 s + 7, rounded once to f16
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float p = fa_exp2(S[r] - mu);
                ps += p;
                pf[r >> 3][r & 7] = (_Float16)p;
            }
            l = l * al + ps;
            if (__ballot(al != 1.0f) != 0) {
#pragma unroll
                for (int db = 0; db < DB; db++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        acc[db][r] *= al;
            }
#pragma unroll
            for (int db = 0; db < DB; db++) {
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    // A operand: element j = V[key 32 sub + 16 s + 8 (j >> 2) + 4 h + (j & 3)][32 db + qi]
                    const uint8_t *vp = Vs + tr_off + (32 * sub + 16 * s) * VROW + db * 64;
                    const fp16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t *)vp);
                    const fp16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t *)(vp + 8 * VROW));
                    const half4_t w0 = __builtin_bit_cast(half4_t, v0), w1 = __builtin_bit_cast(half4_t, v1);
                    const half8_t vt = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
                    acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vt, pf[s], acc[db], 0, 0, 0);
                }
            }
        }
    };

    for (long seg0 = 0; seg0 < n_tiles; seg0 += FA_SEG) {
        const int seg_n = (int)(n_tiles - seg0 < FA_SEG ? n_tiles - seg0 : FA_SEG);
        if (a.mask) { // live[t]: some row of the work-group has a key of tile seg0 + t that is not -inf.  Rows from the last up: causal tiles answer at once
            for (int t = wave; t < seg_n; t += 4) {
                const long k0 = (seg0 + t) * 64 + (lane & 7) * 8;
                bool found = false;
                for (long rb = wg_rows - 1; rb >= 0 && !found; rb -= 8) {
                    const long r = rb - (lane >> 3);
                    bool fin = false;
                    if (r >= 0) {
                        const uint8_t *p = a.mask + (wg_row0 + r) * a.mask_nb1 + k0 * 2;
                        if (a.mask16 && k0 + 8 <= a.n_kv) {
                            const uint4 v = *(const uint4 *)p;
                            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                fin |= (d[e] & 0xffff) != 0xfc00 || (d[e] >> 16) != 0xfc00;
                        } else {
#pragma unroll
                            for (int e = 0; e < 8; e++)
                                fin |= k0 + e < a.n_kv && *(const uint16_t *)(p + e * 2) != 0xfc00;
                        }
                    }
                    found = __ballot(fin) != 0;
                }
                if (lane == 0)
                    live[t] = found;
            }
        } else {
            if (tid < seg_n)
                live[tid] = 1;
        }
        __syncthreads();
        int cur = 0;
        while (cur < seg_n && !live[cur])
            cur++;
        if (cur < seg_n)
            stage_load(seg0 + cur);
        while (cur < seg_n) {
            __syncthreads(); // the previous tile's LDS reads are over
            stage_write();
            __syncthreads();
            int nxt = cur + 1;
            while (nxt < seg_n && !live[nxt])
                nxt++;
            if (nxt < seg_n)
                stage_load(seg0 + nxt);
            if (wave_on)
                compute(seg0 + cur);
            cur = nxt;
        }
        __syncthreads(); // before live[] is rewritten
    }
    if (!wave_on || row0 + qi >= a.n_q)
        return;
    const float lt = l + __shfl_xor(l, 32, 64);
    uint8_t *out = a.dst + i3 * a.dst_nb3 + jq * a.dst_nb2 + (size_t)head * a.dst_nb1;
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            float4 v;
            v.x = acc[db][4 * g] / lt, v.y = acc[db][4 * g + 1] / lt, v.z = acc[db][4 * g + 2] / lt, v.w = acc[db][4 * g + 3] / lt;
            *(float4 *)(out + (32 * db + 8 * g + 4 * h) * 4) = v;
        }
}

// ------------------------------------------------------------------------------------------------------------------------- host

// the split of the decode route: chunks per row (1: no split, no workspace)
static long fa_chunks(long n_q, long n_kv) {
    return n_q > 8 || n_kv <= FA_CHUNK ? 1 : (n_kv + FA_CHUNK - 1) / FA_CHUNK;
}

// the launches of a checked call on the pair (KT, VT)
template <int KT, int VT>
static void fa_go(const fa_args &a, long D, long ne3, hipStream_t s) {
    if (a.n_q <= 8) {
        const int nc = (int)(a.shared ? a.n_q * a.group : a.n_q);
        const dim3 grid((unsigned)a.n_chunks, (unsigned)(ne3 * (a.shared ? a.n_head_kv : a.n_head)), 1);
        if (D == 64)
            lfamd_dispatch_nc(nc, [&](auto c) { fa_decode_kernel<KT, VT, 64, decltype(c)::value><<<grid, 64 * FA_NW, 0, s>>>(a); });
        else
            lfamd_dispatch_nc(nc, [&](auto c) { fa_decode_kernel<KT, VT, 128, decltype(c)::value><<<grid, 64 * FA_NW, 0, s>>>(a); });
        if (a.n_chunks > 1) {
            const unsigned rows = (unsigned)(ne3 * a.n_head * a.n_q);
            if (D == 64)
                fa_combine_kernel<64><<<rows, 512, 0, s>>>(a);
            else
                fa_combine_kernel<128><<<rows, 512, 0, s>>>(a);
        }
    } else {
        const dim3 grid((unsigned)(a.n_head * ne3), (unsigned)((a.n_q + 127) / 128), 1);
        if (D == 64)
            fa_prefill_kernel<KT, VT, 64><<<grid, 256, 0, s>>>(a);
        else
            fa_prefill_kernel<KT, VT, 128><<<grid, 256, 0, s>>>(a);
    }
}

} // namespace

extern "C" size_t lfamd_flash_attn_workspace(long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3) {
    (void)n_head_kv;
    if (D < 1 || n_q < 1 || n_kv < 1 || n_head < 1 || ne3 < 1)
        return 0;
    const long chunks = fa_chunks(n_q, n_kv);
    return chunks > 1 ? (size_t)ne3 * (size_t)n_head * (size_t)n_q * (size_t)chunks * (size_t)(D + 2) * 4 : 0;
}

// The checks of include/lfamd_hip.h in their documented order, as one table for lfamd_run_checks (entry_checks.h: evaluated whole, so
// every row guards itself); no device call.  `entry`: asked by lfamd_flash_attn, to which every flag is reserved; else by
// lfamd_flash_attn_check, which takes LFAMD_CHECK_UNPLACED.  `q`: the table of lfamd_flash_attn_q — the pair rule, K / V on 2-byte
// boundaries, rows of blocks.  true: launch.  false: *rc is the answer (LFAMD_OK: an empty call).
static bool fa_check(bool q, bool entry, const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3, int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2,
                     size_t k_nb3, int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3, const void *d_mask, size_t mask_nb1, long D,
                     long n_q, long n_kv, long n_head, long n_head_kv, long ne3, float max_bias, const float *d_dst, size_t dst_nb1, size_t dst_nb2,
                     size_t dst_nb3, const void *d_workspace, size_t workspace_bytes, unsigned flags, int *rc) {
    const auto [unplaced, reserved] = lfamd_check_flags_of(entry, flags);
    const size_t need = lfamd_flash_attn_workspace(D, n_q, n_kv, n_head, n_head_kv, ne3);
    const bool f16_pair = Ktype == LFAMD_TYPE_F16 && Vtype == LFAMD_TYPE_F16;
    const bool block_pair = Ktype == Vtype && (Ktype == LFAMD_TYPE_Q8_0 || Ktype == LFAMD_TYPE_Q4_0);
    const uintptr_t qd_bits = (uintptr_t)d_Q | q_nb1 | q_nb2 | q_nb3 | (uintptr_t)d_dst | dst_nb1 | dst_nb2 | dst_nb3;
    const uintptr_t kv_bits = (uintptr_t)d_K | k_nb1 | k_nb2 | k_nb3 | (uintptr_t)d_V | v_nb1 | v_nb2 | v_nb3;
    const lfamd_check_row checks[] = {
        {D < 0 || n_q < 0 || n_kv < 0 || n_head < 0 || n_head_kv < 0 || ne3 < 0, LFAMD_ERR_INVALID, "negative dimension"},
        {n_q == 0 || n_head == 0 || ne3 == 0, LFAMD_OK, nullptr},
        {!q && !f16_pair, LFAMD_ERR_UNSUPPORTED, "F16 K and V only"},
        {q && f16_pair, LFAMD_ERR_UNSUPPORTED, "F16 K and V: that is lfamd_flash_attn"},
        {q && !block_pair, LFAMD_ERR_UNSUPPORTED, "the K / V types are not (Q8_0, Q8_0) or (Q4_0, Q4_0)"},
        {D != 64 && D != 128, LFAMD_ERR_UNSUPPORTED, "head size is not 64 or 128"},
        {max_bias != 0.0f, LFAMD_ERR_UNSUPPORTED, "max_bias != 0 (ALiBi)"},
        {n_head > 65535 || ne3 > 65535 || (size_t)n_head * (size_t)ne3 > 65535 || (n_q + 127) / 128 > 65535, LFAMD_ERR_UNSUPPORTED,
         "more than 65535 slices (n_head * ne3) or 128-row query blocks"},
        {n_kv == 0, LFAMD_ERR_UNSUPPORTED, "n_kv == 0"},
        {!unplaced && (!d_Q || !d_K || !d_V || !d_dst || (!d_workspace && workspace_bytes != 0)), LFAMD_ERR_INVALID, "null pointer"},
        {n_head_kv < 1 || n_head % n_head_kv != 0, LFAMD_ERR_INVALID, "n_head is not a multiple of n_head_kv"},
        {!q && (qd_bits | kv_bits) % 16 != 0, LFAMD_ERR_INVALID, "a Q / K / V / dst base or stride is not a multiple of 16"},
        {q && qd_bits % 16 != 0, LFAMD_ERR_INVALID, "a Q / dst base or stride is not a multiple of 16"},
        {q && kv_bits % 2 != 0, LFAMD_ERR_INVALID, "a K / V base or stride is not a multiple of 2"},
        {d_mask && (((uintptr_t)d_mask | mask_nb1) % 2 != 0 || mask_nb1 < (size_t)n_kv * 2), LFAMD_ERR_INVALID,
         "mask base / row stride is odd or the stride is smaller than the row"},
        {k_nb1 < lfamd_row_size(Ktype, D) || v_nb1 < lfamd_row_size(Vtype, D) || q_nb1 < (size_t)D * 4 || dst_nb1 < (size_t)D * 4, LFAMD_ERR_INVALID,
         "a row stride is smaller than the row"},
        {reserved != 0, LFAMD_ERR_INVALID, "flags are reserved (0)"},
        {!unplaced && workspace_bytes < need, LFAMD_ERR_WORKSPACE, "workspace smaller than lfamd_flash_attn_workspace()"},
    };
    return lfamd_run_checks(q ? "lfamd_flash_attn_q" : "lfamd_flash_attn", checks, rc);
}

// the argument lists of the exported calls, written once
#define FA_CHECK_PARAMS                                                                                                                    \
    const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3, int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,     \
        int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3, const void *d_mask, size_t mask_nb1, long D, long n_q,       \
        long n_kv, long n_head, long n_head_kv, long ne3, float max_bias, const float *d_dst, size_t dst_nb1, size_t dst_nb2,              \
        size_t dst_nb3, const void *d_workspace, size_t workspace_bytes, unsigned flags
#define FA_CHECK_ARGS                                                                                                                      \
    d_Q, q_nb1, q_nb2, q_nb3, Ktype, d_K, k_nb1, k_nb2, k_nb3, Vtype, d_V, v_nb1, v_nb2, v_nb3, d_mask, mask_nb1, D, n_q, n_kv, n_head,   \
        n_head_kv, ne3, max_bias, d_dst, dst_nb1, dst_nb2, dst_nb3, d_workspace, workspace_bytes, flags
#define FA_CALL_PARAMS                                                                                                                     \
    const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3, int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,     \
        int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3, const void *d_mask, size_t mask_nb1, long D, long n_q,       \
        long n_kv, long n_head, long n_head_kv, long ne3, float scale, float max_bias, float *d_dst, size_t dst_nb1, size_t dst_nb2,       \
        size_t dst_nb3, void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream
#define FA_CALL_ARGS                                                                                                                       \
    d_Q, q_nb1, q_nb2, q_nb3, Ktype, d_K, k_nb1, k_nb2, k_nb3, Vtype, d_V, v_nb1, v_nb2, v_nb3, d_mask, mask_nb1, D, n_q, n_kv, n_head,   \
        n_head_kv, ne3, scale, max_bias, d_dst, dst_nb1, dst_nb2, dst_nb3, d_workspace, workspace_bytes, flags, stream

// the checks, then the launches of the pair
static int fa_call(bool q, FA_CALL_PARAMS) {
    int rc;
    if (!fa_check(q, true, FA_CHECK_ARGS, &rc))
        return rc;

    fa_args a{};
    a.Q = (const uint8_t *)d_Q, a.K = (const uint8_t *)d_K, a.V = (const uint8_t *)d_V, a.mask = (const uint8_t *)d_mask;
    a.dst = (uint8_t *)d_dst, a.ws = (float *)d_workspace;
    a.q_nb1 = q_nb1, a.q_nb2 = q_nb2, a.q_nb3 = q_nb3, a.k_nb1 = k_nb1, a.k_nb2 = k_nb2, a.k_nb3 = k_nb3;
    a.v_nb1 = v_nb1, a.v_nb2 = v_nb2, a.v_nb3 = v_nb3, a.mask_nb1 = mask_nb1, a.dst_nb1 = dst_nb1, a.dst_nb2 = dst_nb2, a.dst_nb3 = dst_nb3;
    a.n_q = n_q, a.n_kv = n_kv, a.n_chunks = fa_chunks(n_q, n_kv);
    a.n_head = (int)n_head, a.n_head_kv = (int)n_head_kv, a.group = (int)(n_head / n_head_kv);
    a.shared = n_q * a.group <= 8;
    a.mask16 = d_mask && (((uintptr_t)d_mask | mask_nb1) % 16 == 0);
    a.c = scale * FA_LOG2E;
    hipStream_t s = (hipStream_t)stream;
    if (Ktype == LFAMD_TYPE_Q8_0)
        fa_go<LFAMD_TYPE_Q8_0, LFAMD_TYPE_Q8_0>(a, D, ne3, s);
    else if (Ktype == LFAMD_TYPE_Q4_0)
        fa_go<LFAMD_TYPE_Q4_0, LFAMD_TYPE_Q4_0>(a, D, ne3, s);
    else
        fa_go<LFAMD_TYPE_F16, LFAMD_TYPE_F16>(a, D, ne3, s);
    return lfamd_launch_status(hipGetLastError());
}

extern "C" int lfamd_flash_attn_check(FA_CHECK_PARAMS) {
    int rc = LFAMD_OK;
    (void)fa_check(false, false, FA_CHECK_ARGS, &rc);
    return rc;
}

extern "C" int lfamd_flash_attn(FA_CALL_PARAMS) {
    return fa_call(false, FA_CALL_ARGS);
}

extern "C" int lfamd_flash_attn_q_check(FA_CHECK_PARAMS) {
    int rc = LFAMD_OK;
    (void)fa_check(true, false, FA_CHECK_ARGS, &rc);
    return rc;
}

extern "C" int lfamd_flash_attn_q(FA_CALL_PARAMS) {
    return fa_call(true, FA_CALL_ARGS);
}
