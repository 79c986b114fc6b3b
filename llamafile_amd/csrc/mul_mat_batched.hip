// mul_mat_batched.hip — lfamd_mul_mat_batched: a whole attention product (KQ or KQV) in ONE launch.
//
// GGML_OP_MUL_MAT where src0 is the F16 KV cache (a permuted view, ne[2] = KV heads) and src1 is F32 with ne[2] = query heads:
// r2 = ne2 / a_ne2 query heads share one K / V head (grouped-query attention), r3 likewise in dim 3.  Everything is addressed
// through ggml's byte strides, so the call takes the tensors' own pointers and nb[]: no packed image, no workspace, no copy.
// Reference: ggml_cuda_mul_mat_vec_p021 / _nc / ggml_cuda_mul_mat_batched_cublas (ggml-cuda.cu.patch:18424-18433); the broadcast of
// k_compute_batched_ptrs (:18207-18229) is index arithmetic here, not a pointer array.
//
// Two bodies, picked by n alone — the arithmetic of lfamd_mul_mat's float route (gemv_float.hip / the f16 MFMA batch body):
//   n <= 8  mmb_gemv_kernel: f16 weights widened to f32, f32 activations, fmaf.  LPR lanes walk a row in steps of 8 elements
//           (one 16-byte load per lane): 16 lanes for k <= 128 (KQ: a wave takes four rows per load), 64 lanes otherwise (KQV:
//           few rows, long k: the four waves of a work-group share four rows and take every fourth 512-element step of k each).  A work-group item is (KV head, chunk of `hg` query heads of its group): where r2 * n <= 8 the
//           K / V rows are read ONCE for all query heads of the group; larger groups run ceil(r2 / hg) items.
//           Order of one output's sum, a function of k alone: lane l adds its elements 8 (l + LPR c) .. + 7, c = 0, 1, ... (64
//           lanes: c = w, w + 4, ... in wave w), in ascending order into one fmaf chain (elements past k are zeros), then the lanes
//           are added in the DPP tree below (64 lanes: then the four waves' sums as (w0 + w1) + (w2 + w3), through LDS).
//           The element-wise loads of unaligned layouts and of the k tail feed the same chain, so the layout does not move a bit.
//   n > 8   mmb_mfma_kernel: batched.hip's skeleton on byte strides — one wave = 32 columns x two 32-row tiles on
//           v_mfma_f32_32x32x16_f16, four waves = 128 rows x 64 columns, the B fragment from two 16-byte f32 loads rounded to f16
//           (nearest-even) in registers and used for both row tiles.  Slices on blockIdx.z in i12-major order: the r2 heads of a
//           group are neighbours and find their K / V slice in L2.
// Neither body holds anything across slices: a slice's bits are those of the call on that slice alone.
// The argument checks, the slice geometry and the index rule are mul_mat_batched_common.h's, shared with mul_mat_batched_q.hip.
#include "mul_mat_batched_common.h"

namespace {

struct mmb_args : lfamd_batched_geom {
    int hg, hchunks; // GEMV: query heads per item, items per group
};

// eight weights of a row from element k0 on, widened; zeros past k.  ALIGNED: one 16-byte load where the eight lie inside the row
template <bool ALIGNED>
__device__ static inline void mmb_ld_w8(const uint8_t *row, long k0, long k, float (&f)[8]) {
    if (ALIGNED && k0 + 8 <= k) {
        const uint4 v = *(const uint4 *)(row + k0 * 2);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            f[2 * e] = h2f((uint16_t)(d[e] & 0xffff));
            f[2 * e + 1] = h2f((uint16_t)(d[e] >> 16));
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++)
            f[e] = k0 + e < k ? h2f(*(const uint16_t *)(row + (k0 + e) * 2)) : 0.0f;
    }
}

template <bool ALIGNED>
__device__ static inline void mmb_ld_x8(const uint8_t *row, long k0, long k, float (&f)[8]) {
    if (ALIGNED && k0 + 8 <= k) {
        const float4 lo = *(const float4 *)(row + k0 * 4), hi = *(const float4 *)(row + k0 * 4 + 16);
        f[0] = lo.x, f[1] = lo.y, f[2] = lo.z, f[3] = lo.w, f[4] = hi.x, f[5] = hi.y, f[6] = hi.z, f[7] = hi.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++)
            f[e] = k0 + e < k ? *(const float *)(row + (k0 + e) * 4) : 0.0f;
    }
}

// sum over the LPR lanes that share a row, in every one of them: pairs, quads, eights, sixteens; then (LPR = 64) the four rows of 16
template <int LPR>
__device__ static inline float mmb_lane_sum(float v) {
    v += dpp_f32<DPP_XOR1>(v);
    v += dpp_f32<DPP_XOR2>(v);
    v += dpp_f32<DPP_HALF_MIRROR>(v);
    v += dpp_f32<DPP_MIRROR>(v);
    if constexpr (LPR == 64)
        v = (readlane_f32(v, 0) + readlane_f32(v, 16)) + (readlane_f32(v, 32) + readlane_f32(v, 48));
    return v;
}

// NC: columns a lane keeps (query heads of the item x n, rounded up to 1, 2, 4 or 8; the live count is uniform)
template <int LPR, int NC, bool ALIGNED>
__global__ __launch_bounds__(256) void mmb_gemv_kernel(const mmb_args a) {
    constexpr int RPP = 64 / LPR; // rows one wave-wide load covers
    constexpr int RU = 4;         // such loads in flight per wave
    constexpr bool KSPLIT = LPR == 64; // the four waves share the work-group's RU rows and take every fourth step of k
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const lfamd_batched_index it(a.a_ne2, a.r2, a.r3, a.hg, a.hchunks);
    const int n = (int)a.n, nc = it.nh * n;
    const long row0 = KSPLIT ? (long)blockIdx.x * RU : ((long)blockIdx.x * 4 + wave) * (RPP * RU);
    if (row0 >= a.m) // (KSPLIT: uniform over the work-group, so every wave reaches the barrier below)
        return;
    const uint8_t *Ab = it.a_slice(a.A, a.a_nb3, a.a_nb2);
    const uint8_t *wrow[RU];
#pragma unroll
    for (int u = 0; u < RU; u++) { // rows past the edge are clamped for the loads and masked at the store
        const long r = row0 + u * RPP + sub;
        wrow[u] = Ab + (r < a.m ? r : a.m - 1) * a.a_nb1;
    }
    const uint8_t *xrow[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        xrow[c] = it.column(a.B, a.b_nb3, a.b_nb2, a.b_nb1, a.r2, c < nc ? c : 0, n);
    float acc[RU][NC];
#pragma unroll
    for (int u = 0; u < RU; u++)
#pragma unroll
        for (int c = 0; c < NC; c++)
            acc[u][c] = 0.0f;
    for (long kb = KSPLIT ? wave * (LPR * 8) : 0; kb < a.k; kb += (KSPLIT ? 4 : 1) * (LPR * 8)) {
        const long k0 = kb + sl * 8;
        float w[RU][8];
#pragma unroll
        for (int u = 0; u < RU; u++)
            mmb_ld_w8<ALIGNED>(wrow[u], k0, a.k, w[u]);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                float x[8];
                mmb_ld_x8<ALIGNED>(xrow[c], k0, a.k, x);
#pragma unroll
                for (int u = 0; u < RU; u++)
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        acc[u][c] = fmaf(w[u][e], x[e], acc[u][c]);
            }
        }
    }
    if constexpr (KSPLIT) {
        __shared__ float part[4][RU][NC]; // the waves' sums, added as (w0 + w1) + (w2 + w3)
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int u = 0; u < RU; u++) {
                const float s = mmb_lane_sum<LPR>(acc[u][c]);
                if (lane == 0)
                    part[wave][u][c] = s;
            }
        __syncthreads();
        const int u = threadIdx.x / NC, c = threadIdx.x % NC;
        if (u < RU && c < nc && row0 + u < a.m) {
            float *Cc = (float *)it.column(a.C, a.c_nb3, a.c_nb2, a.c_nb1, a.r2, c, n);
            Cc[row0 + u] = (part[0][u][c] + part[1][u][c]) + (part[2][u][c] + part[3][u][c]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                float *Cc = (float *)it.column(a.C, a.c_nb3, a.c_nb2, a.c_nb1, a.r2, c, n);
#pragma unroll
                for (int u = 0; u < RU; u++) {
                    const float s = mmb_lane_sum<LPR>(acc[u][c]);
                    const long r = row0 + u * RPP + sub;
                    if (sl == 0 && r < a.m)
                        Cc[r] = s;
                }
            }
        }
    }
}

// eight halves of a weight row from element k0 on, zeros past k
template <bool ALIGNED>
__device__ static inline half8_t mmb_frag_a(const uint8_t *row, long k0, long k) {
    if (ALIGNED && k0 + 8 <= k)
        return *(const half8_t *)(row + k0 * 2);
    half8_t v;
#pragma unroll
    for (int e = 0; e < 8; e++)
        v[e] = k0 + e < k ? *(const _Float16 *)(row + (k0 + e) * 2) : (_Float16)0;
    return v;
}

// eight activations rounded once to f16, to nearest-even (the (_Float16) conversion: v_cvt_f16_f32 in the default rounding mode)
template <bool ALIGNED>
__device__ static inline half8_t mmb_frag_b(const uint8_t *row, long k0, long k) {
    float x[8];
    mmb_ld_x8<ALIGNED>(row, k0, k, x);
    half8_t v;
#pragma unroll
    for (int e = 0; e < 8; e++)
        v[e] = (_Float16)x[e];
    return v;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void mmb_mfma_kernel(const mmb_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const lfamd_batched_index sl(a.ne2, a.r2, a.r3);
    const long m0 = (long)blockIdx.x * 128 + (wave & 1) * 64, n0 = (long)blockIdx.y * 64 + (wave >> 1) * 32;
    if (m0 >= a.m || n0 >= a.n)
        return;
    const bool two = m0 + 32 < a.m; // (uniform: the wave's second row tile exists)
    // rows past the edge are clamped for the loads and masked at the store
    const long ar0 = m0 + i < a.m ? m0 + i : a.m - 1, ar1 = m0 + 32 + i < a.m ? m0 + 32 + i : a.m - 1;
    const long br = n0 + i < a.n ? n0 + i : a.n - 1;
    const uint8_t *Ab = sl.a_slice(a.A, a.a_nb3, a.a_nb2);
    const uint8_t *A0 = Ab + ar0 * a.a_nb1, *A1 = Ab + ar1 * a.a_nb1;
    const uint8_t *Br = sl.slice(a.B, a.b_nb3, a.b_nb2) + br * a.b_nb1;
    float16_t_ acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
    for (long k0 = 0; k0 < a.k; k0 += 16) {
        const long kk = k0 + 8 * h;
        const half8_t fb = mmb_frag_b<ALIGNED>(Br, kk, a.k);
        const half8_t fa0 = mmb_frag_a<ALIGNED>(A0, kk, a.k);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb, acc0, 0, 0, 0); // A operand = the m index, B operand = the n index
        if (two) {
            const half8_t fa1 = mmb_frag_a<ALIGNED>(A1, kk, a.k);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb, acc1, 0, 0, 0);
        }
    }
    // lane (i, h) holds column n0 + i; register r holds row (r & 3) + 8 (r >> 2) + 4 h of the tile
    const long col = n0 + i;
    if (col >= a.n)
        return;
    float *Cc = (float *)(sl.slice(a.C, a.c_nb3, a.c_nb2) + col * a.c_nb1);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < a.m)
            Cc[row] = acc0[r];
        if (two && row + 32 < a.m)
            Cc[row + 32] = acc1[r];
    }
}

template <int LPR, bool ALIGNED>
void gemv_go(const mmb_args &a, dim3 grid, hipStream_t s) {
    lfamd_dispatch_nc(a.hg * (int)a.n, [&](auto nc) { mmb_gemv_kernel<LPR, decltype(nc)::value, ALIGNED><<<grid, 256, 0, s>>>(a); });
}

} // namespace

extern "C" int lfamd_mul_mat_batched(int Atype, const void *d_A, long m, long k, size_t a_nb1, size_t a_nb2, size_t a_nb3, long a_ne2,
                                     long a_ne3, const float *d_B, long n, size_t b_nb1, size_t b_nb2, size_t b_nb3, long ne2, long ne3,
                                     float *d_C, size_t c_nb1, size_t c_nb2, size_t c_nb3, unsigned flags, void *stream) {
    mmb_args a{{(const uint8_t *)d_A, (const uint8_t *)d_B, (uint8_t *)d_C, m, k, n, a_nb1, a_nb2, a_nb3, b_nb1, b_nb2, b_nb3,
                c_nb1, c_nb2, c_nb3, a_ne2, ne2}};
    const lfamd_batched_desc d{Atype == LFAMD_TYPE_F16, 0, 1, (size_t)k * 2, "F16 weights only", nullptr, nullptr};
    int rc;
    if (!lfamd_batched_check("lfamd_mul_mat_batched", d, a, a_ne3, ne3, flags, &rc))
        return rc;
    lfamd_batched_groups(a, a_ne3, ne3, a.hg, a.hchunks);
    // 16-byte loads need every row of every slice of A and B on a 16-byte boundary (a stride of an extent of 1 is never applied)
    const size_t strides = (m > 1 ? a_nb1 : 0) | (a_ne2 > 1 ? a_nb2 : 0) | (a_ne3 > 1 ? a_nb3 : 0) | (n > 1 ? b_nb1 : 0) |
                           (ne2 > 1 ? b_nb2 : 0) | (ne3 > 1 ? b_nb3 : 0);
    const bool aligned = (((uintptr_t)d_A | (uintptr_t)d_B | strides) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (n <= 8) {
        const bool lanes16 = k <= 128;
        const long rows_wg = lanes16 ? 4 * 16 : 4; // 16 lanes: four waves of 16 rows; 64 lanes: four rows, k split over the waves
        const dim3 grid((unsigned)((m + rows_wg - 1) / rows_wg), (unsigned)(ne3 * a_ne2 * a.hchunks), 1);
        if (lanes16 && aligned)
            gemv_go<16, true>(a, grid, s);
        else if (lanes16)
            gemv_go<16, false>(a, grid, s);
        else if (aligned)
            gemv_go<64, true>(a, grid, s);
        else
            gemv_go<64, false>(a, grid, s);
    } else {
        const dim3 grid((unsigned)((m + 127) / 128), (unsigned)((n + 63) / 64), (unsigned)(ne2 * ne3));
        if (aligned)
            mmb_mfma_kernel<true><<<grid, 256, 0, s>>>(a);
        else
            mmb_mfma_kernel<false><<<grid, 256, 0, s>>>(a);
    }
    return lfamd_launch_status(hipGetLastError());
}
