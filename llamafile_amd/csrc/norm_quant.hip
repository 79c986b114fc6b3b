// norm_quant.hip — the steps in front of the path, fused: RMS-norm x weight, and silu(gate) * up, ->
// the reference's Q8_K activation blocks in ONE kernel each, so that the mat-muls behind a norm (attn_q/k/v, ffn_gate/up, output) receive
// Btype = Q8_K and their prologue is a copy instead of a quantisation.
//
// Reference counterparts: ggml_compute_forward_rms_norm_f32 + the MUL by the norm weight (upstream ggml.c; GPU:
// rms_norm_f32, ggml-cuda.cu.patch:14926-14960) followed by quantize_row_q8_K inside ggml_compute_forward_mul_mat
// (llamafile order {d, bsums, qs}: ggml-common.h.patch:25-35).  Arithmetic restated:
//     sum  = sum_i (double)(x[i] * x[i])          (f32 products, f64 accumulation)
//     mean = (float)(sum / k);  scale = 1.0f / sqrtf(mean + eps)
//     y[i] = (x[i] * scale) * w[i]                (two f32 roundings: the norm, then the MUL node)
//     Q8_K per 256 values: first index of the largest |y| -> iscale = -128 / max, nearest-even codes clamped at 127,
//     d = 1 / iscale, bsums of 16
// The f64 sum is a tree here and a sequential loop on the CPU: they differ only below 1e-15 relative, i.e. the f32 `mean`
// (and everything after it) is identical unless the sum sits within 1e-9 relative of a rounding boundary.
#include "lfamd_device.h"
#include "../../include/lfamd_hip.h"
#include "lfamd_internal.h"

namespace {

__device__ static inline double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// ---- the arithmetic of y, shared by every kernel of this unit (the Q8_K producers, the scaled ones, the 32-block ones): the same
// instructions on the same inputs, so y has the same bits whichever format it is quantised to
__device__ static inline double squares4(const float4 v) { // f32 products, f64 sum
    return (double)(v.x * v.x) + (double)(v.y * v.y) + (double)(v.z * v.z) + (double)(v.w * v.w);
}
// the row's scale from each lane's partial sum of squares (one work-group of 4 waves per row; holds a barrier)
__device__ static inline float rms_scale(double s, double *part, int wave, int lane, long k, float eps) {
    s = wave_sum_f64(s);
    if (lane == 0)
        part[wave] = s;
    __syncthreads();
    const double sum = (part[0] + part[1]) + (part[2] + part[3]);
    const float mean = (float)(sum / (double)k);
    return 1.0f / sqrtf(mean + eps);
}
// y = (x * scale) * w for the four values of a lane; w: the lane's four weights, or NULL (= 1)
__device__ static inline void norm_y(float (&y)[4], const float4 v, float scale, const float *w) {
    y[0] = v.x * scale, y[1] = v.y * scale, y[2] = v.z * scale, y[3] = v.w * scale;
    if (w) {
        const float4 g = *(const float4 *)w;
        y[0] *= g.x, y[1] *= g.y, y[2] *= g.z, y[3] *= g.w;
    }
}
// y = silu(gate) * up
__device__ static inline void swiglu_y(float (&y)[4], const float4 g, const float4 u) {
    const float gv[4] = {g.x, g.y, g.z, g.w}, uv[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
        y[e] = (gv[e] / (1.0f + expf(-gv[e]))) * uv[e];
}

// quantize_row_q8_K on one 256-block held as four values per lane (element 4 lane + e), written in the reference's block
// format {d, bsums[16], qs[256]} (cf. gemv_impl.h stage_f32_q8k_wave: same arithmetic)
__device__ static inline void put_q8k_block(uint8_t *blk, const float (&y)[4], int lane) {
    const float a0 = fabsf(y[0]), a1 = fabsf(y[1]), a2 = fabsf(y[2]), a3 = fabsf(y[3]);
    const float amax = wave_max_f32(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
    const bool m0 = a0 == amax, m1 = a1 == amax, m2 = a2 == amax, m3 = a3 == amax;
    const unsigned long long ball = __builtin_amdgcn_ballot_w64(m0 || m1 || m2 || m3);
    const float cand = m0 ? y[0] : (m1 ? y[1] : (m2 ? y[2] : y[3]));
    const bool nz = amax != 0.0f;
    const float val = nz ? readlane_f32(cand, ball ? __builtin_ctzll(ball) : 0) : 1.0f;
    const float iscale = -128.0f / val;
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int c = (int)rintf(iscale * y[e]);
        q[e] = nz ? (c > 127 ? 127 : c) : 0;
    }
    *(uint32_t *)(blk + 36 + 4 * lane) = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) |
                                        ((uint32_t)(q[3] & 0xff) << 24);
    int bs = q[0] + q[1] + q[2] + q[3];
    bs += (int)dpp_u32<DPP_XOR1>((uint32_t)bs);
    bs += (int)dpp_u32<DPP_XOR2>((uint32_t)bs);
    if ((lane & 3) == 0)
        *(int16_t *)(blk + 4 + 2 * (lane >> 2)) = (int16_t)bs;
    if (lane == 0)
        *(float *)blk = nz ? 1.0f / iscale : 0.0f;
}

// The same block written straight into the staged image of the int8 batch body (csrc/gemm_i8.hip: Xq [nb][n_pad][256] int8 in the
// byte order of its unpacked nibbles, d8T [nb][n_pad] f32, Xs [nb][n_pad][16] f16 bsums): the codes, scale and sums are those of
// put_q8k_block bit for bit — only where they go differs, so the mat-mul behind gives the bits it gives on the f32 row.
// Lane l holds codes 4 l .. 4 l + 3; group g = l >> 1 of eight codes c0..c7 is stored as (c0,c4,c1,c5 | c2,c6,c3,c7) at
// (g >> 2) * 32 + (g & 1) * 16 + ((g >> 1) & 1) * 8 of the token's 256 bytes (prep_i8_kernel).
struct staged_image {
    int8_t *Xq;
    float *d8T;
    _Float16 *Xs;
    long n_pad;
};
__device__ static inline void put_staged_block(const staged_image &im, int b, long tok, const float (&y)[4], int lane) {
    const float a0 = fabsf(y[0]), a1 = fabsf(y[1]), a2 = fabsf(y[2]), a3 = fabsf(y[3]);
    const float amax = wave_max_f32(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
    const bool m0 = a0 == amax, m1 = a1 == amax, m2 = a2 == amax, m3 = a3 == amax;
    const unsigned long long ball = __builtin_amdgcn_ballot_w64(m0 || m1 || m2 || m3);
    const float cand = m0 ? y[0] : (m1 ? y[1] : (m2 ? y[2] : y[3]));
    const bool nz = amax != 0.0f;
    const float val = nz ? readlane_f32(cand, ball ? __builtin_ctzll(ball) : 0) : 1.0f;
    const float iscale = -128.0f / val;
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int c = (int)rintf(iscale * y[e]);
        q[e] = nz ? (c > 127 ? 127 : c) : 0;
    }
    const uint32_t mine = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) | ((uint32_t)(q[3] & 0xff) << 24);
    const uint32_t other = dpp_u32<DPP_XOR1>(mine);
    const size_t o = (size_t)b * im.n_pad + tok;
    if ((lane & 1) == 0) { // mine = c0..c3, other = c4..c7
        const int g = lane >> 1;
        const uint32_t w0 = __builtin_amdgcn_perm(other, mine, 0x05010400u); // (c0, c4, c1, c5)
        const uint32_t w1 = __builtin_amdgcn_perm(other, mine, 0x07030602u); // (c2, c6, c3, c7)
        *(uint2 *)(im.Xq + o * 256 + (g >> 2) * 32 + (g & 1) * 16 + ((g >> 1) & 1) * 8) = make_uint2(w0, w1);
    }
    int bs = q[0] + q[1] + q[2] + q[3];
    bs += (int)dpp_u32<DPP_XOR1>((uint32_t)bs);
    bs += (int)dpp_u32<DPP_XOR2>((uint32_t)bs);
    if ((lane & 3) == 0)
        im.Xs[o * 16 + (lane >> 2)] = (_Float16)(float)bs;
    if (lane == 0)
        im.d8T[o] = nz ? 1.0f / iscale : 0.0f;
}
__device__ static inline void put_staged_zero(const staged_image &im, int b, long tok, int lane) { // a padding token of the image
    const size_t o = (size_t)b * im.n_pad + tok;
    *(uint32_t *)(im.Xq + o * 256 + 4 * lane) = 0u;
    if (lane < 8)
        *(uint32_t *)(im.Xs + o * 16 + 2 * lane) = 0u;
    if (lane == 0)
        im.d8T[o] = 0.0f;
}

// The staged image of the scaled-operand f16 batch bodies (gemm_lw / gemm_ks / gemm_kr; what prep_scaled_kernel of prep.hip writes):
//   Xh [nb][n_pad][256] f16 = q8 * d8 * 2^-e(token), d8T [n_pad] f32 = 2^e(token) (the store multiplies the column by it),
//   Xm [nb][n_pad][16] f16 = the eight 32-code sums times d8 * 2^-e (the mins operand), then eight zeros;
// e(token) from the largest |y| of the whole row, so that every operand sits in f16's normal range: that maximum must be known
// before the first code is emitted — two passes over the row inside the producer.  Same arithmetic as prep_scaled_kernel, so the
// mat-mul behind gives the bits it gives on the f32 row.
struct scaled_image {
    _Float16 *Xh;
    float *tok_scale;
    _Float16 *Xm;
    long n_pad;
};
__device__ static inline _Float16 sat_f16_(float v) {
    return (_Float16)fminf(fmaxf(v, -65504.0f), 65504.0f);
}
__device__ static inline void put_scaled_block(const scaled_image &im, int b, long tok, const float (&y)[4], float scale, int lane) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    float amax = 0.0f, val = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float ax = fabsf(y[e]);
        if (ax > amax)
            amax = ax, val = y[e];
    }
    const float bmax = wave_max_f32(amax);
    const unsigned long long holders = __builtin_amdgcn_ballot_w64(amax == bmax);
    val = readlane_f32(val, holders ? __builtin_ctzll(holders) : 0);
    const bool nz = bmax != 0.0f;
    const float iscale = nz ? -128.0f / val : 0.0f;
    int q[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int c = (int)rintf(iscale * y[e]);
        q[e] = c > 127 ? 127 : c;
    }
    const float d = nz ? 1.0f / iscale : 0.0f;
    const float xs = d * scale;
    const half4_t h4 = {sat_f16_((float)q[0] * xs), sat_f16_((float)q[1] * xs), sat_f16_((float)q[2] * xs), sat_f16_((float)q[3] * xs)};
    const size_t o = (size_t)b * im.n_pad + tok;
    *(half4_t *)(im.Xh + o * 256 + 4 * lane) = h4;
    int S = q[0] + q[1] + q[2] + q[3]; // sum j = lane / 8 covers codes 32 j .. 32 j + 31
    S += (int)dpp_u32<DPP_XOR1>((uint32_t)S);
    S += (int)dpp_u32<DPP_XOR2>((uint32_t)S);
    S += (int)dpp_u32<DPP_HALF_MIRROR>((uint32_t)S);
    if ((lane & 7) == 0) {
        _Float16 *mo = im.Xm + o * 16;
        mo[lane >> 3] = sat_f16_((float)S * xs);
        mo[8 + (lane >> 3)] = (_Float16)0;
    }
}
__device__ static inline void put_scaled_zero(const scaled_image &im, int b, long tok, int lane) {
    const size_t o = (size_t)b * im.n_pad + tok;
    *(uint2 *)(im.Xh + o * 256 + 4 * lane) = make_uint2(0u, 0u);
    if (lane < 8)
        *(uint32_t *)(im.Xm + o * 16 + 2 * lane) = 0u;
}
// the row's power-of-two normalisation from the largest |y| each wave saw (every wave reduces the partial maxima itself)
template <int NWV>
__device__ static inline float row_max(float dmax, float *wmax, int wave, int lane) { // (holds a barrier)
    dmax = wave_max_f32(dmax);
    if (lane == 0)
        wmax[wave] = dmax;
    __syncthreads();
    float m = wmax[lane & (NWV - 1)];
    m = fmaxf(m, dpp_f32<DPP_XOR1>(m));
    return fmaxf(m, dpp_f32<DPP_XOR2>(m));
}
template <int NWV>
__device__ static inline float row_scale(float dmax, float *wmax, int wave, int lane, float *tok_scale_out) {
    const float m = row_max<NWV>(dmax, wmax, wave, lane);
    const bool ok = m > 0.0f && m < 3.0e38f; // (zero / non-finite rows: no normalisation)
    if (tok_scale_out && wave == 0 && lane == 0)
        *tok_scale_out = ok ? ldexpf(1.0f, ilogbf(m) - 9) : 1.0f;
    return ok ? ldexpf(1.0f, 9 - ilogbf(m)) : 1.0f;
}

// one work-group (4 waves) per row; wave w owns the 256-blocks w, w + 4, ...
template <bool STAGED>
__global__ __launch_bounds__(256) void rms_norm_q8k_kernel(const float *__restrict__ x, size_t x_row_bytes, const float *__restrict__ w,
                                                           float eps, long k, uint8_t *__restrict__ yq, size_t yq_row_bytes,
                                                           float *__restrict__ yf, size_t yf_row_bytes, long nrows, staged_image im) {
    __shared__ double part[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (STAGED && row >= nrows) { // (uniform) the image's padding tokens
        for (int b = wave; b < (int)(k / 256); b += 4)
            put_staged_zero(im, b, row, lane);
        return;
    }
    const float *xr = (const float *)((const uint8_t *)x + row * x_row_bytes);
    const int nb = (int)(k / 256);
    double s = 0.0;
    for (int b = wave; b < nb; b += 4)
        s += squares4(*(const float4 *)(xr + (size_t)b * 256 + 4 * lane));
    const float scale = rms_scale(s, part, wave, lane, k, eps);
    uint8_t *qrow = yq ? yq + row * yq_row_bytes : nullptr;
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nb; b += 4) {
        float y[4];
        norm_y(y, *(const float4 *)(xr + (size_t)b * 256 + 4 * lane), scale, w ? w + (size_t)b * 256 + 4 * lane : nullptr); // (second read: L1 / L2)
        if (frow)
            *(float4 *)(frow + (size_t)b * 256 + 4 * lane) = make_float4(y[0], y[1], y[2], y[3]);
        if constexpr (STAGED) {
            put_staged_block(im, b, row, y, lane);
        } else {
            if (!qrow)
                continue;
            put_q8k_block(qrow + (size_t)b * 292, y, lane);
        }
    }
}

// SwiGLU in front of ffn_down: y = silu(gate) * up with silu(x) = x / (1 + expf(-x)) (silu_f32, ggml-cuda.cu.patch:16172-16179;
// ggml_silu_f32, ggml-vector.inc:1662-1664) and the MUL node, then Q8_K.  One wave per 256-block.
template <bool STAGED>
__global__ __launch_bounds__(256) void swiglu_q8k_kernel(const float *__restrict__ gate, size_t gate_row_bytes, const float *__restrict__ up,
                                                         size_t up_row_bytes, long k, uint8_t *__restrict__ yq, size_t yq_row_bytes,
                                                         float *__restrict__ yf, size_t yf_row_bytes, long nrows, staged_image im) {
    const long row = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= (int)(k / 256))
        return;
    if (STAGED && row >= nrows) { // (uniform) the image's padding tokens
        put_staged_zero(im, b, row, lane);
        return;
    }
    const float4 g = *(const float4 *)((const float *)((const uint8_t *)gate + row * gate_row_bytes) + (size_t)b * 256 + 4 * lane);
    const float4 u = *(const float4 *)((const float *)((const uint8_t *)up + row * up_row_bytes) + (size_t)b * 256 + 4 * lane);
    float y[4];
    swiglu_y(y, g, u);
    if (yf)
        *(float4 *)((float *)((uint8_t *)yf + row * yf_row_bytes) + (size_t)b * 256 + 4 * lane) = make_float4(y[0], y[1], y[2], y[3]);
    if constexpr (STAGED)
        put_staged_block(im, b, row, y, lane);
    else if (yq)
        put_q8k_block(yq + row * yq_row_bytes + (size_t)b * 292, y, lane);
}

// RMS-norm x weight -> the scaled image: pass 1 the sum of squares, pass 2 the largest |y| of the row, pass 3 the blocks (the row is
// re-read from L1 / L2; one work-group of 4 waves per row like rms_norm_q8k_kernel, the same y bit for bit)
__global__ __launch_bounds__(256) void rms_norm_scaled_kernel(const float *__restrict__ x, size_t x_row_bytes, const float *__restrict__ w,
                                                              float eps, long k, float *__restrict__ yf, size_t yf_row_bytes, long nrows,
                                                              scaled_image im) {
    __shared__ double part[4];
    __shared__ float wmax[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = (int)(k / 256);
    if (row >= nrows) { // (uniform) the image's padding tokens
        for (int b = wave; b < nb; b += 4)
            put_scaled_zero(im, b, row, lane);
        if (threadIdx.x == 0)
            im.tok_scale[row] = 0.0f;
        return;
    }
    const float *xr = (const float *)((const uint8_t *)x + row * x_row_bytes);
    double s = 0.0;
    for (int b = wave; b < nb; b += 4)
        s += squares4(*(const float4 *)(xr + (size_t)b * 256 + 4 * lane));
    const float scale = rms_scale(s, part, wave, lane, k, eps);
    auto y_of = [&](int b, float (&y)[4]) {
        norm_y(y, *(const float4 *)(xr + (size_t)b * 256 + 4 * lane), scale, w ? w + (size_t)b * 256 + 4 * lane : nullptr);
    };
    float dmax = 0.0f;
    for (int b = wave; b < nb; b += 4) {
        float y[4];
        y_of(b, y);
        dmax = fmaxf(dmax, fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))));
    }
    const float nscale = row_scale<4>(dmax, wmax, wave, lane, im.tok_scale + row);
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nb; b += 4) {
        float y[4];
        y_of(b, y);
        if (frow)
            *(float4 *)(frow + (size_t)b * 256 + 4 * lane) = make_float4(y[0], y[1], y[2], y[3]);
        put_scaled_block(im, b, row, y, nscale, lane);
    }
}

// silu(gate) * up -> the scaled image: one work-group of 4 waves per row; pass 1 the largest |y| (the products are kept in LDS when
// the row fits — 16 KiB per 4096 values — else recomputed), pass 2 the blocks
__global__ __launch_bounds__(256) void swiglu_scaled_kernel(const float *__restrict__ gate, size_t gate_row_bytes, const float *__restrict__ up,
                                                            size_t up_row_bytes, long k, float *__restrict__ yf, size_t yf_row_bytes,
                                                            long nrows, scaled_image im) {
    __shared__ float wmax[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = (int)(k / 256);
    if (row >= nrows) {
        for (int b = wave; b < nb; b += 4)
            put_scaled_zero(im, b, row, lane);
        if (threadIdx.x == 0)
            im.tok_scale[row] = 0.0f;
        return;
    }
    const float *gr = (const float *)((const uint8_t *)gate + row * gate_row_bytes), *ur = (const float *)((const uint8_t *)up + row * up_row_bytes);
    auto y_of = [&](int b, float (&y)[4]) {
        swiglu_y(y, *(const float4 *)(gr + (size_t)b * 256 + 4 * lane), *(const float4 *)(ur + (size_t)b * 256 + 4 * lane));
    };
    float dmax = 0.0f;
    for (int b = wave; b < nb; b += 4) {
        float y[4];
        y_of(b, y);
        dmax = fmaxf(dmax, fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))));
    }
    const float nscale = row_scale<4>(dmax, wmax, wave, lane, im.tok_scale + row);
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nb; b += 4) {
        float y[4];
        y_of(b, y); // (the same instructions on the same inputs: the same bits as in pass 1)
        if (frow)
            *(float4 *)(frow + (size_t)b * 256 + 4 * lane) = make_float4(y[0], y[1], y[2], y[3]);
        put_scaled_block(im, b, row, y, nscale, lane);
    }
}

// ---- the 32-block formats: Q8_0 / Q8_1 rows, what the decode GEMVs of the legacy types and of Q8_0 read, and
// the staged image of the 32-block batch bodies (lfamd_b32_image_of; what prep80_kernel<true, true> of prep.hip writes).
// quantize_row_q8_0 / quantize_row_q8_1 as csrc/quantize.hip has them: d = amax / 127, id = d ? 1 / d : 0, codes roundf(v * id)
// (half away from zero — Q8_K's are nearest-even), d stored as f16, s = f16(sum * d) with d not yet rounded.
// A 256-chunk is four values per lane, so 32-block j of the chunk is lanes 8 j .. 8 j + 7: maximum and code sum are reduced over
// those eight lanes in three DPP steps.  Rows need only k % 32 == 0: the lanes of the last chunk that lie past k hold zeros, load
// and store nothing, and — eight lanes being one whole block — never share a reduction with a block of the row.
enum { B32_Q8_0, B32_Q8_1, B32_IMAGE };
struct b32_image {
    _Float16 *Xh;
    float *d8T, *sT;
    long n_pad;
};
template <int CTRL>
__device__ static inline float max_dpp(float v) {
    return fmaxf(v, dpp_f32<CTRL>(v));
}
__device__ static inline void quantize_b32(const float (&y)[4], int (&q)[4], float &d, int &sum) {
    float amax = fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3])));
    amax = max_dpp<DPP_HALF_MIRROR>(max_dpp<DPP_XOR2>(max_dpp<DPP_XOR1>(amax)));
    d = amax / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
    for (int e = 0; e < 4; e++)
        q[e] = (int)roundf(y[e] * id);
    sum = q[0] + q[1] + q[2] + q[3];
    sum += (int)dpp_u32<DPP_XOR1>((uint32_t)sum);
    sum += (int)dpp_u32<DPP_XOR2>((uint32_t)sum);
    sum += (int)dpp_u32<DPP_HALF_MIRROR>((uint32_t)sum);
}
// chunk: the row's blocks 8 b .. 8 b + 7.  Q8_1 blocks (36 bytes) keep their code words 4-byte aligned; Q8_0 blocks (34 bytes) only
// 2-byte aligned, so a lane's four codes go out as two 16-bit stores.  `valid` is false for the lanes past the end of the row.
template <bool Q81>
__device__ static inline void put_b32_rows(uint8_t *chunk, const float (&y)[4], int lane, bool valid) {
    int q[4], sum;
    float d;
    quantize_b32(y, q, d, sum);
    if (!valid)
        return;
    const uint32_t codes = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) | ((uint32_t)(q[3] & 0xff) << 24);
    uint8_t *blk = chunk + (lane >> 3) * (Q81 ? 36 : 34);
    if constexpr (Q81) {
        *(uint32_t *)(blk + 4 + 4 * (lane & 7)) = codes;
        if ((lane & 7) == 0)
            *(uint32_t *)blk = (uint32_t)f2h_bits(d) | ((uint32_t)f2h_bits_of_product((float)sum, d) << 16);
    } else {
        uint16_t *p = (uint16_t *)(blk + 2 + 4 * (lane & 7));
        p[0] = (uint16_t)codes;
        p[1] = (uint16_t)(codes >> 16);
        if ((lane & 7) == 0)
            *(uint16_t *)blk = f2h_bits(d);
    }
}
__device__ static inline void put_b32_image(const b32_image &im, int b, long tok, const float (&y)[4], int lane) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    int q[4], sum;
    float d;
    quantize_b32(y, q, d, sum);
    const half4_t h4 = {(_Float16)q[0], (_Float16)q[1], (_Float16)q[2], (_Float16)q[3]};
    *(half4_t *)(im.Xh + ((size_t)b * im.n_pad + tok) * 256 + 4 * lane) = h4;
    if ((lane & 7) == 0) {
        const size_t o = ((size_t)b * 8 + (lane >> 3)) * im.n_pad + tok;
        im.d8T[o] = h2f(f2h_bits(d));
        im.sT[o] = h2f(f2h_bits_of_product((float)sum, d));
    }
}
__device__ static inline void put_b32_zero(const b32_image &im, int b, long tok, int lane) { // a padding token of the image
    *(uint2 *)(im.Xh + ((size_t)b * im.n_pad + tok) * 256 + 4 * lane) = make_uint2(0u, 0u);
    if ((lane & 7) == 0) {
        const size_t o = ((size_t)b * 8 + (lane >> 3)) * im.n_pad + tok;
        im.d8T[o] = 0.0f;
        im.sT[o] = 0.0f;
    }
}

// one work-group (4 waves) per row like rms_norm_q8k_kernel; wave w owns the 256-chunks w, w + 4, ..., the last one maybe partial
template <int FMT>
__global__ __launch_bounds__(256) void rms_norm_b32_kernel(const float *__restrict__ x, size_t x_row_bytes, const float *__restrict__ w,
                                                           float eps, long k, uint8_t *__restrict__ yq, size_t yq_row_bytes,
                                                           float *__restrict__ yf, size_t yf_row_bytes, long nrows, b32_image im) {
    __shared__ double part[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc = (int)((k + 255) / 256);
    if (FMT == B32_IMAGE && row >= nrows) { // (uniform) the image's padding tokens
        for (int b = wave; b < nc; b += 4)
            put_b32_zero(im, b, row, lane);
        return;
    }
    const float *xr = (const float *)((const uint8_t *)x + row * x_row_bytes);
    double s = 0.0;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        if (at < k)
            s += squares4(*(const float4 *)(xr + at));
    }
    const float scale = rms_scale(s, part, wave, lane, k, eps);
    uint8_t *qrow = yq ? yq + row * yq_row_bytes : nullptr;
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        const bool valid = at < k;
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            norm_y(y, *(const float4 *)(xr + at), scale, w ? w + at : nullptr); // (second read: L1 / L2)
            if (frow)
                *(float4 *)(frow + at) = make_float4(y[0], y[1], y[2], y[3]);
        }
        if constexpr (FMT == B32_IMAGE) {
            put_b32_image(im, b, row, y, lane); // (k % 256 == 0: every lane is valid)
        } else {
            if (!qrow) // (uniform)
                continue;
            put_b32_rows<FMT == B32_Q8_1>(qrow + (size_t)b * 8 * (FMT == B32_Q8_1 ? 36 : 34), y, lane, valid);
        }
    }
}

// one wave per 256-chunk like swiglu_q8k_kernel
template <int FMT>
__global__ __launch_bounds__(256) void swiglu_b32_kernel(const float *__restrict__ gate, size_t gate_row_bytes, const float *__restrict__ up,
                                                         size_t up_row_bytes, long k, uint8_t *__restrict__ yq, size_t yq_row_bytes,
                                                         float *__restrict__ yf, size_t yf_row_bytes, long nrows, b32_image im) {
    const long row = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= (int)((k + 255) / 256))
        return;
    if (FMT == B32_IMAGE && row >= nrows) { // (uniform) the image's padding tokens
        put_b32_zero(im, b, row, lane);
        return;
    }
    const long at = (long)b * 256 + 4 * lane;
    const bool valid = at < k;
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        swiglu_y(y, *(const float4 *)((const float *)((const uint8_t *)gate + row * gate_row_bytes) + at),
                 *(const float4 *)((const float *)((const uint8_t *)up + row * up_row_bytes) + at));
        if (yf)
            *(float4 *)((float *)((uint8_t *)yf + row * yf_row_bytes) + at) = make_float4(y[0], y[1], y[2], y[3]);
    }
    if constexpr (FMT == B32_IMAGE)
        put_b32_image(im, b, row, y, lane);
    else if (yq)
        put_b32_rows<FMT == B32_Q8_1>(yq + row * yq_row_bytes + (size_t)b * 8 * (FMT == B32_Q8_1 ? 36 : 34), y, lane, valid);
}

// ---- the image of the Q8_0-weight batch body (lfamd_q80_image_of): what lf_tok_scale_kernel and
// prep_lf_kernel of gemm_lf.hip write per call.  Per token a power of two from D = f32(f16(rowmax |y| / 127)) * 127, the row's largest
// block scale as the blocks store it: stage = 2^(9 - ilogb(D)), tok_scale = 2^(ilogb(D) - 9) (D zero or not finite: 1 and 1).  Per
// 128-weight quad and token 256 bytes of f16(f32(f16(d)) * stage * code) of quantize_row_q8_0 — the f32 product is exact (11 + 7
// significant bits), so it is rounded once — where block blk of the quad, elements 4 j .. 4 j + 3, sit at byte
// (2 s + (j >> 2)) * 16 + (blk & 1) * 8, s = 2 (j & 3) + (blk >> 1).  A lane's four values are elements 4 j .. 4 j + 3 of block
// (lane >> 3) & 3 of quad 2 b + (lane >> 5), j = lane & 7.  Rows need k % 128 == 0: lanes 32 .. 63 of a last half chunk hold zeros,
// load and store nothing, and share no DPP step with lanes 0 .. 31 (rows of 16 lanes).
struct q80_image {
    _Float16 *Xh;
    float *stage, *tok_scale;
    long n_pad;
};
__device__ static inline int q80_chunk_byte(int lane) { // where the lane's half4 goes inside the 256 bytes of its quad and token
    const int blk = (lane >> 3) & 3, j = lane & 7, s = 2 * (j & 3) + (blk >> 1);
    return (2 * s + (j >> 2)) * 16 + (blk & 1) * 8;
}
__device__ static inline void put_q80_image(const q80_image &im, int b, long tok, const float (&y)[4], float stage, int lane, bool valid) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    int q[4], sum;
    float d;
    quantize_b32(y, q, d, sum); // (the code sum is not used: its three DPP steps fall away)
    if (!valid)
        return;
    const float ds = h2f(f2h_bits(d)) * stage; // (exact: a power of two)
    const half4_t h4 = {(_Float16)(ds * (float)q[0]), (_Float16)(ds * (float)q[1]), (_Float16)(ds * (float)q[2]), (_Float16)(ds * (float)q[3])};
    uint8_t *dst = (uint8_t *)im.Xh + ((size_t)(2 * b + (lane >> 5)) * im.n_pad + tok) * 256;
    *(half4_t *)(dst + q80_chunk_byte(lane)) = h4;
}
// a padding token of the image: zero operands, factors of 1
__device__ static inline void put_q80_zero_row(const q80_image &im, long tok, long k, int wave, int lane) {
    for (int b = wave; b < (int)((k + 255) / 256); b += 4)
        if ((long)b * 256 + 4 * lane < k)
            *(uint2 *)((uint8_t *)im.Xh + ((size_t)(2 * b + (lane >> 5)) * im.n_pad + tok) * 256 + 8 * (lane & 31)) = make_uint2(0u, 0u);
    if (wave == 0 && lane == 0)
        im.stage[tok] = 1.0f, im.tok_scale[tok] = 1.0f;
}
// the token's two factors from the largest |y| each lane saw (lf_tok_scale_kernel's rule; every wave reduces the partial maxima itself)
__device__ static inline float q80_row_stage(float dmax, float *wmax, const q80_image &im, long tok, int wave, int lane) {
    const float D = h2f(f2h_bits(row_max<4>(dmax, wmax, wave, lane) / 127.0f)) * 127.0f;
    const bool ok = D > 0.0f && D < 3.0e38f; // (zero / non-finite rows: no normalisation)
    const float stage = ok ? ldexpf(1.0f, 9 - ilogbf(D)) : 1.0f;
    if (wave == 0 && lane == 0)
        im.stage[tok] = stage, im.tok_scale[tok] = ok ? ldexpf(1.0f, ilogbf(D) - 9) : 1.0f;
    return stage;
}
__device__ static inline float max_abs4(const float (&y)[4]) {
    return fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3])));
}

// RMS-norm x weight -> the Q8_0 body's image: pass 1 the sum of squares, pass 2 the largest |y| of the row, pass 3 the blocks (the
// skeleton of rms_norm_scaled_kernel: one work-group of 4 waves per token of n_pad, the row re-read from L1 / L2, the same y bit for bit)
__global__ __launch_bounds__(256) void rms_norm_q80_kernel(const float *__restrict__ x, size_t x_row_bytes, const float *__restrict__ w,
                                                           float eps, long k, float *__restrict__ yf, size_t yf_row_bytes, long nrows,
                                                           q80_image im) {
    __shared__ double part[4];
    __shared__ float wmax[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc = (int)((k + 255) / 256);
    if (row >= nrows) { // (uniform) the image's padding tokens
        put_q80_zero_row(im, row, k, wave, lane);
        return;
    }
    const float *xr = (const float *)((const uint8_t *)x + row * x_row_bytes);
    double s = 0.0;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        if (at < k)
            s += squares4(*(const float4 *)(xr + at));
    }
    const float scale = rms_scale(s, part, wave, lane, k, eps);
    auto y_of = [&](long at, float (&y)[4]) { norm_y(y, *(const float4 *)(xr + at), scale, w ? w + at : nullptr); };
    float dmax = 0.0f;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        if (at < k) {
            float y[4];
            y_of(at, y);
            dmax = fmaxf(dmax, max_abs4(y));
        }
    }
    const float stage = q80_row_stage(dmax, wmax, im, row, wave, lane);
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        const bool valid = at < k;
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            y_of(at, y); // (the same instructions on the same inputs: the same bits as in pass 2)
            if (frow)
                *(float4 *)(frow + at) = make_float4(y[0], y[1], y[2], y[3]);
        }
        put_q80_image(im, b, row, y, stage, lane, valid);
    }
}

// silu(gate) * up -> the Q8_0 body's image: the skeleton of swiglu_scaled_kernel — pass 1 the largest |y|, pass 2 the blocks
__global__ __launch_bounds__(256) void swiglu_q80_kernel(const float *__restrict__ gate, size_t gate_row_bytes, const float *__restrict__ up,
                                                         size_t up_row_bytes, long k, float *__restrict__ yf, size_t yf_row_bytes, long nrows,
                                                         q80_image im) {
    __shared__ float wmax[4];
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc = (int)((k + 255) / 256);
    if (row >= nrows) {
        put_q80_zero_row(im, row, k, wave, lane);
        return;
    }
    const float *gr = (const float *)((const uint8_t *)gate + row * gate_row_bytes), *ur = (const float *)((const uint8_t *)up + row * up_row_bytes);
    auto y_of = [&](long at, float (&y)[4]) { swiglu_y(y, *(const float4 *)(gr + at), *(const float4 *)(ur + at)); };
    float dmax = 0.0f;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        if (at < k) {
            float y[4];
            y_of(at, y);
            dmax = fmaxf(dmax, max_abs4(y));
        }
    }
    const float stage = q80_row_stage(dmax, wmax, im, row, wave, lane);
    float *frow = yf ? (float *)((uint8_t *)yf + row * yf_row_bytes) : nullptr;
    for (int b = wave; b < nc; b += 4) {
        const long at = (long)b * 256 + 4 * lane;
        const bool valid = at < k;
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            y_of(at, y); // (the same instructions on the same inputs: the same bits as in pass 1)
            if (frow)
                *(float4 *)(frow + at) = make_float4(y[0], y[1], y[2], y[3]);
        }
        put_q80_image(im, b, row, y, stage, lane, valid);
    }
}

} // namespace

static scaled_image scaled_of(void *image, long k, long nrows) {
    const lfamd_kq_image l = lfamd_kq_image_of(k, nrows);
    uint8_t *p = (uint8_t *)image;
    return {(_Float16 *)p, (float *)(p + l.d8T), (_Float16 *)(p + l.Xm), (long)l.n_pad};
}

extern "C" size_t lfamd_staged_scaled_size(long k, long nrows) { // = the staging part of lfamd_mul_mat_workspace for these bodies
    return k <= 0 || k % 256 || nrows < 0 ? 0 : lfamd_kq_image_of(k, nrows).parts;
}

static staged_image staged_of(void *image, long k, long nrows) {
    const lfamd_i8_image l = lfamd_i8_image_of(k, nrows);
    uint8_t *p = (uint8_t *)image;
    return {(int8_t *)p, (float *)(p + l.d8T), (_Float16 *)(p + l.Xs), (long)l.n_pad};
}

extern "C" size_t lfamd_staged_q8k_size(long k, long nrows) { // = lfamd_gemm_i8_workspace(k, nrows)
    return k <= 0 || k % 256 || nrows < 0 ? 0 : lfamd_i8_image_of(k, nrows).bytes;
}

extern "C" int lfamd_rms_norm_quantize(const float *d_x, size_t x_row_bytes, const float *d_weight, float eps, long nrows, long k,
                                       int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes,
                                       void *stream) {
    const bool scaled = d_yq && vec_dot_type == LFAMD_TYPE_STAGED_SCALED; // d_yq = an image of lfamd_staged_scaled_size(k, nrows) bytes
    const bool staged = scaled || (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_Q8K); // ... of lfamd_staged_q8k_size(k, nrows) bytes
    if (nrows < 0 || k <= 0 || k % 256 || (d_yq && vec_dot_type != LFAMD_TYPE_Q8_K && !staged) || (!d_yq && !d_yf) || !d_x ||
        ((uintptr_t)d_x & 15) || (x_row_bytes & 15) || ((uintptr_t)d_weight & 15) || ((uintptr_t)d_yf & 15) || (yf_row_bytes & 15) ||
        ((uintptr_t)d_yq & (staged ? 15 : 3)) || (!staged && (yq_row_bytes & 3))) {
        lfamd_set_error("lfamd_rms_norm_quantize: k must be a multiple of 256, output format Q8_K (or the staged image, 16-byte aligned), "
                        "16-byte aligned f32 rows");
        return LFAMD_ERR_INVALID;
    }
    if (nrows == 0)
        return LFAMD_OK;
    if (scaled) {
        const scaled_image im = scaled_of(d_yq, k, nrows);
        rms_norm_scaled_kernel<<<(unsigned)im.n_pad, 256, 0, (hipStream_t)stream>>>(d_x, x_row_bytes, d_weight, eps, k, d_yf, yf_row_bytes, nrows,
                                                                                   im);
    } else if (staged) {
        const staged_image im = staged_of(d_yq, k, nrows);
        rms_norm_q8k_kernel<true><<<(unsigned)im.n_pad, 256, 0, (hipStream_t)stream>>>(d_x, x_row_bytes, d_weight, eps, k, nullptr, 0, d_yf,
                                                                                       yf_row_bytes, nrows, im);
    } else {
        rms_norm_q8k_kernel<false><<<(unsigned)nrows, 256, 0, (hipStream_t)stream>>>(d_x, x_row_bytes, d_weight, eps, k, (uint8_t *)d_yq,
                                                                                     yq_row_bytes, d_yf, yf_row_bytes, nrows, staged_image{});
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lfamd_set_error(hipGetErrorString(e));
        return LFAMD_ERR_HIP;
    }
    return LFAMD_OK;
}

extern "C" int lfamd_swiglu_quantize(const float *d_gate, size_t gate_row_bytes, const float *d_up, size_t up_row_bytes, long nrows,
                                     long k, int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes,
                                     void *stream) {
    const bool scaled = d_yq && vec_dot_type == LFAMD_TYPE_STAGED_SCALED; // d_yq = an image of lfamd_staged_scaled_size(k, nrows) bytes
    const bool staged = scaled || (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_Q8K); // ... of lfamd_staged_q8k_size(k, nrows) bytes
    if (nrows < 0 || k <= 0 || k % 256 || (d_yq && vec_dot_type != LFAMD_TYPE_Q8_K && !staged) || (!d_yq && !d_yf) || !d_gate || !d_up ||
        ((uintptr_t)d_gate & 15) || (gate_row_bytes & 15) || ((uintptr_t)d_up & 15) || (up_row_bytes & 15) || ((uintptr_t)d_yf & 15) ||
        (yf_row_bytes & 15) || ((uintptr_t)d_yq & (staged ? 15 : 3)) || (!staged && (yq_row_bytes & 3)) || nrows > 65535 - 127) {
        lfamd_set_error("lfamd_swiglu_quantize: k must be a multiple of 256, output format Q8_K (or the staged image, 16-byte aligned), "
                        "16-byte aligned f32 rows, <= 65408 rows");
        return LFAMD_ERR_INVALID;
    }
    if (nrows == 0)
        return LFAMD_OK;
    if (scaled) {
        const scaled_image im = scaled_of(d_yq, k, nrows);
        swiglu_scaled_kernel<<<(unsigned)im.n_pad, 256, 0, (hipStream_t)stream>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, d_yf, yf_row_bytes,
                                                                                 nrows, im);
    } else if (staged) {
        const staged_image im = staged_of(d_yq, k, nrows);
        const dim3 grid((unsigned)((k / 256 + 3) / 4), (unsigned)im.n_pad);
        swiglu_q8k_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, nullptr, 0, d_yf,
                                                                      yf_row_bytes, nrows, im);
    } else {
        const dim3 grid((unsigned)((k / 256 + 3) / 4), (unsigned)nrows);
        swiglu_q8k_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, (uint8_t *)d_yq,
                                                                       yq_row_bytes, d_yf, yf_row_bytes, nrows, staged_image{});
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lfamd_set_error(hipGetErrorString(e));
        return LFAMD_ERR_HIP;
    }
    return LFAMD_OK;
}

// ---- the 32-block formats: Q8_0 / Q8_1 rows, LFAMD_TYPE_STAGED_B32 and LFAMD_TYPE_STAGED_Q80 (entry points of their own: the two above keep refusing them)
static b32_image b32_of(void *image, long k, long nrows) {
    const lfamd_b32_image l = lfamd_b32_image_of(k, nrows);
    uint8_t *p = (uint8_t *)image;
    return {(_Float16 *)p, (float *)(p + l.d8T), (float *)(p + l.sT), (long)l.n_pad};
}

extern "C" size_t lfamd_staged_b32_size(long k, long nrows) { // = lfamd_mul_mat_workspace of a canon32 call
    return k <= 0 || k % 256 || nrows < 0 ? 0 : lfamd_b32_image_of(k, nrows).bytes;
}

static q80_image q80_of(void *image, long k, long nrows) {
    const lfamd_q80_image l = lfamd_q80_image_of(k, nrows);
    uint8_t *p = (uint8_t *)image;
    return {(_Float16 *)p, (float *)(p + l.stage), (float *)(p + l.tok_scale), (long)l.n_pad};
}

extern "C" size_t lfamd_staged_q80_size(long k, long nrows) { // = lfamd_gemm_lf_workspace(k, nrows)
    return k <= 0 || k % 128 || nrows < 0 ? 0 : lfamd_q80_image_of(k, nrows).bytes;
}

// what both 32-block producers ask of their output arguments (the f32 operands: each entry point's own line)
static bool b32_output_ok(long nrows, long k, int vec_dot_type, const void *d_yq, size_t yq_row_bytes, const float *d_yf, size_t yf_row_bytes) {
    if (nrows < 0 || k <= 0 || k % 32 || (!d_yq && !d_yf) || ((uintptr_t)d_yf & 15) || (yf_row_bytes & 15))
        return false;
    if (!d_yq)
        return true;
    if (vec_dot_type == LFAMD_TYPE_STAGED_B32)
        return k % 256 == 0 && ((uintptr_t)d_yq & 15) == 0;
    if (vec_dot_type == LFAMD_TYPE_STAGED_Q80)
        return k % 128 == 0 && ((uintptr_t)d_yq & 15) == 0;
    if (vec_dot_type != LFAMD_TYPE_Q8_0 && vec_dot_type != LFAMD_TYPE_Q8_1)
        return false;
    const size_t a = vec_dot_type == LFAMD_TYPE_Q8_1 ? 3 : 1, row = (size_t)(k / 32) * (vec_dot_type == LFAMD_TYPE_Q8_1 ? 36 : 34);
    return ((uintptr_t)d_yq & a) == 0 && (yq_row_bytes & a) == 0 && yq_row_bytes >= row;
}

static int b32_launched(void) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lfamd_set_error(hipGetErrorString(e));
        return LFAMD_ERR_HIP;
    }
    return LFAMD_OK;
}

extern "C" int lfamd_rms_norm_quantize_b32(const float *d_x, size_t x_row_bytes, const float *d_weight, float eps, long nrows, long k,
                                           int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes,
                                           void *stream) {
    if (!b32_output_ok(nrows, k, vec_dot_type, d_yq, yq_row_bytes, d_yf, yf_row_bytes) || !d_x || ((uintptr_t)d_x & 15) || (x_row_bytes & 15) ||
        ((uintptr_t)d_weight & 15)) {
        lfamd_set_error("lfamd_rms_norm_quantize_b32: k must be a multiple of 32 (the staged images: B32 of 256, Q80 of 128, 16-byte aligned), output "
                        "format Q8_0 / Q8_1 rows (2- / 4-byte aligned, stride at least the row), LFAMD_TYPE_STAGED_B32 or _Q80, 16-byte aligned f32 rows");
        return LFAMD_ERR_INVALID;
    }
    if (nrows == 0)
        return LFAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    if (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_Q80) {
        const q80_image im = q80_of(d_yq, k, nrows);
        rms_norm_q80_kernel<<<(unsigned)im.n_pad, 256, 0, s>>>(d_x, x_row_bytes, d_weight, eps, k, d_yf, yf_row_bytes, nrows, im);
    } else if (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_B32) {
        const b32_image im = b32_of(d_yq, k, nrows);
        rms_norm_b32_kernel<B32_IMAGE><<<(unsigned)im.n_pad, 256, 0, s>>>(d_x, x_row_bytes, d_weight, eps, k, nullptr, 0, d_yf, yf_row_bytes, nrows, im);
    } else if (d_yq && vec_dot_type == LFAMD_TYPE_Q8_1) {
        rms_norm_b32_kernel<B32_Q8_1><<<(unsigned)nrows, 256, 0, s>>>(d_x, x_row_bytes, d_weight, eps, k, (uint8_t *)d_yq, yq_row_bytes, d_yf,
                                                                      yf_row_bytes, nrows, b32_image{});
    } else { // (Q8_0 rows, or f32 alone)
        rms_norm_b32_kernel<B32_Q8_0><<<(unsigned)nrows, 256, 0, s>>>(d_x, x_row_bytes, d_weight, eps, k, (uint8_t *)d_yq, yq_row_bytes, d_yf,
                                                                      yf_row_bytes, nrows, b32_image{});
    }
    return b32_launched();
}

extern "C" int lfamd_swiglu_quantize_b32(const float *d_gate, size_t gate_row_bytes, const float *d_up, size_t up_row_bytes, long nrows,
                                         long k, int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes,
                                         void *stream) {
    if (!b32_output_ok(nrows, k, vec_dot_type, d_yq, yq_row_bytes, d_yf, yf_row_bytes) || !d_gate || !d_up || ((uintptr_t)d_gate & 15) ||
        (gate_row_bytes & 15) || ((uintptr_t)d_up & 15) || (up_row_bytes & 15) || nrows > 65535 - 127) {
        lfamd_set_error("lfamd_swiglu_quantize_b32: k must be a multiple of 32 (the staged images: B32 of 256, Q80 of 128, 16-byte aligned), output "
                        "format Q8_0 / Q8_1 rows (2- / 4-byte aligned, stride at least the row), LFAMD_TYPE_STAGED_B32 or _Q80, 16-byte aligned f32 "
                        "rows, <= 65408 rows");
        return LFAMD_ERR_INVALID;
    }
    if (nrows == 0)
        return LFAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)(((k + 255) / 256 + 3) / 4);
    if (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_Q80) {
        const q80_image im = q80_of(d_yq, k, nrows);
        swiglu_q80_kernel<<<(unsigned)im.n_pad, 256, 0, s>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, d_yf, yf_row_bytes, nrows, im);
    } else if (d_yq && vec_dot_type == LFAMD_TYPE_STAGED_B32) {
        const b32_image im = b32_of(d_yq, k, nrows);
        swiglu_b32_kernel<B32_IMAGE><<<dim3(gx, (unsigned)im.n_pad), 256, 0, s>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, nullptr, 0, d_yf,
                                                                                 yf_row_bytes, nrows, im);
    } else if (d_yq && vec_dot_type == LFAMD_TYPE_Q8_1) {
        swiglu_b32_kernel<B32_Q8_1><<<dim3(gx, (unsigned)nrows), 256, 0, s>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, (uint8_t *)d_yq,
                                                                             yq_row_bytes, d_yf, yf_row_bytes, nrows, b32_image{});
    } else { // (Q8_0 rows, or f32 alone)
        swiglu_b32_kernel<B32_Q8_0><<<dim3(gx, (unsigned)nrows), 256, 0, s>>>(d_gate, gate_row_bytes, d_up, up_row_bytes, k, (uint8_t *)d_yq,
                                                                             yq_row_bytes, d_yf, yf_row_bytes, nrows, b32_image{});
    }
    return b32_launched();
}
