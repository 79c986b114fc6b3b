// generic.hip — mat-mul on RAW-layout weights.
//
// The untuned kernels serve what has no resident packed layout: the legacy 32-block types when a row is not a whole
// number of 256-weight groups (Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL; tinyblas_cpu_sgemm.inc:45-240, iqk_mul_mat.inc:998-1349) and
// float weights outside the MFMA body's shapes, with the reference's arithmetic: exact integer block dot products, f32
// scales.  Every K-quant and IQ4_XS is packed (lfamd_device.h) and never comes here.
//
// One wave per (weight row, tile of up to 8 activation rows).  Lanes split the row into 32-weight blocks (float rows: single
// elements), each lane unpacks its block once and dots it against up to 8 activation rows, then the wave reduces with shuffles.
#include "lfamd_device.h"
#include "lfamd_internal.h"

__device__ static const int8_t kvalues_iq4nl_dev[16] = {-127, -104, -83, -65, -49, -35, -22, -10,
                                                        1,    13,   25,  38,  53,  69,  89,  113};

// legacy 32-blocks x Q8_0 / Q8_1 (iqk_mul_mat.inc:998-1349)
template <int TYPE, int TS, bool TYPE1>
__global__ __launch_bounds__(256) void generic_legacy_kernel(const uint8_t *__restrict__ A, long m, int nb,
                                                             const uint8_t *__restrict__ B, size_t b_row_bytes, long n,
                                                             float *__restrict__ C, long ldc) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long col0 = (long)blockIdx.y * 8;
    if (row >= m)
        return;
    const int nc = (int)((n - col0) < 8 ? (n - col0) : 8);
    const uint8_t *arow = A + (size_t)row * nb * TS;
    float acc[8];
    for (int c = 0; c < 8; c++)
        acc[c] = 0.0f;
    for (int u = lane; u < nb; u += 64) {
        const uint8_t *blk = arow + (size_t)u * TS;
        int q[32];
        float d = h2f(*(const uint16_t *)blk), mval = 0.0f;
        if constexpr (TYPE == LFAMD_TYPE_Q4_0) {
            for (int j = 0; j < 16; j++) {
                q[j] = (blk[2 + j] & 15) - 8;
                q[j + 16] = (blk[2 + j] >> 4) - 8;
            }
        } else if constexpr (TYPE == LFAMD_TYPE_IQ4_NL) { // Q4_0's block, the nibbles index the codebook
            for (int j = 0; j < 16; j++) {
                q[j] = kvalues_iq4nl_dev[blk[2 + j] & 15];
                q[j + 16] = kvalues_iq4nl_dev[blk[2 + j] >> 4];
            }
        } else if constexpr (TYPE == LFAMD_TYPE_Q4_1) {
            mval = h2f(*(const uint16_t *)(blk + 2));
            for (int j = 0; j < 16; j++) {
                q[j] = blk[4 + j] & 15;
                q[j + 16] = blk[4 + j] >> 4;
            }
        } else if constexpr (TYPE == LFAMD_TYPE_Q5_0) {
            uint32_t qh = blk[2] | (blk[3] << 8) | (blk[4] << 16) | ((uint32_t)blk[5] << 24);
            for (int j = 0; j < 16; j++) {
                q[j] = ((blk[6 + j] & 15) | (((qh >> j) & 1) << 4)) - 16;
                q[j + 16] = ((blk[6 + j] >> 4) | (((qh >> (j + 16)) & 1) << 4)) - 16;
            }
        } else if constexpr (TYPE == LFAMD_TYPE_Q5_1) {
            mval = h2f(*(const uint16_t *)(blk + 2));
            uint32_t qh = blk[4] | (blk[5] << 8) | (blk[6] << 16) | ((uint32_t)blk[7] << 24);
            for (int j = 0; j < 16; j++) {
                q[j] = (blk[8 + j] & 15) | (((qh >> j) & 1) << 4);
                q[j + 16] = (blk[8 + j] >> 4) | (((qh >> (j + 16)) & 1) << 4);
            }
        }
        for (int c = 0; c < nc; c++) {
            const uint8_t *yb = B + (col0 + c) * b_row_bytes + (size_t)u * (TYPE1 ? 36 : 34);
            float dy = h2f(*(const uint16_t *)yb);
            const int8_t *q8 = (const int8_t *)(yb + (TYPE1 ? 4 : 2));
            int dot = 0;
            for (int l = 0; l < 32; l++)
                dot += q[l] * (int)q8[l];
            acc[c] = fmaf(d * dy, (float)dot, acc[c]);
            if constexpr (TYPE1)
                acc[c] += mval * h2f(*(const uint16_t *)(yb + 2));
        }
    }
    for (int c = 0; c < nc; c++) {
        float v = acc[c];
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
        if (lane == 0)
            C[(col0 + c) * ldc + row] = v;
    }
}

// float types (tinyBLAS<> F32/F16/BF16, tinyblas_cpu.h:419-613): f32 accumulate
template <int ATYPE, int BTYPE>
__global__ __launch_bounds__(256) void generic_float_kernel(const uint8_t *__restrict__ A, long m, long k,
                                                            const uint8_t *__restrict__ B, size_t b_row_bytes, long n,
                                                            float *__restrict__ C, long ldc) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long col0 = (long)blockIdx.y * 8;
    if (row >= m)
        return;
    const int nc = (int)((n - col0) < 8 ? (n - col0) : 8);
    constexpr int AS = ATYPE == LFAMD_TYPE_F32 ? 4 : 2;
    const uint8_t *arow = A + (size_t)row * k * AS;
    float acc[8];
    for (int c = 0; c < 8; c++)
        acc[c] = 0.0f;
    auto ld = [](int type, const uint8_t *p, long idx) -> float {
        if (type == LFAMD_TYPE_F32)
            return ((const float *)p)[idx];
        uint16_t h = ((const uint16_t *)p)[idx];
        if (type == LFAMD_TYPE_F16)
            return h2f(h);
        return __builtin_bit_cast(float, (uint32_t)h << 16);
    };
    for (long l = lane; l < k; l += 64) {
        float a = ld(ATYPE, arow, l);
        for (int c = 0; c < nc; c++)
            acc[c] = fmaf(a, ld(BTYPE, B + (col0 + c) * b_row_bytes, l), acc[c]);
    }
    for (int c = 0; c < nc; c++) {
        float v = acc[c];
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
        if (lane == 0)
            C[(col0 + c) * ldc + row] = v;
    }
}

extern "C" hipError_t lfamd_launch_generic(int Atype, const void *A, long m, long k, int Btype, const void *B,
                                           size_t b_row_bytes, long n, float *C, long ldc, hipStream_t s) {
    if (m <= 0 || n <= 0)
        return hipSuccess;
    dim3 grid((unsigned)((m + 3) / 4), (unsigned)((n + 7) / 8));
    const uint8_t *a = (const uint8_t *)A, *b = (const uint8_t *)B;
    int nb32 = (int)(k / 32);
#define LG(T, TS, T1) generic_legacy_kernel<T, TS, T1><<<grid, 256, 0, s>>>(a, m, nb32, b, b_row_bytes, n, C, ldc)
#define FL(TA, TB) generic_float_kernel<TA, TB><<<grid, 256, 0, s>>>(a, m, k, b, b_row_bytes, n, C, ldc)
    switch (Atype) {
    case LFAMD_TYPE_Q4_0:
        LG(LFAMD_TYPE_Q4_0, 18, false);
        break;
    case LFAMD_TYPE_IQ4_NL:
        LG(LFAMD_TYPE_IQ4_NL, 18, false);
        break;
    case LFAMD_TYPE_Q4_1:
        LG(LFAMD_TYPE_Q4_1, 20, true);
        break;
    case LFAMD_TYPE_Q5_0:
        LG(LFAMD_TYPE_Q5_0, 22, false);
        break;
    case LFAMD_TYPE_Q5_1:
        LG(LFAMD_TYPE_Q5_1, 24, true);
        break;
    case LFAMD_TYPE_F32:
        if (Btype != LFAMD_TYPE_F32)
            return hipErrorInvalidValue;
        FL(LFAMD_TYPE_F32, LFAMD_TYPE_F32);
        break;
    case LFAMD_TYPE_F16:
        if (Btype == LFAMD_TYPE_F32)
            FL(LFAMD_TYPE_F16, LFAMD_TYPE_F32);
        else if (Btype == LFAMD_TYPE_F16)
            FL(LFAMD_TYPE_F16, LFAMD_TYPE_F16);
        else
            return hipErrorInvalidValue;
        break;
    case LFAMD_TYPE_BF16:
        if (Btype == LFAMD_TYPE_F32)
            FL(LFAMD_TYPE_BF16, LFAMD_TYPE_F32);
        else if (Btype == LFAMD_TYPE_BF16)
            FL(LFAMD_TYPE_BF16, LFAMD_TYPE_BF16);
        else
            return hipErrorInvalidValue;
        break;
    default:
        return hipErrorInvalidValue;
    }
#undef LG
#undef FL
    return hipGetLastError();
}
