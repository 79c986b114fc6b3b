// gemv_common.h — device-side pieces that the K-quant (gemv_impl.h) and the Q8_0 (gemv_q80_impl.h) decode GEMV kernels share.
#pragma once
#include "lfamd_device.h"
#include "gemv_launch.h"

__device__ static inline void load_piece(float (&v)[16], const float *x, int p) {
    const float4 *src = (const float4 *)(x + (size_t)p * 16);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float4 f = src[e];
        v[4 * e + 0] = f.x, v[4 * e + 1] = f.y, v[4 * e + 2] = f.z, v[4 * e + 3] = f.w;
    }
}

// N values times `scale`, rounded to int8 codes and OR-ed into y, four codes to a dword, first code lowest.  K: Q8_K's rule, nearest
// even and clamped at 127 (quantize_row_q8_K's nearest_int); otherwise Q8_0's, roundf of v * scale (quantize_row_q8_0).
template <bool K, int N>
__device__ static inline void pack_codes(uint32_t (&y)[N / 4], const float (&v)[N], float scale) {
#pragma unroll
    for (int e = 0; e < N; e++) {
        int q;
        if constexpr (K) {
            q = (int)rintf(scale * v[e]);
            q = q > 127 ? 127 : q;
        } else {
            q = (int)roundf(v[e] * scale);
        }
        y[e >> 2] |= (uint32_t)(q & 0xff) << (8 * (e & 3));
    }
}

// The Q8_0 decode kernels' LDS image of the activations (X80_QUAD per quad, gemv_launch.h), written by both of them
// (gemv_q80_impl.h, gemv_q80r_impl.h) through the two functions below, so the quantiser exists once.
//
// Piece p (16 floats, the lane pair (2i, 2i + 1) makes a 32-block; both lanes of a pair must call) of column c's f32 row, quantised
// like quantize_row_q8_0 (upstream): d = amax / 127, id = 1 / d, q = roundf(x * id), d stored as f16.
__device__ __forceinline__ void x80_quantise_piece(uint8_t *lds, int nquads, const float (&v)[16], int c, int p) {
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; e++)
        amax = fmaxf(amax, fabsf(v[e]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    const float d = amax / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t y[4] = {0, 0, 0, 0};
    pack_codes<false>(y, v, id);
    const int l = p >> 1, hf = p & 1;
    uint8_t *dst = lds + (size_t)(c * nquads + (l >> 2)) * X80_QUAD + (l & 3) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++)
        *(uint32_t *)(dst + (4 * hf + e) * 16) = y[e];
    if (hf == 0)
        *(float *)(dst + X80_QD) = h2f(f2h_bits(d)); // the block stores d as f16
}
// Q8_0 rows of columns col0 .. col0 + nc - 1, copied by the nthr threads of the work-group (eight code dwords and the scale per block).
__device__ __forceinline__ void x80_copy_blocks(uint8_t *lds, int nquads, const uint8_t *__restrict__ B, size_t b_row_bytes, long col0, int nc,
                                                int nblocks, int nthr) {
    for (int idx = threadIdx.x; idx < nc * nblocks * 9; idx += nthr) {
        int c = idx / (nblocks * 9), rem = idx % (nblocks * 9);
        int l = rem / 9, w = rem % 9;
        const uint8_t *y = B + (col0 + c) * b_row_bytes + (size_t)l * 34;
        uint32_t v;
        if (w < 8) {
            const uint16_t *p = (const uint16_t *)(y + 2 + 4 * w); // 34-byte blocks: 2-byte aligned
            v = (uint32_t)p[0] | ((uint32_t)p[1] << 16);
        } else {
            v = __builtin_bit_cast(uint32_t, h2f(*(const uint16_t *)y));
        }
        *(uint32_t *)(lds + (size_t)(c * nquads + (l >> 2)) * X80_QUAD + (l & 3) * 4 + (w < 8 ? w * 16 : X80_QD)) = v;
    }
}

#ifndef GEMV_DIAG
#define GEMV_DIAG 0
#endif
#if GEMV_DIAG // development: in-kernel s_memtime stamps of two work-groups (never in the product build)
#ifndef GEMV_DIAG_WG
#define GEMV_DIAG_WG 100 // the second stamped work-group (the first is 0)
#endif
#define DIAG_STAMPS (4 * 16 * 16)
#include "diag_stamps.h"
// entry / exit time and placement (HW_ID, XCC_ID) of wave 0 of every work-group
static __device__ unsigned long long g_gemv_wg[512 * 4];
extern "C" __attribute__((weak)) int lfamd_debug_gemv_wgs(unsigned long long *dst) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_gemv_wg), sizeof(g_gemv_wg));
}
#define GWG(slot)                                                                                                \
    do {                                                                                                         \
        if (blockIdx.x < 512 && threadIdx.x == 0) {                                                              \
            g_gemv_wg[blockIdx.x * 4 + (slot)] = __builtin_amdgcn_s_memrealtime();                               \
            if ((slot) == 0) {                                                                                   \
                g_gemv_wg[blockIdx.x * 4 + 2] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |  \
                                                ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32); \
                gwg_clk0 = __builtin_amdgcn_s_memtime();                                                         \
            } else { /* shader-clock cycles of this work-group's life: with the 100 MHz stamps, the clock it ran at */ \
                g_gemv_wg[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime() - gwg_clk0;                         \
            }                                                                                                    \
        }                                                                                                        \
    } while (0)
#define GSTAMP()                                                                                                 \
    do {                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
        if ((blockIdx.x == 0 || blockIdx.x == GEMV_DIAG_WG) && lane == 0 && stamp_n < 16)                                  \
            g_stamps[((blockIdx.x ? 1 : 0) * 16 + wave) * 16 + stamp_n++] = DIAG_REALTIME();                      \
        __builtin_amdgcn_sched_barrier(0);                                                                       \
    } while (0)
// (diagnostic only: drain the loads first, so the stamp is the arrival time of the item's weights)
#define GSTAMP_ARRIVAL()                                                                                         \
    do {                                                                                                         \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                         \
        GSTAMP();                                                                                                \
    } while (0)
#else
#define GSTAMP()
#define GSTAMP_ARRIVAL()
#define GWG(slot)
#endif
