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

#ifndef GEMV_DIAG
#define GEMV_DIAG 0
#endif
#if GEMV_DIAG // development: in-kernel s_memtime stamps of two work-groups (never in the product build)
#ifndef GEMV_DIAG_WG
#define GEMV_DIAG_WG 100 // the second stamped work-group (the first is 0)
#endif
static __device__ unsigned long long g_gemv_stamps[4 * 16 * 16];
extern "C" __attribute__((weak)) int lfamd_debug_gemv_stamps(unsigned long long *dst) { // per TU; dev only
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_gemv_stamps), sizeof(g_gemv_stamps));
}
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
            g_gemv_stamps[((blockIdx.x ? 1 : 0) * 16 + wave) * 16 + stamp_n++] = __builtin_amdgcn_s_memrealtime(); \
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
