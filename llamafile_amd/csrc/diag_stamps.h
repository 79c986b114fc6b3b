// diag_stamps.h — development only: the in-kernel time stamps of ONE translation unit.  A unit that is built with its diagnostic
// define (GEMM_DIAG == 3 | 4 | 6 | 7, LF_STAMPS, GEMV_DIAG; tools/build_diag.sh builds one unit that way at a time) defines
// DIAG_STAMPS = the number of 64-bit words it records and includes this; its own stamp macro says what goes where.  Never in
// the product build.
#pragma once
#ifdef DIAG_STAMPS
static __device__ unsigned long long g_stamps[DIAG_STAMPS];
// the first n words (n <= DIAG_STAMPS).  Weak: headers instantiated by several units carry it into each of them.
extern "C" __attribute__((weak)) int lfamd_debug_stamps(unsigned long long *dst, size_t n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), (n < (size_t)(DIAG_STAMPS) ? n : (size_t)(DIAG_STAMPS)) * sizeof(unsigned long long));
}
// the shader clock (moves with the engine clock), and the constant 100 MHz one, which work-groups on different XCDs can compare
#define DIAG_CLOCK() __builtin_amdgcn_s_memtime()
#define DIAG_REALTIME() __builtin_amdgcn_s_memrealtime()
#endif
