// gemv_q80b.hip — Q8_0 (bit-exact) decode GEMV, activations already in Q8_0 blocks; kernel in gemv_q80_impl.h
#include "gemv_q80_impl.h"

const void *lfamd_gemv_kernel_q80_q80(int nc, int mode) {
    return q80_kernel<LFAMD_TYPE_Q8_0>(nc, mode);
}
