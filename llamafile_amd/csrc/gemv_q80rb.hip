// gemv_q80rb.hip — Q8_0 relaxed-order decode GEMV, activations already in Q8_0 blocks; kernel in gemv_q80r_impl.h
#include "gemv_q80r_impl.h"

const void *lfamd_gemv_kernel_q80r_q80(int nc, int nw, int ch) {
    return q80r_kernel<LFAMD_TYPE_Q8_0>(nc, nw, ch);
}
