// gemv_q80r.hip — Q8_0 relaxed-order decode GEMV, f32 activations (quantised in-kernel); kernel in gemv_q80r_impl.h
#include "gemv_q80r_impl.h"

const void *lfamd_gemv_kernel_q80r_f32(int nc, int nw, int ch) {
    return q80r_kernel<LFAMD_TYPE_F32>(nc, nw, ch);
}
