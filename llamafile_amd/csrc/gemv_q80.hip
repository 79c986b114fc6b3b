// gemv_q80.hip — Q8_0 (bit-exact) decode GEMV, f32 activations (quantised in-kernel); kernel in gemv_q80_impl.h
#include "gemv_q80_impl.h"

const void *lfamd_gemv_kernel_q80_f32(int nc, int mode) {
    return q80_kernel<LFAMD_TYPE_F32>(nc, mode);
}
