// gemv_q6k.hip — Q6_K instantiations of the decode GEMV, with 32-row items and the expert forms (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q6k(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<q6k_traits, LFAMD_TYPE_Q8_K, true, true>(variant, nc, f32in, nw, ch);
}
