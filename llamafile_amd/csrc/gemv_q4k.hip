// gemv_q4k.hip — Q4_K instantiations of the decode GEMV, with the expert forms (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q4k(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<q4k_traits, LFAMD_TYPE_Q8_K, false, true>(variant, nc, f32in, nw, ch);
}
