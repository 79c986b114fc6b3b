// gemv_q2k.hip — Q2_K instantiations of the decode GEMV, with 32-row items (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q2k(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<pk_traits<LFAMD_TYPE_Q2_K>, LFAMD_TYPE_Q8_K, true, false>(variant, nc, f32in, nw, ch);
}
