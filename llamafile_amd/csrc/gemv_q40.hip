// gemv_q40.hip — Q4_0 instantiations of the decode GEMV (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q40(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<q40_traits, LFAMD_TYPE_Q8_0, false, false>(variant, nc, f32in, nw, ch);
}
