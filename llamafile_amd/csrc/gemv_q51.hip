// gemv_q51.hip — Q5_1 instantiations of the decode GEMV (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q51(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<pcl_traits<LFAMD_TYPE_Q5_1>, LFAMD_TYPE_Q8_1, false, false>(variant, nc, f32in, nw, ch);
}
