// gemv_iq4xs.hip — IQ4_XS instantiations of the decode GEMV, with 32-row items (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_iq4xs(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<iq4c_traits, LFAMD_TYPE_Q8_K, true, false>(variant, nc, f32in, nw, ch);
}
