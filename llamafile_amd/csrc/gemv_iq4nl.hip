// gemv_iq4nl.hip — IQ4_NL instantiations of the decode GEMV (kernels: gemv_impl.h; launched from gemv.hip)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_iq4nl(int variant, int nc, int f32in, int nw, int ch) {
    return kq_unit_kernel<iq4nl_traits, LFAMD_TYPE_Q8_0, true, false>(variant, nc, f32in, nw, ch);
}
