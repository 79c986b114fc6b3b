// gemv_dual.hip — two-type instantiations of the decode GEMV (gemv_impl.h, gemv_kq_dual_kernel): the K-quant pairs a
// Q4_K_M / Q5_K_M file puts on one activation vector (attn_q/k in Q4_K or Q5_K, attn_v in Q6_K)
#include "gemv_impl.h"

const void *lfamd_gemv_kernel_q4k_q6k(int variant, int nc, int f32in, int nw, int ch) {
    return kq_dual_unit_kernel<q4k_traits, q6k_traits>(variant, nc, f32in, nw, ch);
}
const void *lfamd_gemv_kernel_q5k_q6k(int variant, int nc, int f32in, int nw, int ch) {
    return kq_dual_unit_kernel<q5k_traits, q6k_traits>(variant, nc, f32in, nw, ch);
}
