// pad256_host_check.cpp — the host arithmetic of the padded 32-block layout (LFAMD_TYPE_PAD256) walked under a
// host sanitizer: the size and geometry answers of api.hip and the decode plan of gemv.hip.  No device is touched.  Build the two
// units' HOST code with the sanitizer and take every other symbol from the built module:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       tools/pad256_host_check.cpp llamafile_amd/csrc/api.hip llamafile_amd/csrc/gemv.hip \
//       -L llamafile_amd -lllamafile_amd_hip -Wl,-rpath,$PWD/llamafile_amd -o tools/pad256_host_probe && tools/pad256_host_probe
#include <stdio.h>
#include <stdlib.h>

#include "../include/lfamd_hip.h"
#include "../llamafile_amd/csrc/lfamd_internal.h"

#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);                                                    \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

int main() {
    const int types[] = {2, 20, 3, 6, 7}; // Q4_0, IQ4_NL, Q4_1, Q5_0, Q5_1
    const long shapes[][2] = {{67, 32}, {67, 288}, {40, 4000}, {4099, 2080}, {0, 288}, {16, 224}, {1030, 8480}, {300, 32}};
    long checked = 0;
    for (int t : types) {
        const int tp = t | LFAMD_TYPE_PAD256;
        for (const auto &s : shapes) {
            const long rows = s[0], cols = s[1], kp = (cols + 255) / 256 * 256;
            CHECK(lfamd_packed_size(tp, rows, cols) == lfamd_packed_size(t, rows, kp));
            CHECK(lfamd_resident_type(t, cols) == tp && lfamd_resident_type(t, kp) == t);
            for (long n : {1L, 8L, 9L, 40L, 130L, 512L}) {
                CHECK(lfamd_mul_mat_workspace(tp, rows, cols, n) == lfamd_mul_mat_workspace(t, rows, kp, n));
                CHECK(lfamd_mul_mat_workspace_upto(tp, rows, cols, n) == lfamd_mul_mat_workspace_upto(t, rows, kp, n));
                CHECK(lfamd_mul_mat_is_exact(tp, rows, cols, n, 0) == (rows > 0 ? 1 : 0));
                CHECK(lfamd_mul_mat_takes_staged_b32(tp, rows, cols, n, 0) == 0);
                CHECK(lfamd_mul_mat_is_bit_exact(tp, rows, cols, n, 0) == 0);
            }
            CHECK(lfamd_mul_mat_id_workspace(tp, rows, cols, 4, 5, 2) <= lfamd_mul_mat_id_workspace(t, rows, kp, 4, 5, 2));
            CHECK(lfamd_gemv_depth_ok(cols) == 1);
            const int step = lfamd_gemv_cols_per_launch(t, cols);
            CHECK(step == lfamd_gemv_cols_per_launch(t, kp) && step >= 1);
            for (int cus : {256, 64, 32})
                for (int count : {1, 3})
                    for (int nc = 1; nc <= step && rows > 0; nc++) {
                        lfamd_gemv_plan p, q;
                        const long n_ht = (rows + 31) / 32 * 2 * count;
                        CHECK(lfamd_gemv_plan_of(LFAMD_GEMV_MULTI, t, nc, n_ht, 0, cols, count, cus, &p) == 0);
                        CHECK(lfamd_gemv_plan_of(LFAMD_GEMV_MULTI, t, nc, n_ht, 0, kp, count, cus, &q) == 0);
                        CHECK(p.variant == q.variant && p.nw == q.nw && p.ch == q.ch && p.grid == q.grid && p.lds == q.lds && p.rows == q.rows);
                        CHECK((size_t)p.lds == lfamd_gemv_lds_bytes(t, nc, cols, p.nw, p.rows));
                        CHECK(lfamd_gemv_has_kernel(t, 0, &p) && lfamd_gemv_has_kernel(t, 1, &p));
                        checked++;
                    }
        }
        CHECK(lfamd_packed_size(tp, 67, 48) == 0 && lfamd_packed_size(tp, -1, 32) == 0);
    }
    for (int t : {12, 8, 1, 0, 14, 23}) // Q4_K, Q8_0, F16, F32, Q6_K, IQ4_XS: nothing to pad
        CHECK(lfamd_packed_size(t | LFAMD_TYPE_PAD256, 64, 512) == 0 && lfamd_mul_mat_workspace(t | LFAMD_TYPE_PAD256, 64, 512, 40) == 0 &&
              lfamd_resident_type(t, 288) == t);
    printf("pad256 host check ok (%ld planned launches)\n", checked);
    return 0;
}
