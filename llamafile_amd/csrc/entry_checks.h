// entry_checks.h — the host-side frame of the attention and KV-cache entry points (lfamd_mul_mat_batched, lfamd_mul_mat_batched_q,
// lfamd_flash_attn, lfamd_flash_attn_q, lfamd_cpy): how a table of argument checks is run, what LFAMD_CHECK_UNPLACED means to it, how
// a launch is answered, and the column-count dispatch of their decode kernels.  The tables themselves — rows, order, wording: the
// "Checks, before any device call and in this order" of include/lfamd_hip.h — stay with their entry points.
#pragma once
#include <stdio.h>

#include <type_traits>

#include "lfamd_internal.h"

// one row of a table: the first row that hits answers with `code`; `what` == nullptr: an empty call (LFAMD_OK, no message)
struct lfamd_check_row {
    bool hit;
    int code;
    const char *what;
};

// The table is evaluated whole before it gets here, so every row guards itself.  true: every check passed, launch.  false: *rc is
// the entry point's answer and lfamd_last_error() is "<entry>: <what>" (an empty call leaves the last error alone).  No device call.
template <size_t N>
static inline bool lfamd_run_checks(const char *entry, const lfamd_check_row (&rows)[N], int *rc) {
    for (const lfamd_check_row &r : rows)
        if (r.hit) {
            if (r.what) {
                char msg[192];
                snprintf(msg, sizeof(msg), "%s: %s", entry, r.what);
                lfamd_set_error(msg);
            }
            *rc = r.code;
            return false;
        }
    return true;
}

// `flags` as a table reads them.  entry: asked by the entry point, to which every flag is reserved; else by its _check export, which
// takes LFAMD_CHECK_UNPLACED (the tensors have no addresses yet)
struct lfamd_check_flags {
    bool unplaced;     // a NULL pointer is no error, a pointer counts with its alignment bits, the workspace is not looked at
    unsigned reserved; // the flags that must be 0
};
static inline lfamd_check_flags lfamd_check_flags_of(bool entry, unsigned flags) {
    return {!entry && (flags & LFAMD_CHECK_UNPLACED) != 0, entry ? flags : flags & ~LFAMD_CHECK_UNPLACED};
}

// the answer of an entry point that has launched: e = hipGetLastError(), or what a step before the launch gave
static inline int lfamd_launch_status(hipError_t e) {
    if (e != hipSuccess)
        lfamd_set_error(hipGetErrorString(e));
    return e != hipSuccess ? LFAMD_ERR_HIP : LFAMD_OK;
}

// f(lfamd_nc<NC>{}) for the smallest NC of 1, 2, 4, 8 that holds nc_max columns: NC reaches the callable as a compile-time constant
template <int NC>
using lfamd_nc = std::integral_constant<int, NC>;
template <typename F>
static inline void lfamd_dispatch_nc(int nc_max, F &&f) {
    nc_max <= 1 ? f(lfamd_nc<1>{}) : nc_max <= 2 ? f(lfamd_nc<2>{}) : nc_max <= 4 ? f(lfamd_nc<4>{}) : f(lfamd_nc<8>{});
}
