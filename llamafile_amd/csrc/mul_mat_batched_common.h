// mul_mat_batched_common.h — what lfamd_mul_mat_batched (mul_mat_batched.hip, F16 cache) and lfamd_mul_mat_batched_q
// (mul_mat_batched_q.hip, 32-block K cache) share: the argument checks, the slice geometry their kernels receive and the index rule
//     C[i3][i2][j][i] = sum_l A[i3 / r3][i2 / r2][i][l] * B[i3][i2][j][l],   r2 = ne2 / a_ne2, r3 = ne3 / a_ne3
// of include/lfamd_hip.h.  Not shared, on purpose: the load helpers, the arithmetic, the kernels, the units.
#pragma once
#include "entry_checks.h"

// ---- the slice geometry, the head of both kernels' argument structs: initialised from the argument list up to ne2, checked, completed
struct lfamd_batched_geom {
    const uint8_t *A, *B;
    uint8_t *C;
    long m, k, n;
    size_t a_nb1, a_nb2, a_nb3, b_nb1, b_nb2, b_nb3, c_nb1, c_nb2, c_nb3;
    long a_ne2, ne2, r2, r3;
};

// ---- the index rule on the device.  The kernels hand over the fields of their argument struct BY VALUE: a reference keeps the whole
// struct in a private copy until these functions are inlined, and the instruction streams move.
struct lfamd_batched_index {
    long i2, i3, i02, i03, h0;
    int nh;
    // MFMA bodies: blockIdx.z = the slice (i3, i2), i2-major: the r2 heads of a group are neighbours and find their A slice in L2
    __device__ __forceinline__ lfamd_batched_index(long ne2, long r2, long r3) {
        const long z = blockIdx.z;
        i2 = z % ne2, i3 = z / ne2, i02 = i2 / r2, i03 = i3 / r3;
    }
    // GEMV bodies: blockIdx.y = the item (i3, KV head i02, chunk of `hg` of the group's r2 query heads): heads h0 .. h0 + nh - 1
    __device__ __forceinline__ lfamd_batched_index(long a_ne2, long r2, long r3, int hg, int hchunks) {
        long y = blockIdx.y;
        const int hc = (int)(y % hchunks);
        y /= hchunks;
        i02 = y % a_ne2, i3 = y / a_ne2, i03 = i3 / r3;
        h0 = (long)hc * hg;
        nh = (int)(r2 - h0 < hg ? r2 - h0 : hg);
    }
    __device__ __forceinline__ const uint8_t *a_slice(const uint8_t *A, size_t a_nb3, size_t a_nb2) const {
        return A + i03 * a_nb3 + i02 * a_nb2;
    }
    template <typename P> // the B or the C slice of an MFMA work-group (p and ITS strides)
    __device__ __forceinline__ P *slice(P *p, size_t nb3, size_t nb2) const {
        return p + i3 * nb3 + i2 * nb2;
    }
    template <typename P> // column c of a GEMV item = row j = c % n of query head i02 * r2 + h0 + c / n: its B row or its C column
    __device__ __forceinline__ P *column(P *p, size_t nb3, size_t nb2, size_t nb1, long r2, int c, int n) const {
        const long i2 = i02 * r2 + h0 + c / n, j = c % n;
        return p + i3 * nb3 + i2 * nb2 + j * nb1;
    }
};

// ---- the host side
struct lfamd_batched_desc { // what an entry point asks of A, and how it says no
    bool type_ok;
    long k_max, k_mult; // the largest k (0: none); what k must be a multiple of
    size_t a_row;       // bytes of a row of k weights
    const char *type_msg, *k_max_msg, *k_mult_msg;
};

// The checks of include/lfamd_hip.h in their documented order (r2 and r3 are not set yet); no device call.  true: launch.  false: *rc
// is the entry point's answer (LFAMD_OK: an empty call).  The table is evaluated whole, so every condition guards itself (entry_checks.h).
static inline bool lfamd_batched_check(const char *name, const lfamd_batched_desc &d, const lfamd_batched_geom &a, long a_ne3, long ne3,
                                       unsigned flags, int *rc) {
    const lfamd_check_row checks[] = {
        {a.m < 0 || a.k < 0 || a.n < 0 || a.ne2 < 0 || ne3 < 0 || a.a_ne2 < 0 || a_ne3 < 0, LFAMD_ERR_INVALID, "negative dimension"},
        {a.m == 0 || a.n == 0 || a.ne2 == 0 || ne3 == 0, LFAMD_OK, nullptr},
        {!d.type_ok, LFAMD_ERR_UNSUPPORTED, d.type_msg},
        {d.k_max && a.k > d.k_max, LFAMD_ERR_UNSUPPORTED, d.k_max_msg},
        // slices are a grid dimension (65535 at most); so are the 64-column tiles of the batch body
        {a.ne2 > 65535 || ne3 > 65535 || (size_t)a.ne2 * (size_t)ne3 > 65535 || (a.n + 63) / 64 > 65535 || a.m > (1L << 32),
         LFAMD_ERR_UNSUPPORTED, "more than 65535 slices (or 64-column tiles, or 2^32 rows)"},
        {!a.A || !a.B || !a.C, LFAMD_ERR_INVALID, "null pointer"},
        {a.a_ne2 < 1 || a_ne3 < 1 || a.ne2 % a.a_ne2 != 0 || ne3 % a_ne3 != 0, LFAMD_ERR_INVALID,
         "ne2 / ne3 are not multiples of a_ne2 / a_ne3"},
        {a.k % d.k_mult != 0, LFAMD_ERR_INVALID, d.k_mult_msg},
        {a.a_nb1 < d.a_row || a.b_nb1 < (size_t)a.k * 4 || a.c_nb1 < (size_t)a.m * 4, LFAMD_ERR_INVALID, "a row stride is smaller than the row"},
        {((uintptr_t)a.A | a.a_nb1 | a.a_nb2 | a.a_nb3) % 2 != 0, LFAMD_ERR_INVALID, "A base / strides are not multiples of 2"},
        {((uintptr_t)a.B | a.b_nb1 | a.b_nb2 | a.b_nb3 | (uintptr_t)a.C | a.c_nb1 | a.c_nb2 | a.c_nb3) % 4 != 0, LFAMD_ERR_INVALID,
         "B / C bases / strides are not multiples of 4"},
        {flags != 0, LFAMD_ERR_INVALID, "flags are reserved (0)"},
    };
    return lfamd_run_checks(name, checks, rc);
}

// Of a call that passed the checks: r2, r3, and for the GEMV bodies (n <= 8) hg = min(r2, 8 / n) query heads per item, so that a lane
// keeps hg * n <= 8 columns, in hchunks = ceil(r2 / hg) items per group.  The MFMA bodies read neither: 1, 1.
static inline void lfamd_batched_groups(lfamd_batched_geom &a, long a_ne3, long ne3, int &hg, int &hchunks) {
    a.r2 = a.ne2 / a.a_ne2, a.r3 = ne3 / a_ne3;
    hg = a.n > 8 ? 1 : (int)(8 / a.n < a.r2 ? 8 / a.n : a.r2);
    hchunks = a.n > 8 ? 1 : (int)((a.r2 + hg - 1) / hg);
}
