// api.hip — the C ABI of libllamafile_amd_hip.so (include/lfamd_hip.h).
//
// Dispatch policy mirrors ggml_cuda_mul_mat (ggml-cuda.cu.patch:18377-18443): n <= 8 -> GEMV
// kernels (MMVQ_MAX_BATCH_SIZE = 8, :14359), otherwise the MFMA GEMM; types without a tuned kernel
// run the generic kernel.  There is no CPU fallback anywhere in this module.
#include "lfamd_device.h"
#include "../../include/lfamd_hip.h"

#include <stdio.h>
#include <string.h>

extern "C" {
hipError_t lfamd_launch_pack_q4k(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pack_q40(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_prep80(int, const void *, size_t, long, long, long, void *, void *, void *, hipStream_t);
hipError_t lfamd_launch_wprep32(int, const void *, size_t, long, long, void *, hipStream_t);
size_t lfamd_wprep32_bytes(long, long);
hipError_t lfamd_launch_prep_float(int, int, const void *, size_t, long, long, long, void *, hipStream_t);
hipError_t lfamd_launch_wprep8(int, const void *, size_t, long, long, void *, hipStream_t);
size_t lfamd_wprep8_bytes(long, long);
hipError_t lfamd_launch_pack_q5k(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pack_q6k(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pack_q80(const void *, size_t, long, long, void *, hipStream_t);
hipError_t lfamd_launch_pack_raw(const void *, size_t, long, size_t, void *, hipStream_t);
hipError_t lfamd_launch_prep_q8k(const void *, size_t, long, long, long, void *, void *, void *, int, const int32_t *, hipStream_t);
hipError_t lfamd_launch_prep_f32(const void *, size_t, long, long, long, void *, void *, void *, int, const int32_t *, hipStream_t);
bool lfamd_moe_decode_multi_ok(int type, long cols, int Btype, int tasks, long tokens, unsigned flags);
hipError_t lfamd_launch_moe_decode_multi(int type, int count, const void *const *W, long rows, long cols, int experts, size_t expert_bytes,
                                         int Btype, const void *thought, size_t b_row_bytes, long tokens, const int32_t *plan, int thinkers,
                                         float *const *result, hipStream_t s);
bool lfamd_blaslt_ok();
size_t lfamd_blaslt_workspace();
hipError_t lfamd_blaslt_gemm(int dtype, const void *W, long ldw, const void *X, long ldx, long m, long n, long k, float *C, long ldc, void *ws,
                             size_t ws_bytes, hipStream_t s);
hipError_t lfamd_launch_rows_to_16(int dtype, const void *X, size_t x_row_bytes, long n, long k, void *out, hipStream_t s);
hipError_t lfamd_launch_q80_rows_to_f16(int Btype, const void *X, size_t x_row_bytes, long n, long k, void *out, hipStream_t s);
hipError_t lfamd_launch_q80_image(const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s);
size_t lfamd_pk_bytes(int type, long rows, long cols);
hipError_t lfamd_launch_pk4x_pack(const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s);
hipError_t lfamd_launch_pk4x_expand(const void *packed, long rows, long cols, void *out, hipStream_t s);
hipError_t lfamd_launch_pk_pack(int type, const void *raw, size_t raw_row_bytes, long rows, long cols, void *out, hipStream_t s);
hipError_t lfamd_launch_pk_expand(int type, const void *packed, long rows, long cols, void *out, hipStream_t s);
size_t lfamd_gemm_sb_workspace(long k);
bool lfamd_gemm_sb_ok(int Atype, long k, long n);
hipError_t lfamd_launch_gemm_sb(int Atype, const void *A, long m, long k, int Btype, const void *B, size_t b_row_bytes, long n, float *C,
                                long ldc, void *ws, int reuse_stage, hipStream_t s);
hipError_t lfamd_launch_wprep16(int, const void *, size_t, long, long, void *, hipStream_t);
size_t lfamd_wprep16_bytes(long, long);
hipError_t lfamd_launch_generic(int, const void *, long, long, int, const void *, size_t, long, float *, long, hipStream_t);
hipError_t lfamd_launch_gemv_float(int, const void *, long, long, int, const void *, size_t, long, float *, long, hipStream_t);
int lfamd_gemv_float_ok(int, long, long);
hipError_t lfamd_launch_gemv(int, const void *, long, long, int, const void *, size_t, long, float *, long, int, int,
                             hipStream_t);
hipError_t lfamd_launch_gemv_multi(int, int, const void *const *, const long *, long, int, const void *, size_t, long,
                                   float *const *, const long *, int, int, hipStream_t);
hipError_t lfamd_launch_gemm_q80(const void *, long, long, int, const void *, size_t, long, float *, long, void *, int, int,
                                 hipStream_t);
size_t lfamd_gemm_q80_workspace(long, long);
hipError_t lfamd_launch_gemv_dual(int, int, const void *const *, const long *, float *const *, const long *, int, int,
                                  const void *const *, const long *, float *const *, const long *, long, int, const void *, size_t,
                                  hipStream_t);
hipError_t lfamd_launch_scaled_ok(int, long, long, const void *, int *, hipStream_t);
int lfamd_gemm_wide_scaled_ok(int, int);
// (the wide launchers take `mode`: bit 0 plain body, bit 1 activations staged scaled — gemm_wide.hip)
hipError_t lfamd_launch_gemm_wide_multi(int, int, const void *const *, const long *, long, const void *, const void *,
                                        const void *, long, long, float *const *, const long *, int, void *, size_t, hipStream_t);
hipError_t lfamd_launch_gemm_wide(int, const void *, long, long, const void *, const void *, const void *, long, long,
                                  float *, long, int, void *, size_t, hipStream_t);
size_t lfamd_gemm_lw_ksplit_bytes(long, long);
hipError_t lfamd_launch_gemm_wide_dual(int, int, const void *const *, const long *, float *const *, const long *, int, int,
                                       const void *const *, const long *, float *const *, const long *, long, const void *,
                                       const void *, const void *, long, long, int, hipStream_t);
hipError_t lfamd_launch_gemm_kq(int, const void *, long, long, const void *, const void *, const void *, long, long,
                                float *, long, hipStream_t);
hipError_t lfamd_launch_quantize(int, const float *, long, long, size_t, void *, size_t, hipStream_t);
hipError_t lfamd_launch_moe(int, const void *, long, long, int, size_t, int, const void *, size_t, int, long,
                            const int32_t *, int, float *, void *, size_t, unsigned, hipStream_t);
size_t lfamd_moe_workspace(int, long, long, int, long, int);
int lfamd_gemm_i8_ok(int Atype, long row_blocks128, long n);
size_t lfamd_gemm_i8_workspace(long k, long n);
hipError_t lfamd_launch_gemm_lf_q80(int count, const void *const *A, const long *m, long k, int Btype, const void *B, size_t b_row_bytes, long n,
                                    float *const *C, const long *ldc, void *ws, hipStream_t s);
size_t lfamd_gemm_lf_workspace(long k, long n);
hipError_t lfamd_launch_gemm_lf_float(int Atype, const void *A, size_t a_row_bytes, long m, long k, const void *Xh, long n, long n_pad, float *C,
                                      long ldc, hipStream_t s);
hipError_t lfamd_launch_gemm_i8_staged(int count, const void *const *A, const long *m, long k, const void *image, long n, float *const *C,
                                       const long *ldc, hipStream_t s);
hipError_t lfamd_launch_gemm_i8(int count, const void *const *A, const long *m, long k, int Btype, const void *B, size_t b_row_bytes, long n,
                                float *const *C, const long *ldc, void *ws, const int32_t *src_idx, hipStream_t s);
hipError_t lfamd_launch_get_rows(int type, const void *img, long rows, long cols, const int32_t *ids, long row0, long n_ids, int out_type,
                                 void *out, size_t out_row_bytes, hipStream_t s);
hipError_t lfamd_launch_unpack(int type, const void *img, long rows, long cols, void *raw, size_t raw_row_bytes, hipStream_t s);
}

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, const char *detail) {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

static int hip_fail(hipError_t e, const char *where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return LFAMD_ERR_HIP;
}

#define HIPCHK(expr, where)                                                                                            \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return hip_fail(e_, where);                                                                                \
    } while (0)

static inline size_t align_up(size_t x, size_t a) {
    return (x + a - 1) / a * a;
}

extern "C" {

int lfamd_abi_version(void) {
    return LFAMD_ABI_VERSION;
}

const char *lfamd_last_error(void) {
    return g_err;
}

void lfamd_set_error(const char *msg) { // (for the module's other translation units: comm.hip, backend glue)
    snprintf(g_err, sizeof(g_err), "%s", msg);
}

int lfamd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int lfamd_device_name(int device, char *buf, size_t len) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device), "hipGetDeviceProperties");
    snprintf(buf, len, "%s (%s)", p.name, p.gcnArchName);
    return LFAMD_OK;
}

int lfamd_init(int device) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device), "hipGetDeviceProperties");
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(LFAMD_ERR_UNSUPPORTED, "device arch %s is not gfx950 (MI355X); this module has no other code objects",
                    p.gcnArchName);
    HIPCHK(hipSetDevice(device), "hipSetDevice");
    return LFAMD_OK;
}

int lfamd_malloc(void **dptr, size_t bytes) {
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 16), "hipMalloc");
    return LFAMD_OK;
}
int lfamd_free(void *dptr) {
    HIPCHK(hipFree(dptr), "hipFree");
    return LFAMD_OK;
}
int lfamd_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync h2d");
    return LFAMD_OK;
}
int lfamd_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync d2h");
    return LFAMD_OK;
}
// Pinned, device-mapped host memory (the address is valid on the device too): lets a decode-sized call read its activations and
// write its result in place over PCIe instead of through two DMA transfers (sgemm_host.cpp, n = 1).
int lfamd_host_alloc(void **p, size_t bytes) {
    (void)hipGetLastError();
    HIPCHK(hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocPortable), "hipHostMalloc");
    return LFAMD_OK;
}
int lfamd_host_free(void *p) {
    if (p)
        HIPCHK(hipHostFree(p), "hipHostFree");
    return LFAMD_OK;
}
int lfamd_memset(void *dst, int value, size_t bytes, void *stream) {
    HIPCHK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream), "hipMemsetAsync");
    return LFAMD_OK;
}
int lfamd_stream_sync(void *stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    return LFAMD_OK;
}

// ---------------------------------------------------------------------------------------------

static bool type_known(int t) {
    switch (t) {
    case LFAMD_TYPE_F32:
    case LFAMD_TYPE_F16:
    case LFAMD_TYPE_BF16:
    case LFAMD_TYPE_Q4_0:
    case LFAMD_TYPE_Q4_1:
    case LFAMD_TYPE_Q5_0:
    case LFAMD_TYPE_Q5_1:
    case LFAMD_TYPE_Q8_0:
    case LFAMD_TYPE_Q2_K:
    case LFAMD_TYPE_Q3_K:
    case LFAMD_TYPE_Q4_K:
    case LFAMD_TYPE_Q5_K:
    case LFAMD_TYPE_Q6_K:
    case LFAMD_TYPE_IQ4_XS:
        return true;
    default:
        return false;
    }
}

// Q8_0: bytes of the P80 image (256-aligned: the PC8 image starts behind it)
static size_t q80_p80_bytes(long rows, long cols) {
    return align_up((size_t)((rows + 7) / 8) * (size_t)((cols / 32 + 3) / 4) * P80_TILE, 256);
}

size_t lfamd_packed_size(int type, long rows, long cols) {
    if (!type_known(type) || rows < 0 || cols < 0 || cols % lfamd_blck_size(type))
        return 0;
    switch (type) {
    case LFAMD_TYPE_Q4_K:
        return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * P4K_TILE;
    case LFAMD_TYPE_Q4_0:
        if (cols % 256 == 0) // P40; other row lengths stay RAW (generic kernels)
            return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * P4K_TILE;
        return (size_t)rows * lfamd_row_size(type, cols);
    case LFAMD_TYPE_Q5_K:
        return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * P5K_TILE;
    case LFAMD_TYPE_Q6_K:
        return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * P6K_TILE;
    case LFAMD_TYPE_Q8_0: // P80, the ONE resident image (1.0625 bytes per weight, the file's): the bit-exact vecdot GEMV, the exact
                          // batch kernel and the f16 MFMA batch body (gemm_lf.hip) all read it.  A host that opted into the vendor GEMM
                          // (LFAMD_USE_BLASLT=1) also keeps the plain f16(d * q) rows that library needs (3.1 bytes per weight)
        if (lfamd_blaslt_ok())
            return q80_p80_bytes(rows, cols) + (size_t)rows * (size_t)cols * 2;
        return q80_p80_bytes(rows, cols);
    case LFAMD_TYPE_Q2_K:
    case LFAMD_TYPE_Q3_K: // PK2 / PK3: compact images (84 / 116 bytes per 256 weights) the decode GEMV reads; batches expand them
        return lfamd_pk_bytes(type, rows, cols); // into the canonical PCK image in the workspace, per call
    case LFAMD_TYPE_IQ4_XS: // codebook indices on the P4K nibble lattice + 16 header bytes per row (144 bytes per 256 weights, 1.06 x
                            // the file); batches expand it per call into the PC8 byte image in the workspace
        return (size_t)((rows + 31) / 32) * (size_t)(cols / 256) * P4K_TILE;
    case LFAMD_TYPE_Q4_1:
    case LFAMD_TYPE_Q5_0:
    case LFAMD_TYPE_Q5_1:
        if (cols % 256 == 0) // PCL; other row lengths stay RAW (generic kernels)
            return lfamd_wprep32_bytes(rows, cols);
        return (size_t)rows * lfamd_row_size(type, cols);
    default:
        return (size_t)rows * lfamd_row_size(type, cols);
    }
}

int lfamd_pack_weights(int type, long rows, long cols, const void *d_raw, size_t raw_row_bytes, void *d_packed,
                       void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    if (!type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "pack_weights: unsupported ggml type%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(type) || raw_row_bytes < lfamd_row_size(type, cols))
        return fail(LFAMD_ERR_INVALID, "pack_weights: bad shape%s", "");
    if (rows == 0 || cols == 0)
        return LFAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (type) {
    case LFAMD_TYPE_Q4_K:
        HIPCHK(lfamd_launch_pack_q4k(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_q4k");
        break;
    case LFAMD_TYPE_Q4_0:
        if (cols % 256 == 0) {
            HIPCHK(lfamd_launch_pack_q40(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_q40");
        } else {
            HIPCHK(lfamd_launch_pack_raw(d_raw, raw_row_bytes, rows, lfamd_row_size(type, cols), d_packed, s), "pack_raw");
        }
        break;
    case LFAMD_TYPE_Q5_K:
        HIPCHK(lfamd_launch_pack_q5k(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_q5k");
        break;
    case LFAMD_TYPE_Q6_K:
        HIPCHK(lfamd_launch_pack_q6k(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_q6k");
        break;
    case LFAMD_TYPE_Q8_0:
        HIPCHK(lfamd_launch_pack_q80(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_q80");
        if (lfamd_blaslt_ok())
            HIPCHK(lfamd_launch_q80_image(d_raw, raw_row_bytes, rows, cols, (uint8_t *)d_packed + q80_p80_bytes(rows, cols), s), "pack_f16 (Q8_0)");
        break;
    case LFAMD_TYPE_Q2_K:
    case LFAMD_TYPE_Q3_K:
        HIPCHK(lfamd_launch_pk_pack(type, d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_pk");
        break;
    case LFAMD_TYPE_IQ4_XS:
        HIPCHK(lfamd_launch_pk4x_pack(d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_pk4x");
        break;
    case LFAMD_TYPE_Q4_1:
    case LFAMD_TYPE_Q5_0:
    case LFAMD_TYPE_Q5_1:
        if (cols % 256 == 0) {
            HIPCHK(lfamd_launch_wprep32(type, d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_pcl");
        } else {
            HIPCHK(lfamd_launch_pack_raw(d_raw, raw_row_bytes, rows, lfamd_row_size(type, cols), d_packed, s), "pack_raw");
        }
        break;
    default:
        HIPCHK(lfamd_launch_pack_raw(d_raw, raw_row_bytes, rows, lfamd_row_size(type, cols), d_packed, s), "pack_raw");
    }
    return LFAMD_OK;
}

// Reading a resident image back (dequant.hip).  Neither call enters plan_mul_mat: no dispatch decision depends on them, they take no
// workspace, allocate nothing and read nothing back, so both are capturable like lfamd_mul_mat.
int lfamd_get_rows(int type, const void *d_packed, long rows, long cols, const int32_t *d_ids, long row0, long n_ids, int out_type,
                   void *d_out, size_t out_row_bytes, void *stream) {
    (void)hipGetLastError(); // (as lfamd_pack_weights)
    if (!type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "get_rows: unsupported ggml type%s", "");
    if (out_type != LFAMD_TYPE_F32 && out_type != LFAMD_TYPE_F16)
        return fail(LFAMD_ERR_UNSUPPORTED, "get_rows: out_type must be F32 or F16%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(type) || n_ids < 0)
        return fail(LFAMD_ERR_INVALID, "get_rows: bad shape%s", "");
    const size_t esz = out_type == LFAMD_TYPE_F32 ? 4 : 2;
    if (out_row_bytes < (size_t)cols * esz || out_row_bytes % esz)
        return fail(LFAMD_ERR_INVALID, "get_rows: out_row_bytes %s", "smaller than a row or not a multiple of the element");
    if (!d_ids && (row0 < 0 || row0 > rows || n_ids > rows - row0))
        return fail(LFAMD_ERR_INVALID, "get_rows: rows row0 .. row0 + n_ids %s", "outside the matrix");
    if (n_ids == 0 || cols == 0)
        return LFAMD_OK;
    if (!d_packed || !d_out)
        return fail(LFAMD_ERR_INVALID, "get_rows: null pointer%s", "");
    if ((uintptr_t)d_out % esz)
        return fail(LFAMD_ERR_INVALID, "get_rows: d_out %s", "not aligned to the element");
    HIPCHK(lfamd_launch_get_rows(type, d_packed, rows, cols, d_ids, d_ids ? 0 : row0, n_ids, out_type, d_out, out_row_bytes, (hipStream_t)stream),
           "get_rows");
    return LFAMD_OK;
}

int lfamd_unpack_weights(int type, long rows, long cols, const void *d_packed, void *d_raw, size_t raw_row_bytes, void *stream) {
    (void)hipGetLastError();
    if (!type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "unpack_weights: unsupported ggml type%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(type) || raw_row_bytes < lfamd_row_size(type, cols))
        return fail(LFAMD_ERR_INVALID, "unpack_weights: bad shape%s", "");
    if (rows == 0 || cols == 0)
        return LFAMD_OK;
    if (!d_packed || !d_raw)
        return fail(LFAMD_ERR_INVALID, "unpack_weights: null pointer%s", "");
    HIPCHK(lfamd_launch_unpack(type, d_packed, rows, cols, d_raw, raw_row_bytes, (hipStream_t)stream), "unpack_weights");
    return LFAMD_OK;
}

int lfamd_scaled_gemm_ok(int type, long rows, long cols, const void *d_packed, void *stream) {
    (void)hipGetLastError();
    if (!type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "scaled_gemm_ok: unsupported ggml type%s", "");
    if ((type != LFAMD_TYPE_Q4_K && type != LFAMD_TYPE_Q5_K && type != LFAMD_TYPE_Q6_K && type != LFAMD_TYPE_Q8_0) || rows <= 0 || cols <= 0)
        return 1;
    if (cols % (type == LFAMD_TYPE_Q8_0 ? 32 : 256) || !d_packed)
        return fail(LFAMD_ERR_INVALID, "scaled_gemm_ok: bad shape%s", "");
    hipStream_t s = (hipStream_t)stream;
    int *d_flag = nullptr, h_flag = 0;
    HIPCHK(hipMalloc(&d_flag, sizeof(int)), "hipMalloc");
    hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(int), s);
    if (e == hipSuccess)
        e = lfamd_launch_scaled_ok(type, rows, cols, d_packed, d_flag, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)hipFree(d_flag);
    HIPCHK(e, "scaled_gemm_ok");
    return h_flag ? 0 : 1;
}

int lfamd_quantize_rows(int vec_dot_type, const float *d_x, long nrows, long cols, size_t x_row_bytes, void *d_y,
                        size_t y_row_bytes, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    if (vec_dot_type != LFAMD_TYPE_Q8_0 && vec_dot_type != LFAMD_TYPE_Q8_1 && vec_dot_type != LFAMD_TYPE_Q8_K)
        return fail(LFAMD_ERR_UNSUPPORTED, "quantize_rows: unsupported activation type%s", "");
    if (cols % lfamd_blck_size(vec_dot_type) || y_row_bytes < lfamd_row_size(vec_dot_type, cols))
        return fail(LFAMD_ERR_INVALID, "quantize_rows: bad shape%s", "");
    HIPCHK(lfamd_launch_quantize(vec_dot_type, d_x, nrows, cols, x_row_bytes, d_y, y_row_bytes, (hipStream_t)stream),
           "quantize_rows");
    return LFAMD_OK;
}

// ---------------------------------------------------------------------------------------------
// Dispatch.  plan_mul_mat answers, once per call, which body runs it; lfamd_mul_mat launches that body, and lfamd_mul_mat_is_exact,
// _takes_staged, _takes_staged_scaled and _workspace read the same plan.  DESIGN.md "Dispatch" has the table.  The plan makes no
// HIP call (lfamd_blaslt_ok() touches the device only when a host opted into the vendor library, LFAMD_USE_BLASLT=1).

// Q4_0 rows that are whole 256-weight groups are kept in the P40 layout and served by the tuned kernels
static bool packed40(int Atype, long k) {
    return Atype == LFAMD_TYPE_Q4_0 && k % 256 == 0;
}
// legacy 32-block types whose rows are whole 256-weight groups (Q4_1, Q5_0, Q5_1): resident PCL image
static bool packed_pcl(int Atype, long k) {
    return k % 256 == 0 && (Atype == LFAMD_TYPE_Q4_1 || Atype == LFAMD_TYPE_Q5_0 || Atype == LFAMD_TYPE_Q5_1);
}
static bool kquant(int Atype) {
    return Atype == LFAMD_TYPE_Q4_K || Atype == LFAMD_TYPE_Q5_K || Atype == LFAMD_TYPE_Q6_K;
}
static bool float_type(int Atype) {
    return Atype == LFAMD_TYPE_F32 || Atype == LFAMD_TYPE_F16 || Atype == LFAMD_TYPE_BF16;
}
// weights in a layout only the tuned kernels read: the decode GEMVs take them, the generic kernels do not
static bool packed(int Atype, long k) {
    return kquant(Atype) || Atype == LFAMD_TYPE_Q8_0 || Atype == LFAMD_TYPE_Q2_K || Atype == LFAMD_TYPE_Q3_K || Atype == LFAMD_TYPE_IQ4_XS ||
           packed40(Atype, k) || packed_pcl(Atype, k);
}
// F16 / BF16 matrices the loader-wave body can address (32-bit byte offsets)
static bool float_lf_fits(int Atype, long m, long k) {
    return (size_t)m * lfamd_row_size(Atype, k) < ((size_t)1 << 32);
}

static size_t gemm_act_ws(long k, long n) { // Xh + d8T + Xm of the K-quant GEMM
    size_t n_pad = align_up((size_t)n, 128), nb = (size_t)(k / 256);
    return align_up(n_pad * (size_t)k * 2, 256) + align_up(nb * n_pad * 4, 256) + align_up(n_pad * nb * 32, 256);
}
static size_t gemm_lt_ws(long k, long n) { // the 16-bit activation rows, then the library's workspace
    return align_up((size_t)n * (size_t)k * 2, 256) + lfamd_blaslt_workspace();
}

// Small batches of Q4_K / Q5_K / Q6_K (up to 32 tokens) on gemm_sb.hip, where it is the fastest route (MI355X; old -> new, us).
// Q4_K up to 8 tokens runs the int8-MFMA body, whose time barely depends on the token count (profiles/r03_small_batch_i8.txt):
//   4096 x 4096 7.8 .. 8.5 (GEMV: 6.6 at 2 tokens, 14.8 at 8), 14336 x 4096 ~ 13 (11.1 .. 24.6), 4096 x 14336 11.9 .. 13.3
//   (15.4 .. 45.4), 128256 x 4096 51 .. 54 (58 .. 138): from 2 tokens on deep rows and tall matrices, 3 with several row tiles
//   per CU, 4 with one.
// The f16 bodies (Q5_K, Q6_K, 9 .. 32 tokens; profiles/r03_small_batch.txt):
//   deep rows (k > 8192, ffn_down)          : n >= 3   (n = 8: 66 -> 20.3 Q6_K; n = 32: 28 -> 25.8)
//   at most one row tile per CU (m <= 8192) : n >= 5   (4096 x 4096: n = 32 16.9 -> 12.2)
//   up to four row tiles per CU             : 6 <= n <= 24, not Q6_K
// Below that the multi-column GEMV is faster (one launch, no staging pass); taller matrices keep the GEMV / the 128-token GEMM
// tiles.  The testing flags that force a GEMM body or the generic kernels keep their meaning.
static bool sb_takes(int Atype, long m, long k, long n, unsigned flags) {
    if ((flags & (LFAMD_FLAG_FORCE_GENERIC | LFAMD_FLAG_GEMM_NARROW | LFAMD_FLAG_GEMM_WIDE | LFAMD_FLAG_GEMM_PLAIN)) || !lfamd_gemm_sb_ok(Atype, k, n))
        return false;
    const long tiles_per_cu = ((m + 31) / 32 + 255) / 256;
    if (Atype == LFAMD_TYPE_Q4_K && n <= 8) // the int8 body
        return k > 8192 || tiles_per_cu > 4 ? n >= 2 : tiles_per_cu > 1 ? n >= 3 : n >= 4;
    if (k > 8192)
        return n >= 3;
    if (tiles_per_cu <= 1)
        return n >= 5;
    return tiles_per_cu <= 4 && Atype != LFAMD_TYPE_Q6_K && n >= 6 && n <= 24;
}

// Q4_K batches on the int8 matrix cores (gemm_i8.hip): exact integer dots; every launch whose 128 x 64 tiles fill at least half
// the CUs (row_blocks: of all the matrices of the launch), unless a testing flag asks for one of the f16 bodies
static bool i8_takes(int Atype, long k, long n, unsigned flags, long row_blocks) {
    if (flags & (LFAMD_FLAG_FORCE_GENERIC | LFAMD_FLAG_GEMM_NARROW | LFAMD_FLAG_GEMM_WIDE | LFAMD_FLAG_GEMM_PLAIN | LFAMD_FLAG_PRECISE))
        return false;
    return n > 8 && k > 0 && k % 256 == 0 && lfamd_gemm_i8_ok(Atype, row_blocks, n);
}

// The bodies of one lfamd_mul_mat call and their arithmetic (exact: integer block dots or 16-bit products with f32 sums, what
// lfamd_mul_mat_is_exact calls 1; f16-rounded: one f16 rounding per operand, <= 1e-3).
enum class mm_body {
    gemv,       // n <= 8, packed weights: the decode GEMVs (gemv.hip); exact (Q8_0: bit-exact)
    gemv_float, // n <= 8, F32 / F16 / BF16 (gemv_float.hip); exact.  Operands that are not 16-byte aligned: generic
    sb,         // 2 .. 32 tokens of Q4_K / Q5_K / Q6_K (gemm_sb.hip); exact
    i8,         // Q4_K batches on the int8 matrix cores (gemm_i8.hip); exact; reads LFAMD_TYPE_STAGED_Q8K
    kq_narrow,  // K-quant batches, the 128 x 64 split-K body on integer codes (gemm_mfma.hip); exact, Q6_K f16-rounded
    wide,       // K-quant batches, the 128 x 128 family (gemm_wide.hip).  scaled: f16-rounded, reads LFAMD_TYPE_STAGED_SCALED;
                // else integer codes: exact, Q6_K f16-rounded
    q40_wide,   // P40 Q4_0 batches on Q8_0-quantised activations, the 128 x 128 body; exact
    canon,      // Q2_K / Q3_K / IQ4_XS batches: canonical image expanded per call, the 128 x 128 body; exact, IQ4_XS f16-rounded
    canon32,    // PCL Q4_1 / Q5_0 / Q5_1 batches, the 128 x 128 body; exact
    float_lt,   // F16 / BF16 batches on the vendor GEMM (LFAMD_USE_BLASLT=1); exact.  Declined or unaligned: float_lf / float_wide
    float_lf,   // F16 / BF16 batches, the loader-wave body on the RAW rows (gemm_lf.hip); exact.  Unaligned weights: float_wide
    float_wide, // F16 / BF16 batches that the testing flags or a 32-bit byte offset keep off gemm_lf, the 128 x 128 body; exact
    q80_lt,     // Q8_0 batches on the vendor f16 GEMM (second resident image); f16-rounded.  Declined: q80_exact
    q80_lf,     // Q8_0 batches, rows of whole 128-weight quads: the f16 MFMA body on the P80 image (gemm_lf.hip); f16-rounded
    q80_exact,  // Q8_0 batches, the bit-exact kernel (gemm_q80.hip)
    generic,    // every other call (generic.hip); exact.  f32 activations of quantised weights are quantised into the workspace first
    refused,    // LFAMD_FLAG_FORCE_GENERIC on packed weights: LFAMD_ERR_UNSUPPORTED (is_exact answers 1, the flag's promise)
};
struct mm_plan {
    mm_body body;
    bool scaled;      // wide: the activations are staged scaled (prep mode 2) for the scaled-operand loader-wave bodies
    bool exact;       // lfamd_mul_mat_is_exact
    size_t workspace; // bytes lfamd_mul_mat asks for (generic: only when it quantises f32 activations)
};

static mm_plan plan_mul_mat(int Atype, long m, long k, long n, unsigned flags) {
    const unsigned forced = flags & (LFAMD_FLAG_GEMM_NARROW | LFAMD_FLAG_GEMM_WIDE | LFAMD_FLAG_GEMM_PLAIN); // (a module body, by name)
    const bool f16_q80 = !(flags & (LFAMD_FLAG_PRECISE | LFAMD_FLAG_Q80_EXACT));
    mm_plan p = {mm_body::generic, false, true, 0};
    if (flags & LFAMD_FLAG_FORCE_GENERIC)
        p.body = packed(Atype, k) ? mm_body::refused : mm_body::generic;
    else if (sb_takes(Atype, m, k, n, flags))
        p.body = mm_body::sb;
    else if (n > 8 && (kquant(Atype) || packed40(Atype, k))) {
        if (i8_takes(Atype, k, n, flags, (m + 127) / 128))
            p.body = mm_body::i8;
        else if (Atype == LFAMD_TYPE_Q4_0)
            p.body = mm_body::q40_wide;
        else {
            // Two families: 128 x 128 / 256 x 128 tiles with K streamed once (gemm_wide.hip and its loader-wave / K-split-wave /
            // row-split descendants), and the 128 x 64 split-K body (gemm_mfma.hip, exact codes) for grids below 192 tiles.  The
            // wide family runs scaled operands unless the caller wants the integer codes (LFAMD_FLAG_PRECISE / _GEMM_PLAIN); its
            // 128 x 64 tile replaces the split-K body then at every grid.
            const long tiles128 = ((m + 127) / 128) * (long)(align_up((size_t)n, 128) / 128);
            const bool can_scale = !(flags & LFAMD_FLAG_PRECISE) && lfamd_gemm_wide_scaled_ok(Atype, (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0);
            const bool narrow = (flags & LFAMD_FLAG_GEMM_NARROW) || (!(flags & LFAMD_FLAG_GEMM_WIDE) && tiles128 < 192 && !can_scale);
            p.body = narrow ? mm_body::kq_narrow : mm_body::wide;
            p.scaled = !narrow && can_scale;
            p.exact = !p.scaled && Atype != LFAMD_TYPE_Q6_K; // (both Q6_K batch bodies round sc * (q - 32) above 2048)
        }
    } else if (n > 8 && k % 256 == 0 && (Atype == LFAMD_TYPE_F16 || Atype == LFAMD_TYPE_BF16))
        p.body = forced                  ? mm_body::float_wide
                 : lfamd_blaslt_ok()     ? mm_body::float_lt
                 : float_lf_fits(Atype, m, k) ? mm_body::float_lf
                                         : mm_body::float_wide;
    else if (n <= 8 && float_type(Atype) && lfamd_gemv_float_ok(Atype, k, n))
        p.body = mm_body::gemv_float;
    else if (n > 8 && packed_pcl(Atype, k))
        p.body = mm_body::canon32;
    else if (n > 8 && (Atype == LFAMD_TYPE_Q2_K || Atype == LFAMD_TYPE_Q3_K || Atype == LFAMD_TYPE_IQ4_XS)) {
        p.body = mm_body::canon;
        p.exact = Atype != LFAMD_TYPE_IQ4_XS; // (the canonical image rounds |sc * kvalue| above 2048 to f16; Q2_K / Q3_K: |sc * q| <= 128)
    } else if (n > 8 && Atype == LFAMD_TYPE_Q8_0) {
        p.body = f16_q80 && k % 32 == 0 && lfamd_blaslt_ok()     ? mm_body::q80_lt
                 : f16_q80 && k % 128 == 0 && !lfamd_blaslt_ok() ? mm_body::q80_lf
                                                                 : mm_body::q80_exact;
        p.exact = p.body == mm_body::q80_exact;
    } else if (n <= 8 && packed(Atype, k))
        p.body = mm_body::gemv;

    const size_t n_pad = align_up((size_t)n, 128), nb = (size_t)(k / 256);
    switch (p.body) {
    case mm_body::sb:
        p.workspace = align_up(lfamd_gemm_sb_workspace(k), 256);
        break;
    case mm_body::i8: // (the staging layout every K-quant batch body shares, then partial tiles of a K-split launch)
    case mm_body::kq_narrow:
    case mm_body::wide:
        p.workspace = gemm_act_ws(k, n) + lfamd_gemm_lw_ksplit_bytes(m, n);
        break;
    case mm_body::q40_wide:
        p.workspace = gemm_act_ws(k, n);
        break;
    case mm_body::canon: // (+ the canonical image of the matrix, rebuilt from the compact one per call)
        p.workspace = gemm_act_ws(k, n) + align_up(Atype == LFAMD_TYPE_IQ4_XS ? lfamd_wprep8_bytes(m, k) : lfamd_wprep16_bytes(m, k), 256);
        break;
    case mm_body::canon32: // Xh, d8T [nb*8][n_pad], sT [nb*8][n_pad]
        p.workspace = align_up(n_pad * (size_t)k * 2, 256) + 2 * align_up(nb * 8 * n_pad * 4, 256);
        break;
    case mm_body::float_lt: // (each one may fall back on the others)
    case mm_body::float_lf:
    case mm_body::float_wide: {
        const size_t own = align_up(n_pad * (size_t)k * 2, 256), lt = lfamd_blaslt_ok() ? gemm_lt_ws(k, n) : 0;
        p.workspace = own > lt ? own : lt;
        break;
    }
    case mm_body::q80_lt:
        p.workspace = gemm_lt_ws(k, n);
        break;
    case mm_body::q80_lf:
        p.workspace = align_up(lfamd_gemm_lf_workspace(k, n), 256);
        break;
    case mm_body::q80_exact:
        p.workspace = align_up(lfamd_gemm_q80_workspace(k, n), 256);
        break;
    case mm_body::generic:
        p.workspace = float_type(Atype) ? 0 : align_up((size_t)n * lfamd_row_size(lfamd_vec_dot_type(Atype), k), 256);
        break;
    default:
        break;
    }
    return p;
}

int lfamd_mul_mat_is_exact(int Atype, long m, long k, long n, unsigned flags) {
    if (!type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).exact ? 1 : 0;
}

// Does a call accept the scaled-operand staged image a fused producer wrote (LFAMD_TYPE_STAGED_SCALED)?  The K-quant batches whose
// body reads it: what lfamd_mul_mat would stage with prep_scaled_kernel itself.
int lfamd_mul_mat_takes_staged_scaled(int Atype, long m, long k, long n, unsigned flags) {
    if (!type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    const mm_plan p = plan_mul_mat(Atype, m, k, n, flags);
    return p.body == mm_body::wide && p.scaled ? 1 : 0;
}

// Does a call accept the staged image a fused producer wrote (LFAMD_TYPE_STAGED_Q8K)?  Exactly the calls that run the int8 body.
int lfamd_mul_mat_takes_staged(int Atype, long m, long k, long n, unsigned flags) {
    if (!type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).body == mm_body::i8 ? 1 : 0;
}

// The largest workspace of the bodies this call can run: the default one and any a testing flag can force.
size_t lfamd_mul_mat_workspace(int Atype, long m, long k, long n) {
    if (!type_known(Atype))
        return 0;
    size_t best = 0;
    for (unsigned f : {0u, (unsigned)LFAMD_FLAG_PRECISE, (unsigned)LFAMD_FLAG_Q80_EXACT, (unsigned)LFAMD_FLAG_GEMM_NARROW,
                       (unsigned)LFAMD_FLAG_GEMM_WIDE, (unsigned)LFAMD_FLAG_GEMM_PLAIN}) {
        const size_t w = plan_mul_mat(Atype, m, k, n, f).workspace;
        best = w > best ? w : best;
    }
    return best;
}

// The largest workspace any batch of 1 .. n rows can ask for (which body serves a batch depends on n, so the size is not monotonic
// in n: a K-split launch of few tiles keeps partial tiles a larger batch does not need).  For callers that size ONE buffer for
// per-group calls of varying n (csrc/moe.hip).  Evaluated at n and at every point where a body's choice or tile count can change.
size_t lfamd_mul_mat_workspace_upto(int Atype, long m, long k, long n) {
    size_t best = 0;
    auto take = [&](long v) {
        if (v >= 1 && v <= n) {
            const size_t w = lfamd_mul_mat_workspace(Atype, m, k, v);
            best = w > best ? w : best;
        }
    };
    take(n);
    for (long v : {1L, 2L, 3L, 4L, 5L, 6L, 7L, 8L, 9L, 16L, 17L, 32L, 33L})
        take(v);
    for (long v = 64; v <= n + 63; v += 64) // token tiles of 64 and 128: the last batch of a tile count and the first of the next
        take(v), take(v + 1);
    return best;
}

struct scaled_image_ptrs {
    const void *Xh, *d8T, *Xm;
    size_t n_pad;
};
static scaled_image_ptrs scaled_image_of(const void *image, long k, long n) {
    scaled_image_ptrs p;
    p.n_pad = align_up((size_t)n, 128);
    const size_t nb = (size_t)(k / 256);
    p.Xh = image;
    p.d8T = (const uint8_t *)image + align_up(p.n_pad * (size_t)k * 2, 256);
    p.Xm = (const uint8_t *)p.d8T + align_up(nb * p.n_pad * 4, 256);
    return p;
}

static bool aligned16(const void *p) {
    return ((uintptr_t)p & 15) == 0;
}

// Everything lfamd_mul_mat checks before its first launch: LFAMD_OK and the plan, or the error the call returns.
static int check_mul_mat(int Atype, long m, long k, int Btype, const void *d_B, size_t b_row_bytes, long n, long ldc, const void *d_ws,
                         size_t ws_bytes, unsigned flags, mm_plan &p) {
    if (!type_known(Atype))
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: unsupported weight type%s", "");
    if (m < 0 || n < 0 || k < 0 || ldc < m || k % lfamd_blck_size(Atype))
        return fail(LFAMD_ERR_INVALID, "mul_mat: bad shape%s", "");
    const bool staged = Btype == LFAMD_TYPE_STAGED_Q8K || Btype == LFAMD_TYPE_STAGED_SCALED;
    if (!staged) {
        if (float_type(Atype)) {
            if (!(Btype == LFAMD_TYPE_F32 || Btype == Atype))
                return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: float weights need F32 or same-type activations%s", "");
        } else if (Btype != lfamd_vec_dot_type(Atype) && Btype != LFAMD_TYPE_F32) {
            // f32 activations (the GGML_OP_MUL_MAT boundary) are quantised on the device to the vec_dot type
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: activations must be F32 or the weight type's vec_dot format%s", "");
        }
        if (b_row_bytes < lfamd_row_size(Btype, k))
            return fail(LFAMD_ERR_INVALID, "mul_mat: activation row stride too small%s", "");
    }
    if (m == 0 || n == 0)
        return LFAMD_OK;
    p = plan_mul_mat(Atype, m, k, n, flags);
    size_t need = p.workspace;
    bool uses_ws = !(p.body == mm_body::gemv || p.body == mm_body::gemv_float || p.body == mm_body::refused ||
                     (p.body == mm_body::generic && (float_type(Atype) || Btype != LFAMD_TYPE_F32)));
    if (Btype == LFAMD_TYPE_STAGED_Q8K) { // a fused producer wrote the int8 body's staged image
        if (p.body != mm_body::i8 || !d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: this call does not run the int8 batch body (lfamd_mul_mat_takes_staged)%s", "");
        uses_ws = false;
    } else if (Btype == LFAMD_TYPE_STAGED_SCALED) { // a fused producer wrote the scaled-operand bodies' staged image
        if (p.body != mm_body::wide || !p.scaled || !d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: this call does not run a scaled-operand batch body (lfamd_mul_mat_takes_staged_scaled)%s", "");
        need = lfamd_gemm_lw_ksplit_bytes(m, n); // partial tiles of a K-split launch: the only workspace left
        uses_ws = need != 0;
    }
    if (p.body == mm_body::refused)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: FORCE_GENERIC needs RAW-layout weights; this type is packed%s", "");
    if (uses_ws && (ws_bytes < need || !d_ws))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat: workspace too small%s", "");
    return LFAMD_OK;
}

static int launch_mul_mat(const mm_plan &p, int Atype, const void *d_A, long m, long k, int Btype, const void *d_B, size_t b_row_bytes,
                          long n, float *d_C, long ldc, void *d_ws, size_t ws_bytes, unsigned flags, hipStream_t s) {
    const int plain = (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0;
    const int vregs32 = (flags & LFAMD_FLAG_Q0_VREGS32) ? 1 : 0, precise = (flags & LFAMD_FLAG_PRECISE) ? 1 : 0;
    const int vdt = lfamd_vec_dot_type(Atype);
    const size_t n_pad = align_up((size_t)n, 128), nb = (size_t)(k / 256);
    uint8_t *ws = (uint8_t *)d_ws; // the staging layout of the K-quant batch bodies: Xh, d8T, Xm
    void *Xh = ws, *d8T = ws + align_up(n_pad * (size_t)k * 2, 256), *Xm = (uint8_t *)d8T + align_up(nb * n_pad * 4, 256);
    if (Btype == LFAMD_TYPE_STAGED_Q8K) { // the GEMM alone, no staging launch
        HIPCHK(lfamd_launch_gemm_i8_staged(1, &d_A, &m, k, d_B, n, &d_C, &ldc, s), "gemm_i8 (staged input)");
        return LFAMD_OK;
    }
    if (Btype == LFAMD_TYPE_STAGED_SCALED) {
        const scaled_image_ptrs im = scaled_image_of(d_B, k, n);
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, im.Xh, im.d8T, im.Xm, n, (long)im.n_pad, d_C, ldc, plain | 2, d_ws, ws_bytes, s),
               "gemm_wide (staged input)");
        return LFAMD_OK;
    }
    switch (p.body) {
    case mm_body::sb: // a handful of tokens: weights streamed once, MFMA tile of 32 token slots
        HIPCHK(lfamd_launch_gemm_sb(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, 0, s), "gemm_sb");
        return LFAMD_OK;
    case mm_body::i8:
        HIPCHK(lfamd_launch_gemm_i8(1, &d_A, &m, k, Btype, d_B, b_row_bytes, n, &d_C, &ldc, d_ws, nullptr, s), "gemm_i8");
        return LFAMD_OK;
    case mm_body::q40_wide: // Q8_0-quantised activations, eight scales per 256 (they take the Xm area too)
        HIPCHK(lfamd_launch_prep80(Btype, d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, nullptr, s), "prep80");
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, Xh, d8T, nullptr, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    case mm_body::kq_narrow:
    case mm_body::wide: {
        const int mode = p.scaled ? 2 : 0;
        if (Btype == LFAMD_TYPE_F32)
            HIPCHK(lfamd_launch_prep_f32(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mode, nullptr, s), "prep_f32");
        else
            HIPCHK(lfamd_launch_prep_q8k(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mode, nullptr, s), "prep_q8k");
        if (p.body == mm_body::kq_narrow) {
            HIPCHK(lfamd_launch_gemm_kq(Atype, d_A, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, s), "gemm_kq");
        } else {
            uint8_t *Pp = (uint8_t *)Xm + align_up(n_pad * nb * 32, 256); // after Xh, d8T, Xm
            HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, plain | mode, Pp, (size_t)(ws + ws_bytes - Pp), s),
                   "gemm_wide");
        }
        return LFAMD_OK;
    }
    case mm_body::canon32: {
        void *sT = (uint8_t *)d8T + align_up(nb * 8 * n_pad * 4, 256);
        const bool q81 = vdt == LFAMD_TYPE_Q8_1;
        HIPCHK(lfamd_launch_prep80(Btype, d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, q81 ? sT : nullptr, s), "prep80");
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, Xh, d8T, q81 ? sT : nullptr, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    }
    case mm_body::canon: {
        const int mins16 = Atype == LFAMD_TYPE_Q2_K;
        if (Btype == LFAMD_TYPE_F32)
            HIPCHK(lfamd_launch_prep_f32(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mins16, nullptr, s), "prep_f32");
        else
            HIPCHK(lfamd_launch_prep_q8k(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mins16, nullptr, s), "prep_q8k");
        // the resident image is the compact one; the MFMA body reads the canonical form, rebuilt here per call
        void *img = ws + gemm_act_ws(k, n);
        if (Atype == LFAMD_TYPE_IQ4_XS)
            HIPCHK(lfamd_launch_pk4x_expand(d_A, m, k, img, s), "pk4x_expand");
        else
            HIPCHK(lfamd_launch_pk_expand(Atype, d_A, m, k, img, s), "pk_expand");
        HIPCHK(lfamd_launch_gemm_wide(Atype, img, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    }
    case mm_body::float_lt: // the vendor's GEMM on plain 16-bit float weights
        if (aligned16(d_A) && (Btype == LFAMD_TYPE_F32 || (aligned16(d_B) && !(b_row_bytes & 15)))) {
            const void *X16 = d_B;
            long ldx = (long)(b_row_bytes / 2);
            if (Btype == LFAMD_TYPE_F32) {
                HIPCHK(lfamd_launch_rows_to_16(Atype, d_B, b_row_bytes, n, k, ws, s), "rows_to_16");
                X16 = ws, ldx = k;
            }
            if (lfamd_blaslt_gemm(Atype, d_A, k, X16, ldx, m, n, k, d_C, ldc, ws + align_up((size_t)n * (size_t)k * 2, 256),
                                  lfamd_blaslt_workspace(), s) == hipSuccess)
                return LFAMD_OK;
            (void)hipGetLastError(); // the library declined this shape: this module's body
        }
        [[fallthrough]];
    case mm_body::float_lf:
    case mm_body::float_wide:
        HIPCHK(lfamd_launch_prep_float(Atype, Btype, d_B, b_row_bytes, n, (long)n_pad, k, d_ws, s), "prep_float");
        if (p.body != mm_body::float_wide && aligned16(d_A) && float_lf_fits(Atype, m, k)) {
            HIPCHK(lfamd_launch_gemm_lf_float(Atype, d_A, lfamd_row_size(Atype, k), m, k, d_ws, n, (long)n_pad, d_C, ldc, s), "gemm_lf (float)");
            return LFAMD_OK;
        }
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, d_ws, d_ws, d_ws, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    case mm_body::q80_lt: {
        const void *img = (const uint8_t *)d_A + q80_p80_bytes(m, k); // f16(d * q) rows, built once by lfamd_pack_weights
        HIPCHK(lfamd_launch_q80_rows_to_f16(Btype, d_B, b_row_bytes, n, k, ws, s), "q80_rows_to_f16");
        if (lfamd_blaslt_gemm(LFAMD_TYPE_F16, img, k, ws, k, m, n, k, d_C, ldc, ws + align_up((size_t)n * (size_t)k * 2, 256),
                              lfamd_blaslt_workspace(), s) == hipSuccess)
            return LFAMD_OK;
        // the library declined this shape or this device: the bit-exact kernel on the resident P80 image (the workspace is sized for
        // either, lfamd_mul_mat_workspace)
        (void)hipGetLastError();
        if (ws_bytes < align_up(lfamd_gemm_q80_workspace(k, n), 256))
            return fail(LFAMD_ERR_WORKSPACE, "mul_mat: workspace too small%s", "");
        HIPCHK(lfamd_launch_gemm_q80(d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, vregs32, precise, s), "gemm_q80 (library declined)");
        return LFAMD_OK;
    }
    case mm_body::q80_lf:
        HIPCHK(lfamd_launch_gemm_lf_q80(1, &d_A, &m, k, Btype, d_B, b_row_bytes, n, &d_C, &ldc, d_ws, s), "gemm_lf (Q8_0)");
        return LFAMD_OK;
    case mm_body::q80_exact:
        HIPCHK(lfamd_launch_gemm_q80(d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, vregs32, precise, s), "gemm_q80");
        return LFAMD_OK;
    case mm_body::gemv:
        HIPCHK(lfamd_launch_gemv(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, vregs32, precise, s), "gemv");
        return LFAMD_OK;
    case mm_body::gemv_float: // decode on float weights (16-byte loads)
        if (aligned16(d_A) && aligned16(d_B) && !(b_row_bytes & 15)) {
            HIPCHK(lfamd_launch_gemv_float(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, s), "gemv_float");
            return LFAMD_OK;
        }
        [[fallthrough]];
    case mm_body::generic:
        if (!float_type(Atype) && Btype == LFAMD_TYPE_F32) {
            const size_t qrow = lfamd_row_size(vdt, k);
            HIPCHK(lfamd_launch_quantize(vdt, (const float *)d_B, n, k, b_row_bytes, d_ws, qrow, s), "quantize_rows");
            HIPCHK(lfamd_launch_generic(Atype, d_A, m, k, vdt, d_ws, qrow, n, d_C, ldc, s), "generic");
            return LFAMD_OK;
        }
        HIPCHK(lfamd_launch_generic(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, s), "generic");
        return LFAMD_OK;
    default: // (refused: check_mul_mat returned the error)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: no body for this call%s", "");
    }
}

int lfamd_mul_mat(int Atype, const void *d_A, long m, long k, int Btype, const void *d_B, size_t b_row_bytes, long n, float *d_C, long ldc,
                  void *d_ws, size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    mm_plan p = {};
    const int r = check_mul_mat(Atype, m, k, Btype, d_B, b_row_bytes, n, ldc, d_ws, ws_bytes, flags, p);
    if (r != LFAMD_OK || m == 0 || n == 0)
        return r;
    return launch_mul_mat(p, Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Sibling matrices of one type on the same activations (lfamd_mul_mat_multi): one group-level route, decided and checked by
// check_multi before anything is launched.
enum class mm_route {
    none,         // nothing to launch
    each,         // one lfamd_mul_mat per matrix (every one of them checked first)
    staged_i8,    // LFAMD_TYPE_STAGED_Q8K: the int8 body over up to four matrices per launch
    staged_wide,  // LFAMD_TYPE_STAGED_SCALED: the scaled wide body over the concatenated row blocks
    sb_shared,    // gemm_sb per matrix on activations staged once
    gemv_multi,   // one fused decode GEMV launch
    i8_multi,     // the int8 body over the concatenated row blocks
    wide_multi,   // one staging, the wide body over the concatenated row blocks
    q80_lf_multi, // one staging, gemm_lf_q80 over the concatenated row blocks
};

// sibling matrices of one type on one launch of the int8 body: their row blocks together must make a grid it takes
static bool multi_i8_ok(int Atype, int count, const long *m, const long *ldc, long k, long n, unsigned flags) {
    long rbs = 0;
    for (int j = 0; j < count; j++) {
        if (m[j] < 0 || ldc[j] < m[j])
            return false;
        rbs += (m[j] + 127) / 128;
    }
    return rbs > 0 && i8_takes(Atype, k, n, flags, rbs);
}

// 2 .. 4 K-quant siblings whose concatenated row blocks fill the chip with 128 x 128 tiles (or LFAMD_FLAG_GEMM_WIDE asks for it)
static bool wide_group_ok(int Atype, int count, const long *m, const long *ldc, long k, long n, unsigned flags) {
    if (count < 2 || count > 4 || n <= 8 || !kquant(Atype) || k <= 0 || k % 256 || (flags & (LFAMD_FLAG_FORCE_GENERIC | LFAMD_FLAG_GEMM_NARROW)))
        return false;
    long rbs = 0;
    for (int j = 0; j < count; j++) {
        if (m[j] < 0 || ldc[j] < m[j])
            return false;
        rbs += (m[j] + 127) / 128;
    }
    return rbs * (long)(align_up((size_t)n, 128) / 128) >= 192 || (flags & LFAMD_FLAG_GEMM_WIDE);
}

static bool scaled_ok(int Atype, unsigned flags) { // may the wide body run on scaled operands?
    return !(flags & LFAMD_FLAG_PRECISE) && lfamd_gemm_wide_scaled_ok(Atype, (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0);
}

static int check_multi(int Atype, int count, const long *m, long k, int Btype, const void *d_B, size_t b_row_bytes, long n, const long *ldc,
                       const void *d_ws, size_t ws_bytes, unsigned flags, mm_route &route) {
    route = mm_route::none;
    if (count <= 0 || ((Btype == LFAMD_TYPE_STAGED_Q8K || Btype == LFAMD_TYPE_STAGED_SCALED) && n == 0))
        return LFAMD_OK;
    if (Btype == LFAMD_TYPE_STAGED_Q8K) { // every matrix must take the image
        if (!(count > 1 && count <= 4 && multi_i8_ok(Atype, count, m, ldc, k, n, flags))) // (else: each matrix by itself)
            for (int j = 0; j < count; j++)
                if (m[j] > 0 && (ldc[j] < m[j] || !lfamd_mul_mat_takes_staged(Atype, m[j], k, n, flags)))
                    return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: a matrix of this call does not run the int8 batch body%s", "");
        route = mm_route::staged_i8;
        return LFAMD_OK;
    }
    route = mm_route::each;
    if (Btype == LFAMD_TYPE_STAGED_SCALED) { // the route the same call takes on f32 rows
        if (!d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_INVALID, "mul_mat_multi: the staged image must be 16-byte aligned%s", "");
        if (count > 1 && count <= 4 && multi_i8_ok(Atype, count, m, ldc, k, n, flags))
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: these matrices run the int8 batch body together (LFAMD_TYPE_STAGED_Q8K)%s", "");
        if (wide_group_ok(Atype, count, m, ldc, k, n, flags) && scaled_ok(Atype, flags))
            route = mm_route::staged_wide;
    } else if (!(count == 1 && sb_takes(Atype, m[0], k, n, flags))) { // (a handful of tokens on one matrix, attn_output / ffn_down: gemm_sb by itself)
        const bool rows_ok = (Btype == LFAMD_TYPE_F32 || Btype == lfamd_vec_dot_type(Atype)) && b_row_bytes >= lfamd_row_size(Btype, k);
        // several tokens (6 and more) on sibling matrices that all take the small-batch MFMA kernel (ffn_gate + ffn_up): the
        // activations are staged once, then one launch per matrix — 14336 x 4096 x 2 at 8 tokens: 39.8 us on the multi-column GEMV,
        // 32.7 us as two separate calls, less with the shared staging
        const bool i8_body = Atype == LFAMD_TYPE_Q4_K && n <= 8;
        bool all_sb = count > 1 && n >= (i8_body ? 4 : 6) && rows_ok;
        for (int j = 0; j < count && all_sb; j++) // (small siblings — attn_k / attn_v — are faster on the fused GEMV below 8 tokens)
            all_sb = (m[j] > 8192 || (i8_body && n >= 8)) && ldc[j] >= m[j] && sb_takes(Atype, m[j], k, n, flags);
        // one fused launch when the GEMV path applies to every matrix
        bool gemv = count <= 4 && n <= 8 && !(flags & LFAMD_FLAG_FORCE_GENERIC) && packed(Atype, k) && rows_ok && k > 0 &&
                    k % lfamd_blck_size(Atype) == 0 && (Atype == LFAMD_TYPE_Q8_0 || k % 256 == 0);
        for (int j = 0; j < count && gemv; j++)
            gemv = m[j] >= 0 && ldc[j] >= m[j];
        bool q80_lf = count > 1 && count <= 4 && Atype == LFAMD_TYPE_Q8_0 && k > 0 && rows_ok &&
                      plan_mul_mat(Atype, m[0], k, n, flags).body == mm_body::q80_lf;
        for (int j = 0; j < count && q80_lf; j++)
            q80_lf = m[j] >= 0 && ldc[j] >= m[j];
        size_t need = 0;
        if (all_sb)
            route = mm_route::sb_shared, need = align_up(lfamd_gemm_sb_workspace(k), 256);
        else if (gemv)
            route = n == 0 ? mm_route::none : mm_route::gemv_multi;
        // Q4_K siblings whose tiles TOGETHER make a grid the int8 body takes (attn_q/k/v of an all-Q4_K layer: 48 row blocks at 512
        // tokens): one staging, one launch over the concatenated row blocks, exact integer dots (6144 x 4096 x 512: 47.5 us against 56.8)
        else if (count > 1 && count <= 4 && rows_ok && k > 0 && multi_i8_ok(Atype, count, m, ldc, k, n, flags))
            route = mm_route::i8_multi, need = lfamd_gemm_i8_workspace(k, n);
        // K-quant batches: ONE activation prep for all the matrices, and one launch of the 128 x 128 body over their concatenated
        // row blocks when that grid fills the chip (attn_q/k/v: 48 + 8 + 8 row blocks instead of three launches of which two fill a
        // quarter of the CUs)
        else if (rows_ok && wide_group_ok(Atype, count, m, ldc, k, n, flags))
            route = mm_route::wide_multi, need = gemm_act_ws(k, n);
        // Q8_0 batches on sibling matrices: one staging of the activations, one launch over the concatenated row blocks
        else if (q80_lf)
            route = mm_route::q80_lf_multi, need = lfamd_gemm_lf_workspace(k, n);
        const bool uses_ws = route == mm_route::sb_shared || route == mm_route::i8_multi || route == mm_route::wide_multi ||
                             route == mm_route::q80_lf_multi;
        if (uses_ws && (ws_bytes < need || !d_ws))
            return fail(LFAMD_ERR_WORKSPACE, "mul_mat_multi: workspace too small%s", "");
    }
    if (route == mm_route::each) // one call per matrix: each must pass lfamd_mul_mat's checks before the first is launched
        for (int j = 0; j < count; j++) {
            mm_plan p = {};
            const int r = check_mul_mat(Atype, m[j], k, Btype, d_B, b_row_bytes, n, ldc[j], d_ws, ws_bytes, flags, p);
            if (r != LFAMD_OK)
                return r;
        }
    return LFAMD_OK;
}

int lfamd_mul_mat_multi(int Atype, int count, const void *const *d_A, const long *m, long k, int Btype, const void *d_B,
                        size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws, size_t ws_bytes,
                        unsigned flags, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    mm_route route;
    const int r = check_multi(Atype, count, m, k, Btype, d_B, b_row_bytes, n, ldc, d_ws, ws_bytes, flags, route);
    if (r != LFAMD_OK)
        return r;
    hipStream_t s = (hipStream_t)stream;
    const int plain = (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0;
    const size_t n_pad = align_up((size_t)n, 128), nb = (size_t)(k / 256);
    switch (route) {
    case mm_route::none:
        return LFAMD_OK;
    case mm_route::each:
        for (int j = 0; j < count; j++) {
            const int rj = lfamd_mul_mat(Atype, d_A[j], m[j], k, Btype, d_B, b_row_bytes, n, d_C[j], ldc[j], d_ws, ws_bytes, flags, stream);
            if (rj != LFAMD_OK)
                return rj;
        }
        return LFAMD_OK;
    case mm_route::staged_i8:
        for (int j0 = 0; j0 < count; j0 += 4) {
            const int c = count - j0 < 4 ? count - j0 : 4;
            HIPCHK(lfamd_launch_gemm_i8_staged(c, d_A + j0, m + j0, k, d_B, n, d_C + j0, ldc + j0, s), "gemm_i8 (staged input, multi)");
        }
        return LFAMD_OK;
    case mm_route::staged_wide: {
        const scaled_image_ptrs im = scaled_image_of(d_B, k, n);
        HIPCHK(lfamd_launch_gemm_wide_multi(Atype, count, d_A, m, k, im.Xh, im.d8T, im.Xm, n, (long)im.n_pad, d_C, ldc, plain | 2, nullptr, 0, s),
               "gemm_wide_multi (staged input)");
        return LFAMD_OK;
    }
    case mm_route::sb_shared:
        for (int j = 0; j < count; j++)
            HIPCHK(lfamd_launch_gemm_sb(Atype, d_A[j], m[j], k, Btype, d_B, b_row_bytes, n, d_C[j], ldc[j], d_ws, j > 0, s), "gemm_sb (multi)");
        return LFAMD_OK;
    case mm_route::gemv_multi:
        HIPCHK(lfamd_launch_gemv_multi(Atype, count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, (flags & LFAMD_FLAG_Q0_VREGS32) ? 1 : 0,
                                       (flags & LFAMD_FLAG_PRECISE) ? 1 : 0, s),
               "gemv_multi");
        return LFAMD_OK;
    case mm_route::i8_multi:
        HIPCHK(lfamd_launch_gemm_i8(count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, nullptr, s), "gemm_i8 (multi)");
        return LFAMD_OK;
    case mm_route::wide_multi: {
        uint8_t *ws = (uint8_t *)d_ws;
        void *Xh = ws, *d8T = ws + align_up(n_pad * (size_t)k * 2, 256), *Xm = (uint8_t *)d8T + align_up(nb * n_pad * 4, 256);
        const int mode = scaled_ok(Atype, flags) ? 2 : 0;
        if (Btype == LFAMD_TYPE_F32)
            HIPCHK(lfamd_launch_prep_f32(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mode, nullptr, s), "prep_f32");
        else
            HIPCHK(lfamd_launch_prep_q8k(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, mode, nullptr, s), "prep_q8k");
        HIPCHK(lfamd_launch_gemm_wide_multi(Atype, count, d_A, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, plain | mode, nullptr, 0, s),
               "gemm_wide_multi");
        return LFAMD_OK;
    }
    case mm_route::q80_lf_multi:
        HIPCHK(lfamd_launch_gemm_lf_q80(count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, s), "gemm_lf (Q8_0, multi)");
        return LFAMD_OK;
    }
    return LFAMD_OK;
}

// Sibling mat-muls on the same activations whose weight types may differ (a backend's graph_compute sees attn_q/k/v as
// three MUL_MAT nodes with one src1; in a Q4_K_M file q and k are Q4_K, v is Q6_K).  Decode (n = 1) with exactly two
// K-quant types {Q4_K | Q5_K, Q6_K}: ONE launch (gemv_kq_dual_kernel).  Everything else: one lfamd_mul_mat_multi per
// run of equal types.
int lfamd_mul_mat_multi_types(int count, const int *Atype, const void *const *d_A, const long *m, long k, int Btype,
                              const void *d_B, size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws,
                              size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError();
    if (count <= 0)
        return LFAMD_OK;
    if (!Atype || !d_A || !m || !d_C || !ldc)
        return fail(LFAMD_ERR_INVALID, "mul_mat_multi_types: null argument%s", "");
    int ta = -1, tb = -1, na = 0, nb_ = 0;
    const void *Aa[4], *Ab[4];
    long ma[4], mb[4], la[4], lb[4];
    float *Ca[4], *Cb[4];
    bool dual = n == 1 && count <= 8 && k > 0 && k % 256 == 0 && !(flags & LFAMD_FLAG_FORCE_GENERIC) &&
                (Btype == LFAMD_TYPE_F32 || Btype == LFAMD_TYPE_Q8_K) && b_row_bytes >= lfamd_row_size(Btype, k);
    for (int j = 0; j < count && dual; j++) {
        const int t = Atype[j];
        if (m[j] <= 0 || ldc[j] < m[j]) {
            dual = false;
        } else if (t == LFAMD_TYPE_Q6_K) {
            if (nb_ == 4)
                dual = false;
            else
                Ab[nb_] = d_A[j], mb[nb_] = m[j], lb[nb_] = ldc[j], Cb[nb_] = d_C[j], nb_++, tb = t;
        } else if ((t == LFAMD_TYPE_Q4_K || t == LFAMD_TYPE_Q5_K) && (ta < 0 || ta == t)) {
            if (na == 4)
                dual = false;
            else
                Aa[na] = d_A[j], ma[na] = m[j], la[na] = ldc[j], Ca[na] = d_C[j], na++, ta = t;
        } else {
            dual = false;
        }
    }
    if (dual && na > 0 && nb_ > 0) {
        HIPCHK(lfamd_launch_gemv_dual(ta, na, Aa, ma, Ca, la, tb, nb_, Ab, mb, Cb, lb, k, Btype, d_B, b_row_bytes,
                                      (hipStream_t)stream),
               "gemv_dual");
        return LFAMD_OK;
    }
    // Batches whose nodes are all K-quants with a resident layout (attn_q/k = Q4_K with attn_v = Q6_K at prefill): the
    // scaled-operand GEMM of every type reads the SAME staged activations, so they are prepared once; then one launch of
    // the loader-wave body per run of equal types.
    {
        const bool staged_in = Btype == LFAMD_TYPE_STAGED_SCALED; // (a fused producer wrote the scaled image: d_B, 16-byte aligned)
        bool share = n > 8 && count > 1 && k > 0 && k % 256 == 0 && !(flags & (LFAMD_FLAG_PRECISE | LFAMD_FLAG_FORCE_GENERIC |
                                                                                LFAMD_FLAG_GEMM_NARROW)) &&
                     (staged_in ? d_B && ((uintptr_t)d_B & 15) == 0
                                : (Btype == LFAMD_TYPE_F32 || Btype == LFAMD_TYPE_Q8_K) && b_row_bytes >= lfamd_row_size(Btype, k));
        const int plain = (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0;
        bool mixed = false;
        for (int j = 0; j < count && share; j++) {
            const int t = Atype[j];
            share = (t == LFAMD_TYPE_Q4_K || t == LFAMD_TYPE_Q5_K || t == LFAMD_TYPE_Q6_K) && lfamd_gemm_wide_scaled_ok(t, plain) &&
                    m[j] >= 0 && ldc[j] >= m[j];
            mixed = mixed || t != Atype[0];
        }
        const size_t n_pad = align_up((size_t)n, 128), nbk = (size_t)(k / 256);
        const size_t need = align_up(n_pad * (size_t)k * 2, 256) + align_up(nbk * n_pad * 4, 256) + align_up(n_pad * nbk * 32, 256);
        if (share && mixed && (staged_in || (d_ws && ws_bytes >= need))) {
            hipStream_t s = (hipStream_t)stream;
            uint8_t *ws = staged_in ? (uint8_t *)const_cast<void *>(d_B) : (uint8_t *)d_ws; // (the image has the workspace's layout)
            void *Xh = ws;
            void *d8T = ws + align_up(n_pad * (size_t)k * 2, 256);
            void *Xm = (uint8_t *)d8T + align_up(nbk * n_pad * 4, 256);
            if (staged_in)
                ; // nothing to stage
            else if (Btype == LFAMD_TYPE_F32)
                HIPCHK(lfamd_launch_prep_f32(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, 2, nullptr, s), "prep_f32");
            else
                HIPCHK(lfamd_launch_prep_q8k(d_B, b_row_bytes, n, (long)n_pad, k, Xh, d8T, Xm, 2, nullptr, s), "prep_q8k");
            { // {Q4_K | Q5_K, Q6_K} whose tiles fill more than half the chip in one round: one launch for both types
                const void *Aa[4], *Ab[4];
                long ma_[4], mb_[4], la[4], lb[4];
                float *Ca[4], *Cb[4];
                int ta = -1, na = 0, nbq = 0;
                bool two = true;
                for (int j = 0; j < count && two; j++) {
                    if (Atype[j] == LFAMD_TYPE_Q6_K) {
                        two = nbq < 4;
                        if (two)
                            Ab[nbq] = d_A[j], mb_[nbq] = m[j], lb[nbq] = ldc[j], Cb[nbq] = d_C[j], nbq++;
                    } else if (ta < 0 || ta == Atype[j]) {
                        two = na < 4;
                        if (two)
                            Aa[na] = d_A[j], ma_[na] = m[j], la[na] = ldc[j], Ca[na] = d_C[j], na++, ta = Atype[j];
                    } else {
                        two = false;
                    }
                }
                if (two && na > 0 && nbq > 0) {
                    hipError_t e = lfamd_launch_gemm_wide_dual(ta, na, Aa, ma_, Ca, la, LFAMD_TYPE_Q6_K, nbq, Ab, mb_, Cb, lb, k, Xh, d8T,
                                                               Xm, n, (long)n_pad, plain | 2, s);
                    if (e == hipSuccess)
                        return LFAMD_OK;
                    if (e != hipErrorNotSupported)
                        HIPCHK(e, "gemm_wide_dual");
                }
            }
            for (int j0 = 0; j0 < count;) {
                int j1 = j0 + 1;
                while (j1 < count && Atype[j1] == Atype[j0] && j1 - j0 < 4)
                    j1++;
                HIPCHK(lfamd_launch_gemm_wide_multi(Atype[j0], j1 - j0, d_A + j0, m + j0, k, Xh, d8T, Xm, n, (long)n_pad, d_C + j0,
                                                    ldc + j0, plain | 2, nullptr, 0, s),
                       "gemm_wide_multi");
                j0 = j1;
            }
            return LFAMD_OK;
        }
    }
    // runs of equal types (up to four matrices each): every run is checked before the first one is launched
    for (int launch = 0; launch < 2; launch++)
        for (int j0 = 0; j0 < count;) {
            int j1 = j0 + 1;
            while (j1 < count && Atype[j1] == Atype[j0] && j1 - j0 < 4)
                j1++;
            mm_route route;
            const int r = launch ? lfamd_mul_mat_multi(Atype[j0], j1 - j0, d_A + j0, m + j0, k, Btype, d_B, b_row_bytes, n, d_C + j0, ldc + j0,
                                                       d_ws, ws_bytes, flags, stream)
                                 : check_multi(Atype[j0], j1 - j0, m + j0, k, Btype, d_B, b_row_bytes, n, ldc + j0, d_ws, ws_bytes, flags, route);
            if (r != LFAMD_OK)
                return r;
            j0 = j1;
        }
    return LFAMD_OK;
}

size_t lfamd_mul_mat_id_workspace(int type, long rows, long cols, int experts, long tokens, int thinkers) {
    return lfamd_moe_workspace(type, rows, cols, experts, tokens, thinkers);
}

int lfamd_mul_mat_id(int type, const void *d_W, long rows, long cols, int experts, int Btype, const void *d_thought,
                     size_t b_row_bytes, int tasks, long tokens, const int32_t *d_plan, int thinkers, float *d_result,
                     void *d_ws, size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    if (!type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_id: unsupported weight type%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(type) || experts <= 0 || tasks <= 0 || thinkers <= 0 ||
        tasks > thinkers || thinkers > experts)
        return fail(LFAMD_ERR_INVALID, "mul_mat_id: bad shape%s", "");
    // f32 activations (the GGML_OP_MUL_MAT_ID boundary) are served by the decode path, which quantises in-kernel
    const bool f32_decode = Btype == LFAMD_TYPE_F32 && !(flags & LFAMD_FLAG_FORCE_GENERIC) &&
                            ((tokens <= 4 && (type == LFAMD_TYPE_Q4_K || type == LFAMD_TYPE_Q5_K || type == LFAMD_TYPE_Q6_K)) ||
                             (tokens > 4 && cols % 256 == 0 && experts < 255 && tokens * thinkers <= 60 * 1024 &&
                              (type == LFAMD_TYPE_Q4_K || type == LFAMD_TYPE_Q5_K || type == LFAMD_TYPE_Q6_K)));
    if (Btype != lfamd_vec_dot_type(type) && !f32_decode)
        return fail(LFAMD_ERR_UNSUPPORTED,
                    "mul_mat_id: activations must be in the weight type's vec_dot format (F32 only for Q4_K / Q5_K / Q6_K experts)%s", "");
    if (tokens == 0 || rows == 0)
        return LFAMD_OK;
    size_t need = lfamd_moe_workspace(type, rows, cols, experts, tokens, thinkers);
    if (need && (ws_bytes < need || !d_ws))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat_id: workspace too small%s", "");
    HIPCHK(lfamd_launch_moe(type, d_W, rows, cols, experts, lfamd_packed_size(type, rows, cols), Btype, d_thought,
                            b_row_bytes, tasks, tokens, d_plan, thinkers, d_result, d_ws, ws_bytes, flags,
                            (hipStream_t)stream),
           "mul_mat_id");
    return LFAMD_OK;
}

int lfamd_vendor_gemm_available(void) {
    return lfamd_blaslt_ok() ? 1 : 0;
}

int lfamd_mul_mat_id_multi(int type, int count, const void *const *d_W, long rows, long cols, int experts, int Btype, const void *d_thought,
                           size_t b_row_bytes, int tasks, long tokens, const int32_t *d_plan, int thinkers, float *const *d_result,
                           void *d_ws, size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError();
    if (count <= 0)
        return LFAMD_OK;
    if (!d_W || !d_result || !d_plan || !d_thought)
        return fail(LFAMD_ERR_INVALID, "mul_mat_id_multi: null argument%s", "");
    for (int j = 0; j < count; j++) // (the fused launch below goes straight into the kernel: a null stack or result would be a device fault)
        if (!d_W[j] || !d_result[j])
            return fail(LFAMD_ERR_INVALID, "mul_mat_id_multi: null expert stack or result%s", "");
    if (tasks <= 0 || tasks > thinkers || !type_known(Btype))
        return fail(LFAMD_ERR_INVALID, "mul_mat_id_multi: bad shape or activation type%s", "");
    if (count <= 4 && type_known(type) && rows > 0 && cols > 0 && experts > 0 && thinkers > 0 && thinkers <= experts && tokens > 0 &&
        b_row_bytes >= lfamd_row_size(Btype, cols) && lfamd_moe_decode_multi_ok(type, cols, Btype, tasks, tokens, flags)) {
        HIPCHK(lfamd_launch_moe_decode_multi(type, count, d_W, rows, cols, experts, lfamd_packed_size(type, rows, cols), Btype, d_thought,
                                             b_row_bytes, tokens, d_plan, thinkers, d_result, (hipStream_t)stream),
               "mul_mat_id_multi");
        return LFAMD_OK;
    }
    for (int j = 0; j < count; j++) { // batches, other types, per-thinker activations: one operator at a time
        const int r = lfamd_mul_mat_id(type, d_W[j], rows, cols, experts, Btype, d_thought, b_row_bytes, tasks, tokens, d_plan, thinkers,
                                       d_result[j], d_ws, ws_bytes, flags, stream);
        if (r)
            return r;
    }
    return LFAMD_OK;
}

int lfamd_time_mul_mat(int Atype, const void *d_A, long m, long k, int Btype, const void *d_B, size_t b_row_bytes, long n,
                       float *d_C, long ldc, void *d_ws, size_t ws_bytes, unsigned flags, void *stream, int warmup,
                       int iters, float *avg_us) {
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < warmup; i++) {
        int r = lfamd_mul_mat(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags, stream);
        if (r)
            return r;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0), "hipEventCreate");
    HIPCHK(hipEventCreate(&e1), "hipEventCreate");
    HIPCHK(hipEventRecord(e0, s), "hipEventRecord");
    for (int i = 0; i < iters; i++) {
        int r = lfamd_mul_mat(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags, stream);
        if (r)
            return r;
    }
    HIPCHK(hipEventRecord(e1, s), "hipEventRecord");
    HIPCHK(hipEventSynchronize(e1), "hipEventSynchronize");
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_us = iters > 0 ? ms * 1000.0f / iters : 0.0f;
    return LFAMD_OK;
}
}
