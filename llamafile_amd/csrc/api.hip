// api.hip — the C ABI of libllamafile_amd_hip.so (include/lfamd_hip.h).
//
// Dispatch policy mirrors ggml_cuda_mul_mat (ggml-cuda.cu.patch:18377-18443): n <= 8 -> GEMV
// kernels (MMVQ_MAX_BATCH_SIZE = 8, :14359), otherwise the MFMA GEMM; types without a tuned kernel
// run the generic kernel.  There is no CPU fallback anywhere in this module.
#include "lfamd_device.h"
#include "../../include/lfamd_hip.h"
#include "lfamd_internal.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>

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

// LFAMD_TYPE_PAD256 (include/lfamd_hip.h): a layout modifier OR-ed into a legacy 32-block weight type.  This file is where it ends:
// lfamd_image_of (lfamd_internal.h) splits an id into the base type and the weight geometry (the columns of the resident image); the
// launchers below this file get those and the activation length (the call's own k) as separate values.

// Q8_0: bytes of the P80 image (256-aligned: the PC8 image starts behind it)
static size_t q80_p80_bytes(long rows, long cols) {
    return align_up((size_t)((rows + 7) / 8) * (size_t)((cols / 32 + 3) / 4) * P80_TILE, 256);
}

// Tiles x tile bytes, or rows x row size.  Q8_0, P80, is the ONE resident image (1.0625 bytes per weight, the file's): the bit-exact
// vecdot GEMV, the exact batch kernel and the f16 MFMA batch body (gemm_lf.hip) all read it.  A host that opted into the vendor GEMM
// (LFAMD_USE_BLASLT=1) also keeps the plain f16(d * q) rows that library needs behind it (3.1 bytes per weight).
size_t lfamd_packed_size(int type, long rows, long cols) {
    const lfamd_image im = lfamd_image_of(type, cols);
    if (im.ly == LY_NONE || rows < 0 || cols < 0 || cols % lfamd_blck_size(im.type))
        return 0;
    if (im.ly == LY_P80)
        return q80_p80_bytes(rows, cols) + (lfamd_blaslt_ok() ? (size_t)rows * (size_t)cols * 2 : 0);
    return im.tile ? im.tiles(rows) * (size_t)im.tile : (size_t)rows * lfamd_row_size(im.type, cols);
}

int lfamd_pack_weights(int type, long rows, long cols, const void *d_raw, size_t raw_row_bytes, void *d_packed,
                       void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    const lfamd_image im = lfamd_image_of(type, cols); // (the 32-block types' tile image: its packer writes a row's padded tail)
    if (im.ly == LY_NONE)
        return fail(LFAMD_ERR_UNSUPPORTED, "pack_weights: unsupported ggml type%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(im.type) || raw_row_bytes < lfamd_row_size(im.type, cols))
        return fail(LFAMD_ERR_INVALID, "pack_weights: bad shape%s", "");
    if (rows == 0 || cols == 0)
        return LFAMD_OK;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(lfamd_launch_pack(im, d_raw, raw_row_bytes, rows, cols, d_packed, s), "pack_weights");
    if (im.ly == LY_P80 && lfamd_blaslt_ok())
        HIPCHK(lfamd_launch_q80_image(d_raw, raw_row_bytes, rows, cols, (uint8_t *)d_packed + q80_p80_bytes(rows, cols), s), "pack_f16 (Q8_0)");
    return LFAMD_OK;
}

// Reading a resident image back (dequant.hip).  Neither call enters plan_mul_mat: no dispatch decision depends on them, they take no
// workspace, allocate nothing and read nothing back, so both are capturable like lfamd_mul_mat.
int lfamd_get_rows(int type, const void *d_packed, long rows, long cols, const int32_t *d_ids, long row0, long n_ids, int out_type,
                   void *d_out, size_t out_row_bytes, void *stream) {
    (void)hipGetLastError(); // (as lfamd_pack_weights)
    const lfamd_image im = lfamd_image_of(type, cols);
    if (im.ly == LY_NONE)
        return fail(LFAMD_ERR_UNSUPPORTED, "get_rows: unsupported ggml type%s", "");
    type = im.type;
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
    HIPCHK(lfamd_launch_get_rows(im, d_packed, rows, cols, d_ids, d_ids ? 0 : row0, n_ids, out_type, d_out, out_row_bytes, (hipStream_t)stream),
           "get_rows");
    return LFAMD_OK;
}

int lfamd_unpack_weights(int type, long rows, long cols, const void *d_packed, void *d_raw, size_t raw_row_bytes, void *stream) {
    (void)hipGetLastError();
    const lfamd_image im = lfamd_image_of(type, cols);
    if (im.ly == LY_NONE)
        return fail(LFAMD_ERR_UNSUPPORTED, "unpack_weights: unsupported ggml type%s", "");
    type = im.type;
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(type) || raw_row_bytes < lfamd_row_size(type, cols))
        return fail(LFAMD_ERR_INVALID, "unpack_weights: bad shape%s", "");
    if (rows == 0 || cols == 0)
        return LFAMD_OK;
    if (!d_packed || !d_raw)
        return fail(LFAMD_ERR_INVALID, "unpack_weights: null pointer%s", "");
    HIPCHK(lfamd_launch_unpack(im, d_packed, rows, cols, d_raw, raw_row_bytes, (hipStream_t)stream), "unpack_weights");
    return LFAMD_OK;
}

int lfamd_scaled_gemm_ok(int type, long rows, long cols, const void *d_packed, void *stream) {
    (void)hipGetLastError();
    if (!lfamd_type_known(type))
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
    if (nrows > 65535 || (nrows > 0 && cols > 0 && (!d_x || !d_y))) // (one grid row per input row: the launch's y limit)
        return fail(LFAMD_ERR_INVALID, "quantize_rows: null pointer or more than 65535 rows%s", "");
    HIPCHK(lfamd_launch_quantize(vec_dot_type, d_x, nrows, cols, x_row_bytes, d_y, y_row_bytes, (hipStream_t)stream),
           "quantize_rows");
    return LFAMD_OK;
}

// ---------------------------------------------------------------------------------------------
// Dispatch.  plan_mul_mat answers, once per call, which body runs it; lfamd_mul_mat launches that body, and lfamd_mul_mat_is_exact,
// _takes_staged, _takes_staged_scaled, _takes_staged_b32, _takes_staged_q80 and _workspace read the same plan.  DESIGN.md "Dispatch" has the table.  The plan makes no
// HIP call (lfamd_blaslt_ok() touches the device only when a host opted into the vendor library, LFAMD_USE_BLASLT=1).

static bool kquant(int Atype) {
    return Atype == LFAMD_TYPE_Q4_K || Atype == LFAMD_TYPE_Q5_K || Atype == LFAMD_TYPE_Q6_K;
}
static bool float_type(int Atype) {
    return Atype == LFAMD_TYPE_F32 || Atype == LFAMD_TYPE_F16 || Atype == LFAMD_TYPE_BF16;
}
// F16 / BF16 matrices the loader-wave body can address (32-bit byte offsets)
static bool float_lf_fits(int Atype, long m, long k) {
    return (size_t)m * lfamd_row_size(Atype, k) < ((size_t)1 << 32);
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
    q40_wide,   // P40 Q4_0 / IQ4_NL batches on Q8_0-quantised activations, the 128 x 128 body; exact
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
    bool bit_exact;   // lfamd_mul_mat_is_bit_exact: the result reproduces the CPU reference's bits
    bool relaxed;     // gemv on Q8_0: the relaxed-order kernel (LFAMD_FLAG_Q80_RELAXED where nothing overrides it and its plan accepts k)
    size_t workspace; // bytes lfamd_mul_mat asks for (generic: only when it quantises f32 activations)
};

// May a Q8_0 decode GEMV of this call run the relaxed-order kernel?  The flag, unless one of the flags that keep today's routes is
// set, and only where the kernel's plan takes the row (deep rows: the bit-exact kernel).  The launch passes the answer down.
static bool q80_relaxed(int Atype, long k, long n, unsigned flags) {
    return Atype == LFAMD_TYPE_Q8_0 && n <= 8 && (flags & LFAMD_FLAG_Q80_RELAXED) &&
           !(flags & (LFAMD_FLAG_PRECISE | LFAMD_FLAG_Q80_EXACT | LFAMD_FLAG_FORCE_GENERIC)) && lfamd_gemv_q80_relaxed_cols(k) > 0;
}

static mm_plan plan_mul_mat(int Atype, long m, long k, long n, unsigned flags) {
    const lfamd_image im = lfamd_image_of(Atype, k);
    if (im.type != Atype) // the padded image: the route, the answers and the workspace of the base type on rows of whole groups
        return plan_mul_mat(im.type, m, im.cols, n, flags);
    const unsigned forced = flags & (LFAMD_FLAG_GEMM_NARROW | LFAMD_FLAG_GEMM_WIDE | LFAMD_FLAG_GEMM_PLAIN); // (a module body, by name)
    const bool f16_q80 = !(flags & (LFAMD_FLAG_PRECISE | LFAMD_FLAG_Q80_EXACT));
    mm_plan p = {mm_body::generic, false, true, false, false, 0};
    if (flags & LFAMD_FLAG_FORCE_GENERIC)
        p.body = im.tuned() ? mm_body::refused : mm_body::generic;
    else if (sb_takes(Atype, m, k, n, flags))
        p.body = mm_body::sb;
    else if (n > 8 && (kquant(Atype) || im.p40())) {
        if (i8_takes(Atype, k, n, flags, (m + 127) / 128))
            p.body = mm_body::i8;
        else if (Atype == LFAMD_TYPE_Q4_0 || Atype == LFAMD_TYPE_IQ4_NL)
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
    else if (n > 8 && im.pcl())
        p.body = mm_body::canon32;
    else if (n > 8 && (Atype == LFAMD_TYPE_Q2_K || Atype == LFAMD_TYPE_Q3_K || Atype == LFAMD_TYPE_IQ4_XS)) {
        p.body = mm_body::canon;
        p.exact = Atype != LFAMD_TYPE_IQ4_XS; // (the canonical image rounds |sc * kvalue| above 2048 to f16; Q2_K / Q3_K: |sc * q| <= 128)
    } else if (n > 8 && Atype == LFAMD_TYPE_Q8_0) {
        p.body = f16_q80 && k % 32 == 0 && lfamd_blaslt_ok()     ? mm_body::q80_lt
                 : f16_q80 && k % 128 == 0 && !lfamd_blaslt_ok() ? mm_body::q80_lf
                                                                 : mm_body::q80_exact;
        p.exact = p.body == mm_body::q80_exact;
    } else if (n <= 8 && im.tuned()) {
        p.body = mm_body::gemv;
        p.relaxed = q80_relaxed(Atype, k, n, flags);
    }
    // the CPU reference's bits: the Q8_0 chains, decode and the q80_exact batches (no float route is held to more than 2e-6 of it)
    p.bit_exact = Atype == LFAMD_TYPE_Q8_0 && ((p.body == mm_body::gemv && !p.relaxed) || p.body == mm_body::q80_exact);

    const size_t n_pad = align_up((size_t)n, 128), act = lfamd_kq_image_of(k, n).parts; // (the staged K-quant image, lfamd_internal.h)
    switch (p.body) {
    case mm_body::sb:
        p.workspace = align_up(lfamd_gemm_sb_workspace(k), 256);
        break;
    case mm_body::i8: // (the staging layout every K-quant batch body shares, then partial tiles of a K-split launch)
    case mm_body::kq_narrow:
    case mm_body::wide:
        p.workspace = act + lfamd_gemm_lw_ksplit_bytes(m, n);
        break;
    case mm_body::q40_wide:
        p.workspace = act;
        break;
    case mm_body::canon: // (+ the canonical image of the matrix, rebuilt from the compact one per call)
        p.workspace = act + align_up(Atype == LFAMD_TYPE_IQ4_XS ? lfamd_wprep8_bytes(m, k) : lfamd_wprep16_bytes(m, k), 256);
        break;
    case mm_body::canon32:
        p.workspace = lfamd_b32_image_of(k, n).bytes;
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
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).exact ? 1 : 0;
}

// Does the call reproduce the CPU reference's bits (tinyBLAS_Q0's f32 chain for Q8_0)?  Read from the plan the launch reads: 0 for
// a Q8_0 decode call that LFAMD_FLAG_Q80_RELAXED moves to the relaxed-order kernel, 1 for the same call where that kernel declines.
int lfamd_mul_mat_is_bit_exact(int Atype, long m, long k, long n, unsigned flags) {
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).bit_exact ? 1 : 0;
}

// Does a call accept the scaled-operand staged image a fused producer wrote (LFAMD_TYPE_STAGED_SCALED)?  The K-quant batches whose
// body reads it: what lfamd_mul_mat would stage with prep_scaled_kernel itself.
int lfamd_mul_mat_takes_staged_scaled(int Atype, long m, long k, long n, unsigned flags) {
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    const mm_plan p = plan_mul_mat(Atype, m, k, n, flags);
    return p.body == mm_body::wide && p.scaled ? 1 : 0;
}

// Does a call accept the staged image a fused producer wrote (LFAMD_TYPE_STAGED_Q8K)?  Exactly the calls that run the int8 body.
int lfamd_mul_mat_takes_staged(int Atype, long m, long k, long n, unsigned flags) {
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).body == mm_body::i8 ? 1 : 0;
}

// Does a call accept the 32-block staged image a fused producer wrote (LFAMD_TYPE_STAGED_B32)?  The batches of the legacy 32-block
// types on the 128 x 128 body: what lfamd_mul_mat would stage with prep80_kernel itself.
int lfamd_mul_mat_takes_staged_b32(int Atype, long m, long k, long n, unsigned flags) {
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    if (lfamd_image_of(Atype, k).cols != k) // (the producers write rows of whole 256-weight groups)
        return 0;
    const mm_body b = plan_mul_mat(Atype, m, k, n, flags).body;
    return b == mm_body::q40_wide || b == mm_body::canon32 ? 1 : 0;
}

// Does a call accept the image of the Q8_0-weight loader-wave body a fused producer wrote (LFAMD_TYPE_STAGED_Q80)?  The Q8_0 batches
// on gemm_lf_q80 (what lfamd_mul_mat would stage with lf_tok_scale_kernel and prep_lf_kernel itself) whose P80 image the loaders can address.
int lfamd_mul_mat_takes_staged_q80(int Atype, long m, long k, long n, unsigned flags) {
    if (!lfamd_type_known(Atype) || m <= 0 || k <= 0 || n <= 0)
        return 0;
    return plan_mul_mat(Atype, m, k, n, flags).body == mm_body::q80_lf && lfamd_gemm_lf_q80_fits(m, k) ? 1 : 0;
}

// The largest workspace of the bodies this call can run: the default one and any a testing flag can force.
size_t lfamd_mul_mat_workspace(int Atype, long m, long k, long n) {
    if (!lfamd_type_known(Atype))
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

static bool aligned16(const void *p) {
    return ((uintptr_t)p & 15) == 0;
}

static bool staged_type(int Btype) { // a staged activation image: no rows, no stride, staging of its own
    return Btype == LFAMD_TYPE_STAGED_Q8K || Btype == LFAMD_TYPE_STAGED_SCALED || Btype == LFAMD_TYPE_STAGED_B32 || Btype == LFAMD_TYPE_STAGED_Q80;
}

static bool workspace_short(size_t need, const void *d_ws, size_t ws_bytes) {
    return need && (ws_bytes < need || !d_ws);
}

// The largest lfamd_mul_mat_workspace of sibling matrices (type of matrix j: Atype[j * type_stride]), whichever route runs them; a
// staged image brings its own staging, so those calls keep the sizes their routes check
static size_t set_workspace(int count, const int *Atype, int type_stride, const long *m, long k, int Btype, long n) {
    size_t need = 0;
    for (int j = 0; j < count && !staged_type(Btype); j++)
        if (m[j] > 0)
            need = std::max(need, lfamd_mul_mat_workspace(Atype[j * type_stride], m[j], k, n));
    return need;
}

// The operand layouts every mat-mul entry point takes (include/lfamd_hip.h, "Operand layout"), checked before the first launch:
// activation rows (not a staged image) at the alignment their readers need, with a stride that keeps it; f32 results; a workspace
// at an allocation's alignment.  quantised: one of the weight types of the call is not a float type (its f32 rows are read as
// float4 by the staging kernels and the decode GEMVs).
static int check_operands(const char *who, bool quantised, int Btype, const void *d_B, size_t b_row_bytes, int count, float *const *d_C,
                          const void *d_ws, size_t ws_bytes) {
    if (!staged_type(Btype)) {
        const size_t a = Btype == LFAMD_TYPE_F32    ? (quantised ? 16 : 4)
                         : Btype == LFAMD_TYPE_Q8_K ? 4
                         : Btype == LFAMD_TYPE_Q8_1 ? 4
                                                    : 2; // (Q8_0, F16, BF16)
        if ((uintptr_t)d_B % a || b_row_bytes % a)
            return fail(LFAMD_ERR_INVALID, "%s: activation rows are not aligned (base and row stride) as include/lfamd_hip.h asks", who);
    }
    for (int j = 0; j < count; j++)
        if ((uintptr_t)d_C[j] % 4)
            return fail(LFAMD_ERR_INVALID, "%s: a result pointer is not 4-byte aligned", who);
    if (d_ws && ws_bytes && (uintptr_t)d_ws % 256)
        return fail(LFAMD_ERR_INVALID, "%s: the workspace is not 256-byte aligned", who);
    return LFAMD_OK;
}

// Everything lfamd_mul_mat checks before its first launch: LFAMD_OK and the plan, or the error the call returns.
static int check_mul_mat(int Atype, long m, long k, int Btype, const void *d_B, size_t b_row_bytes, long n, long ldc, const void *d_ws,
                         size_t ws_bytes, unsigned flags, mm_plan &p) {
    if (!lfamd_type_known(Atype))
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: unsupported weight type%s", "");
    if (m < 0 || n < 0 || k < 0 || ldc < m || k % lfamd_blck_size(lfamd_base_type(Atype)))
        return fail(LFAMD_ERR_INVALID, "mul_mat: bad shape%s", "");
    const bool staged = staged_type(Btype);
    if (!staged) {
        if (float_type(Atype)) {
            if (!(Btype == LFAMD_TYPE_F32 || Btype == Atype))
                return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: float weights need F32 or same-type activations%s", "");
        } else if (Btype != lfamd_vec_dot_type(lfamd_base_type(Atype)) && Btype != LFAMD_TYPE_F32) {
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
    } else if (Btype == LFAMD_TYPE_STAGED_B32) { // a fused producer wrote the 32-block bodies' staged image
        if ((p.body != mm_body::q40_wide && p.body != mm_body::canon32) || lfamd_image_of(Atype, k).cols != k)
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: this call does not run a 32-block batch body (lfamd_mul_mat_takes_staged_b32)%s", "");
        if (!d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_INVALID, "mul_mat: the staged image must be 16-byte aligned%s", "");
        uses_ws = false;
    } else if (Btype == LFAMD_TYPE_STAGED_Q80) { // a fused producer wrote the Q8_0-weight loader-wave body's image
        if (!lfamd_mul_mat_takes_staged_q80(Atype, m, k, n, flags))
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: this call does not run the Q8_0 loader-wave batch body (lfamd_mul_mat_takes_staged_q80)%s", "");
        if (!d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_INVALID, "mul_mat: the staged image must be 16-byte aligned%s", "");
        uses_ws = false;
    }
    if (p.body == mm_body::refused)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat: FORCE_GENERIC needs RAW-layout weights; this type is packed%s", "");
    if (uses_ws && (ws_bytes < need || !d_ws))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat: workspace too small%s", "");
    // the size the header asks for, whichever body runs: a caller that sizes the workspace by anything but lfamd_mul_mat_workspace()
    // learns it on every call, not on the day a flag or a shape picks the body with the largest one
    if (!staged && workspace_short(lfamd_mul_mat_workspace(Atype, m, k, n), d_ws, ws_bytes))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat: workspace smaller than lfamd_mul_mat_workspace()%s", "");
    return LFAMD_OK;
}

// f32 or Q8_K activation rows -> the K-quant image at img (mode: prep mode 2 stages scaled operands; the canonical bodies pass mins16)
static int prep_kq(int Btype, const void *d_B, size_t b_row_bytes, long n, long k, uint8_t *img, int mode, hipStream_t s) {
    const lfamd_kq_image im = lfamd_kq_image_of(k, n);
    if (Btype == LFAMD_TYPE_F32)
        HIPCHK(lfamd_launch_prep_f32(d_B, b_row_bytes, n, (long)im.n_pad, k, img, img + im.d8T, img + im.Xm, mode, nullptr, s), "prep_f32");
    else
        HIPCHK(lfamd_launch_prep_q8k(d_B, b_row_bytes, n, (long)im.n_pad, k, img, img + im.d8T, img + im.Xm, mode, nullptr, s), "prep_q8k");
    return LFAMD_OK;
}

static int launch_mul_mat(const mm_plan &p, int Atype, const void *d_A, long m, long k, int Btype, const void *d_B, size_t b_row_bytes,
                          long n, float *d_C, long ldc, void *d_ws, size_t ws_bytes, unsigned flags, hipStream_t s) {
    // A padded image (LFAMD_TYPE_PAD256): the weights and the staged image have kw columns, the activation rows k.  Only the bodies of
    // the 32-block types see kw != k: the decode GEMV and prep80 take k and pad what they stage, gemm_wide reads whole super-blocks.
    const long kw = lfamd_image_of(Atype, k).cols;
    Atype = lfamd_base_type(Atype);
    const int plain = (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0;
    const int vregs32 = (flags & LFAMD_FLAG_Q0_VREGS32) ? 1 : 0, precise = (flags & LFAMD_FLAG_PRECISE) ? 1 : 0;
    const int vdt = lfamd_vec_dot_type(Atype);
    const lfamd_kq_image im = lfamd_kq_image_of(kw, n);
    const size_t n_pad = im.n_pad;
    uint8_t *ws = (uint8_t *)d_ws; // the staging layout of the K-quant batch bodies: Xh, d8T, Xm
    void *Xh = ws, *d8T = ws + im.d8T, *Xm = ws + im.Xm;
    if (Btype == LFAMD_TYPE_STAGED_Q8K) { // the GEMM alone, no staging launch
        HIPCHK(lfamd_launch_gemm_i8_staged(1, &d_A, &m, k, d_B, n, &d_C, &ldc, s), "gemm_i8 (staged input)");
        return LFAMD_OK;
    }
    if (Btype == LFAMD_TYPE_STAGED_SCALED) {
        const uint8_t *img = (const uint8_t *)d_B;
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, img, img + im.d8T, img + im.Xm, n, (long)n_pad, d_C, ldc, plain | 2, d_ws, ws_bytes, s),
               "gemm_wide (staged input)");
        return LFAMD_OK;
    }
    if (Btype == LFAMD_TYPE_STAGED_B32) { // (q40_wide reads Xh and d8T, canon32 sT too under Q8_1 types)
        const uint8_t *img = (const uint8_t *)d_B;
        const lfamd_b32_image b32 = lfamd_b32_image_of(k, n);
        const void *sT = p.body == mm_body::canon32 && vdt == LFAMD_TYPE_Q8_1 ? img + b32.sT : nullptr;
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, img, img + b32.d8T, sT, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s),
               "gemm_wide (staged input)");
        return LFAMD_OK;
    }
    if (Btype == LFAMD_TYPE_STAGED_Q80) { // the GEMM alone on the image's parts
        HIPCHK(lfamd_launch_gemm_lf_q80_staged(1, &d_A, &m, k, d_B, n, &d_C, &ldc, s), "gemm_lf (Q8_0, staged input)");
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
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, kw, Xh, d8T, nullptr, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    case mm_body::kq_narrow:
    case mm_body::wide: {
        const int mode = p.scaled ? 2 : 0;
        if (const int r = prep_kq(Btype, d_B, b_row_bytes, n, k, ws, mode, s))
            return r;
        if (p.body == mm_body::kq_narrow) {
            HIPCHK(lfamd_launch_gemm_kq(Atype, d_A, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, s), "gemm_kq");
        } else {
            uint8_t *Pp = ws + im.parts; // after Xh, d8T, Xm
            HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, plain | mode, Pp, (size_t)(ws + ws_bytes - Pp), s),
                   "gemm_wide");
        }
        return LFAMD_OK;
    }
    case mm_body::canon32: {
        const lfamd_b32_image b32 = lfamd_b32_image_of(kw, n);
        void *sT = vdt == LFAMD_TYPE_Q8_1 ? ws + b32.sT : nullptr;
        HIPCHK(lfamd_launch_prep80(Btype, d_B, b_row_bytes, n, (long)n_pad, k, Xh, ws + b32.d8T, sT, s), "prep80");
        HIPCHK(lfamd_launch_gemm_wide(Atype, d_A, m, kw, Xh, ws + b32.d8T, sT, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    }
    case mm_body::canon: {
        if (const int r = prep_kq(Btype, d_B, b_row_bytes, n, k, ws, Atype == LFAMD_TYPE_Q2_K, s)) // (mins16)
            return r;
        // the resident image is the compact one; the MFMA body reads the canonical form, rebuilt here per call
        void *img = ws + im.parts;
        if (Atype == LFAMD_TYPE_IQ4_XS)
            HIPCHK(lfamd_launch_pk4x_expand(d_A, m, k, img, s), "pk4x_expand");
        else
            HIPCHK(lfamd_launch_pk_expand(Atype, d_A, m, k, img, s), "pk_expand");
        HIPCHK(lfamd_launch_gemm_wide(Atype, img, m, k, Xh, d8T, Xm, n, (long)n_pad, d_C, ldc, plain, nullptr, 0, s), "gemm_wide");
        return LFAMD_OK;
    }
    case mm_body::float_lt: // the vendor's GEMM on plain 16-bit float weights
        if (aligned16(d_A) && aligned16(d_B) && !(b_row_bytes & 15)) { // (rows_to_16 reads f32 rows as float4)
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
        HIPCHK(lfamd_launch_gemv(Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, vregs32, precise, p.relaxed ? 1 : 0, s), "gemv");
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
    int r = check_mul_mat(Atype, m, k, Btype, d_B, b_row_bytes, n, ldc, d_ws, ws_bytes, flags, p);
    if (r != LFAMD_OK || m == 0 || n == 0)
        return r;
    if ((r = check_operands("mul_mat", !float_type(Atype), Btype, d_B, b_row_bytes, 1, &d_C, d_ws, ws_bytes)) != LFAMD_OK)
        return r;
    return launch_mul_mat(p, Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Sibling matrices on the same activations: lfamd_mul_mat_multi (one weight type) and lfamd_mul_mat_multi_types (a type per matrix).
// plan_group / plan_types decide the route of a call and the workspace it needs before anything is launched; check_group checks
// every matrix against that route, and one switch launches it.  DESIGN.md section 14 lists the routes in this order.
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
    staged_q80_lf, // LFAMD_TYPE_STAGED_Q80: gemm_lf_q80 over the concatenated row blocks, no staging
    gemv_dual,    // (multi_types) decode, a {Q4_K | Q5_K} group and a Q6_K group: one launch of the dual GEMV
    wide_dual,    // (multi_types) K-quants of mixed types on one scaled staging: both groups in one loader-wave launch
    wide_runs,    // (multi_types) K-quants of mixed types on one scaled staging: one wide launch per run of equal types
    runs,         // (multi_types) a lfamd_mul_mat_multi route per run of equal types (every run checked first)
};

// 128-row blocks of a group of matrices, or -1 when one of them has a negative height or a short ldc
static long group_row_blocks(int count, const long *m, const long *ldc) {
    long rbs = 0;
    for (int j = 0; j < count; j++) {
        if (m[j] < 0 || ldc[j] < m[j])
            return -1;
        rbs += (m[j] + 127) / 128;
    }
    return rbs;
}

// sibling matrices of one type on one launch of the int8 body: their row blocks together must make a grid it takes
static bool multi_i8_ok(int Atype, int count, const long *m, const long *ldc, long k, long n, unsigned flags) {
    const long rbs = group_row_blocks(count, m, ldc);
    return rbs > 0 && i8_takes(Atype, k, n, flags, rbs);
}

// 2 .. 4 K-quant siblings whose concatenated row blocks fill the chip with 128 x 128 tiles (or LFAMD_FLAG_GEMM_WIDE asks for it)
static bool wide_group_ok(int Atype, int count, const long *m, const long *ldc, long k, long n, unsigned flags) {
    if (count < 2 || count > 4 || n <= 8 || !kquant(Atype) || k <= 0 || k % 256 || (flags & (LFAMD_FLAG_FORCE_GENERIC | LFAMD_FLAG_GEMM_NARROW)))
        return false;
    const long rbs = group_row_blocks(count, m, ldc);
    return rbs >= 0 && (rbs * (long)(align_up((size_t)n, 128) / 128) >= 192 || (flags & LFAMD_FLAG_GEMM_WIDE));
}

static bool scaled_ok(int Atype, unsigned flags) { // may the wide body run on scaled operands?
    return !(flags & LFAMD_FLAG_PRECISE) && lfamd_gemm_wide_scaled_ok(Atype, (flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0);
}

// One side of a two-type launch: a {Q4_K | Q5_K} group (one of the two types) or a Q6_K group, at most four matrices.
struct mm_side {
    int type, count;
    long m[4], ldc[4];
    const void *A[4];
    float *C[4];
};
struct mm_group_plan {
    mm_route route;
    bool i8_group;    // 2 .. 4 matrices whose row blocks together make a grid the int8 body takes
    size_t workspace; // bytes the route stages into (0: it takes none)
    mm_side a, b;     // (plan_types) gemv_dual / wide_dual: the two groups
    bool relaxed;     // gemv_multi on Q8_0: the relaxed-order kernel (q80_relaxed), decided here and read by the launch
};

// The route of sibling matrices of one type (a lfamd_mul_mat_multi call, or one run of a lfamd_mul_mat_multi_types call).
static mm_group_plan plan_group(int Atype, int count, const long *m, long k, int Btype, size_t b_row_bytes, long n, const long *ldc,
                                unsigned flags) {
    const lfamd_image im = lfamd_image_of(Atype, k); // a padded image: the base type's route at kw weight columns, activation rows of k
    const long kw = im.cols;
    Atype = im.type;
    mm_group_plan g = {mm_route::each, count > 1 && count <= 4 && multi_i8_ok(Atype, count, m, ldc, k, n, flags), 0, {}, {}, false};
    if (count <= 0 || (staged_type(Btype) && n == 0))
        g.route = mm_route::none;
    else if (Btype == LFAMD_TYPE_STAGED_B32) // one GEMM per matrix on the one image (check_group: every matrix must take it)
        g.route = mm_route::each;
    else if (Btype == LFAMD_TYPE_STAGED_Q80) { // the route the same call takes on f32 rows, minus the staging (check_group: every matrix must take it)
        if (count > 1 && count <= 4 && Atype == LFAMD_TYPE_Q8_0 && k > 0 && plan_mul_mat(Atype, m[0], k, n, flags).body == mm_body::q80_lf &&
            group_row_blocks(count, m, ldc) >= 0)
            g.route = mm_route::staged_q80_lf;
    } else if (Btype == LFAMD_TYPE_STAGED_Q8K) // (check_group: every matrix must take the image, unless the group takes it together)
        g.route = mm_route::staged_i8;
    else if (Btype == LFAMD_TYPE_STAGED_SCALED) { // the route the same call takes on f32 rows
        if (wide_group_ok(Atype, count, m, ldc, k, n, flags) && scaled_ok(Atype, flags))
            g.route = mm_route::staged_wide;
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
        const bool gemv = count <= 4 && n <= 8 && !(flags & LFAMD_FLAG_FORCE_GENERIC) && im.tuned() && rows_ok && k > 0 &&
                          k % lfamd_blck_size(Atype) == 0 && (Atype == LFAMD_TYPE_Q8_0 || kw % 256 == 0) && group_row_blocks(count, m, ldc) >= 0;
        const bool q80_lf = count > 1 && count <= 4 && Atype == LFAMD_TYPE_Q8_0 && k > 0 && rows_ok &&
                            plan_mul_mat(Atype, m[0], k, n, flags).body == mm_body::q80_lf && group_row_blocks(count, m, ldc) >= 0;
        if (all_sb)
            g.route = mm_route::sb_shared, g.workspace = align_up(lfamd_gemm_sb_workspace(k), 256);
        else if (gemv)
            g.route = n == 0 ? mm_route::none : mm_route::gemv_multi, g.relaxed = q80_relaxed(Atype, k, n, flags);
        // Q4_K siblings whose tiles TOGETHER make a grid the int8 body takes (attn_q/k/v of an all-Q4_K layer: 48 row blocks at 512
        // tokens): one staging, one launch over the concatenated row blocks, exact integer dots (6144 x 4096 x 512: 47.5 us against 56.8)
        else if (rows_ok && g.i8_group)
            g.route = mm_route::i8_multi, g.workspace = lfamd_i8_image_of(k, n).bytes;
        // K-quant batches: ONE activation prep for all the matrices, and one launch of the 128 x 128 body over their concatenated
        // row blocks when that grid fills the chip (attn_q/k/v: 48 + 8 + 8 row blocks instead of three launches of which two fill a
        // quarter of the CUs)
        else if (rows_ok && wide_group_ok(Atype, count, m, ldc, k, n, flags))
            g.route = mm_route::wide_multi, g.workspace = lfamd_kq_image_of(k, n).parts;
        // Q8_0 batches on sibling matrices: one staging of the activations, one launch over the concatenated row blocks
        else if (q80_lf)
            g.route = mm_route::q80_lf_multi, g.workspace = lfamd_gemm_lf_workspace(k, n);
    }
    return g;
}

// Everything a group's route needs before its first launch: LFAMD_OK, or the error the call returns.
static int check_group(const mm_group_plan &g, int Atype, int count, const long *m, long k, int Btype, const void *d_B, size_t b_row_bytes,
                       long n, const long *ldc, const void *d_ws, size_t ws_bytes, unsigned flags) {
    if (g.route == mm_route::none)
        return LFAMD_OK;
    if (Btype == LFAMD_TYPE_STAGED_Q8K && !g.i8_group) // every matrix must take the image (each one by itself)
        for (int j = 0; j < count; j++)
            if (m[j] > 0 && (ldc[j] < m[j] || !lfamd_mul_mat_takes_staged(Atype, m[j], k, n, flags)))
                return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: a matrix of this call does not run the int8 batch body%s", "");
    if (Btype == LFAMD_TYPE_STAGED_SCALED && (!d_B || !aligned16(d_B)))
        return fail(LFAMD_ERR_INVALID, "mul_mat_multi: the staged image must be 16-byte aligned%s", "");
    if (g.route == mm_route::staged_q80_lf) {
        for (int j = 0; j < count; j++)
            if (m[j] > 0 && !lfamd_mul_mat_takes_staged_q80(Atype, m[j], k, n, flags))
                return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: a matrix of this call does not run the Q8_0 loader-wave batch body%s", "");
        if (!d_B || !aligned16(d_B))
            return fail(LFAMD_ERR_INVALID, "mul_mat_multi: the staged image must be 16-byte aligned%s", "");
    }
    if (Btype == LFAMD_TYPE_STAGED_SCALED && g.i8_group)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: these matrices run the int8 batch body together (LFAMD_TYPE_STAGED_Q8K)%s", "");
    if (g.workspace && (ws_bytes < g.workspace || !d_ws))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat_multi: workspace too small%s", "");
    if (g.route == mm_route::each) // one call per matrix: each must pass lfamd_mul_mat's checks before the first is launched
        for (int j = 0; j < count; j++) {
            mm_plan p = {};
            if (const int r = check_mul_mat(Atype, m[j], k, Btype, d_B, b_row_bytes, n, ldc[j], d_ws, ws_bytes, flags, p))
                return r;
        }
    return LFAMD_OK;
}

static int launch_group(const mm_group_plan &g, int Atype, int count, const void *const *d_A, const long *m, long k, int Btype,
                        const void *d_B, size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws, size_t ws_bytes,
                        unsigned flags, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const lfamd_kq_image im = lfamd_kq_image_of(k, n);
    switch (g.route) {
    case mm_route::each:
        for (int j = 0; j < count; j++)
            if (const int r = lfamd_mul_mat(Atype, d_A[j], m[j], k, Btype, d_B, b_row_bytes, n, d_C[j], ldc[j], d_ws, ws_bytes, flags, stream))
                return r;
        return LFAMD_OK;
    case mm_route::staged_i8:
        for (int j0 = 0; j0 < count; j0 += 4) {
            const int c = count - j0 < 4 ? count - j0 : 4;
            HIPCHK(lfamd_launch_gemm_i8_staged(c, d_A + j0, m + j0, k, d_B, n, d_C + j0, ldc + j0, s), "gemm_i8 (staged input, multi)");
        }
        return LFAMD_OK;
    case mm_route::sb_shared:
        for (int j = 0; j < count; j++)
            HIPCHK(lfamd_launch_gemm_sb(Atype, d_A[j], m[j], k, Btype, d_B, b_row_bytes, n, d_C[j], ldc[j], d_ws, j > 0, s), "gemm_sb (multi)");
        return LFAMD_OK;
    case mm_route::gemv_multi:
        HIPCHK(lfamd_launch_gemv_multi(lfamd_base_type(Atype), count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, (flags & LFAMD_FLAG_Q0_VREGS32) ? 1 : 0,
                                       (flags & LFAMD_FLAG_PRECISE) ? 1 : 0, g.relaxed ? 1 : 0, s),
               "gemv_multi");
        return LFAMD_OK;
    case mm_route::i8_multi:
        HIPCHK(lfamd_launch_gemm_i8(count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, nullptr, s), "gemm_i8 (multi)");
        return LFAMD_OK;
    case mm_route::wide_multi:
        if (const int r = prep_kq(Btype, d_B, b_row_bytes, n, k, (uint8_t *)d_ws, scaled_ok(Atype, flags) ? 2 : 0, s))
            return r;
        [[fallthrough]];
    case mm_route::staged_wide: { // (staged_wide: the plan asked scaled_ok)
        const bool staged = g.route == mm_route::staged_wide;
        const uint8_t *img = (const uint8_t *)(staged ? d_B : d_ws);
        HIPCHK(lfamd_launch_gemm_wide_multi(Atype, count, d_A, m, k, img, img + im.d8T, img + im.Xm, n, (long)im.n_pad, d_C, ldc,
                                            ((flags & LFAMD_FLAG_GEMM_PLAIN) ? 1 : 0) | (scaled_ok(Atype, flags) ? 2 : 0), nullptr, 0, s),
               staged ? "gemm_wide_multi (staged input)" : "gemm_wide_multi");
        return LFAMD_OK;
    }
    case mm_route::q80_lf_multi:
        HIPCHK(lfamd_launch_gemm_lf_q80(count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, s), "gemm_lf (Q8_0, multi)");
        return LFAMD_OK;
    case mm_route::staged_q80_lf:
        HIPCHK(lfamd_launch_gemm_lf_q80_staged(count, d_A, m, k, d_B, n, d_C, ldc, s), "gemm_lf (Q8_0, staged input, multi)");
        return LFAMD_OK;
    default: // (none)
        return LFAMD_OK;
    }
}

int lfamd_mul_mat_multi(int Atype, int count, const void *const *d_A, const long *m, long k, int Btype, const void *d_B,
                        size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws, size_t ws_bytes,
                        unsigned flags, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    if (count > 0 && !lfamd_type_known(Atype)) // (plan_group strips the layout modifier: an unknown id must not be planned as its base type)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi: unsupported weight type%s", "");
    const mm_group_plan g = plan_group(Atype, count, m, k, Btype, b_row_bytes, n, ldc, flags);
    int r = check_group(g, Atype, count, m, k, Btype, d_B, b_row_bytes, n, ldc, d_ws, ws_bytes, flags);
    if (r == LFAMD_OK && g.route != mm_route::none && n > 0) {
        if (workspace_short(set_workspace(count, &Atype, 0, m, k, Btype, n), d_ws, ws_bytes))
            return fail(LFAMD_ERR_WORKSPACE, "mul_mat_multi: workspace smaller than the largest lfamd_mul_mat_workspace() of the set%s", "");
        r = check_operands("mul_mat_multi", !float_type(Atype), Btype, d_B, b_row_bytes, count, d_C, d_ws, ws_bytes);
    }
    return r != LFAMD_OK ? r : launch_group(g, Atype, count, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags, stream);
}

// The matrices of a call as the two sides of a two-type launch; false when they do not split so.
static bool split_pair(int count, const int *Atype, const void *const *d_A, const long *m, float *const *d_C, const long *ldc, mm_side &a,
                       mm_side &b) {
    a.type = -1, b.type = LFAMD_TYPE_Q6_K, a.count = b.count = 0;
    for (int j = 0; j < count; j++) {
        const int t = Atype[j];
        if (t != LFAMD_TYPE_Q6_K && ((t != LFAMD_TYPE_Q4_K && t != LFAMD_TYPE_Q5_K) || (a.count && a.type != t)))
            return false;
        mm_side &g = t == LFAMD_TYPE_Q6_K ? b : a;
        if (g.count == 4)
            return false;
        g.type = t, g.A[g.count] = d_A[j], g.m[g.count] = m[j], g.ldc[g.count] = ldc[j], g.C[g.count] = d_C[j], g.count++;
    }
    return a.count > 0 && b.count > 0;
}

// Runs of up to four consecutive matrices of one type: fn(j0, j1) for each, until one answers other than LFAMD_OK.
extern "C++" {
template <class F> static int each_run(int count, const int *Atype, F fn) {
    for (int j0 = 0, j1; j0 < count; j0 = j1) {
        for (j1 = j0 + 1; j1 < count && Atype[j1] == Atype[j0] && j1 - j0 < 4;)
            j1++;
        const int r = fn(j0, j1);
        if (r != LFAMD_OK)
            return r;
    }
    return LFAMD_OK;
}
}

// The route of a lfamd_mul_mat_multi_types call: gemv_dual, wide_dual, wide_runs or runs (a backend's graph_compute sees attn_q/k/v
// as three MUL_MAT nodes with one src1; in a Q4_K_M file q and k are Q4_K, v is Q6_K).
static mm_group_plan plan_types(int count, const int *Atype, const void *const *d_A, const long *m, long k, int Btype, const void *d_B,
                                size_t b_row_bytes, long n, float *const *d_C, const long *ldc, const void *d_ws, size_t ws_bytes,
                                unsigned flags) {
    mm_group_plan p = {mm_route::runs, false, 0, {}, {}, false};
    const bool paired = split_pair(count, Atype, d_A, m, d_C, ldc, p.a, p.b);
    const bool rows_ok = (Btype == LFAMD_TYPE_F32 || Btype == LFAMD_TYPE_Q8_K) && b_row_bytes >= lfamd_row_size(Btype, k);
    // decode (n = 1) with exactly two K-quant types {Q4_K | Q5_K, Q6_K}: ONE launch (gemv_kq_dual_kernel)
    bool dual = paired && n == 1 && k > 0 && k % 256 == 0 && !(flags & LFAMD_FLAG_FORCE_GENERIC) && rows_ok;
    for (int j = 0; j < count && dual; j++)
        dual = m[j] > 0 && ldc[j] >= m[j];
    if (dual) // (n = 1: none of the routes below applies)
        p.route = mm_route::gemv_dual;
    // K-quant batches of mixed types (attn_q/k = Q4_K with attn_v = Q6_K at prefill): the scaled-operand GEMM of every type reads the
    // SAME staged activations, prepared once (or written by a fused producer: d_B); a workspace too small for them leaves `runs`
    const bool staged_in = Btype == LFAMD_TYPE_STAGED_SCALED;
    bool share = n > 8 && count > 1 && k > 0 && k % 256 == 0 &&
                 !(flags & (LFAMD_FLAG_PRECISE | LFAMD_FLAG_FORCE_GENERIC | LFAMD_FLAG_GEMM_NARROW)) && (staged_in ? d_B && aligned16(d_B) : rows_ok);
    bool mixed = false;
    for (int j = 0; j < count && share; j++) {
        share = kquant(Atype[j]) && scaled_ok(Atype[j], flags) && m[j] >= 0 && ldc[j] >= m[j];
        mixed = mixed || Atype[j] != Atype[0];
    }
    const lfamd_kq_image im = lfamd_kq_image_of(k, n);
    if (share && mixed && (staged_in || (d_ws && ws_bytes >= im.parts))) {
        const long rb_a = group_row_blocks(p.a.count, p.a.m, p.a.ldc), rb_b = group_row_blocks(p.b.count, p.b.m, p.b.ldc);
        p.route = paired && lfamd_gemm_wide_dual_ok(rb_a, rb_b, (long)im.n_pad) ? mm_route::wide_dual : mm_route::wide_runs;
        p.workspace = staged_in ? 0 : im.parts;
    }
    return p;
}

int lfamd_mul_mat_multi_types(int count, const int *Atype, const void *const *d_A, const long *m, long k, int Btype,
                              const void *d_B, size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws,
                              size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError();
    if (count <= 0)
        return LFAMD_OK;
    if (!Atype || !d_A || !m || !d_C || !ldc)
        return fail(LFAMD_ERR_INVALID, "mul_mat_multi_types: null argument%s", "");
    for (int j = 0; j < count; j++)
        if (!lfamd_type_known(Atype[j]))
            return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi_types: unsupported weight type%s", "");
    if (Btype == LFAMD_TYPE_STAGED_B32 || Btype == LFAMD_TYPE_STAGED_Q80)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_multi_types: the 32-block staged images are taken by lfamd_mul_mat / lfamd_mul_mat_multi%s", "");
    const mm_group_plan p = plan_types(count, Atype, d_A, m, k, Btype, d_B, b_row_bytes, n, d_C, ldc, d_ws, ws_bytes, flags);
    auto run_plan = [&](int j0, int j1) { return plan_group(Atype[j0], j1 - j0, m + j0, k, Btype, b_row_bytes, n, ldc + j0, flags); };
    if (p.route == mm_route::runs) { // every run is checked before the first one is launched
        const int r = each_run(count, Atype, [&](int j0, int j1) {
            return check_group(run_plan(j0, j1), Atype[j0], j1 - j0, m + j0, k, Btype, d_B, b_row_bytes, n, ldc + j0, d_ws, ws_bytes, flags);
        });
        if (r != LFAMD_OK)
            return r;
    }
    if (n > 0) {
        bool quantised = false;
        for (int j = 0; j < count; j++)
            quantised = quantised || !float_type(Atype[j]);
        if (workspace_short(set_workspace(count, Atype, 1, m, k, Btype, n), d_ws, ws_bytes))
            return fail(LFAMD_ERR_WORKSPACE, "mul_mat_multi_types: workspace smaller than the largest lfamd_mul_mat_workspace() of the set%s", "");
        if (const int r = check_operands("mul_mat_multi_types", quantised, Btype, d_B, b_row_bytes, count, d_C, d_ws, ws_bytes))
            return r;
    }
    hipStream_t s = (hipStream_t)stream;
    const lfamd_kq_image im = lfamd_kq_image_of(k, n);
    uint8_t *img = p.workspace ? (uint8_t *)d_ws : (uint8_t *)const_cast<void *>(d_B); // (a staged image has the workspace's layout)
    switch (p.route) {
    case mm_route::gemv_dual:
        HIPCHK(lfamd_launch_gemv_dual(p.a.type, p.a.count, p.a.A, p.a.m, p.a.C, p.a.ldc, p.b.type, p.b.count, p.b.A, p.b.m, p.b.C, p.b.ldc, k,
                                      Btype, d_B, b_row_bytes, s),
               "gemv_dual");
        return LFAMD_OK;
    case mm_route::wide_dual:
    case mm_route::wide_runs: // (the plan took scaled operands for every type, so `plain` is 0: mode 2)
        if (const int r = p.workspace ? prep_kq(Btype, d_B, b_row_bytes, n, k, img, 2, s) : LFAMD_OK)
            return r;
        if (p.route == mm_route::wide_dual) {
            HIPCHK(lfamd_launch_gemm_wide_dual(p.a.type, p.a.count, p.a.A, p.a.m, p.a.C, p.a.ldc, p.b.type, p.b.count, p.b.A, p.b.m, p.b.C,
                                               p.b.ldc, k, img, img + im.d8T, img + im.Xm, n, (long)im.n_pad, 2, s),
                   "gemm_wide_dual");
            return LFAMD_OK;
        }
        return each_run(count, Atype, [&](int j0, int j1) -> int {
            HIPCHK(lfamd_launch_gemm_wide_multi(Atype[j0], j1 - j0, d_A + j0, m + j0, k, img, img + im.d8T, img + im.Xm, n, (long)im.n_pad,
                                                d_C + j0, ldc + j0, 2, nullptr, 0, s),
                   "gemm_wide_multi");
            return LFAMD_OK;
        });
    default: // (runs)
        return each_run(count, Atype, [&](int j0, int j1) {
            return launch_group(run_plan(j0, j1), Atype[j0], j1 - j0, d_A + j0, m + j0, k, Btype, d_B, b_row_bytes, n, d_C + j0, ldc + j0,
                                d_ws, ws_bytes, flags, stream);
        });
    }
}

size_t lfamd_mul_mat_id_workspace(int type, long rows, long cols, int experts, long tokens, int thinkers) {
    return lfamd_moe_workspace(type, rows, cols, experts, tokens, thinkers);
}

// f32 activations (the GGML_OP_MUL_MAT_ID boundary) are served by the decode path, which quantises in-kernel, and past 4 tokens by the
// routed launch within its limits
int lfamd_mul_mat_id_takes_f32(int type, long cols, int experts, long tokens, int thinkers, unsigned flags) {
    const bool kq = type == LFAMD_TYPE_Q4_K || type == LFAMD_TYPE_Q5_K || type == LFAMD_TYPE_Q6_K;
    return kq && !(flags & LFAMD_FLAG_FORCE_GENERIC) && (tokens <= 4 || (cols % 256 == 0 && experts < 255 && tokens * thinkers <= 60 * 1024));
}

int lfamd_mul_mat_id(int type, const void *d_W, long rows, long cols, int experts, int Btype, const void *d_thought,
                     size_t b_row_bytes, int tasks, long tokens, const int32_t *d_plan, int thinkers, float *d_result,
                     void *d_ws, size_t ws_bytes, unsigned flags, void *stream) {
    (void)hipGetLastError(); // a stale error of an earlier call (e.g. an invalidated stream capture) must not fail this one
    if (!lfamd_type_known(type))
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_id: unsupported weight type%s", "");
    if (rows < 0 || cols < 0 || cols % lfamd_blck_size(lfamd_base_type(type)) || experts <= 0 || tasks <= 0 || thinkers <= 0 ||
        tasks > thinkers || thinkers > experts)
        return fail(LFAMD_ERR_INVALID, "mul_mat_id: bad shape%s", "");
    const bool f32_decode = Btype == LFAMD_TYPE_F32 && lfamd_mul_mat_id_takes_f32(type, cols, experts, tokens, thinkers, flags);
    if (Btype != lfamd_vec_dot_type(lfamd_base_type(type)) && !f32_decode)
        return fail(LFAMD_ERR_UNSUPPORTED,
                    "mul_mat_id: activations must be in the weight type's vec_dot format (F32 only for Q4_K / Q5_K / Q6_K experts)%s", "");
    if (tokens == 0 || rows == 0)
        return LFAMD_OK;
    size_t need = lfamd_moe_workspace(type, rows, cols, experts, tokens, thinkers);
    if (need && (ws_bytes < need || !d_ws))
        return fail(LFAMD_ERR_WORKSPACE, "mul_mat_id: workspace too small%s", "");
    if (b_row_bytes < lfamd_row_size(Btype, cols) || !d_plan || (uintptr_t)d_plan % 4)
        return fail(LFAMD_ERR_INVALID, "mul_mat_id: activation row stride too small, or the routing table is NULL or not 4-byte aligned%s", "");
    if (const int r = check_operands("mul_mat_id", true, Btype, d_thought, b_row_bytes, 1, &d_result, d_ws, ws_bytes))
        return r;
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
    if (Btype == LFAMD_TYPE_STAGED_B32 || Btype == LFAMD_TYPE_STAGED_Q80)
        return fail(LFAMD_ERR_UNSUPPORTED, "mul_mat_id_multi: no staged image is taken here%s", "");
    if (tasks <= 0 || tasks > thinkers || !lfamd_type_known(Btype))
        return fail(LFAMD_ERR_INVALID, "mul_mat_id_multi: bad shape or activation type%s", "");
    if ((uintptr_t)d_plan % 4)
        return fail(LFAMD_ERR_INVALID, "mul_mat_id_multi: the routing table is not 4-byte aligned%s", "");
    if (tokens > 0 && rows > 0)
        if (const int r = check_operands("mul_mat_id_multi", true, Btype, d_thought, b_row_bytes, count, d_result, d_ws, ws_bytes))
            return r;
    if (count <= 4 && lfamd_type_known(type) && rows > 0 && cols > 0 && experts > 0 && thinkers > 0 && thinkers <= experts && tokens > 0 &&
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
