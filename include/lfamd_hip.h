/*
 * lfamd_hip.h — C ABI of the MI355X (gfx950) quantized-matmul module, libllamafile_amd_hip.so.
 *
 * This is the thin device-side boundary the host plug-in (include/llamafile_sgemm.h) dlopen()s,
 * the way the reference's llamafile/cuda.c:701-753 dlopen()s ggml-rocm.so and imports a fixed
 * symbol list.  The reference's module exposes a whole ggml backend (12 symbols, cuda.c:726-737);
 * this tier only accelerates GGML_OP_MUL_MAT / MUL_MAT_ID, so the ABI is the small set below:
 * plain pointers and sizes, no C++/torch types.  Every function returns 0 on success or a
 * negative lfamd_status; lfamd_last_error() gives a message.  Nothing here falls back to the CPU.
 *
 * Reference counterparts (paths relative to /root/reference):
 *   lfamd_pack_weights   <- ggml_backend_cuda_buffer_set_tensor (weights upload; the backend owns
 *                           the device copy and may re-lay it out), ggml-cuda.cu.patch:16971-16977
 *   lfamd_mul_mat        <- ggml_cuda_mul_mat policy + ggml_cuda_op_mul_mat_vec_q / _mul_mat_q,
 *                           ggml-cuda.cu.patch:18377-18443, 14714-14806, 14188-14284;
 *                           numerics follow the CPU path llamafile_sgemm, tinyblas_cpu_sgemm.inc:274-331
 *   lfamd_mul_mat_id     <- ggml_cuda_mul_mat_id, ggml-cuda.cu.patch:18499-18635; numerics follow
 *                           iqk_mul_mat_moe (iqk_mul_mat.inc:204-221) / llamafile_mixmul
 *   lfamd_quantize_rows  <- quantize_q8_1 (ggml-cuda.cu.patch:15259-15293); formats follow the CPU
 *                           vec_dot types Q8_0 / Q8_1 / Q8_K
 */
#ifndef LFAMD_HIP_H_
#define LFAMD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "lfamd_blocks.h" /* the LFAMD_TYPE_* ids */

#ifdef __cplusplus
extern "C" {
#endif

#define LFAMD_ABI_VERSION 1

enum lfamd_status {
    LFAMD_OK = 0,
    LFAMD_ERR_UNSUPPORTED = -1, /* type / shape this module has no kernel for (caller decides) */
    LFAMD_ERR_INVALID = -2,     /* precondition violated (the reference asserts) */
    LFAMD_ERR_HIP = -3,         /* HIP runtime error; see lfamd_last_error() */
    LFAMD_ERR_WORKSPACE = -4,   /* workspace too small */
};

/* numerics flags for lfamd_mul_mat */
#define LFAMD_FLAG_Q0_VREGS32 1u /* restate the reference's 32-vector-register (AVX512) build of
                                    tinyBLAS_Q0: Kahan on 2x1/1x2/1x1 edge tiles (tinyblas_cpu.h:797-830) */
#define LFAMD_FLAG_PRECISE 2u    /* FLAG_precise (--precise): Kahan everywhere in the Q0 kernels */
#define LFAMD_FLAG_FORCE_GENERIC 4u /* debugging: the generic one-wave-per-row kernel — only for tensors kept as GGUF rows
                                       (floats, legacy 32-block rows that are not whole 256-weight groups: RAW rows, unless the
                                       caller asked for the padded image, LFAMD_TYPE_PAD256); packed types answer
                                       LFAMD_ERR_UNSUPPORTED */
#define LFAMD_FLAG_GEMM_NARROW 8u   /* testing: force the 128x64 split-K MFMA body (default: chosen by grid size) */
#define LFAMD_FLAG_GEMM_WIDE 16u    /* testing: force the 128x128 MFMA body */
#define LFAMD_FLAG_GEMM_PLAIN 32u   /* testing: the 128x128 body without loader waves (Q4_K / Q5_K default to them) */
#define LFAMD_FLAG_Q80_EXACT 64u    /* Q8_0 batches (n > 8): the BIT-EXACT restatement of tinyBLAS_Q0's 8-lane chains (VALU, ~12x
                                       slower) instead of the default: this module's f16 MFMA body on the resident image, f16(d * q) x
                                       f16(d8 * code), <= 1e-3 (csrc/gemm_lf.hip; rows that are not whole 128-weight groups run the exact
                                       kernel anyway).  n <= 8 — the Q8_0 vecdot of the north star — is bit-exact unless the caller
                                       asks for LFAMD_FLAG_Q80_RELAXED; LFAMD_FLAG_PRECISE implies this flag. */
#define LFAMD_FLAG_Q80_RELAXED 128u /* Q8_0 weights, n <= 8 (decode): the GEMV that splits K over the waves of a work-group
                                       (csrc/gemv_q80r_impl.h).  The same integer block dots, added in f32 in this module's own fixed
                                       order instead of tinyBLAS_Q0's chain: deterministic, within 2e-6 of the CPU reference, NOT its
                                       bits (lfamd_mul_mat_is_bit_exact answers 0; lfamd_mul_mat_is_exact still 1).  The order depends
                                       on k alone — not on m, n, the column's position, the sibling count or the activation format.
                                       Ignored for every other type and for n > 8; LFAMD_FLAG_PRECISE, LFAMD_FLAG_Q80_EXACT and
                                       LFAMD_FLAG_FORCE_GENERIC override it (their routes are unchanged), LFAMD_FLAG_Q0_VREGS32 has no
                                       effect under it; rows too deep for the kernel's LDS run the bit-exact kernel.  lfamd_mul_mat
                                       and lfamd_mul_mat_multi serve it (siblings stay one launch); lfamd_mul_mat_multi_types and the
                                       MUL_MAT_ID calls pass `flags` on, so their per-matrix / per-expert calls of n <= 8 inherit it.
                                       No workspace, no staged image; workspace sizes and refusals are those of the call without it. */

int lfamd_abi_version(void);
const char *lfamd_last_error(void);

/* Device management. */
int lfamd_device_count(void);
int lfamd_init(int device); /* hipSetDevice + arch check (gfx950 required) */
int lfamd_device_name(int device, char *buf, size_t len);

/* Device memory (thin wrappers so a C host needs no HIP headers). */
int lfamd_malloc(void **dptr, size_t bytes);
int lfamd_free(void *dptr);
int lfamd_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int lfamd_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int lfamd_memset(void *dst, int value, size_t bytes, void *stream);
/* Pinned host memory mapped into the device's address space (the same pointer is valid on both sides): a decode-sized
 * lfamd_mul_mat may take its activation row from it and write its result to it directly (no float atomics on it: n = 1 or
 * n = 2 only, see lfamd_mul_mat).  What llamafile_sgemm's host-pointer path uses for single-column calls. */
int lfamd_host_alloc(void **p, size_t bytes);
int lfamd_host_free(void *p);
int lfamd_stream_sync(void *stream);

/* ---- weights ----------------------------------------------------------------------------
 * Weights are kept on the device in a PACKED layout chosen per type so that every kernel reads
 * them with coalesced 16-byte-per-lane loads (DESIGN.md "Data layout in HBM").  `raw` is the
 * tensor exactly as GGUF/ggml stores it: `rows` rows, `raw_row_bytes` apart, each a sequence of
 * blocks (include/lfamd_blocks.h).  Packing is a device kernel: raw and packed are device
 * pointers.  lfamd_packed_size is the ONLY source of the packed byte count: Q4_K / Q5_K / Q6_K / Q4_0 / IQ4_NL images are
 * the GGUF size (+ tile round-up; IQ4_NL is Q4_0's block shape and takes Q4_0's image byte for byte, its nibbles being codebook
 * indices); Q2_K / Q3_K / IQ4_XS are compact images of 84 / 116 / 144 bytes per 256 weights (1.00x /
 * 1.055x / 1.06x the file: DESIGN.md section 10.10; batches expand them per call into the canonical image in the workspace); Q8_0 is
 * ONE image of the file's size (1.0625 bytes per weight) that the bit-exact vecdot, the exact batch kernel and the f16 MFMA batch
 * body all read — only a process that opted into the vendor GEMM (LFAMD_USE_BLASLT=1) keeps f16(d * q) rows behind it (3.1 bytes
 * per weight in all); Q4_1 / Q5_0 / Q5_1 are kept as the canonical image their MFMA and decode kernels read (192 bytes per 256
 * weights: 1.2 - 1.5x the file); legacy 32-block rows that are not whole
 * 256-weight groups and float tensors stay as GGUF rows. */
size_t lfamd_packed_size(int type, long rows, long cols);
/* 1 when the process opted into the vendor's GEMM (LFAMD_USE_BLASLT=1 in the environment before the first call, and hipBLASLt
 * loads): batches on PLAIN 16-bit float matrices — F16 / BF16 weight tensors and a second, f16(d * q) image of Q8_0 weights — then
 * go through it (a shape or device it declines falls back to this module's kernels).  0 (the default): every batch runs on this
 * module's own MFMA bodies and nothing depends on the library.  Constant for the life of the process. */
int lfamd_vendor_gemm_available(void);
int lfamd_pack_weights(int type, long rows, long cols, const void *d_raw, size_t raw_row_bytes,
                       void *d_packed, void *stream);

/* Reading a resident image back (csrc/dequant.hip).  The packed image is not write-only: a host that freed the GGUF rows after
 * lfamd_pack_weights can still look rows up, dequantise the tensor and get the file's bytes again, so no tensor has to be held twice
 * (token_embd.weight of a tied-embedding model IS output.weight: one image serves the row lookup and the mat-mul).
 *
 * lfamd_get_rows: rows d_ids[0 .. n_ids) of the packed rows x cols matrix as out_type (LFAMD_TYPE_F32 or LFAMD_TYPE_F16) rows,
 * out_row_bytes apart.  d_ids == NULL: rows row0 .. row0 + n_ids (whole-tensor dequantisation: row0 = 0, n_ids = rows).  Stands for
 * GGML_OP_GET_ROWS (k_get_rows / ggml_cuda_op_get_rows, ggml-cuda.cu.patch:10687-10860) and for the to_fp16 / to_fp32 converters
 * (ggml_get_to_fp16_cuda / ggml_get_to_fp32_cuda, :3929-4040), for every type and shape lfamd_packed_size answers non-zero for.
 *   EXACT: every value is the f32 ((d * sc) * q) - (dmin * mn) (K-quants, IQ4_XS) or (d * q) + m (32-blocks) of the block's own
 *   fields (IQ4_NL: q = the codebook value of the index, m = +0), in that order, uncontracted — the same bits as dequantising the
 *   GGUF row on the CPU (oracle.c: ora_dequantize_row),
 *   the sign of zero included; F16 output is that value rounded to nearest-even (subnormals kept, overflow to inf); F32 / F16 /
 *   BF16 tensors convert exactly.
 *   An index outside [0, rows) leaves its output row untouched (the rule lfamd_mul_mat_id has for expert ids); bytes of an output
 *   row beyond `cols` elements are never written; n_ids == 0 is LFAMD_OK with nothing launched.  d_out aligned to 16 bytes with
 *   out_row_bytes a multiple of 16 gets whole 16 / 8-byte stores; any element-aligned buffer works.
 *   Asynchronous on `stream`: no workspace, no allocation, no host read-back — capturable in a graph like lfamd_mul_mat.
 *   Errors, before any launch: unknown type or out_type -> LFAMD_ERR_UNSUPPORTED; cols not a block multiple, out_row_bytes smaller
 *   than cols elements or not a multiple of the element, a null pointer, row0 + n_ids > rows with d_ids == NULL -> LFAMD_ERR_INVALID.
 *   An expert stack needs nothing new: expert e is (const char *)d_packed + e * lfamd_packed_size(type, rows, cols).
 *
 * lfamd_unpack_weights: the inverse of lfamd_pack_weights (ggml_backend_cuda_buffer_get_tensor, ggml-cuda.cu.patch:16890-17027):
 * the image back to GGUF rows, raw_row_bytes apart, BYTE FOR BYTE, for every type.  Every image is a permutation of the file's bits
 * plus derived fields; where a header field is kept re-coded (the sixteen int8 scales of PK3 for Q3_K's scales[12], the eight of the
 * compact IQ4_XS image for scales_l / scales_h) the re-coding is a bijection and is inverted.  No type answers LFAMD_ERR_UNSUPPORTED.
 * One caveat, inherited from packing: the Q2_K / Q3_K images hold d and dmin after an f16 -> f32 -> f16 round trip, which is the
 * identity on every value except a signalling NaN (it comes back quiet).  Same stream and error rules as lfamd_pack_weights. */
int lfamd_get_rows(int type, const void *d_packed, long rows, long cols, const int32_t *d_ids, long row0, long n_ids, int out_type,
                   void *d_out, size_t out_row_bytes, void *stream);
int lfamd_unpack_weights(int type, long rows, long cols, const void *d_packed, void *d_raw, size_t raw_row_bytes, void *stream);

/* Batches (n > 8) of Q4_K / Q5_K / Q6_K run the scaled-operand MFMA body by default: weights as f16(d * sc * q), activations as
 * f16(d8 * code), f32 accumulate — one f16 rounding per operand, relative error ~1e-4 (north star: 1e-3), no scaling per
 * super-block.  Its constants need f16(|d| * 63) * 1024 <= 65504 and |dmin| * 63 <= 65504 for every block, which every ggml-quantised
 * model satisfies (d = max|w| / (15 * 63)).  lfamd_scaled_gemm_ok checks a packed matrix once after the upload
 * (synchronises the stream): 1 = in range, 0 = out of range -> pass LFAMD_FLAG_PRECISE with this matrix (exact integer
 * codes, f32 scales; out-of-range scales would otherwise surface as inf / NaN outputs), < 0 = error.  Types other than
 * the K-quants and Q8_0: always 1.  (Q4_K / Q5_K: the body forms f16(d * sc) * -1024, so f16(|d| * 63) * 1024 <= 65504;
 * Q6_K: |d| * 127 * 32 <= 65504; Q8_0: the f16 batch body's weight image f16(d * q) needs |d| * 127 <= 65504 — an
 * out-of-range Q8_0 matrix passes LFAMD_FLAG_Q80_EXACT instead, lfamd_exact_flag.)
 * Activations are normalised per token by a power of two before the f16 staging and the output column is scaled back
 * (exact), so their magnitude is not limited by f16; only a spread of more than ~2^24 INSIDE one token underflows its
 * smallest super-blocks (they contribute < 1e-7 of the result). */
int lfamd_scaled_gemm_ok(int type, long rows, long cols, const void *d_packed, void *stream);
/* The flag a call on a matrix that lfamd_scaled_gemm_ok answered 0 for must carry: LFAMD_FLAG_Q80_EXACT for Q8_0 (type 8; its
 * GEMVs keep their arithmetic), LFAMD_FLAG_PRECISE for the K-quants. */
static inline unsigned lfamd_exact_flag(int type) {
    return type == 8 ? LFAMD_FLAG_Q80_EXACT : LFAMD_FLAG_PRECISE;
}

/* Which arithmetic a lfamd_mul_mat call with these arguments runs: 1 = exact integer block dot products with f32 scales (the
 * reference's CPU arithmetic, iqk_mul_mat.inc:601-643; within 2e-6 of it: only the order of the f32 sums differs); 0 = scaled
 * operands on the f16 matrix cores (one f16 rounding per operand, <= 1e-3, measured ~3e-4).  In order:
 *   LFAMD_FLAG_FORCE_GENERIC: 1 (the generic kernels; packed types refuse the flag);
 *   every call of up to 8 columns (the GEMVs; Q8_0 bit-exact, or this module's own order under LFAMD_FLAG_Q80_RELAXED): 1;
 *   F32 / F16 / BF16 weights: 1 — the activations are taken in, or rounded from F32 to, the weight's own type, as the
 *     reference's vec_dot_type conversion does, and the products of two 16-bit values are exact in f32;
 *   Q8_0 batches: 0 on the f16 MFMA body (rows of whole 128-weight quads, or the vendor GEMM), 1 on the bit-exact kernel
 *     (LFAMD_FLAG_Q80_EXACT / LFAMD_FLAG_PRECISE, other row lengths);
 *   IQ4_XS batches: 0 (the canonical image rounds |sc * kvalue| above 2048 to f16); Q2_K / Q3_K (|sc * q| <= 128), the
 *     legacy 32-block bodies and IQ4_NL (codebook values |v| <= 127 are exact in f16, d is applied in f32 per block): 1;
 *   Q4_K / Q5_K / Q6_K batches of 9 .. 32 columns that run the small-batch kernel (gemm_sb.hip; where lfamd_mul_mat picks it:
 *     at most a few row tiles per CU, or deep rows): 1; other Q6_K batches: 0 (both batch bodies round sc * (q - 32) above
 *     2048); LFAMD_FLAG_PRECISE / _GEMM_NARROW / _GEMM_PLAIN: 1; the Q4_K batches on the int8 matrix cores (gemm_i8.hip: grids
 *     of at most 256 tiles of 128 x 128 that still fill half the chip): 1; the rest: 0.
 * The answer is per matrix: it does not hold for a matrix inside a mixed-type lfamd_mul_mat_multi_types launch (a Q4_K matrix
 * that would run the int8 body alone shares the scaled f16 staging with its Q6_K sibling there).  A matrix that
 * lfamd_scaled_gemm_ok found out of range is asked about with lfamd_exact_flag(type) in `flags`.  No device call is made. */
int lfamd_mul_mat_is_exact(int Atype, long m, long k, long n, unsigned flags);
/* 1 where the call reproduces the CPU reference's BITS, 0 otherwise.  1: Q8_0 weights with n <= 8 (the vecdot) and Q8_0 batches on
 * the bit-exact kernel (lfamd_mul_mat_is_exact answers 1 for them).  0: a Q8_0 call of n <= 8 that LFAMD_FLAG_Q80_RELAXED moves to
 * the relaxed-order GEMV (1 again where that kernel declines the row, or a flag overrides it), and every other type — their bodies
 * are held to a tolerance, not to bits.  Read from the plan the launch reads.  No device call is made. */
int lfamd_mul_mat_is_bit_exact(int Atype, long m, long k, long n, unsigned flags);

/* ---- activations --------------------------------------------------------------------------
 * f32 rows -> the reference's activation block format (vec_dot_type: Q8_0, Q8_1 or Q8_K in
 * llamafile's field order).  Same rounding as the scalar reference quantisers.  cols a multiple of the block (32; Q8_K: 256),
 * y_row_bytes at least the row's size, x rows 4-byte and Q8_K output rows 4-byte (Q8_0 / Q8_1: 2-byte) aligned, at most 65535
 * rows per call, no NULL pointer: otherwise LFAMD_ERR_INVALID before any launch.  nrows <= 0 is LFAMD_OK with nothing done. */
int lfamd_quantize_rows(int vec_dot_type, const float *d_x, long nrows, long cols, size_t x_row_bytes,
                        void *d_y, size_t y_row_bytes, void *stream);

/* ---- GGML_OP_MUL_MAT -----------------------------------------------------------------------
 * C[j*ldc + i] = sum_l A[i][l] * B[j][l]   (C = A^T B, column-major C like llamafile_sgemm)
 *   A: packed weights (lfamd_pack_weights), m rows x k elements, type Atype
 *   B: n rows, either in the reference's activation format Btype (= vec_dot_type of Atype; the
 *      llamafile_sgemm boundary) or F32 (the GGML_OP_MUL_MAT boundary: quantised on the device,
 *      bit-identically to quantize_row_q8_K / q8_0 / q8_1, fused into the kernels); row stride
 *      b_row_bytes
 *   C: f32, ldc >= m; ORDINARY device memory (hipMalloc / lfamd_malloc): the small-batch kernels add their two K halves
 *      with hardware float atomics, which fine-grained or host-mapped memory does not honour
 * Policy (cf. ggml_cuda_mul_mat): one token -> wave-reduction GEMV kernels; 2 .. 8 tokens -> multi-column GEMVs or, where
 * faster, the small-batch MFMA kernel (also 9 .. 32 tokens on deep rows and matrices of at most 8192 rows: csrc/gemm_sb.hip);
 * larger batches -> dequant-to-MFMA GEMM on 64- / 128-token tiles (plain F16 / BF16 weights and Q8_0: the vendor GEMM instead when
 * lfamd_vendor_gemm_available()).  `workspace` must hold lfamd_mul_mat_workspace() bytes (may be NULL
 * if that is 0).
 *
 * Operand layout of lfamd_mul_mat, lfamd_mul_mat_multi, lfamd_mul_mat_multi_types, lfamd_mul_mat_id and lfamd_mul_mat_id_multi,
 * checked before any launch (LFAMD_ERR_INVALID, nothing written; a workspace smaller than lfamd_mul_mat_workspace() — of the
 * set's largest for the _multi calls — or lfamd_mul_mat_id_workspace() is LFAMD_ERR_WORKSPACE, whichever body the call would run):
 *   - d_B / d_thought, F32 rows under QUANTISED weights: 16-byte aligned, b_row_bytes a multiple of 16 (the staging kernels and the
 *     decode GEMVs read the rows as float4);
 *   - d_B / d_thought in the vec_dot format: the format's own alignment and no more — Q8_K and Q8_1 rows 4-byte aligned with
 *     b_row_bytes a multiple of 4, Q8_0 rows 2-byte aligned with b_row_bytes a multiple of 2 (292-, 36- and 34-byte blocks put every
 *     block behind the first at that alignment anyway; the kernels read fields and code words, never more);
 *   - d_B under F32 / F16 / BF16 weights: aligned to the element (4 / 2 bytes), b_row_bytes a multiple of it.  Rows that are also
 *     16-byte aligned with b_row_bytes a multiple of 16 take the 16-byte-load GEMV (n <= 8); any other layout runs the generic
 *     kernel instead — the same products summed in another order, within 2e-6.  Batches stage the rows element by element where
 *     they are not aligned and give the same bits either way;
 *   - b_row_bytes is at least the row's size and otherwise free: the bytes between rows are never read or written;
 *   - d_C / d_result: 4-byte aligned, ldc >= m and otherwise free; nothing outside the m x n results is written;
 *   - d_workspace: 256-byte aligned (every device allocation is).  Its contents on entry do not matter — nothing in it is read
 *     before the same call wrote it — and no byte beyond lfamd_mul_mat_workspace() / lfamd_mul_mat_id_workspace() is touched;
 *   - d_plan: 4-byte aligned int32, contiguous [tokens][thinkers];
 *   - a staged image (LFAMD_TYPE_STAGED_*): 16-byte aligned, b_row_bytes ignored (below). */
size_t lfamd_mul_mat_workspace(int Atype, long m, long k, long n);
int lfamd_mul_mat(int Atype, const void *d_A_packed, long m, long k, int Btype, const void *d_B,
                  size_t b_row_bytes, long n, float *d_C, long ldc, void *d_workspace,
                  size_t workspace_bytes, unsigned flags, void *stream);

/* Several GGML_OP_MUL_MAT nodes that read the SAME activations (attn_q/k/v; ffn_gate/up) with weights
 * of one type and row length: what a backend's graph_compute may fuse (ggml_backend_cuda_graph_compute,
 * ggml-cuda.cu.patch:18945, walks the node list and is free to).  For n <= 8 and Q4_K / Q6_K weights
 * this is ONE kernel launch over the concatenated rows; otherwise it runs lfamd_mul_mat per matrix
 * (workspace: the largest lfamd_mul_mat_workspace of the set).  Results are identical either way. */
int lfamd_mul_mat_multi(int Atype, int count, const void *const *d_A_packed, const long *m, long k, int Btype,
                        const void *d_B, size_t b_row_bytes, long n, float *const *d_C, const long *ldc,
                        void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* The same for sibling nodes whose weight TYPES may differ (attn_q/k = Q4_K or Q5_K with attn_v = Q6_K in the *_K_M
 * files): at decode (n = 1) those two groups run as ONE launch (bit-identical to the separate calls); batches of
 * Q4_K / Q5_K / Q6_K nodes share one staged copy of the activations (scaled-operand body, see above) and, when the two types'
 * tiles fill one round of the chip, one launch; any other mix falls
 * back to one lfamd_mul_mat_multi per run of equal types. */
int lfamd_mul_mat_multi_types(int count, const int *Atype, const void *const *d_A_packed, const long *m, long k, int Btype,
                              const void *d_B, size_t b_row_bytes, long n, float *const *d_C, const long *ldc, void *d_ws,
                              size_t ws_bytes, unsigned flags, void *stream);

/* ---- GGML_OP_MUL_MAT_ID (mixture of experts) -------------------------------------------------
 * For every (token, thinker): result[token][thinker][:] = W[plan[token][thinker]] x
 * thought[token][thinker % tasks][:]   (tinyblas_cpu_mixmul.inc:39-50).
 *   d_W_packed: `experts` packed matrices, each lfamd_packed_size(type, rows, cols) bytes apart
 *   d_thought : activation rows in vec_dot format, index (token*tasks + task), stride b_row_bytes
 *   d_plan    : int32 [tokens][thinkers]
 *   d_result  : f32 [tokens][thinkers][rows]
 * Decode (tokens <= 4, Q4_K / Q6_K experts): the GEMV kernels read the expert index from d_plan themselves; thinkers
 * sharing their activations (tasks == 1) are one launch.  Batches of Q4_K / Q5_K / Q6_K experts (up to 60 Ki rows): a
 * one-work-group routing kernel groups the rows by expert on the device and ONE launch of the 128x128 MFMA body covers
 * (expert, row block, token tile) — Q4_K / Q5_K on scaled operands like lfamd_mul_mat's batches (exact integer codes with
 * LFAMD_FLAG_PRECISE; lfamd_scaled_gemm_ok over the whole stack: rows = experts * roundup(rows, 32)).  Both are
 * asynchronous and graph-capturable — no host read-back (the reference
 * synchronises, ggml-cuda.cu.patch:18528-18531) — and accept Btype F32 (quantised on the device).  Rows whose expert id
 * is out of range are left untouched.  Other expert types gather rows per expert after a routing read-back and run one
 * mat-mul per expert.
 * lfamd_mul_mat_id_takes_f32() says whether a call accepts Btype F32 (1) or wants the activations in the weight type's vec_dot format
 * (0): Q4_K / Q5_K / Q6_K experts without LFAMD_FLAG_FORCE_GENERIC, up to 4 tokens, or more through the routed launch and its limits
 * (cols % 256 == 0, fewer than 255 experts, tokens * thinkers <= 60 Ki).  It makes no device call; lfamd_mul_mat_id asks it. */
int lfamd_mul_mat_id_takes_f32(int type, long cols, int experts, long tokens, int thinkers, unsigned flags);
size_t lfamd_mul_mat_id_workspace(int type, long rows, long cols, int experts, long tokens, int thinkers);
int lfamd_mul_mat_id(int type, const void *d_W_packed, long rows, long cols, int experts, int Btype,
                     const void *d_thought, size_t b_row_bytes, int tasks, long tokens,
                     const int32_t *d_plan, int thinkers, float *d_result, void *d_workspace,
                     size_t workspace_bytes, unsigned flags, void *stream);

/* Several GGML_OP_MUL_MAT_ID nodes of one weight type and shape over the SAME activations and routing table (ffn_gate_exps and
 * ffn_up_exps of a layer, ggml-cuda.cu.patch:18945 graph_compute sees them back to back): at decode (tokens <= 4, tasks == 1, Q4_K / Q5_K
 * / Q6_K experts) all (tensor, thinker) GEMVs of a token share launches of up to four — one launch for Mixtral's two tensors x two
 * thinkers; otherwise one lfamd_mul_mat_id per tensor.  d_result[j]: f32 [tokens][thinkers][rows] of tensor j. */
int lfamd_mul_mat_id_multi(int type, int count, const void *const *d_W_packed, long rows, long cols, int experts, int Btype,
                           const void *d_thought, size_t b_row_bytes, int tasks, long tokens, const int32_t *d_plan, int thinkers,
                           float *const *d_result, void *d_ws, size_t ws_bytes, unsigned flags, void *stream);

/* The staged activation image of the int8 batch body as an OUTPUT format of the two fused producers below (vec_dot_type =
 * LFAMD_TYPE_STAGED_Q8K, d_yq = a 16-byte aligned buffer of lfamd_staged_q8k_size(k, nrows) bytes, yq_row_bytes ignored) and as an
 * INPUT format of lfamd_mul_mat / lfamd_mul_mat_multi (Btype = LFAMD_TYPE_STAGED_Q8K, d_B = that buffer, b_row_bytes ignored):
 * the Q8_K codes, scales and block sums of quantize_row_q8_K, laid out the way the Q4_K batch body on the int8 matrix cores reads
 * them — a graph that owns the producer runs NO staging launch in front of the mat-mul (reference: quantize_q8_1 fused in front
 * of MMQ, ggml-cuda.cu.patch:15259-15292, 17896).  The result has the bits of the same call on the producer's f32 output.
 * lfamd_mul_mat_takes_staged() says whether a call accepts the image (Q4_K batches that run the int8 body: grids of at most 256
 * tiles of 128 x 128 whose 128 x 64 tiles fill half the chip — attn_q / attn_output / ffn_down of the Llama shapes at 512 tokens;
 * sibling matrices of one lfamd_mul_mat_multi call count together); other calls answer LFAMD_ERR_UNSUPPORTED for it and want Q8_K
 * blocks or f32 rows. */
#define LFAMD_TYPE_STAGED_Q8K 0x1000
size_t lfamd_staged_q8k_size(long k, long nrows);
int lfamd_mul_mat_takes_staged(int Atype, long m, long k, long n, unsigned flags);
/* The same for the scaled-operand f16 batch bodies (Q4_K / Q5_K / Q6_K batches that do not run the int8 body: attn_q/k/v and
 * ffn_gate/up behind a norm, Q6_K ffn_down behind the SwiGLU): LFAMD_TYPE_STAGED_SCALED, a buffer of lfamd_staged_scaled_size(k,
 * nrows) bytes — f16(q8 * d8 * 2^-e(token)) operands with a per-token power-of-two normalisation, the mins operand, 2^e per token;
 * one image serves sibling matrices of different K-quant types (lfamd_mul_mat_multi / _multi_types).  The bits of the same call on
 * the producer's f32 output.  lfamd_mul_mat_takes_staged_scaled() says whether a call accepts it. */
#define LFAMD_TYPE_STAGED_SCALED 0x1001
size_t lfamd_staged_scaled_size(long k, long nrows);
int lfamd_mul_mat_takes_staged_scaled(int Atype, long m, long k, long n, unsigned flags);
/* The same for the batch bodies of the legacy 32-block weight types, whose activations are Q8_0 / Q8_1 blocks: LFAMD_TYPE_STAGED_B32, a
 * buffer of lfamd_staged_b32_size(k, nrows) bytes written by the two _b32 producers below.  With n_pad = roundup(nrows, 128) and nb
 * = k / 256 it holds, each part starting on 256 bytes:
 *     Xh  f16 [nb][n_pad][256]   the codes of quantize_row_q8_0 as f16
 *     d8T f32 [nb * 8][n_pad]    the blocks' f32(f16(d))
 *     sT  f32 [nb * 8][n_pad]    the blocks' f32(f16(sum * d)) of quantize_row_q8_1 (d not yet rounded); always filled
 * so one image serves Q4_0 / IQ4_NL (which read Xh and d8T) and Q4_1 / Q5_0 / Q5_1 (Q4_1 / Q5_1 read sT too).  k % 256 == 0.
 * lfamd_mul_mat_takes_staged_b32() says whether a call accepts it: batches (n > 8) of Q4_0, IQ4_NL, Q4_1, Q5_0, Q5_1 whose rows are
 * whole 256-weight groups, without LFAMD_FLAG_FORCE_GENERIC.  lfamd_mul_mat and lfamd_mul_mat_multi then run the GEMM alone — no
 * staging launch, the workspace untouched — and give the bits of the same call on the producer's f32 output.  Other calls answer
 * LFAMD_ERR_UNSUPPORTED for it (lfamd_mul_mat_multi_types, lfamd_mul_mat_id and lfamd_mul_mat_id_multi always do); a NULL image or
 * one not 16-byte aligned is LFAMD_ERR_INVALID.  Q8_0 weight batches stage in a layout of their own and take Q8_0 rows or f32. */
#define LFAMD_TYPE_STAGED_B32 0x1002
size_t lfamd_staged_b32_size(long k, long nrows);
int lfamd_mul_mat_takes_staged_b32(int Atype, long m, long k, long n, unsigned flags);
/* The same for Q8_0 WEIGHT batches on the f16 loader-wave body (rows of whole 128-weight quads; lfamd_mul_mat and, for 2 .. 4 sibling
 * matrices in one launch, lfamd_mul_mat_multi): LFAMD_TYPE_STAGED_Q80, a buffer of lfamd_staged_q80_size(k, nrows) = n_pad * k * 2 +
 * n_pad * 8 bytes written by the two _b32 producers below, n_pad = roundup(nrows, 128), packed without padding:
 *     Xh        f16 [k / 128][n_pad][128]  per token and 128-weight quad 256 bytes: f16(f32(f16(d)) * stage * code) of quantize_row_q8_0
 *                                          (the f32 product is exact, so it is rounded once); block blk of the quad, elements 4 j .. 4 j + 3,
 *                                          at byte (2 s + (j >> 2)) * 16 + (blk & 1) * 8, s = 2 (j & 3) + (blk >> 1)
 *     stage     f32 [n_pad]                2^(9 - ilogb(D)), D = f32(f16(max |y| of the row / 127)) * 127
 *     tok_scale f32 [n_pad]                2^(ilogb(D) - 9): the store multiplies the token's column by it
 * A row whose D is zero or not finite has 1 in both; the padding tokens nrows .. n_pad hold zero operands and 1 in both.  k % 128 == 0.
 * It is the layout lfamd_mul_mat stages per call for this body (two launches in front of every GEMM), so the call on the image runs
 * the GEMM alone, touches no workspace (d_workspace = NULL is legal) and gives the bits of the same call on the producer's f32 output.
 * lfamd_mul_mat_takes_staged_q80() says whether a call accepts it: Q8_0 weights, n > 8, k % 128 == 0, a packed matrix below 4 GiB,
 * without LFAMD_FLAG_PRECISE, LFAMD_FLAG_Q80_EXACT or LFAMD_FLAG_FORCE_GENERIC, in a process that did not opt into the vendor GEMM; it
 * makes no device call.  lfamd_mul_mat_multi takes it when every matrix of the call does.  Other calls answer LFAMD_ERR_UNSUPPORTED for
 * it (lfamd_mul_mat_multi_types, lfamd_mul_mat_id and lfamd_mul_mat_id_multi always do); a NULL image or one not 16-byte aligned is
 * LFAMD_ERR_INVALID.  The bit-exact Q8_0 body and the F16 / BF16 bodies take no image. */
#define LFAMD_TYPE_STAGED_Q80 0x1003
size_t lfamd_staged_q80_size(long k, long nrows);
int lfamd_mul_mat_takes_staged_q80(int Atype, long m, long k, long n, unsigned flags);

/* A layout modifier of the WEIGHT type, OR-ed into the type of any call that takes one: LFAMD_TYPE_Q4_0 | LFAMD_TYPE_PAD256 means "Q4_0
 * weights, resident as the tile image with the last super-block padded".  The legacy 32-block types (Q4_0, IQ4_NL, Q4_1, Q5_0, Q5_1)
 * reach the tuned kernels only as the tile image of rows of whole 256-weight groups; their unmodified ids keep any other row length as
 * GGUF rows on the generic kernels.  With the modifier, and cols % 32 == 0, the resident image is the P40 (Q4_0, IQ4_NL) / PCL (Q4_1,
 * Q5_0, Q5_1) image of a matrix of kp = 256 * ceil(cols / 256) columns, as if every GGUF row continued with all-zero-byte blocks
 * (d = +0, m = +0, quants and fifth bits 0):
 *   - lfamd_packed_size(T | PAD256, rows, cols) == lfamd_packed_size(T, rows, kp); lfamd_pack_weights reads cols / 32 blocks per raw
 *     row and writes the zero tail itself; lfamd_unpack_weights and lfamd_get_rows read back `cols` columns, bit for bit, and touch
 *     nothing beyond them;
 *   - the mat-mul calls (lfamd_mul_mat, _multi, _multi_types, lfamd_mul_mat_id(_multi), lfamd_time_mul_mat) and their queries
 *     (_workspace(_upto), _is_exact, _is_bit_exact) take the route the base type takes at k = kp and answer as it does there: the
 *     decode GEMV up to 8 columns (siblings in one launch), the 128 x 128 MFMA body beyond, exact.  The ACTIVATIONS keep their true
 *     length: f32 rows of k floats or k / 32 Q8_0 / Q8_1 blocks, b_row_bytes checked against k; nothing behind a row's k values is read;
 *   - LFAMD_FLAG_FORCE_GENERIC is refused, as on any packed image; the lfamd_mul_mat_takes_staged_* answer 0 where k % 256 != 0 (the
 *     fused producers write rows of whole groups only);
 *   - where cols % 256 == 0 the modifier changes nothing: same size, same bytes, same routes, same results to the bit.
 * On any other base type the modified id is unknown: lfamd_packed_size answers 0, every other call LFAMD_ERR_UNSUPPORTED. */
#define LFAMD_TYPE_PAD256 0x2000
/* The id a caller that packs its own resident copy of a `type` tensor of row length `cols` should use for every size, pack, unpack
 * and mat-mul call on that copy: type | LFAMD_TYPE_PAD256 where that moves the tensor from the generic kernels to the tuned ones (the
 * five types above, rows of whole 32-blocks that are not whole 256-weight groups), else the type unchanged. */
static inline int lfamd_resident_type(int type, long cols) {
    const int pads = type == LFAMD_TYPE_Q4_0 || type == LFAMD_TYPE_Q4_1 || type == LFAMD_TYPE_Q5_0 || type == LFAMD_TYPE_Q5_1 ||
                     type == LFAMD_TYPE_IQ4_NL;
    return pads && cols % 256 != 0 && cols % 32 == 0 ? type | LFAMD_TYPE_PAD256 : type;
}

/* ---- the step in front of the path, fused: RMS-norm x weight -> Q8_K -----------------------------
 * y[i] = (x[i] * 1/sqrtf(mean(x^2) + eps)) * weight[i] per row (ggml_compute_forward_rms_norm_f32 + the MUL node; GPU
 * reference rms_norm_f32, ggml-cuda.cu.patch:14926-14960), written as the reference's Q8_K activation blocks
 * (quantize_row_q8_K, llamafile field order) to d_yq and / or as f32 to d_yf (either may be NULL; d_weight may be NULL = 1).
 * The mat-muls behind the norm then take Btype = Q8_K: no quantisation left in their prologue.  k % 256 == 0;
 * vec_dot_type must be Q8_K (the K-quant and IQ4_XS weights' activation format) or one of the two staged images above.
 * Requirements of both producers, checked before any launch (LFAMD_ERR_INVALID, nothing written):
 *   - f32 operands (d_x, d_gate, d_up, d_weight, d_yf) are 16-byte aligned and their row strides multiples of 16 bytes (rows are
 *     read and written as float4); input pointers are not NULL; d_weight has k elements;
 *   - Q8_K rows (d_yq with vec_dot_type Q8_K) are 4-byte aligned, yq_row_bytes a multiple of 4 and at least k / 256 * 292;
 *   - a staged image (d_yq) is 16-byte aligned and lfamd_staged_q8k_size / lfamd_staged_scaled_size(k, nrows) bytes long: the
 *     whole image is written, its padding tokens nrows .. roundup(nrows, 128) as zeros; yq_row_bytes is ignored;
 *   - at least one of d_yq, d_yf is given; d_yq = NULL writes f32 only, whatever vec_dot_type says; the bytes of either output
 *     do not depend on whether the other is requested;
 *   - nrows >= 0 (0: LFAMD_OK, nothing launched); lfamd_swiglu_quantize takes at most 65408 rows (one grid row per token of the
 *     padded image);
 *   - no output may overlap an input or the other output (the kernels read through __restrict__ pointers and re-read their
 *     inputs after the first stores).
 * Domain: finite inputs.  A 256-block whose largest |y| is non-zero and below about 4e-37 has no Q8_K representation (-128 / max overflows, in
 * the reference quantiser as here).  The scaled image forms 2^(9 - ilogb(max |y| of the row)) in f32: rows whose largest |y| is
 * non-zero and below 2^-118 (about 3e-36) overflow it, so the "magnitude is not limited" of the scaled bodies above holds from
 * there up; an all-zero row is exact (scale 1).  eps = 0 on an all-zero row gives NaN, as the reference does. */
int lfamd_rms_norm_quantize(const float *d_x, size_t x_row_bytes, const float *d_weight, float eps, long nrows, long k,
                            int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes, void *stream);

/* The step in front of ffn_down, fused the same way: y = silu(gate) * up, silu(x) = x / (1 + expf(-x)) (silu_f32,
 * ggml-cuda.cu.patch:16172-16179, + the MUL node), written as Q8_K blocks to d_yq and / or f32 to d_yf.  k % 256 == 0.  The
 * operations are those three in that order, each rounded to f32 — not (gate * up) / (1 + e) and no reciprocal-multiply; expf is
 * the device library's (measured within 1 unit in the last place of the exact exponential on the tests' inputs).  Same
 * requirements and domain as lfamd_rms_norm_quantize; at most 65408 rows. */
int lfamd_swiglu_quantize(const float *d_gate, size_t gate_row_bytes, const float *d_up, size_t up_row_bytes, long nrows, long k,
                          int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes, void *stream);

/* ---- the same two steps for the 32-block activation formats ---------------------------------------
 * RMS-norm x weight, and silu(gate) * up, written as Q8_0 or Q8_1 rows (the vec_dot formats of Q8_0, Q4_0, Q5_0, IQ4_NL and of
 * Q4_1, Q5_1 weights: the decode GEMVs behind then take Btype = Q8_0 / Q8_1 and quantise nothing) or as one of the two staged images
 * above (vec_dot_type = LFAMD_TYPE_STAGED_B32 for batches of the legacy 4- / 5-bit weights, LFAMD_TYPE_STAGED_Q80 for batches of Q8_0
 * weights: no staging launch in front of the batch).  y is the value of lfamd_rms_norm_quantize /
 * lfamd_swiglu_quantize bit for bit; the blocks are quantize_row_q8_0 / quantize_row_q8_1 of it, as lfamd_quantize_rows writes them:
 * d = amax / 127, codes roundf(y / d) (halves away from zero; Q8_K rounds to even), d stored as f16, Q8_1's s = f16(sum * d).
 * Requirements, checked before any launch (LFAMD_ERR_INVALID, nothing written) — those of the two producers above, except:
 *   - k % 32 == 0 for rows (k = 96 or 4128 are legal); k % 256 == 0 for the B32 image, k % 128 == 0 for the Q80 image;
 *   - Q8_0 rows (34-byte blocks) are 2-byte aligned with yq_row_bytes a multiple of 2, Q8_1 rows (36-byte blocks) 4-byte aligned
 *     with yq_row_bytes a multiple of 4 — what lfamd_mul_mat asks of such rows; yq_row_bytes is at least k / 32 blocks, and the
 *     bytes between rows are never written;
 *   - the image (d_yq) is 16-byte aligned, not NULL and lfamd_staged_b32_size / lfamd_staged_q80_size(k, nrows) bytes long: all of
 *     it is written, the padding tokens nrows .. roundup(nrows, 128) as zeros (the Q80 image: with 1 in stage and tok_scale);
 *     yq_row_bytes is ignored;
 *   - vec_dot_type is Q8_0, Q8_1, LFAMD_TYPE_STAGED_B32 or LFAMD_TYPE_STAGED_Q80 (Q8_K and the K-quant images: the two producers above); d_yq = NULL
 *     writes f32 only, whatever vec_dot_type says.
 * Asynchronous and graph-capturable; no workspace, no host read-back.
 * Domain: lfamd_quantize_rows' own — finite inputs.  A block whose amax / 127 exceeds 65504 stores the f16 infinity as its d, as the
 * reference quantiser does (Q8_1's s overflows earlier, from |y| of about 2047 on); a block whose largest |y| is non-zero and below
 * about 4e-37 has no representation (1 / d overflows, in the reference as here).  The Q80 image holds the products f16(d) * code:
 * a block with an infinite d puts inf / NaN into it, as the in-call staging of lfamd_mul_mat does on such a row. */
int lfamd_rms_norm_quantize_b32(const float *d_x, size_t x_row_bytes, const float *d_weight, float eps, long nrows, long k,
                                int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes, void *stream);
int lfamd_swiglu_quantize_b32(const float *d_gate, size_t gate_row_bytes, const float *d_up, size_t up_row_bytes, long nrows, long k,
                              int vec_dot_type, void *d_yq, size_t yq_row_bytes, float *d_yf, size_t yf_row_bytes, void *stream);

/* ---- F16 batched GEMM (attention KQ / KQV) ------------------------------------------------------
 * The interface of tinyblasGemmStridedBatchedEx / tinyblasGemmBatchedEx (llamafile/tinyblas.h:59-71, tinyblas.cu:652-857)
 * for the operand arrangement ggml calls them with (ggml_cuda_mul_mat_batched_cublas, ggml-cuda.cu.patch:18231-18376):
 * transa = T, transb = N, f16 operands, result type Ctype = F16 or F32, f32 accumulation on MFMA:
 *     C_b[j * ldc + i] = alpha * sum_l A_b[i * lda + l] * B_b[j * ldb + l] + beta * C_b[j * ldc + i],   b < batch
 * Leading dimensions and strides in ELEMENTS (lda, ldb >= k; ldc >= m); beta is only applied when nonzero.  The
 * pointer-array form takes DEVICE arrays of `batch` device pointers. */
int lfamd_gemm_strided_batched_f16(long m, long n, long k, float alpha, const void *d_A, long lda, long long strideA,
                                   const void *d_B, long ldb, long long strideB, float beta, void *d_C, int Ctype, long ldc,
                                   long long strideC, int batch, void *stream);
int lfamd_gemm_batched_f16(long m, long n, long k, float alpha, const void *const *d_Aarray, long lda, const void *const *d_Barray,
                           long ldb, float beta, void *const *d_Carray, int Ctype, long ldc, int batch, void *stream);

/* ---- batched GGML_OP_MUL_MAT: F16 x F32, a whole attention product in one launch ------------------
 * The two attention products of a llama.cpp graph (KQ: src0 = the permuted F16 K cache; KQV: src0 = the F16 V cache), on the
 * tensors' own pointers and strides (csrc/mul_mat_batched.hip; reference: ggml_cuda_mul_mat_vec_p021 / _nc /
 * ggml_cuda_mul_mat_batched_cublas, ggml-cuda.cu.patch:18424-18433).  For i3 < ne3, i2 < ne2, j < n, i < m:
 *     C[i3][i2][j][i] = sum_l A[i3 / r3][i2 / r2][i][l] * B[i3][i2][j][l],   r2 = ne2 / a_ne2, r3 = ne3 / a_ne3
 * (r2 query heads share one K / V head: grouped-query attention).
 *   A: raw F16 rows of k elements — no resident image, no pack call, no workspace (the KV cache is rewritten every step);
 *      a_ne2 x a_ne3 slices; element (i03, i02, i, l) at d_A + i03 * a_nb3 + i02 * a_nb2 + i * a_nb1 + l * 2
 *   B: F32, ne2 x ne3 slices of n rows;  element (i3, i2, j, l) at d_B + i3 * b_nb3 + i2 * b_nb2 + j * b_nb1 + l * 4
 *   C: F32 in ORDINARY device memory;    element (i3, i2, j, i) at d_C + i3 * c_nb3 + i2 * c_nb2 + j * c_nb1 + i * 4
 * All strides are ggml's nb[] in BYTES and free beyond the checks below (a_nb2 < a_nb1, the permuted K cache, is legal).  Any
 * element-aligned layout works; A and B with 16-byte aligned bases and strides (of every dimension of extent > 1) are read with
 * 16-byte loads.  The bits of the result do not depend on which loads ran.  Nothing outside the m x n results of each slice is
 * written; nothing behind a row's k values is read.
 * Asynchronous on `stream`, graph-capturable: no allocation, no host read-back, no float atomics; deterministic.
 * Arithmetic — lfamd_mul_mat's float route, selected by n alone:
 *   n <= 8: the f16 weights widened to f32, the activations kept as f32, f32 fused multiply-add, in this module's own fixed order
 *           (a function of k alone).  Where r2 * n <= 8 the K / V rows are read once for all r2 query heads of a group.
 *   n > 8:  each activation rounded once to f16, to nearest-even (a value f16 cannot hold becomes inf or 0, as the reference's
 *           to_fp16 conversion makes it), the products on the f16 matrix cores with f32 accumulation.
 *   Both within 2e-6 (normwise, per slice) of the f64 product of the operands as that route sees them.  A slice's bits do not
 *   depend on how many slices the call has or where the slice sits: the call on ne2 x ne3 slices gives the bits of ne2 x ne3
 *   calls on one slice each.  Domain: finite inputs.
 * Checks, before any launch and in this order:
 *   1. a negative dimension (m, k, n, ne2, ne3, a_ne2, a_ne3)                               -> LFAMD_ERR_INVALID
 *   2. m, n, ne2 or ne3 == 0 -> LFAMD_OK, nothing launched, no pointer looked at (k == 0 is not empty: it writes zeros)
 *   3. Atype != LFAMD_TYPE_F16; more than 65535 slices (ne2 * ne3: they are a grid dimension), more than 65535 * 64 columns or
 *      more than 2^32 rows                                                                  -> LFAMD_ERR_UNSUPPORTED
 *   4. a NULL pointer; a_ne2 < 1 or a_ne3 < 1; ne2 % a_ne2 != 0 or ne3 % a_ne3 != 0; a_nb1 < 2 k, b_nb1 < 4 k or c_nb1 < 4 m; an A
 *      base or stride that is not a multiple of 2; a B or C base or stride that is not a multiple of 4; flags != 0 (reserved)
 *                                                                                           -> LFAMD_ERR_INVALID */
int lfamd_mul_mat_batched(int Atype, const void *d_A, long m, long k, size_t a_nb1, size_t a_nb2, size_t a_nb3, long a_ne2, long a_ne3,
                          const float *d_B, long n, size_t b_nb1, size_t b_nb2, size_t b_nb3, long ne2, long ne3,
                          float *d_C, size_t c_nb1, size_t c_nb2, size_t c_nb3, unsigned flags, void *stream);

/* ---- batched GGML_OP_MUL_MAT on a QUANTISED K cache: 32-block rows x F32, the KQ product in one launch --------------
 * What lfamd_mul_mat_batched is for an F16 cache, for the cache types of -ctk q8_0 / q4_0 / q4_1 / q5_0 / q5_1 / iq4_nl (src0 = a
 * permuted view of a 32-block tensor that is rewritten every step; csrc/mul_mat_batched_q.hip).  The argument list and the index rule
 * are lfamd_mul_mat_batched's: for i3 < ne3, i2 < ne2, j < n, i < m:
 *     C[i3][i2][j][i] = sum_l A[i3 / r3][i2 / r2][i][l] * B[i3][i2][j][l],   r2 = ne2 / a_ne2, r3 = ne3 / a_ne3
 *   A: raw GGUF rows of k / 32 blocks of Atype — no resident image, no pack call, no workspace; row (i03, i02, i) at
 *      d_A + i03 * a_nb3 + i02 * a_nb2 + i * a_nb1
 *   B: F32, element (i3, i2, j, l) at d_B + i3 * b_nb3 + i2 * b_nb2 + j * b_nb1 + l * 4
 *   C: F32 in ORDINARY device memory, element (i3, i2, j, i) at d_C + i3 * c_nb3 + i2 * c_nb2 + j * c_nb1 + i * 4
 * All strides are ggml's nb[] in BYTES and free beyond the checks below (a_nb2 < a_nb1, the permuted K cache, is legal).  Every
 * layout that passes the checks works: a block is read as aligned dwords plus at most one 2-byte load, the activations with 16-byte
 * loads where an address allows; the bits of the result do not depend on which loads ran.  Nothing behind a row's last block is
 * read; nothing outside the m x n results of each slice is written.
 * Asynchronous on `stream`, graph-capturable: no allocation, no host read-back, no float atomics; deterministic.
 * Arithmetic — the reference's CPU path, with exact integer block dots for every n:
 *   activation row (i3, i2, j) is quantised on the device per 32-block, bit for bit as lfamd_quantize_rows does it: Q8_0 for Q8_0,
 *   Q4_0, Q5_0 and IQ4_NL weights, Q8_1 for Q4_1 and Q5_1 (d stored as f16, s = f16(sum * d)).  Block b contributes
 *   (f32(d_w) * f32(d_a)) * isum_b, isum_b the exact int32 dot of the weight codes (Q8_0 qs; Q4_0 q - 8; Q5_0 q - 16; IQ4_NL the
 *   codebook values; Q4_1 / Q5_1 the unsigned q) with the activation codes, and for Q4_1 / Q5_1 then f32(m_w) * f32(s_a).  The
 *   contributions are added in f32 in ascending block order — a function of k and the type alone, not of m, n, the slice or the
 *   layout.  Within 2e-6 (normwise, per slice) of the f64 value of the same sums.  A slice's bits do not depend on the call's other
 *   slices.  Domain: finite inputs.
 * Checks, before any device call and in this order:
 *   1. a negative dimension (m, k, n, ne2, ne3, a_ne2, a_ne3)                               -> LFAMD_ERR_INVALID
 *   2. m, n, ne2 or ne3 == 0 -> LFAMD_OK, nothing launched, no pointer, type, stride or flag looked at (k == 0 is not empty: it
 *      writes zeros)
 *   3. Atype is not Q8_0, Q4_0, Q4_1, Q5_0, Q5_1 or IQ4_NL (an id with LFAMD_TYPE_PAD256, the K-quants, F16, F32, BF16: refused);
 *      k > 1024 (a work-group keeps its quantised activations in LDS); more than 65535 slices, more than 65535 * 64 columns or
 *      more than 2^32 rows                                                                  -> LFAMD_ERR_UNSUPPORTED
 *   4. a NULL pointer; a_ne2 < 1 or a_ne3 < 1; ne2 % a_ne2 != 0 or ne3 % a_ne3 != 0; k % 32 != 0; a_nb1 < lfamd_row_size(Atype, k),
 *      b_nb1 < 4 k or c_nb1 < 4 m; an A base or stride that is not a multiple of 2 (34- and 18-byte blocks guarantee no more); a B
 *      or C base or stride that is not a multiple of 4; flags != 0 (reserved)               -> LFAMD_ERR_INVALID */
int lfamd_mul_mat_batched_q(int Atype, const void *d_A, long m, long k, size_t a_nb1, size_t a_nb2, size_t a_nb3, long a_ne2, long a_ne3,
                            const float *d_B, long n, size_t b_nb1, size_t b_nb2, size_t b_nb3, long ne2, long ne3,
                            float *d_C, size_t c_nb1, size_t c_nb2, size_t c_nb3, unsigned flags, void *stream);

/* ---- GGML_OP_FLASH_ATTN_EXT on an F16 K / V cache: scores, mask, softmax and PV in one fused launch --------------
 * What a llama.cpp graph built with -fa holds per layer in place of KQ, scale + mask, soft_max and KQV (csrc/flash_attn.hip;
 * reference: ggml_cuda_flash_attn_ext, ggml-cuda.cu.patch:8280-8400, its argument list at :8361-8375).  For i3 < ne3, h < n_head,
 * j < n_q, with hk = h / (n_head / n_head_kv) (grouped-query attention):
 *     s_t = scale * sum_l Q[i3][h][j][l] * K[i3][hk][t][l] + mask[j][t],   p_t = exp(s_t - max_t s_t),   t < n_kv
 *     dst[i3][j][h][l] = (sum_t p_t * V[i3][hk][t][l]) / sum_t p_t,        l < D
 *   Q:    F32, element (i3, h, j, l) at d_Q + i3 * q_nb3 + h * q_nb2 + j * q_nb1 + 4 l
 *   K, V: F16 rows of D elements, n_kv rows per KV head; row (i3, hk, t) at + i3 * nb3 + hk * nb2 + t * nb1.  V is NOT transposed
 *         (the -fa cache layout)
 *   mask: F16 or NULL (no mask); element (j, t) at d_mask + j * mask_nb1 + 2 t; one mask for all heads and i3
 *   dst:  F32 in ORDINARY device memory; element (i3, j, h, l) at d_dst + i3 * dst_nb3 + j * dst_nb2 + h * dst_nb1 + 4 l (ggml's
 *         order: heads inside tokens)
 * All strides are ggml's nb[] in BYTES.  Memory contract: nothing behind row n_kv - 1 of K or V and nothing between rows is read;
 * no mask element outside [n_q][n_kv] is read (rows n_q .. of a padded mask never); nothing outside the D * n_head * n_q * ne3
 * results is written.
 * Domain: finite Q, K, V and scale; mask entries finite or -inf; every query row has at least one key whose mask is not -inf.
 * Asynchronous on `stream`, graph-capturable: no allocation, no host read-back, no float atomics; deterministic.
 * Arithmetic — two routes, selected by n_q alone.  Scores are kept in log2 units: s2_t = S_t * (scale * log2 e) + mask * log2 e (one
 * f32 fused multiply-add on the unscaled f32 dot S_t), p_t = exp2(s2_t - m) with the running maximum m; a maximum that is still
 * -inf (every key so far masked) counts as 0 inside the exponentials.
 *   n_q <= 8: Q stays f32, K / V are widened to f32; scores, p and the accumulators are f32 (fmaf).  The keys are cut into chunks of
 *             256, a compile-time constant chosen by timing (128 is faster up to about 4096 keys and loses a
 *             third at 16384, 512 the reverse).  A work-group takes one chunk of one KV head; where n_q * (n_head / n_head_kv)
 *             <= 8 it serves all query heads of the group from one read of the K / V rows, else one query head.  Inside a chunk
 *             wave w of eight takes keys 128 i + 16 w .. (D = 128; D = 64: 256 i + 32 w ..), a lane group one key of every 4 (8),
 *             four keys per online-softmax step; lane groups merge pairwise by lane exchange, the eight waves in wave order.
 *             n_kv <= 256: the work-group writes dst.  Longer: each chunk's (o[D], m, l) goes to the workspace and a second launch
 *             merges the chunks in an order that is a function of the chunk count alone (the maximum first; then o over the
 *             chunks c = g, g + G, ... of each of G = 512 / D groups in ascending order, the groups in ascending g; l by halving).
 *   n_q > 8:  Q is rounded once to f16, unscaled, to nearest-even.  Both products run on the f16 matrix cores with f32
 *             accumulation, in KV tiles of 64 keys; p is rounded once to f16 for the PV product, the row sum is taken from the f32
 *             p.  A 64-key tile whose mask is -inf for every query row of a work-group's 128 is not loaded, and a 32-key half that
 *             is -inf for all 32 rows of a wave is not computed (the causal upper triangle): neither moves a bit.
 *   The bits of a result row are a function of that row's own operands, D and n_kv alone: not of n_head, ne3, where the slice sits,
 *   the other rows, or the device's CU count.  A call on many heads gives the bits of calls on one head each.
 * lfamd_flash_attn_workspace is the only source of the workspace size: 0 where no split runs (n_q > 8 or n_kv <= 256, or a
 * dimension < 1), else ne3 * n_head * n_q * ceil(n_kv / 256) * (D + 2) * 4 bytes.  It makes no device call.
 * Checks, before any device call and in this order (lfamd_flash_attn_check: the same table, exported — below):
 *   1. a negative dimension (D, n_q, n_kv, n_head, n_head_kv, ne3)                          -> LFAMD_ERR_INVALID
 *   2. n_q, n_head or ne3 == 0 -> LFAMD_OK, nothing launched, no pointer looked at
 *   3. Ktype or Vtype is not LFAMD_TYPE_F16 (quantised K / V: refused here; Q8_0 and Q4_0 caches are lfamd_flash_attn_q's, below);
 *      D is not 64 or 128; max_bias != 0 (ALiBi: refused); more than 65535 slices (n_head * ne3: a grid dimension) or 128-row query
 *      blocks; n_kv == 0                                                                    -> LFAMD_ERR_UNSUPPORTED
 *   4. a NULL pointer other than the mask or a zero-size workspace; n_head_kv < 1 or n_head % n_head_kv != 0; a Q / K / V / dst base
 *      or stride that is not a multiple of 16; a mask base or mask_nb1 that is not a multiple of 2, or mask_nb1 < 2 n_kv; k_nb1 or
 *      v_nb1 < 2 D, q_nb1 < 4 D or dst_nb1 < 4 D; flags != 0 (reserved)                       -> LFAMD_ERR_INVALID
 *   5. workspace_bytes < lfamd_flash_attn_workspace(...)                                    -> LFAMD_ERR_WORKSPACE
 * Not served, by design (a host declines the node): quantised K / V (by this call: see lfamd_flash_attn_q), ALiBi, GGML_PREC_F32 (the n_q > 8 route rounds Q and p to
 * f16), head sizes other than 64 / 128, logit soft-capping (the call has no parameter for it).
 * lfamd_flash_attn_check is that list by itself — the call's arguments without scale and stream, no device call, host-only: the code
 * lfamd_flash_attn would answer before it launches (LFAMD_OK: the call passes, or is empty), lfamd_last_error() set the same way.
 * lfamd_flash_attn calls it first.  It is what a host's supports_op asks, and for that it alone takes LFAMD_CHECK_UNPLACED in `flags`
 * (the tensors have no addresses yet): a NULL pointer is then no error and a pointer argument counts with its alignment bits only, and
 * the workspace arguments are not looked at (neither the NULL test of step 4 nor step 5); every other row is evaluated as above.  To
 * lfamd_flash_attn the flag is a reserved flag like any other. */
#define LFAMD_CHECK_UNPLACED 0x40000000u
size_t lfamd_flash_attn_workspace(long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3);
int lfamd_flash_attn_check(const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3,
                           int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,
                           int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3,
                           const void *d_mask, size_t mask_nb1,
                           long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3, float max_bias,
                           const float *d_dst, size_t dst_nb1, size_t dst_nb2, size_t dst_nb3,
                           const void *d_workspace, size_t workspace_bytes, unsigned flags);
int lfamd_flash_attn(const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3,
                     int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,
                     int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3,
                     const void *d_mask, size_t mask_nb1,
                     long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3,
                     float scale, float max_bias,
                     float *d_dst, size_t dst_nb1, size_t dst_nb2, size_t dst_nb3,
                     void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* ---- GGML_OP_FLASH_ATTN_EXT on a Q8_0 / Q4_0 K and V cache (-fa -ctk q8_0 -ctv q8_0, or q4_0) --------------------
 * lfamd_flash_attn for a cache of 32-blocks, an entry point of its own as lfamd_mul_mat_batched_q is beside lfamd_mul_mat_batched
 * (csrc/flash_attn.hip: the same kernels, instantiated on the operand types; reference: the stock pairs of ggml_cuda_flash_attn_ext,
 * ggml-cuda.cu.patch:8240-8265, dispatch :9930-9980).  The argument list, semantics, shapes, strides, mask, dst layout, domain, the
 * two routes picked by n_q alone, the workspace (lfamd_flash_attn_workspace, unchanged: the types do not enter it) and the bit
 * guarantees (a row's bits are a function of its own operands, D, n_kv and the pair alone; many heads give the bits of calls on one
 * head each; asynchronous, capturable, no atomics, no allocation) are lfamd_flash_attn's.  What differs:
 *   Pairs: (Ktype, Vtype) is (Q8_0, Q8_0) or (Q4_0, Q4_0).  Everything else — F16 on either side, mixed pairs, Q4_1 / Q5_0 / Q5_1 /
 *          IQ4_NL, the K-quants — is LFAMD_ERR_UNSUPPORTED; for (F16, F16) the message names lfamd_flash_attn.
 *   Rows:  a K / V row is D / 32 blocks {f16 d, payload}, 34 bytes each for Q8_0 (32 int8 codes) and 18 for Q4_0 (element j < 16 is
 *          the low nibble of payload byte j, element j + 16 its high nibble; the value is d * (nibble - 8)): the bytes lfamd_cpy
 *          stores.  Row (i3, hk, t) at + i3 * nb3 + hk * nb2 + t * nb1.  A block lies on a 2-byte boundary and no better: K / V bases
 *          and strides are multiples of 2 (not 16), k_nb1 / v_nb1 >= D / 32 * the block size.  Q and dst keep their 16-byte rule.
 *   Memory contract: no byte outside the D / 32 blocks of rows 0 .. n_kv - 1 of K or V is read (a payload is read by dword loads
 *          off their boundary, exactly its own bytes and, in front of them, bytes of the same block).
 *   Domain, in addition: every d * code is finite in f16 (it is for any cache lfamd_cpy wrote from values inside f16's range).
 * Arithmetic:
 *   n_q <= 8: a K / V element is f32(d) * (float)code, which is exact in f32; everything from there is lfamd_flash_attn's n_q <= 8
 *             route (f32 fmaf dots, log2-unit scores, four keys per online-softmax step, the wave-order merge, the same workspace
 *             records and the same merge of the chunks).  Q is NOT quantised: ggml's CPU path and the reference's vector kernels
 *             quantise Q to Q8_0 / Q8_1 first; this route does not, and is the more accurate for it.
 *   n_q > 8:  the 64-key K and V tiles are written to on-chip memory as f16, each element f16(d * code) rounded once to nearest
 *             even; from there the arithmetic is lfamd_flash_attn's n_q > 8 route, instruction for instruction.  THE RESULT IS BIT
 *             FOR BIT THAT OF lfamd_flash_attn ON AN F16 CACHE HOLDING f16(d * code).  Limits: this route does not use the int8
 *             matrix cores with a quantised Q; and the f16 rounding of d * code is its property — 2^-11 relative, far below the
 *             cache's own quantisation step (2^-8 of a block's largest value for Q8_0); DESIGN.md section 31 has the measured distance
 *             from the f64 value on the exact block values.
 * Checks: lfamd_flash_attn's five steps in their order, messages prefixed "lfamd_flash_attn_q:".  Step 3's first clause is the pair
 * rule above; step 4's alignment clause is two — a Q / dst base or stride that is not a multiple of 16, then a K / V base or stride
 * that is not a multiple of 2; step 4's row-stride clause takes k_nb1 / v_nb1 against the row of blocks.  lfamd_flash_attn_q_check
 * is that list by itself and takes LFAMD_CHECK_UNPLACED exactly as lfamd_flash_attn_check does; lfamd_flash_attn_q calls it first. */
int lfamd_flash_attn_q_check(const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3,
                             int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,
                             int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3,
                             const void *d_mask, size_t mask_nb1,
                             long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3, float max_bias,
                             const float *d_dst, size_t dst_nb1, size_t dst_nb2, size_t dst_nb3,
                             const void *d_workspace, size_t workspace_bytes, unsigned flags);
int lfamd_flash_attn_q(const float *d_Q, size_t q_nb1, size_t q_nb2, size_t q_nb3,
                       int Ktype, const void *d_K, size_t k_nb1, size_t k_nb2, size_t k_nb3,
                       int Vtype, const void *d_V, size_t v_nb1, size_t v_nb2, size_t v_nb3,
                       const void *d_mask, size_t mask_nb1,
                       long D, long n_q, long n_kv, long n_head, long n_head_kv, long ne3,
                       float scale, float max_bias,
                       float *d_dst, size_t dst_nb1, size_t dst_nb2, size_t dst_nb3,
                       void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* ---- GGML_OP_CPY: the store into an offloaded K / V cache, and the same-type moves of its defragmentation ----------
 * What a llama.cpp graph holds per layer to fill the cache: src = the F32 k_cur / v_cur, dst = a view into the cache tensor
 * (csrc/cpy.hip; reference: ggml_cuda_cpy, ggml-cuda.cu.patch:4242-4760, dispatch :5150-5260).  ggml's semantics: both tensors have
 * the same number of elements, element i of the flattened source (index 0 fastest) becomes element i of the flattened destination;
 * the shapes may differ.  ne[] / nb[] are ggml's, host arrays of four read before the call returns; nb[] in BYTES; for a block type
 * ne[0] counts elements and nb[0] is the block size.
 * Type pairs: F32 -> F32, F16, Q8_0, Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL (the list lfamd_mul_mat_batched_q reads); F16 -> F16 and each of
 * the six block types onto itself (bytes unchanged, whole blocks moved).  Everything else (F16 -> F32, BF16, the K-quants) is
 * LFAMD_ERR_UNSUPPORTED.
 * Arithmetic — a function of the element or of the 32-block alone, never of the route, the shape description or the alignment:
 *   F32 -> F16: round to nearest even; beyond F16's range +-inf; NaN stays NaN (numpy's astype(float16), bit for bit).
 *   F32 -> block type: the scalar rule of ggml's quantize_row_<type>_reference as the reference's device copies restate it
 *   (ggml-cuda.cu.patch:4330-4722), in f32, every product rounded before the add that follows it (no fused multiply-add),
 *   id = d != 0 ? 1 / d : 0 by an IEEE division, the stored d / m = f16(d) / f16(min):
 *     Q8_0   d = amax / 127, codes roundf(x * id)
 *     Q4_0   vmax = the first element of the largest |x|; d = vmax / -8; code min(15, (int8_t)(x * id + 8.5f))
 *     Q5_0   d = vmax / -16; code min(31, (int8_t)(x * id + 16.5f)); bit 4 of code j -> bit j of qh
 *     Q4_1   d = (max - min) / 15; code min(15, (int8_t)((x - min) * id + 0.5f)); min / max = the first of equal values
 *     Q5_1   d = (max - min) / 31; code (uint8_t)((x - min) * id + 0.5f)
 *     IQ4_NL d0 = vmax / -127; codes = the nearest codebook value of x * id0, a tie to the upper index; then, with w = x * x and q the
 *            codebook value, d = sumq2 > 0 ? sumqx / sumq2 : d0 where, for j = 0 .. 15 in ascending order,
 *            sumqx += w[j] * q[j] * x[j] + w[j + 16] * q[j + 16] * x[j + 16] and sumq2 += w[j] * q[j] * q[j] + w[j + 16] * ...
 *            (the reference's pairing of j with j + 16 inside one step, each product chain left to right)
 *   Domain of the block types: finite inputs whose 1 / d is finite.
 * Routes, by the layouts alone; all give the same bytes:
 *   rows        both sides contiguous over runs of at least 128 elements (F32 -> block type; 64 destination bytes for any other pair): 16-byte
 *               loads, eight lanes per 32-block, the run's image assembled in LDS and written with 16-byte stores between a head and a
 *               tail of 2-byte stores (a Q8_0 row is only 2-byte aligned).  The K store, the V store under -fa, defragmentation.
 *   transposed  F32 -> F16, two dimensions of the same extents on both sides, src nb[1] == 4 != src nb[0], dst nb[0] == 2, ne[0] >= 8,
 *               ne[1] >= 2 (the V store without -fa): 64 x 32 tiles through padded LDS, coalesced on both sides, 16-byte stores inside a
 *               destination row.  ne[0] < 8 (one token: every destination row is one element) takes the general route.
 *   general     any other layout: an element per lane, a block per eight lanes.
 * Memory contract: no byte outside the destination's elements is written — not the neighbouring cache cells, not the gap between
 * strided rows, not the bytes in front of an unaligned run or behind it; nothing outside the source's elements is read.  Source and
 * destination must not overlap.  Asynchronous on `stream`, graph-capturable: no allocation, no host read-back, no atomics, no
 * workspace; deterministic.
 * Checks, before any device call and in this order (lfamd_cpy_check: the same table, exported — below):
 *   1. a NULL ne / nb array; a negative extent on either side                               -> LFAMD_ERR_INVALID
 *   2. a destination without elements (a zero extent) -> LFAMD_OK, nothing launched, no pointer, type or stride looked at
 *   3. a type pair outside the list; more than 2^31 - 1 elements on either side (the grid)  -> LFAMD_ERR_UNSUPPORTED
 *   4. a NULL pointer; unequal element counts; beside a block type: ne[0] % 32 != 0 on either side, dst nb[0] not the block size, src
 *      nb[0] not its element / block size (4 for F32); a base or stride that is not a multiple of the element alignment (4 for F32, 2
 *      for F16 and the blocks); where nb[0] is the element size, a stride of a dimension of extent > 1 that is smaller than the row;
 *      flags != 0 (reserved)                                                                -> LFAMD_ERR_INVALID
 * lfamd_cpy_check is that list by itself — the call's arguments without the stream, no device call, host-only: the code lfamd_cpy
 * would answer before it launches (LFAMD_OK: the call passes, or is empty), lfamd_last_error() set the same way.  lfamd_cpy calls it
 * first.  It alone takes LFAMD_CHECK_UNPLACED in `flags` (above: a NULL d_src / d_dst is no error, a pointer counts with its alignment
 * bits only); to lfamd_cpy the flag is a reserved flag like any other. */
int lfamd_cpy_check(int src_type, const void *d_src, const long src_ne[4], const size_t src_nb[4],
                    int dst_type, const void *d_dst, const long dst_ne[4], const size_t dst_nb[4], unsigned flags);
int lfamd_cpy(int src_type, const void *d_src, const long src_ne[4], const size_t src_nb[4],
              int dst_type, void *d_dst, const long dst_ne[4], const size_t dst_nb[4],
              unsigned flags, void *stream);

/* ---- collectives (tensor parallel, one process per GPU) ---------------------------------------
 * The exchange step of the sharded path: attn_output / ffn_down are split by input columns and
 * the f32 partial sums of the residual stream are all-reduced; output.weight is split by vocabulary rows and the logits
 * all-gathered.  The reference has no collective — its row split gathers every result on a main GPU with peer copies
 * (ggml_cuda_op_mul_mat, ggml-cuda.cu.patch:17853-18153; :17781-17851, 18077-18121); these calls replace that step.
 * All of them are asynchronous on `stream` and hipGraph-capturable.
 *
 * Bootstrap: rank 0 calls lfamd_comm_unique_id and hands the 128 bytes to every rank through whatever transport the
 * host has (torch.distributed, MPI, a pipe); every rank calls lfamd_comm_init.  id128 may be NULL for world 1 or for a
 * communicator that only ever uses the one-shot path.  RCCL (librccl.so.1) is dlopen()ed at that point, not before.
 *
 * One-shot all-reduce for decode-sized messages (n_embd * 4 bytes = 16-32 KB): every rank allocates an exchange block of
 * lfamd_oneshot_bytes(max_message_bytes) bytes with lfamd_oneshot_alloc — FINE-GRAINED (uncached) device memory: ordinary
 * hipMalloc memory is coherent between GPUs only at kernel boundaries, and attach refuses it —, exports it (64-byte IPC
 * handle), the host gathers
 * the world's handles in rank order and every rank attaches them (the host must barrier between attach and the first
 * all-reduce).  lfamd_comm_allreduce_add_f32 then runs ONE kernel per call for messages that fit: publish (write-through),
 * flag every peer, wait (bounded), sum the world's partials in rank order — bit-identical on every rank — and add the
 * residual in the same pass.  Larger messages (the 8-16 MB prefill tensors) go through ncclAllReduce.
 * A peer is waited for up to LFAMD_ONESHOT_TIMEOUT_S (default 4) seconds of wall time; then the error is latched (later
 * calls do not wait again, their results are void) until lfamd_comm_clear_error.  lfamd_comm_check() != 0 reports it
 * (1 + the rank that never arrived): a host must call it before trusting results — bench.py does after every timed region. */
typedef struct lfamd_comm lfamd_comm;
int lfamd_comm_unique_id(void *id128);
int lfamd_comm_init(lfamd_comm **comm, int rank, int world, const void *id128);
int lfamd_comm_destroy(lfamd_comm *comm);
/* The single-process form (the shape of ncclCommInitAll): one host thread drives `ndev` devices,
 * comms[i] is rank i on HIP device devices[i].  The exchange blocks are allocated here (fine-grained) and shared as plain
 * pointers — nothing to export or attach —, every collective call below makes the rank's device current for its launch
 * (and restores the caller's), and `stream` must be a stream of that device (or NULL).  Issue every rank's call before
 * synchronising any of them.  RCCL communicators are added when the devices are distinct and the library has
 * ncclCommInitAll; otherwise only messages up to max_message_bytes are served.  1 <= ndev <= 8; a device may repeat (how one
 * GPU rehearses two).  Errors: LFAMD_ERR_INVALID (arguments), LFAMD_ERR_HIP (no device / no peer access / out of memory). */
int lfamd_comm_init_all(lfamd_comm **comms, int ndev, const int *devices, size_t max_message_bytes);
size_t lfamd_oneshot_bytes(size_t max_message_bytes);
int lfamd_oneshot_alloc(void **d_block, size_t bytes);
int lfamd_oneshot_free(void *d_block);
int lfamd_oneshot_export(void *d_block, void *handle64);
int lfamd_oneshot_attach(lfamd_comm *comm, void *d_local_block, size_t block_bytes, const void *handles_world_x_64,
                         size_t max_message_bytes);
/* d_out = (d_residual ? d_residual : 0) + sum over ranks of d_partial   (d_out may alias d_partial) */
int lfamd_comm_allreduce_add_f32(lfamd_comm *comm, const float *d_partial, const float *d_residual, float *d_out, long count,
                                 void *stream);
int lfamd_comm_allreduce_sum_f32(lfamd_comm *comm, float *d_inout, long count, void *stream);
int lfamd_comm_allgather(lfamd_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);

int lfamd_comm_check(lfamd_comm *comm);
int lfamd_comm_clear_error(lfamd_comm *comm);

/* ---- instrumentation ------------------------------------------------------------------------
 * Average device time (microseconds, HIP events on `stream`) of `iters` back-to-back launches of
 * the same lfamd_mul_mat call, after `warmup` untimed ones. */
int lfamd_time_mul_mat(int Atype, const void *d_A_packed, long m, long k, int Btype, const void *d_B,
                       size_t b_row_bytes, long n, float *d_C, long ldc, void *d_workspace,
                       size_t workspace_bytes, unsigned flags, void *stream, int warmup, int iters,
                       float *avg_us);

#ifdef __cplusplus
}
#endif
#endif /* LFAMD_HIP_H_ */
