// gemv_q80r_impl.h — the relaxed-order Q8_0 decode GEMV (LFAMD_FLAG_Q80_RELAXED; instantiated by gemv_q80r.hip and gemv_q80rb.hip,
// launched from gemv.hip).
//
// Same resident P80 image, same LDS image of the activations and same integer block dots as gemv_q80_kernel (gemv_q80_impl.h), but
// the f32 sum of a row's block terms is NOT tinyBLAS_Q0's chain: K is split over the NW waves of a persistent work-group, as in
// the K-quant GEMVs.  An item is one 8-row group of one matrix (nquads P80 tiles); wave w takes quads w, w + NW, ... in chunks of
// CH; lane (r = lane >> 3, j = lane & 7) owns dword j of row r and runs ONE fma chain over its wave's quads,
//     acc = fma(f32(dA[dd]) * d8[dd], f32(dot4), acc),   dd = 0..3 per quad,
// then the eight lanes of a row are added as ((v0+v4)+(v2+v6)) + ((v1+v5)+(v3+v7)) and the waves through LDS as
// ((0 + w0) + w1) + ... — fixed, so the result is deterministic, and a function of k alone (the plan picks NW and CH from k), so
// it does not depend on m, n, the column's position, the sibling count or the activation format (tests/q80r_ref.py states it).
#pragma once
#include "gemv_common.h"

// The activations of columns col0 .. col0 + NC - 1 into the LDS image (X80_QUAD per quad, gemv_launch.h), by all NTHR threads of
// the work-group: f32 rows quantised like quantize_row_q8_0, Q8_0 rows copied — by the functions gemv_q80_kernel stages with
// (gemv_common.h: x80_quantise_piece, x80_copy_blocks).  v0: this thread's first piece of column 0, fetched by
// the caller ahead of the weights (f32 rows).  The blocks between the row's end and the end of its last quad are zero-filled,
// and so is the dummy quad a wave reads for a quad past the row.
template <int NC, int BT, int NTHR>
__device__ __forceinline__ void q80r_stage(uint8_t *lds, uint8_t *dummy, const uint8_t *__restrict__ B, size_t b_row_bytes, long col0,
                                           int nblocks, int nquads, const float (&v0)[16]) {
    const int tid = threadIdx.x;
    if constexpr (BT == LFAMD_TYPE_F32) {
        const int pieces = nblocks * 2; // 16 floats per lane, two lanes per 32-block
        // (pieces is even and NTHR a multiple of 64: the lane pair (2i, 2i + 1) of a block is either both in or out)
        if (tid < pieces) // the piece fetched ahead of the weights: straight-line, waits for that load alone
            x80_quantise_piece(lds, nquads, v0, 0, tid);
        // the rest one piece at a time (not unrolled over the columns: 16 VGPRs per piece in flight beside the weights' buffers)
#pragma unroll 1
        for (int c = 0; c < NC; c++) {
            const float *x = (const float *)(B + (col0 + c) * b_row_bytes);
#pragma unroll 1
            for (int p = (c == 0 ? NTHR : 0) + tid; p < pieces; p += NTHR) {
                float v[16];
                load_piece(v, x, p);
                x80_quantise_piece(lds, nquads, v, c, p);
            }
        }
    } else {
        x80_copy_blocks(lds, nquads, B, b_row_bytes, col0, NC, nblocks, NTHR);
    }
    // past the row: the last quad's missing blocks (their weights are d = 0, codes 0 in the image, and 0 * garbage could be NaN)
    const int npad = nquads * 4 - nblocks;
    for (int idx = tid; idx < NC * npad * 9; idx += NTHR) {
        int c = idx / (npad * 9), rem = idx % (npad * 9);
        int l = nblocks + rem / 9, w = rem % 9;
        *(uint32_t *)(lds + (size_t)(c * nquads + (l >> 2)) * X80_QUAD + (l & 3) * 4 + (w < 8 ? w * 16 : X80_QD)) = 0u;
    }
    if (tid < X80_QUAD / 4)
        ((uint32_t *)dummy)[tid] = 0u;
}

// One chunk of weights in flight: CH quads of one wave, 16 code bytes and the row's four f16 scales per lane and quad.
template <int CH>
struct q80r_chunk {
    uint4 q[CH];
    uint2 d[CH];
};

template <int NC, int BT, int NW, int CH>
__global__ __launch_bounds__(NW * 64) void gemv_q80r_kernel(const uint8_t *__restrict__ B, size_t b_row_bytes, long col0, int nblocks, int nquads,
                                                           int n_items, int gdim, const q80_mats mats) {
    // (activation pointer and sizes lead the argument list: they arrive preloaded in SGPRs — Makefile, -amdgpu-kernarg-preload-count)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane >> 3, j = lane & 7;
    const q80r_lds lay = q80r_lds_of(NC, nquads, NW);
    uint8_t *dummy = lds + lay.dummy;
    float *red = (float *)(lds + lay.red); // [2][NW][NC][8]

    // f32 rows: this thread's first piece goes out before the weights (vmcnt retires in order: the staging then waits for it alone)
    float v0[16];
    if constexpr (BT == LFAMD_TYPE_F32) {
        if ((int)threadIdx.x < nblocks * 2)
            load_piece(v0, (const float *)(B + col0 * b_row_bytes), threadIdx.x);
        __builtin_amdgcn_sched_barrier(0);
    }

    const int qpw = (nquads + NW - 1) / NW; // quads per wave
    const int cpt = (qpw + CH - 1) / CH;    // chunks per item
    const uint32_t rg_bytes = (uint32_t)nquads * P80_TILE;

    // item `it` (an 8-row group of the concatenated matrices) -> its matrix and its row group there
    auto pick = [&](int it, int &mj, long &rg) __attribute__((always_inline)) {
        mj = 0;
        rg = it;
#pragma unroll
        for (int jj = 1; jj < GEMV_MAX_MATS; jj++)
            if (jj < mats.count && it >= mats.rg_end[jj - 1])
                mj = jj;
        if (mj > 0)
            rg -= mats.rg_end[mj - 1];
    };
    // Bounds-checked, unconditional loads: an item past the launch's last gets a descriptor of 0 records, a quad past the row lies
    // behind the row group's records — zeros, no memory request, and hipcc's counted vmcnt stays exact.
    auto issue = [&](q80r_chunk<CH> &buf, int it, int chunk) __attribute__((always_inline)) {
        int mj;
        long rg;
        pick(it < n_items ? it : 0, mj, rg);
        const lfamd_rsrc rA = make_rsrc(mats.A[mj] + (size_t)rg * rg_bytes, it < n_items ? rg_bytes : 0u);
#pragma unroll
        for (int s = 0; s < CH; s++) {
            const uint32_t off = (uint32_t)(wave + NW * (chunk * CH + s)) * P80_TILE;
            buf.q[s] = buf_ld16_nt(rA, off + lane * 16);
            buf.d[s] = buf_ld8(rA, off + P80_D + r * 8);
        }
    };

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[c] = 0.0f;
    int par = 0;

    // one chunk against the image; at the end of an item: the row's 8 lanes, then the waves through LDS, in a fixed order
    auto consume = [&](const q80r_chunk<CH> &buf, int it, int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < CH; s++) {
            const int q = wave + NW * (chunk * CH + s);
            const uint4 q4 = buf.q[s];
            const uint2 d2 = buf.d[s];
            const uint32_t qw[4] = {q4.x, q4.y, q4.z, q4.w};
            const float da[4] = {h2f((uint16_t)(d2.x & 0xffff)), h2f((uint16_t)(d2.x >> 16)), h2f((uint16_t)(d2.y & 0xffff)),
                                 h2f((uint16_t)(d2.y >> 16))};
#pragma unroll
            for (int c = 0; c < NC; c++) {
                // (a quad past the row was loaded as zeros and reads the zero quad: q is wave-uniform, the select is scalar)
                const uint8_t *xb = lds + (q < nquads ? (uint32_t)(c * nquads + q) * X80_QUAD : (uint32_t)lay.dummy);
                const uint4 xq4 = *(const uint4 *)(xb + j * 16);
                const float4 xd4 = *(const float4 *)(xb + X80_QD);
                const uint32_t xq[4] = {xq4.x, xq4.y, xq4.z, xq4.w};
                const float xd[4] = {xd4.x, xd4.y, xd4.z, xd4.w};
#pragma unroll
                for (int dd = 0; dd < 4; dd++)
                    acc[c] = __builtin_fmaf(da[dd] * xd[dd], (float)sdot4(qw[dd], xq[dd], 0), acc[c]);
                // several columns: left alone, the compiler gathers the LDS reads of every column and quad of the chunk (8 VGPRs
                // each) in front of the first dot and spills.  The empty asm pins two columns' sums behind their reads and the next
                // reads behind it; the other waves of the SIMD cover the LDS latency
                if constexpr (NC > 2)
                    if (c & 1)
                        asm volatile("" : "+v"(acc[c - 1]), "+v"(acc[c])::"memory");
            }
        }
        if (chunk == cpt - 1) {
            float *rb = red + par * (NW * NC * 8);
            par ^= 1;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float v = acc[c];
                v = v + __shfl_xor(v, 4, 64);
                v = v + __shfl_xor(v, 2, 64);
                v = v + __shfl_xor(v, 1, 64);
                if (j == 0)
                    rb[(wave * NC + c) * 8 + r] = v;
                acc[c] = 0.0f;
            }
            __syncthreads();
            if (threadIdx.x < NC * 8) {
                const int c = threadIdx.x >> 3, rr = threadIdx.x & 7;
                float t = 0.0f;
#pragma unroll
                for (int w = 0; w < NW; w++)
                    t += rb[(w * NC + c) * 8 + rr];
                int mj;
                long rg;
                pick(it, mj, rg);
                const long row = rg * 8 + rr;
                if (row < mats.m[mj])
                    ((__attribute__((address_space(1))) float *)mats.C[mj])[(col0 + c) * mats.ldc[mj] + row] = t; // (not FLAT)
            }
        }
    };

    // cursors of the next chunk to issue and the next to consume: (item, chunk)
    int ii = blockIdx.x, ic = 0, ci = blockIdx.x, cc = 0;
#define Q80R_ADVANCE(it, ch)                                                                                           \
    do {                                                                                                               \
        if (++(ch) == cpt)                                                                                             \
            (ch) = 0, (it) += gdim;                                                                                    \
    } while (0)
    q80r_chunk<CH> bufA, bufB;
    issue(bufA, ii, ic);
    Q80R_ADVANCE(ii, ic);
    __builtin_amdgcn_sched_barrier(0);

    q80r_stage<NC, BT, NW * 64>(lds, dummy, B, b_row_bytes, col0, nblocks, nquads, v0);
    __syncthreads();

    // pairs of chunks without a branch inside (a conditionally skipped consume would leave its buffer's loads pending at the loop
    // header for hipcc's wait-count pass), then the odd one — the loop of gemv_kq_body1
    for (;;) {
        int ni = ci, nc = cc;
        Q80R_ADVANCE(ni, nc);
        if (ni >= n_items)
            break;
        issue(bufB, ii, ic);
        Q80R_ADVANCE(ii, ic);
        consume(bufA, ci, cc);
        Q80R_ADVANCE(ci, cc);
        issue(bufA, ii, ic);
        Q80R_ADVANCE(ii, ic);
        consume(bufB, ci, cc);
        Q80R_ADVANCE(ci, cc);
    }
    if (ci < n_items)
        consume(bufA, ci, cc);
#undef Q80R_ADVANCE
}

// every column count 1..8 in the plan's forms (NW = 16; CH = 1, 2 or 4 quads per chunk); one activation format per unit
template <int NC, int BT>
static const void *q80r_kernel_n(int nw, int ch) {
    if (nw != Q80R_WAVES)
        return nullptr;
    return ch == 1   ? (const void *)gemv_q80r_kernel<NC, BT, Q80R_WAVES, 1>
           : ch == 2 ? (const void *)gemv_q80r_kernel<NC, BT, Q80R_WAVES, 2>
           : ch == 4 ? (const void *)gemv_q80r_kernel<NC, BT, Q80R_WAVES, 4>
                     : nullptr;
}
template <int BT>
static const void *q80r_kernel(int nc, int nw, int ch) {
    static const void *(*const cols[])(int, int) = {q80r_kernel_n<1, BT>, q80r_kernel_n<2, BT>, q80r_kernel_n<3, BT>, q80r_kernel_n<4, BT>,
                                                    q80r_kernel_n<5, BT>, q80r_kernel_n<6, BT>, q80r_kernel_n<7, BT>, q80r_kernel_n<8, BT>};
    return nc >= 1 && nc <= 8 ? cols[nc - 1](nw, ch) : nullptr;
}
