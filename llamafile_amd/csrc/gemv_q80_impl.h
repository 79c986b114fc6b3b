// gemv_q80_impl.h — the Q8_0 decode GEMV kernel (instantiated by gemv_q80.hip and gemv_q80b.hip; launched from gemv.hip).
//
// Q8_0 x Q8_0, bit-exact restatement of tinyBLAS_Q0_AVX2::gemm (tinyblas_cpu.h:934-971).
// One wave = 8 weight rows, lane = (r = lane>>3, j = lane&7) owns f32 lane j of row r's accumulator
// Cv; blocks are visited in order l = 0..nblocks-1 exactly like the reference's loop, so every
// rounding is the same:  a = f32(dA)*f32(dB);  b = f32(int dot of bytes 4j..4j+3);
// Cv = fma(a, b, Cv)   or, on a PRECISE tile, madder (tinyblas_cpu.h:203-209) with the compiler's
// contraction of sub(mul(a,b),e) into fma(a,b,-e).
#pragma once
#include "gemv_common.h"

// (the LDS image of the activations, X80_QUAD, and the matrix table q80_mats: gemv_launch.h)
// quads (1 KiB per wave each) kept in flight per wave: the row's blocks MUST be visited in order by one lane
// (bit-exact f32 chain), so a matrix offers only m/8 waves (2 per CU at m = 4096) and memory-level parallelism
// has to come from depth.  n = 1: 32 (a whole k = 4096 row group in flight, 192 ring VGPRs); batches: 16.

// MODE: 0 = every output plain fma, 1 = every output Kahan (uniform for n = 1: tinyblas_cpu.h:797-925),
// 2 = per-output choice from the mnpack geometry (small batches n > 1)
template <int NC, int BT, int MODE, int Q80_DEPTH>
__global__ __launch_bounds__(Q80_WAVES * 64) void gemv_q80_kernel(const uint8_t *__restrict__ B, size_t b_row_bytes, long col0, int nblocks,
                                                                 int nquads, long n_total, int vregs32, int precise,
                                                                 const q80_mats mats) {
    // (activation pointer and sizes lead the argument list: they arrive preloaded in SGPRs — Makefile,
    // -amdgpu-kernarg-preload-count — and the activation loads below need nothing else)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane >> 3, j = lane & 7;
#if GEMV_DIAG
    int stamp_n = 0;
#endif
    GSTAMP();
    // the first two activation pieces of this thread go out before anything else: they need only the preloaded leading
    // arguments, while the matrix pick below waits for three dependent rounds of scalar loads
    float va0[16], vb0[16];
    if constexpr (BT == LFAMD_TYPE_F32) {
        const float *x0 = (const float *)(B + col0 * b_row_bytes);
        const int pieces0 = nblocks * 2;
        if ((int)threadIdx.x < pieces0)
            load_piece(va0, x0, threadIdx.x);
        if ((int)threadIdx.x + Q80_WAVES * 64 < pieces0)
            load_piece(vb0, x0, threadIdx.x + Q80_WAVES * 64);
        __builtin_amdgcn_sched_barrier(0);
    }
    long rg = (long)blockIdx.x * Q80_WAVES + wave;
    int mj = 0;
#pragma unroll
    for (int jj = 1; jj < GEMV_MAX_MATS; jj++)
        if (jj < mats.count && rg >= mats.rg_end[jj - 1])
            mj = jj;
    if (mj > 0)
        rg -= mats.rg_end[mj - 1];
    const uint8_t *__restrict__ A = mats.A[mj];
    float *__restrict__ C = mats.C[mj];
    const long m = mats.m[mj], ldc = mats.ldc[mj];
    const long n_rg = (m + 7) / 8;
    const long row = rg * 8 + r;
    // bounds-checked, unconditional weight loads (zeros past the row group / for an idle wave): keeps
    // hipcc's counted vmcnt exact so Q80_DEPTH KiB per wave really stay in flight
    const uint32_t rg_bytes = (uint32_t)nquads * P80_TILE;
    const lfamd_rsrc rA = make_rsrc(A + (size_t)(rg < n_rg ? rg : 0) * rg_bytes, rg < n_rg ? rg_bytes : 0u);

    uint4 qa[Q80_DEPTH];
    uint2 ds[Q80_DEPTH];
    auto issue = [&](int s, int L) {
        qa[s] = buf_ld16_nt(rA, (uint32_t)L * P80_TILE + lane * 16);
        ds[s] = buf_ld8(rA, (uint32_t)L * P80_TILE + P80_D + r * 8);
    };

    if constexpr (BT == LFAMD_TYPE_F32) {
        // quantize_row_q8_0 (x80_quantise_piece, gemv_common.h): 16 floats per lane, two lanes per 32-block.
        // The first piece of each thread is fetched BEFORE the weights (vmcnt retires in order), the weights
        // are issued, then the activations are quantised under their flight.
        const int pieces = nblocks * 2, nthr = Q80_WAVES * 64;
        for (int c = 0; c < NC; c++) {
            const float *x = (const float *)(B + (col0 + c) * b_row_bytes);
            // two pieces per thread and round: both loads go out together (one memory latency per round, not two)
            for (int p0 = 0; p0 < pieces; p0 += 2 * nthr) {
                const int pa = p0 + threadIdx.x, pb = pa + nthr;
                float va[16], vb[16];
                if (c == 0 && p0 == 0) { // (fetched at the top of the kernel)
#pragma unroll
                    for (int e = 0; e < 16; e++)
                        va[e] = va0[e], vb[e] = vb0[e];
                } else {
                    if (pa < pieces)
                        load_piece(va, x, pa);
                    if (pb < pieces)
                        load_piece(vb, x, pb);
                }
                if (c == 0 && p0 == 0) {
#pragma unroll
                    for (int s = 0; s < Q80_DEPTH; s++)
                        issue(s, s);
                }
                // (pieces is even and nthr a multiple of 64: the lane pair (2i, 2i+1) of a block is either both in or out)
                if (pa < pieces)
                    x80_quantise_piece(lds, nquads, va, c, pa);
                if (pb < pieces)
                    x80_quantise_piece(lds, nquads, vb, c, pb);
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < Q80_DEPTH; s++)
            issue(s, s);
        x80_copy_blocks(lds, nquads, B, b_row_bytes, col0, NC, nblocks, Q80_WAVES * 64);
    }
    GSTAMP();
    __syncthreads();
    GSTAMP();

    bool kahan[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        kahan[c] = MODE == 2 ? q0_is_kahan(row < m ? row : m - 1, col0 + c, m, n_total, vregs32 != 0, precise != 0) : MODE == 1;

    float Cv[NC], Ce[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
        Cv[c] = Ce[c] = 0.0f;

    // One block: a = f32(dA)*f32(dB), b = f32(int dot of bytes 4j..4j+3), then the reference's update.  The update is a
    // chain of dependent f32 ops (four per block under Kahan) that ONE lane must run in block order; everything else
    // (scale products, integer dots) is independent of it.  A row offers a single wave no other work, so the loop is
    // software-pipelined by hand: the products of quad L+1 are prepared (prep) before the chain of quad L runs and
    // fill its latency bubbles (measured: the fused form spent ~80 cycles per block, 4-5 us per k = 4096 row).
    struct prepd {
        float a[4][NC], b[4][NC];
    };
    auto prep = [&](int sl, int L, prepd &P) {
        const uint4 q4 = qa[sl];
        const uint2 d2 = ds[sl];
        const uint32_t qw[4] = {q4.x, q4.y, q4.z, q4.w};
        const float da[4] = {h2f((uint16_t)(d2.x & 0xffff)), h2f((uint16_t)(d2.x >> 16)), h2f((uint16_t)(d2.y & 0xffff)),
                             h2f((uint16_t)(d2.y >> 16))};
        const int Lc = L < nquads ? L : nquads - 1; // clamped: the LDS reads are unconditional
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const uint8_t *xb = lds + (size_t)(c * nquads + Lc) * X80_QUAD;
            const uint4 xq4 = *(const uint4 *)(xb + j * 16);
            const float4 xd4 = *(const float4 *)(xb + X80_QD);
            const uint32_t xq[4] = {xq4.x, xq4.y, xq4.z, xq4.w};
            const float xd[4] = {xd4.x, xd4.y, xd4.z, xd4.w};
#pragma unroll
            for (int dd = 0; dd < 4; dd++) {
                P.a[dd][c] = da[dd] * xd[dd];
                P.b[dd][c] = (float)sdot4(qw[dd], xq[dd], 0);
            }
        }
    };
    auto chain = [&](const prepd &P, int dd) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const float a = P.a[dd][c], bq = P.b[dd][c];
            if constexpr (MODE == 0) {
                Cv[c] = __builtin_fmaf(a, bq, Cv[c]);
            } else if constexpr (MODE == 1) {
                const float y = __builtin_fmaf(a, bq, -Ce[c]);
                const float t = Cv[c] + y;
                Ce[c] = (t - Cv[c]) - y;
                Cv[c] = t;
            } else { // branch-free select
                const float plain = __builtin_fmaf(a, bq, Cv[c]);
                const float y = __builtin_fmaf(a, bq, -Ce[c]);
                const float t = Cv[c] + y;
                const float e2 = (t - Cv[c]) - y;
                Cv[c] = kahan[c] ? t : plain;
                Ce[c] = kahan[c] ? e2 : 0.0f;
            }
        }
    };

    // Blocks past the row (zero padding of the last quad, zero-filled prefetch slots) must NOT run: a Kahan
    // step with a*b = 0 still folds the pending compensation into the sum.  Full quads run unguarded.
    const int nq_full = nblocks >> 2;
    prepd P[2];
    prep(0, 0, P[0]);
    issue(0, Q80_DEPTH);
    // rounds of Q80_DEPTH full quads run without a branch in the body (k = 4096 and 14336: every round);
    // the remainder round carries the guards
    int L0 = 0;
    for (; L0 + Q80_DEPTH <= nq_full; L0 += Q80_DEPTH) {
#pragma unroll
        for (int s = 0; s < Q80_DEPTH; s++) {
            const int sn = (s + 1) % Q80_DEPTH;
            prep(sn, L0 + s + 1, P[(s + 1) & 1]); // slot sn holds quad L+1
            issue(sn, L0 + s + 1 + Q80_DEPTH);    // and is refilled as soon as its registers are read
            const prepd &Pc = P[s & 1];
            chain(Pc, 0);
            chain(Pc, 1);
            chain(Pc, 2);
            chain(Pc, 3);
        }
    }
    if (L0 < nquads) {
#pragma unroll
        for (int s = 0; s < Q80_DEPTH; s++) {
            const int L = L0 + s;
            const int sn = (s + 1) % Q80_DEPTH;
            prep(sn, L + 1, P[(s + 1) & 1]);
            const prepd &Pc = P[s & 1];
            if (L < nq_full) {
                chain(Pc, 0);
                chain(Pc, 1);
                chain(Pc, 2);
                chain(Pc, 3);
            } else if (L == nq_full) {
                if (4 * L + 0 < nblocks)
                    chain(Pc, 0);
                if (4 * L + 1 < nblocks)
                    chain(Pc, 1);
                if (4 * L + 2 < nblocks)
                    chain(Pc, 2);
            }
        }
    }
    GSTAMP();
    // hsum(__m256), tinyblas_cpu.h:277-296: ((v0+v4)+(v2+v6)) + ((v1+v5)+(v3+v7))
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float v = Cv[c];
        v = v + __shfl_xor(v, 4, 64);
        v = v + __shfl_xor(v, 2, 64);
        v = v + __shfl_xor(v, 1, 64);
        if (j == 0 && row < m)
            C[(col0 + c) * ldc + row] = v;
    }
}

// every column count 1..8 in the three summation modes; one activation format per unit
template <int NC, int BT>
static const void *q80_kernel_n(int mode) {
    return mode == 0   ? (const void *)gemv_q80_kernel<NC, BT, 0, 16>
           : mode == 1 ? (const void *)gemv_q80_kernel<NC, BT, 1, 16>
           : mode == 2 ? (const void *)gemv_q80_kernel<NC, BT, 2, 16>
                       : nullptr;
}
template <int BT>
static const void *q80_kernel(int nc, int mode) {
    static const void *(*const cols[])(int) = {q80_kernel_n<1, BT>, q80_kernel_n<2, BT>, q80_kernel_n<3, BT>, q80_kernel_n<4, BT>,
                                               q80_kernel_n<5, BT>, q80_kernel_n<6, BT>, q80_kernel_n<7, BT>, q80_kernel_n<8, BT>};
    return nc >= 1 && nc <= 8 ? cols[nc - 1](mode) : nullptr;
}
