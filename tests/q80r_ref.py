"""NumPy statement of the relaxed-order Q8_0 decode GEMV (csrc/gemv_q80r_impl.h, LFAMD_FLAG_Q80_RELAXED) and of what it is held to.

An output (row i, column c) sums 8 * nblocks terms
    t[l, j] = (f32(dA[i, l]) * f32(dB[c, l]))  *  dot4(qA[i, l, 4j .. 4j+3], qB[c, l, 4j .. 4j+3]),      l = block, j = 0..7,
the scale product rounded to f32, the integer dot exact.  The reference of the tests is their f64 sum G; the bounds are stated
against sum |t|.  The kernel adds them in an order that depends on k and the plan's NW alone:
  * wave w of NW takes quads (four blocks) w, w + NW, ...; lane j of the row runs ONE chain over them in block order,
    acc = fma(a, f32(dot4), acc), starting from +0 (blocks past the row in the last quad: a = 0, dot = 0);
  * the row's eight lanes: ((v0 + v4) + (v2 + v6)) + ((v1 + v5) + (v3 + v7));
  * the waves: ((0 + w0) + w1) + ... + w[NW-1].
How many quads of a wave are in flight together (the plan's `ch`) does not enter."""
import numpy as np


def decode_q8_0(raw):
    """uint8 [rows, nb * 34] -> (d f32 [rows, nb], q int8 [rows, nb, 32])."""
    rows = raw.shape[0]
    blk = np.ascontiguousarray(raw).reshape(rows, -1, 34)
    d = blk[:, :, :2].copy().view(np.float16)[:, :, 0].astype(np.float32)
    q = blk[:, :, 2:].copy().view(np.int8)
    return d, q


def block_terms(A, B):
    """(a f32 [n, m, nb], dot int64 [n, m, nb, 8]): the scale products and the integer dots of every output."""
    dA, qA = decode_q8_0(A)
    dB, qB = decode_q8_0(B)
    a = dB[:, None, :] * dA[None, :, :]  # f32 x f32 -> f32, one rounding (the kernel: f32(dA) * d8)
    qa = qA.astype(np.int64).reshape(qA.shape[0], -1, 8, 4)
    qb = qB.astype(np.int64).reshape(qB.shape[0], -1, 8, 4)
    dot = np.einsum("mljx,nljx->nmlj", qa, qb)
    return a.astype(np.float32), dot


def f64_reference(A, B):
    """G [n, m] = the f64 sum of the terms, S [n, m] = sum |t| (non-finite where a scale product is)."""
    a, dot = block_terms(A, B)
    with np.errstate(invalid="ignore", over="ignore"):
        t = a.astype(np.float64)[..., None] * dot.astype(np.float64)
        return t.sum(axis=(2, 3)), np.abs(t).sum(axis=(2, 3))


def _fma(a, b, c):
    # a: f32 scale product (24 bits), b: |dot4| <= 4 * 127 * 127 (17 bits): a * b is exact in f64; one f64 rounding of the sum
    # before the f32 one (a double rounding moves a result only on an exact f32 tie of the f64 sum)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def relaxed_model(A, B, nw):
    """C [n, m] f32 in the kernel's order, for a plan of `nw` waves."""
    a, dot = block_terms(A, B)
    n, m, nb = a.shape
    nquads = (nb + 3) // 4
    slots = (nquads + nw - 1) // nw * nw  # quads rounded up to whole rounds of the waves: the padding is a = 0, dot = 0
    ap = np.zeros((n, m, slots * 4), np.float32)
    dp = np.zeros((n, m, slots * 4, 8), np.float32)
    ap[:, :, :nb] = a
    dp[:, :, :nb] = dot.astype(np.float32)  # (float)dot: exact
    ap = ap.reshape(n, m, slots // nw, nw, 4)      # [round, wave, dd]
    dp = dp.reshape(n, m, slots // nw, nw, 4, 8)   # [round, wave, dd, lane]
    acc = np.zeros((n, m, nw, 8), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for rnd in range(slots // nw):
            for dd in range(4):
                acc = _fma(ap[:, :, rnd, :, dd, None], dp[:, :, rnd, :, dd, :], acc)
        v = acc
        s4 = v[..., 0:4] + v[..., 4:8]            # v0+v4, v1+v5, v2+v6, v3+v7
        s2 = s4[..., 0:2] + s4[..., 2:4]          # (v0+v4)+(v2+v6), (v1+v5)+(v3+v7)
        row = s2[..., 0] + s2[..., 1]             # [n, m, wave]
        t = np.zeros((n, m), np.float32)
        for w in range(nw):
            t = t + row[:, :, w]
    return t
