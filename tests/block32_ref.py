"""NumPy yardstick for the sums of lfamd_mul_mat_batched_q (include/lfamd_hip.h) on Q4_1 and Q5_1 rows against Q8_1 activation blocks:
per 32-block  f32(d_w) * f32(d_a) * isum + f32(m_w) * f32(s_a),  isum the exact integer dot of the unsigned weight codes with the
activation codes, every product and the sum over the blocks in f64.

Why the oracle's f64_gemm is not this value for the two types: it dequantises both operands and multiplies, (d_w q + m_w) * (d_a q_a),
which amounts to m_w * (f16(d_a) * sum(q_a)) — the block's s field without its f16 rounding.  The reference's vec_dot, and the call,
read the STORED s = f16(sum * d): each of its roundings moves a term by up to 2^-11 of itself, about 1e-5 of a result on synthetic
inputs.  stored_s_allowance() bounds that distance from the operands alone, so a result can be held to both."""
import numpy as np

from llamafile_amd import ggml_types as T


def _f16(blk, off):
    return np.ascontiguousarray(blk[..., off:off + 2]).view(np.float16)[..., 0].astype(np.float64)


def weights(t, raw):
    """(d, m, codes): f64 [rows, blocks], f64 [rows, blocks], int64 [rows, blocks, 32] of Q4_1 / Q5_1 rows."""
    assert t in (T.Q4_1, T.Q5_1)
    ts = T.TYPE_SIZE[t]
    blk = np.ascontiguousarray(raw).reshape(raw.shape[0], raw.shape[1] // ts, ts)
    qs = blk[..., ts - 16:]
    q = np.concatenate([qs & 15, qs >> 4], axis=2).astype(np.int64)
    if t == T.Q5_1:
        qh = np.ascontiguousarray(blk[..., 4:8]).view(np.uint32)[..., 0].astype(np.int64)
        q |= ((qh[..., None] >> np.arange(32)) & 1) << 4
    return _f16(blk, 0), _f16(blk, 2), q


def activations(Bq):
    """(d, s, codes) of block_q8_1 rows [n, k / 32 * 36]."""
    blk = np.ascontiguousarray(Bq).reshape(Bq.shape[0], Bq.shape[1] // 36, 36)
    return _f16(blk, 0), _f16(blk, 2), blk[..., 4:].view(np.int8).astype(np.int64)


def sums_ref(t, raw, Bq):
    """f64 [n, m]."""
    dw, mw, qw = weights(t, raw)
    da, sa, qa = activations(Bq)
    isum = np.einsum("jbl,ibl->jib", qa, qw)
    return np.einsum("jb,ib,jib->ji", da, dw, isum.astype(np.float64)) + sa @ mw.T


def stored_s_allowance(t, raw, Bq):
    """The largest distance, over the outputs, between sums_ref and the oracle's f64_gemm that the f16 roundings of s (and of d inside
    it) can make: sum_b |m_w| * (|s_a| * 2^-10 (1 + 2^-10) + 2^-25), the last term for an s among the f16 subnormals."""
    _, mw, _ = weights(t, raw)
    _, sa, _ = activations(Bq)
    return float(((np.abs(sa) * 2.0 ** -10 * (1 + 2.0 ** -10) + 2.0 ** -25) @ np.abs(mw).T).max())
