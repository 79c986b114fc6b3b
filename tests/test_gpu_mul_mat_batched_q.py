"""lfamd_mul_mat_batched_q on the device: the KQ product of a quantised K cache, all heads in one launch (csrc/mul_mat_batched_q.hip).

Every case is built as ggml would hand it over — A a strided byte image whose gaps hold the byte 0x7e (a block read from a gap has a NaN
d), B with NaN in every gap, the result buffer pre-filled with a sentinel pattern, padded rows and a padded row per slice — and checked for
  (a) per-slice rel_err <= 2e-6 against the f64 value of the call's own sums: the activations quantised by the CPU oracle
      (quantize_row_q8_0 / q8_1), per block f32(d_w) * f32(d_a) * the exact integer dot (+ f32(m_w) * f32(s_a)), added in f64
      (oracle f64_gemm; tests/iq4nl_ref.dot_ref for IQ4_NL, which the oracle does not know; tests/block32_ref.sums_ref for Q4_1 and
      Q5_1, where f64_gemm is NOT that value: it multiplies the dequantised operands, i.e. takes m_w * (d_a * sum) where the
      reference's vec_dot and this call read the block's stored s = f16(sum * d).  Measured on the device, Q4_1 m = 96 k = 128 n = 1:
      1.35e-5 from f64_gemm, the f16 rounding of s.  The two types are ALSO held to f64_gemm, within 2e-6 plus the bound of that
      rounding computed from the operands, block32_ref.stored_s_allowance);
  (b) rel_err > 1e-3 against the f64 product of the dequantised weights with the UNQUANTISED activations: the two references lie at
      least 2.7e-3 apart on these inputs (k = 32 .. 576, n = 1 .. 40), so this pins that the activations were quantised as the CPU
      path quantises them;
  (c) bit equality with the same slices computed by calls on one slice each;
  (d) every byte outside the m x n results of each slice unchanged.
Tolerance: the call adds k / 32 <= 32 f32 terms sequentially, each the rounding of an exact product: at most (k / 32 + 2) * 2^-24 of the
sum of the terms' magnitudes, below 2e-6 normwise with room to spare (a sequential f32 block sum emulated on these inputs stays at or
below 1.6e-7 for k <= 576); an f16-operand body would miss it by two orders of magnitude."""
import numpy as np
import pytest

from llamafile_amd import _hip, ggml_types as T, synth
from batched_case import Dev, b_image, run_strided_call, span, strided
from helpers import rel_err
import block32_ref
import iq4nl_ref

TOL = 2e-6
APART = 1e-3
GAP = 0x7e


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def make_layout(row, m, k, n, kvh, heads, unaligned):
    """Byte strides (nb3, nb2, nb1) of A, B and C.  Default: the permuted K cache — A memory [m][kv head][row + 4 bytes of gap]
    (a_nb1 > a_nb2 with several KV heads), B memory [n][head][k + 4 floats of gap].  unaligned: a_nb1 = row + 2 (A memory [kv head][m]),
    b_nb1 = (k + 1) * 4, c_nb1 = (m + 1) * 4.  C always has padded rows and one padded row per slice."""
    if unaligned:
        a1 = row + 2
        a = (kvh * m * a1, m * a1, a1)
        b1 = (k + 1) * 4
        b = (heads * n * b1, n * b1, b1)
        c1 = (m + 1) * 4
    else:
        a2 = row + 4
        a = (m * kvh * a2, a2, kvh * a2)
        b2 = (k + 4) * 4
        b = (n * heads * b2, b2, heads * b2)
        c1 = (m + 3) * 4
    c = (heads * (n + 1) * c1 + 8, (n + 1) * c1, c1)
    return a, b, c


def run_case(dev, t, Av, Bv, unaligned=False, k_call=None):
    """Av: uint8 [a_ne3][kv_heads][m][row bytes] (GGUF rows of type t), Bv: f32 [ne3][heads][n][k].  Returns the results
    [ne3][heads][n][m] after the layout, sentinel and single-slice checks.  k_call: the k handed to the call (0: the k == 0 variant of
    the same call, on the same buffers)."""
    a_ne3, kvh, m, row = Av.shape
    ne3, heads, n, k = Bv.shape
    kc = k if k_call is None else k_call
    a_nb, b_nb, c_nb = make_layout(row, m, k, n, kvh, heads, unaligned)
    A_img = np.full(span(Av.shape, a_nb + (1,), 1) + 6, GAP, np.uint8)
    strided(A_img, np.uint8, Av.shape, a_nb + (1,))[...] = Av
    # (c) the same slices by single-slice calls: the same bits; (d) every byte outside the results is unchanged
    return run_strided_call(dev, dev.lib.lfamd_mul_mat_batched_q, t, A_img, b_image(Bv, b_nb, 4), (m, kc, n, kvh, a_ne3, heads, ne3),
                            a_nb, b_nb, c_nb, unaligned)


def dequantize(t, raw, k):
    from oracle import ora
    return iq4nl_ref.dequantize(raw) if t == T.IQ4_NL else ora.dequantize(t, np.ascontiguousarray(raw), k)


def own_sums(t, A, Bq, m, n, k):
    """f64 [n][m]: the value of the call's sums — and, for the types with an m field, the room the stored s leaves around the
    oracle's f64_gemm (relative to the largest output; 0 for the other types)."""
    from oracle import ora
    if t == T.IQ4_NL:
        return iq4nl_ref.dot_ref(A, Bq), None, 0.0
    G = ora.f64_gemm(t, A, T.VEC_DOT[t], Bq, m, n, k)
    if t in (T.Q4_1, T.Q5_1):
        return block32_ref.sums_ref(t, A, Bq), G, block32_ref.stored_s_allowance(t, A, Bq) / max(np.abs(G).max(), 1e-30)
    return G, None, 0.0


def references(t, Av, Bv, got=None):
    """f64 [ne3][heads][n][m]: (a) the call's own sums, (b) dequantised weights x unquantised activations.  got: the call's results,
    held to the oracle's f64_gemm as well where that is not (a) itself."""
    from oracle import ora
    a_ne3, kvh, m, row = Av.shape
    ne3, heads, n, k = Bv.shape
    group, r3 = heads // kvh, ne3 // a_ne3
    bt = T.VEC_DOT[t]
    own, other = np.empty((ne3, heads, n, m)), np.empty((ne3, heads, n, m))
    W = {(i03, i02): dequantize(t, Av[i03, i02], k).astype(np.float64) for i03 in range(a_ne3) for i02 in range(kvh)}
    for i3 in range(ne3):
        for i2 in range(heads):
            A = np.ascontiguousarray(Av[i3 // r3, i2 // group])
            Bq = ora.quantize(bt, Bv[i3, i2])
            own[i3, i2], G, room = own_sums(t, A, Bq, m, n, k)
            if G is not None and got is not None:
                e = rel_err(got[i3, i2], G)
                print(T.NAMES[t], (i3, i2), "f64_gemm %.3g, room for the stored s %.3g" % (e, room))
                assert e <= TOL + room
            other[i3, i2] = Bv[i3, i2].astype(np.float64) @ W[i3 // r3, i2 // group].T
    return own, other


def synth_case(t, m, k, n, kvh, group, ne3, a_ne3, seed):
    row = T.row_size(t, k)
    Av = synth.random_weights(t, a_ne3 * kvh * m, k, seed).reshape(a_ne3, kvh, m, row)
    Bv = synth.random_activations(ne3 * kvh * group * n, k, seed + 1).reshape(ne3, kvh * group, n, k)
    return Av, Bv


def check(dev, t, m, k, n, kvh, group, ne3=1, a_ne3=1, unaligned=False, seed=0):
    Av, Bv = synth_case(t, m, k, n, kvh, group, ne3, a_ne3, seed)
    got = run_case(dev, t, Av, Bv, unaligned)
    own, other = references(t, Av, Bv, got)
    errs = [(rel_err(got[i3, i2], own[i3, i2]), rel_err(got[i3, i2], other[i3, i2])) for i3 in range(ne3) for i2 in range(kvh * group)]
    print(T.NAMES[t], (m, k, n, kvh, group, ne3, a_ne3), "unaligned" if unaligned else "",
          "max own %.3g, min other %.3g" % (max(e[0] for e in errs), min(e[1] for e in errs)))
    for e_own, e_other in errs:
        assert e_own <= TOL, errs      # (a)
        assert e_other > APART, errs   # (b)
    return Av, Bv, got


SIX = [T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL]
name = lambda t: T.NAMES[t]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("t", SIX, ids=name)
def test_grouped_read(dev, t, n):
    """2 KV heads x 4 query heads, r2 * n <= 8: one item per KV head reads the K rows once for the whole group; a partial last
    work-group of rows (96 = 64 + 32)."""
    check(dev, t, 96, 128, n, 2, 4, seed=1000 + 10 * t + n)


@pytest.mark.gpu
@pytest.mark.parametrize("t", SIX, ids=name)
def test_mfma_body_ragged_tiles(dev, t):
    """n = 40: the matrix-core body; 130 rows = a 128-row tile + 2 (a wave with one row tile of two rows), 40 columns = a wave's 32 + 8."""
    check(dev, t, 130, 128, 40, 2, 4, seed=2000 + t)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_1], ids=name)
def test_one_block_chunked_heads_ne3_broadcast(dev, t):
    """k = 32 (three of a quad's four lanes idle), n = 5: hg = 1 < r2 = 3, so three items per KV head; ne3 = 2 over a_ne3 = 1."""
    check(dev, t, 33, 32, 5, 1, 3, ne3=2, a_ne3=1, seed=3000 + t)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9])
@pytest.mark.parametrize("t", [T.Q8_0, T.Q5_0], ids=name)
def test_route_boundary_single_row(dev, t, n):
    """n = 8 is the last decode shape, n = 9 the first batch shape; m = 1; ne3 = a_ne3 = 2."""
    check(dev, t, 1, 96, n, 2, 1, ne3=2, a_ne3=2, seed=4000 + 10 * t + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 65])
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_0, T.Q5_1], ids=name)
def test_eighteen_blocks(dev, t, n):
    """k = 576 (the largest head dimension in use): 18 blocks = four rounds of a quad and two lanes of a fifth; n = 65: a second
    column tile of one column."""
    check(dev, t, 70, 576, n, 1, 2, seed=5000 + 10 * t + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("t", [T.Q8_0, T.IQ4_NL], ids=name)
def test_k_cap(dev, t, n):
    """k = 1024: the largest k the call takes (the batch body's LDS image is above 64 KiB there)."""
    Av, Bv = synth_case(t, 64, 1024, n, 1, 1, 1, 1, 6000 + 10 * t + n)
    got = run_case(dev, t, Av, Bv)
    own, _ = references(t, Av, Bv)
    err = rel_err(got[0, 0], own[0, 0])
    print(T.NAMES[t], n, "own %.3g" % err)
    assert err <= TOL  # ((b) is stated for k <= 576)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 12])
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_0], ids=name)
def test_unaligned_layout(dev, t, n):
    """A base 2 bytes past a 16-byte boundary, a_nb1 = row_size + 2 (every second row starts off a 4-byte boundary); B and C bases 4
    bytes past one, b_nb1 = (k + 1) * 4, c_nb1 = (m + 1) * 4.  The bits are those of the aligned layout."""
    Av, Bv, got = check(dev, t, 45, 128, n, 2, 2, unaligned=True, seed=7000 + 10 * t + n)
    aligned = run_case(dev, t, Av, Bv)
    assert np.array_equal(got.view(np.uint32), aligned.view(np.uint32)), "the bits depend on which loads ran"


@pytest.mark.gpu
def test_k_zero_writes_exact_zeros(dev):
    Av, Bv, got = check(dev, T.Q8_0, 40, 64, 4, 1, 1, seed=8000)
    zeros = run_case(dev, T.Q8_0, Av, Bv, k_call=0)
    assert np.array_equal(zeros.view(np.uint32), np.zeros_like(zeros).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 12])
def test_bits_do_not_depend_on_the_body(dev, n):
    """The blocks are added in ascending order in both bodies: a column's bits are the same in a decode call (n columns) and in a batch
    call that carries the same columns among 12."""
    t, m, k = T.Q5_1, 70, 160
    Av, Bv = synth_case(t, m, k, 12, 1, 2, 1, 1, 8100)
    wide = run_case(dev, t, Av, Bv)
    narrow = run_case(dev, t, Av, np.ascontiguousarray(Bv[:, :, :n]))
    assert np.array_equal(narrow.view(np.uint32), wide[:, :, :n].view(np.uint32))


def f16_bytes(v):
    return np.array([v], np.float16).view(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 12])
@pytest.mark.parametrize("t", [T.Q8_0, T.Q4_1], ids=name)
def test_extremes(dev, t, n):
    """By hand, m = 8, k = 64: row 0 holds a block of the largest codes under d = 1 (Q8_0: all -128; Q4_1: all 15, m = 1) against an
    activation row of constant -1; row 1 a block with d = +0 and one with d = -0; the last activation row is all zeros and its outputs
    must be == 0."""
    m, k, kvh, group = 8, 64, 1, 2
    Av, Bv = synth_case(t, m, k, n, kvh, group, 1, 1, 9000 + 10 * t + n)
    Av, Bv = Av.copy(), Bv.copy()
    ts, off = T.TYPE_SIZE[t], (2 if t == T.Q8_0 else 4)
    blk = Av.reshape(1, kvh, m, k // 32, ts)
    blk[0, 0, 0, 0, off:] = 0x80 if t == T.Q8_0 else 0xff
    blk[0, 0, 0, 0, 0:2] = f16_bytes(1.0)
    if t == T.Q4_1:
        blk[0, 0, 0, 0, 2:4] = f16_bytes(1.0)
    blk[0, 0, 1, 0, 0:2] = f16_bytes(0.0)
    blk[0, 0, 1, 1, 0:2] = f16_bytes(-0.0)
    Bv[:, :, 0, :] = -1.0
    Bv[:, :, n - 1, :] = 0.0
    got = run_case(dev, t, Av, Bv)
    own, _ = references(t, Av, Bv, got)
    for i2 in range(kvh * group):
        assert rel_err(got[0, i2], own[0, i2]) <= TOL
        assert np.all(got[0, i2, n - 1] == 0.0)
        assert np.isfinite(got[0, i2]).all()


def graph_case():
    """Body of test_calls_in_a_captured_graph; runs in a process of its own (see there)."""
    import torch
    from llamafile_amd import sgemm
    sgemm.init(0)
    lib = _hip.lib()
    t, m, kvh, group = T.Q4_1, 70, 2, 2
    heads = kvh * group
    jobs = []
    for k, n in ((128, 2), (1024, 12)):  # the decode body; the batch body with its LDS image above 64 KiB
        row = T.row_size(t, k)
        A = torch.from_numpy(synth.random_weights(t, kvh * m, k, 9100 + n)).cuda()
        B = torch.from_numpy(synth.random_activations(heads * n, k, 9200 + n)).cuda()
        C = torch.zeros((heads, n, m), device="cuda")
        jobs.append((A, B, C, k, n, row))

    def issue(stream):
        for A, B, C, k, n, row in jobs:
            rc = lib.lfamd_mul_mat_batched_q(t, A.data_ptr(), m, k, row, m * row, kvh * m * row, kvh, 1, B.data_ptr(), n, k * 4, n * k * 4,
                                             heads * n * k * 4, heads, 1, C.data_ptr(), m * 4, n * m * 4, heads * n * m * 4, 0, stream)
            assert rc == 0, lib.lfamd_last_error()

    def eager(seed):
        for A, B, C, k, n, row in jobs:
            B.copy_(torch.from_numpy(synth.random_activations(heads * n, k, seed + n)))
            C.zero_()
        issue(None)
        torch.cuda.synchronize()
        return [C.clone() for _, _, C, _, _, _ in jobs]

    want = {seed: eager(seed) for seed in (1, 2)}  # (also loads the kernels before the capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: two kernel nodes
        issue(torch.cuda.current_stream().cuda_stream)
    for seed in (2, 1):
        for A, B, C, k, n, row in jobs:
            B.copy_(torch.from_numpy(synth.random_activations(heads * n, k, seed + n)))
            C.zero_()
        g.replay()
        torch.cuda.synchronize()
        for (_, _, C, _, _, _), w in zip(jobs, want[seed]):
            assert torch.equal(C.view(torch.int32), w.view(torch.int32)), seed
    print("graph case ok")


@pytest.mark.gpu
def test_calls_in_a_captured_graph(gpu):
    """A decode call and a batch call (k = 1024: dynamic LDS above 64 KiB) captured with torch.cuda.graph on the capture stream and
    replayed twice with other activations give the bits of the eager calls.  The capture runs in a fresh child process, as the other
    capture tests of this suite do (tests/test_gpu_get_rows.py says why)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_mul_mat_batched_q as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
