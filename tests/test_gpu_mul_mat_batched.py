"""lfamd_mul_mat_batched on the device: the attention products KQ and KQV, all heads in one launch (csrc/mul_mat_batched.hip).

Every case is built as ggml would hand it over — strided byte images with NaN in every gap a kernel must not read, the result
buffer pre-filled with a sentinel pattern, padded rows and padded slices — and checked for
  - per-slice rel_err <= 2e-6 against the f64 product of the operands as the route sees them (n <= 8: f32 activations; n > 8:
    activations rounded to f16 by numpy, nearest-even), and > 2e-6 against the OTHER route's reference: the two references lie
    ~1e-4 apart on uniform(-1, 1) inputs, so the bound also pins which arithmetic ran;
  - bit equality with the same slices computed by calls on one slice each;
  - every byte outside the m x n results of each slice unchanged.
Tolerance: one sequential f32 chain of k = 1000 uniform(-1, 1) products stays below 6.4e-7 of the largest output; the kernels'
chains are shorter (k / 16 or k / 64 per lane, then a tree; the matrix cores add exact f16 products in f32)."""
import numpy as np
import pytest

from llamafile_amd import ggml_types as T
from batched_case import Dev, b_image, run_strided_call, span, strided
from helpers import rel_err

TOL = 2e-6
NAN16 = 0x7e00


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def make_layout(kind, m, k, n, kvh, group, ne3, a_ne3, unaligned):
    """Byte strides (nb3, nb2, nb1) of A, B and C.  kq: A memory [m][kv][k] (nb1 > nb2), B memory [n][heads][k]; kqv: A rows n_ctx
    halves apart, B contiguous; edge: kqv with B rows 64 floats apart (16-byte loads with a k tail); unaligned: the prescribed row
    strides (k + 1 elements, m + 1 results).  C always has padded rows and one padded row per slice."""
    heads = kvh * group
    if unaligned:
        a1 = (k + 1) * 2
        a = (kvh * m * a1, m * a1, a1)
        b1 = (k + 1) * 4
        b = (heads * n * b1, n * b1, b1)
        c1 = (m + 1) * 4
    else:
        if kind == "kq":
            a = (m * kvh * k * 2, k * 2, kvh * k * 2)
            b = (n * heads * k * 4, k * 4, heads * k * 4)
        else:
            n_ctx = 256 if k < 256 else 1024 if k < 1024 else 8192
            a = (kvh * m * n_ctx * 2, m * n_ctx * 2, n_ctx * 2)
            b1 = 64 * 4 if kind == "edge" else k * 4
            b = (heads * n * b1, n * b1, b1)
        c1 = (m + 3) * 4
    c = (heads * (n + 1) * c1 + 8, (n + 1) * c1, c1)
    return a, b, c


def run_case(dev, Av, Bv, kind="kq", unaligned=False):
    """Av: f16 [a_ne3][kv_heads][m][k], Bv: f32 [ne3][heads][n][k].  Returns the results [ne3][heads][n][m] after the layout, sentinel
    and single-slice checks."""
    a_ne3, kvh, m, k = Av.shape
    ne3, heads, n, _ = Bv.shape
    group = heads // kvh
    a_nb, b_nb, c_nb = make_layout(kind, m, k, n, kvh, group, ne3, a_ne3, unaligned)
    A_img = np.full(span(Av.shape, a_nb + (2,), 2) // 2, NAN16, np.uint16)
    strided(A_img, np.uint16, Av.shape, a_nb + (2,))[...] = Av.view(np.uint16)
    return run_strided_call(dev, dev.lib.lfamd_mul_mat_batched, T.F16, A_img, b_image(Bv, b_nb), (m, k, n, kvh, a_ne3, heads, ne3),
                            a_nb, b_nb, c_nb, unaligned)


def references(Av, Bv):
    """f64 products [ne3][heads][n][m]: (the route's own, the other route's)."""
    a_ne3, kvh, m, k = Av.shape
    ne3, heads, n, _ = Bv.shape
    group, r3 = heads // kvh, ne3 // a_ne3
    A64 = Av.astype(np.float64)
    B32, B16 = Bv.astype(np.float64), Bv.astype(np.float16).astype(np.float64)
    G = [np.empty((ne3, heads, n, m)) for _ in range(2)]
    for i3 in range(ne3):
        for i2 in range(heads):
            At = A64[i3 // r3, i2 // group].T
            G[0][i3, i2], G[1][i3, i2] = B32[i3, i2] @ At, B16[i3, i2] @ At
    return (G[0], G[1]) if n <= 8 else (G[1], G[0])


def uniform_case(shape, seed):
    m, k, n, kvh, group = shape[:5]
    ne3, a_ne3 = shape[5] if len(shape) > 5 else (1, 1)
    rng = np.random.default_rng(seed)
    Av = (rng.random((a_ne3, kvh, m, k), dtype=np.float32) * 2 - 1).astype(np.float16)
    Bv = (rng.random((ne3, kvh * group, n, k), dtype=np.float32) * 2 - 1).astype(np.float32)
    return Av, Bv


def check_uniform(dev, shape, seed, kind, unaligned=False):
    Av, Bv = uniform_case(shape, seed)
    got = run_case(dev, Av, Bv, kind, unaligned)
    own, other = references(Av, Bv)
    errs = [(rel_err(got[i3, i2], own[i3, i2]), rel_err(got[i3, i2], other[i3, i2])) for i3 in range(Bv.shape[0]) for i2 in range(Bv.shape[1])]
    print(shape, kind, "unaligned" if unaligned else "", "max own %.3g, min other %.3g" % (max(e[0] for e in errs), min(e[1] for e in errs)))
    for e_own, e_other in errs:
        assert e_own <= TOL, errs
        assert e_other > TOL, errs  # the other route's arithmetic did not run


KQ = [(96, 128, 1, 2, 4), (97, 128, 2, 2, 4), (33, 64, 8, 3, 1), (65, 128, 9, 2, 4), (96, 256, 40, 2, 1, (2, 1)), (130, 128, 65, 1, 3, (2, 2))]
KQV = [(128, 32, 1, 2, 4), (128, 100, 1, 2, 4), (40, 304, 5, 2, 1), (128, 100, 17, 2, 4), (64, 1000, 12, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KQ, ids=str)
def test_kq_layout(dev, shape):
    """A memory [m][kv][k] (the permuted K cache: a_nb1 > a_nb2), B memory [n][heads][k]."""
    check_uniform(dev, shape, 100 + KQ.index(shape), "kq")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KQV, ids=str)
def test_kqv_layout(dev, shape):
    """A rows of k halves n_ctx halves apart (n_ctx = 256 or 1024), a_nb2 = m * a_nb1; B contiguous."""
    check_uniform(dev, shape, 200 + KQV.index(shape), "kqv")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 1537, 1, 2, 4), (7, 2056, 2, 1, 4), (5, 4100, 3, 2, 1), (9, 2500, 8, 1, 2)], ids=str)
def test_long_k_decode(dev, shape):
    """KQV layout (rows 8192 halves apart).  At k > 128 the four waves of a work-group split k in steps of 512 elements: three, four,
    five and nine steps — a wave with no step, every wave with one, waves with two or three, a tail step — over a partial last
    work-group of rows, at one, two, four and eight live columns."""
    check_uniform(dev, shape, 600 + shape[1], "kqv")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("k", [1, 7, 8, 9, 15, 16, 17, 23, 31, 33])
def test_k_edges(dev, k, n):
    """m = 5, two slices (one KV head under two query heads); rows on 16-byte boundaries, so the 16-byte loads run up to the last
    whole group of eight and the element loads take the tail."""
    check_uniform(dev, (5, k, n, 1, 2), 300 + k, "edge")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("kq", KQ[1]), ("kq", KQ[3]), ("kqv", KQV[1]), ("kqv", KQV[3])], ids=str)
def test_unaligned_layouts(dev, kind, shape):
    """A base 2 bytes, B and C bases 4 bytes past a 16-byte boundary; a_nb1 = (k + 1) * 2, b_nb1 = (k + 1) * 4, c_nb1 = (m + 1) * 4."""
    check_uniform(dev, shape, 400 + len(kind) + shape[2], kind, unaligned=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 12])
def test_magnitudes_are_exact(dev, n):
    """A in {+-65504, +-0}, B in {+-1, +-60000}, k = 16.  For the sums to be exact in f32 IN ANY ORDER every partial sum must fit 24
    bits: 65504 * 60000 = 3838125 * 2^10 has 22, so a weight row holds four non-zero values among its sixteen (|sum| <= 4 * 3838125 <
    2^24; the other twelve are zeros of either sign), and an activation row takes ONE of the two magnitudes (signs free; a row mixing 1
    and 60000 would need 31 bits).  Then the result is the f64 reference rounded to f32, bit for bit (60000 and 1 are f16 values: the
    n = 12 route rounds nothing away)."""
    m, k, kvh, group = 40, 16, 2, 2
    rng = np.random.default_rng(500 + n)
    Av = rng.choice(np.array([0.0, -0.0], np.float32), (1, kvh, m, k))
    big = rng.choice(np.array([65504.0, -65504.0], np.float32), (1, kvh, m, k))
    pos = np.argsort(rng.random((1, kvh, m, k)), axis=-1)[..., :4]
    np.put_along_axis(Av, pos, np.take_along_axis(big, pos, axis=-1), axis=-1)
    Av = Av.astype(np.float16)
    mag = rng.choice(np.array([1.0, 60000.0], np.float32), (1, kvh * group, n, 1))
    Bv = (mag * rng.choice(np.array([1.0, -1.0], np.float32), (1, kvh * group, n, k))).astype(np.float32)
    got = run_case(dev, Av, Bv, "kqv")
    own, _ = references(Av, Bv)
    want = (own + 0.0).astype(np.float32)  # (an all-cancelling sum is +0 in round-to-nearest)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(want).max() >= 65504.0 * 60000.0
