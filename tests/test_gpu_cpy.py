"""lfamd_cpy on the device (csrc/cpy.hip): GGML_OP_CPY into a K / V cache in device memory, every route.

Every case fills the destination ALLOCATION with a byte pattern, runs one call and compares the whole allocation with the image
tests/cpy_ref.py builds from the same operands: the destination's elements by the NumPy rules, every other byte — the neighbouring
cache cells, the gaps between strided rows, the bytes in front of an unaligned run and behind it — as it was.  A 16-byte store that
reached past a run's end fails the comparison.  Device allocations start on a 16-byte boundary, so a view's offset alone decides how
a run sits in its 16-byte lines."""
import ctypes as C

import numpy as np
import pytest

import cpy_ref as R
from batched_case import Dev
from llamafile_amd import _hip, ggml_types as T

CELLS = 40
F32 = np.float32
STORE_TYPES = (T.F16,) + R.BLOCK_TYPES


@pytest.fixture(scope="module")
def dev(gpu):
    return Dev()


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8)


def values(n, seed):
    """Finite f32 of mixed magnitude, some zeros and repeated extremes (ties of |x| inside a block)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))).astype(F32)
    x[rng.integers(0, n, max(1, n // 16))] = 0.0
    if n >= 64:
        x[5], x[9], x[40], x[41] = 7.25, -7.25, -3.5, 3.5
    return x


def contiguous(t, ne):
    ts, blck = T.TYPE_SIZE.get(t, 4 if t == T.F32 else 2), T.BLCK.get(t, 1)
    nb = [ts, ts * ne[0] // blck]
    nb += [nb[1] * ne[1], nb[1] * ne[1] * ne[2]]
    return tuple(nb)


def arr(ctype, v):
    return (ctype * 4)(*v)


def call(lib, st, ps, s_ne, s_nb, dt, pd, d_ne, d_nb, stream=None):
    rc = lib.lfamd_cpy(st, ps, arr(C.c_long, s_ne), arr(C.c_size_t, s_nb), dt, pd, arr(C.c_long, d_ne), arr(C.c_size_t, d_nb), 0, stream)
    assert rc == 0, _hip.lib().lfamd_last_error()


def run(dev, st, src_buf, s_base, s_ne, s_nb, dt, dst_buf, d_base, d_ne, d_nb):
    """One call; src_buf None: the source lives in the destination's allocation (a move inside one cache).  Returns the allocation
    after the call, compared with the expected image."""
    hd = dev.put(dst_buf, 0)
    hs = hd if src_buf is None else dev.put(src_buf, 0)
    call(dev.lib, st, dev.ptr(hs) + s_base, s_ne, s_nb, dt, dev.ptr(hd) + d_base, d_ne, d_nb)
    got = dev.get(hd)
    want = R.expected_image(dst_buf, d_base, dt, d_ne, d_nb, dst_buf if src_buf is None else src_buf, s_base, st, s_ne, s_nb)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("first differing byte", int(bad[0]), "of", got.size, "destination starts at", d_base)
    return got


def f32_bytes(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint8).reshape(-1)


def k_store(dev, t, D, heads, n_tok, head, s_ne=None, d_ne=None):
    """k_cur [D, heads, n_tok] contiguous into cells head .. of a CELLS-cell cache of type t; the shapes as the caller describes them."""
    n = D * heads * n_tok
    row = T.row_size(t, D * heads)
    s_ne = s_ne or (D, heads, n_tok, 1)
    d_ne = d_ne or (n, 1, 1, 1)
    d_nb = list(contiguous(t, d_ne))
    if d_ne[1] > 1:
        assert d_ne[0] == D * heads and d_nb[1] == row
    src = f32_bytes(values(n, 1000 * D + 10 * n_tok + head))
    return run(dev, T.F32, src, 0, s_ne, contiguous(T.F32, s_ne), t, pattern(CELLS * row), head * row, d_ne, tuple(d_nb))


@pytest.mark.gpu
@pytest.mark.parametrize("D,heads", [(128, 2), (64, 1)])
@pytest.mark.parametrize("t", STORE_TYPES, ids=lambda t: T.NAMES[t])
def test_k_store(dev, t, D, heads):
    """(64, 1): a Q8_0 row is 68 bytes, cell 5 starts 4 bytes into a 16-byte line; one token of it is two blocks (the general route),
    three tokens one short run, seventeen a run of two tiles."""
    for n_tok in (1, 3, 17):
        for head in (0, 5):
            k_store(dev, t, D, heads, n_tok, head)


@pytest.mark.gpu
@pytest.mark.parametrize("t", STORE_TYPES, ids=lambda t: T.NAMES[t])
def test_the_bytes_do_not_depend_on_the_shape_description_or_the_route(dev, t):
    D, heads, n_tok, head = 64, 1, 3, 5
    n, row = D * heads * n_tok, T.row_size(t, D * heads)
    a = k_store(dev, t, D, heads, n_tok, head, s_ne=(n, 1, 1, 1))
    b = k_store(dev, t, D, heads, n_tok, head)
    c = k_store(dev, t, D, heads, n_tok, head, s_ne=(D * heads, n_tok, 1, 1), d_ne=(D * heads, n_tok, 1, 1))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    # the first token alone (64 elements: below the rows route's threshold for the block types) gives the first cell's bytes
    src = f32_bytes(values(n, 1000 * D + 10 * n_tok + head)[:D * heads])
    one = run(dev, T.F32, src, 0, (D, heads, 1, 1), contiguous(T.F32, (D, heads, 1, 1)), t, pattern(CELLS * row), head * row, (D * heads, 1, 1, 1),
              contiguous(t, (D * heads, 1, 1, 1)))
    assert np.array_equal(one[head * row:(head + 1) * row], a[head * row:(head + 1) * row])


N_CTX, N_EMBD_V = 96, 256


def v_store_t(dev, n_tok, head, src_row, s_ne=None, s_nb=None, d_ne=None, d_nb=None, x=None):
    """v_cur [N_EMBD_V, n_tok] (rows src_row floats apart) through its transposed view into the transposed F16 V cache: [n_tok,
    N_EMBD_V] rows N_CTX elements apart, from element head of each."""
    x = values(n_tok * N_EMBD_V, 77 + n_tok) if x is None else x
    img = np.full(n_tok * src_row, np.nan, F32)
    img.reshape(n_tok, src_row)[:, :N_EMBD_V] = x.reshape(n_tok, N_EMBD_V)
    s_ne = s_ne or (n_tok, N_EMBD_V, 1, 1)
    s_nb = s_nb or (src_row * 4, 4, src_row * 4 * n_tok, src_row * 4 * n_tok)
    d_ne = d_ne or (n_tok, N_EMBD_V, 1, 1)
    d_nb = d_nb or (2, N_CTX * 2, N_CTX * 2 * N_EMBD_V, N_CTX * 2 * N_EMBD_V)
    return run(dev, T.F32, f32_bytes(img), 0, s_ne, s_nb, T.F16, pattern(N_CTX * 2 * N_EMBD_V), head * 2, d_ne, d_nb)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tok", [1, 3, 8, 17, 70])
def test_v_store_transposed(dev, n_tok):
    """One and three tokens take the general route (a destination row is one or three elements), eight and more the tile; 70 is more
    than one tile wide.  head 0, 5, 8: rows that start on a 16-byte line, at an odd element, and 16 bytes in.  Source rows of 256 floats
    (16-byte loads) and of 257 (4-byte loads)."""
    for head in (0, 5, 8):
        for src_row in (N_EMBD_V, N_EMBD_V + 1):
            v_store_t(dev, n_tok, head, src_row)


@pytest.mark.gpu
def test_the_transposed_route_gives_the_general_routes_bytes(dev):
    """The same operands described with a dimension of extent 1 between the two (a layout the transposed route does not take)."""
    n_tok, head = 17, 5
    a = v_store_t(dev, n_tok, head, N_EMBD_V)
    b = v_store_t(dev, n_tok, head, N_EMBD_V, s_ne=(n_tok, 1, N_EMBD_V, 1), s_nb=(N_EMBD_V * 4, 4, 4, N_EMBD_V * 4 * n_tok),
                  d_ne=(n_tok, 1, N_EMBD_V, 1), d_nb=(2, N_CTX * 2, N_CTX * 2, N_CTX * 2 * N_EMBD_V))
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [T.F32, T.F16], ids=lambda t: T.NAMES[t])
def test_general_route_permuted_source_into_strided_rows(dev, dt):
    ne = (5, 3, 2, 2)
    s_nb = (12, 4, 60, 120)  # a contiguous [3, 5, 2, 2] tensor with its first two dimensions exchanged
    es = 4 if dt == T.F32 else 2
    d_nb = (es, 8 * es, 32 * es, 72 * es)  # rows of 5 in 8, slices of 3 rows in 4, and a row more between the outer slices
    src = f32_bytes(values(60, 3))
    nbytes = R.unit_offsets(dt, ne, d_nb).max() + es + 6 * es
    run(dev, T.F32, src, 0, ne, s_nb, dt, pattern(int(nbytes) + 4 * es), 4 * es, ne, d_nb)


@pytest.mark.gpu
@pytest.mark.parametrize("t,width", [(T.F16, 256), (T.Q8_0, 256), (T.Q8_0, 64), (T.Q4_0, 64), (T.F32, 64)], ids=lambda v: T.NAMES.get(v, v))
def test_moves_inside_one_cache(dev, t, width):
    """Defragmentation: cells moved between two ranges of one cache, bytes unchanged.  Width 64: a Q8_0 cell is 68 bytes, so cells 5
    and 21 sit alike in their 16-byte lines (16-byte loads) and cells 5 and 22 do not (2-byte loads, 16-byte stores)."""
    row = T.row_size(t, width)
    for src_cell, dst_cell, cells in ((20, 3, 8), (21, 5, 3), (22, 5, 3), (30, 0, 1)):
        ne = (width * cells, 1, 1, 1)
        run(dev, t, None, src_cell * row, ne, contiguous(t, ne), t, pattern(CELLS * row), dst_cell * row, ne, contiguous(t, ne))


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [3, 40])
def test_a_transposed_v_move_inside_one_cache(dev, cells):
    """Two strided 2-D views of the transposed F16 V cache: rows of `cells` elements N_CTX apart (three: the general route)."""
    ne, nb = (cells, N_EMBD_V, 1, 1), (2, N_CTX * 2, N_CTX * 2 * N_EMBD_V, N_CTX * 2 * N_EMBD_V)
    run(dev, T.F16, None, 50 * 2, ne, nb, T.F16, pattern(N_CTX * 2 * N_EMBD_V), 3 * 2, ne, nb)


@pytest.mark.gpu
def test_f16_overflow_and_specials_on_every_route(dev):
    """Beyond F16's range -> +-inf, infinities stay, NaN stays NaN, the smallest values round to subnormals or zero: numpy's
    astype(float16), bit for bit."""
    sp = np.array([1e5, -1e5, 65504.0, 65519.9, 65520.0, -65520.0, np.inf, -np.inf, np.nan, -np.nan, 1e-8, 2.98e-8, 2.9802322e-8, 6e-8,
                   -6e-5, 6.1e-5, 3.4e38, -3.4e38, 0.0, -0.0, 1.0009766, 1.0004883, 1.0014648], F32)
    x = values(17 * N_EMBD_V, 5)
    x[:sp.size] = sp
    x[300:300 + sp.size] = sp
    for head in (0, 5):
        v_store_t(dev, 17, head, N_EMBD_V, x=x)       # the tile
        v_store_t(dev, 3, head, N_EMBD_V, x=x[:3 * N_EMBD_V])  # the general route
    src = f32_bytes(x)
    ne = (x.size, 1, 1, 1)
    run(dev, T.F32, src, 0, ne, contiguous(T.F32, ne), T.F16, pattern(2 * x.size + 64), 6, ne, contiguous(T.F16, ne))  # rows


def graph_case():
    """Body of test_calls_on_a_stream_and_in_a_captured_graph; runs in a process of its own (see there)."""
    import torch
    from llamafile_amd import sgemm
    sgemm.init(0)
    lib = _hip.lib()
    n_tok, width = 17, 256
    row = T.row_size(T.Q8_0, width)
    k_src = torch.zeros(n_tok * width, device="cuda")
    v_src = torch.zeros(n_tok * N_EMBD_V, device="cuda")
    k_cache = torch.zeros(CELLS * row, dtype=torch.uint8, device="cuda")
    v_cache = torch.zeros(N_CTX * 2 * N_EMBD_V, dtype=torch.uint8, device="cuda")

    def issue(stream):
        ne = (n_tok * width, 1, 1, 1)
        call(lib, T.F32, k_src.data_ptr(), ne, contiguous(T.F32, ne), T.Q8_0, k_cache.data_ptr() + 5 * row, ne, contiguous(T.Q8_0, ne), stream)
        vne = (n_tok, N_EMBD_V, 1, 1)
        call(lib, T.F32, v_src.data_ptr(), vne, (N_EMBD_V * 4, 4, 4 * n_tok * N_EMBD_V, 4 * n_tok * N_EMBD_V), T.F16, v_cache.data_ptr() + 5 * 2, vne,
             (2, N_CTX * 2, N_CTX * 2 * N_EMBD_V, N_CTX * 2 * N_EMBD_V), stream)

    def rewrite(seed):
        k_src.copy_(torch.from_numpy(values(n_tok * width, seed)))
        v_src.copy_(torch.from_numpy(values(n_tok * N_EMBD_V, seed + 50)))
        k_cache.fill_(0x5a), v_cache.fill_(0x5a)
        torch.cuda.synchronize()

    def results():
        torch.cuda.synchronize()
        return k_cache.clone(), v_cache.clone()

    def same(got, want, what):
        for g, w in zip(got, want):
            assert (w != 0x5a).any() and torch.equal(g, w), what

    want = {}
    for seed in (1, 2):  # eager, NULL stream (also loads the kernels before the capture)
        rewrite(seed)
        issue(None)
        want[seed] = results()
    assert not torch.equal(want[1][0], want[2][0])
    side = torch.cuda.Stream()
    rewrite(2)
    issue(side.cuda_stream)
    side.synchronize()
    same(results(), want[2], "a non-default stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # a single chain: two kernel nodes
        issue(torch.cuda.current_stream().cuda_stream)
    for seed in (1, 2):
        rewrite(seed)
        g.replay()
        same(results(), want[seed], ("replay", seed))
    print("graph case ok")


@pytest.mark.gpu
def test_calls_on_a_stream_and_in_a_captured_graph(gpu):
    """'Asynchronous on `stream`, graph-capturable': a Q8_0 K store and a transposed V store on a non-default stream, then captured as
    one chain and replayed twice with the sources rewritten in place, give the bytes of the eager NULL-stream calls.  The capture
    runs in a fresh child process, as the other capture tests of this suite do (tests/test_gpu_get_rows.py says why)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_cpy as m; m.graph_case()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph case ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
