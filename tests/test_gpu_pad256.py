"""LFAMD_TYPE_PAD256 on the device: the legacy 32-block types resident as the tile image at row lengths that
are not whole 256-weight groups — pack / unpack, get_rows, the decode GEMV, the 128 x 128 MFMA batches, siblings and MUL_MAT_ID.

Yardsticks: the CPU oracle for Q4_0 / Q4_1 / Q5_0 / Q5_1, tests/iq4nl_ref.py for IQ4_NL, activations from synth.quantize_q8_0 /
_q8_1.  Bounds: those of the exact bodies (tests/test_gpu_iq4nl.py) — 2e-6 normwise and no element beyond helpers.elem_err's rtol
1e-5.  The padding semantics need no tolerance: a call on the padded image has the BITS of the unmodified type on the matrix
zero-extended to kp = 256 * ceil(k / 256) columns with zero-extended activations.

Every activation buffer carries slack behind column k inside its own allocation — NaN for f32 rows, 0xFF bytes (f16 NaN scales) for
Q8_0 / Q8_1 rows — so a kernel that reads past k shows as a non-finite result, and nothing can fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamafile_amd import _hip, ggml_types as T, synth
from llamafile_amd.sgemm import PackedWeights
import extremes
import iq4nl_ref as R
from helpers import elem_err, rel_err
from test_backend_glue import host_exe  # noqa: F401  (the fixture that builds tests/backend_host/backend_host)

pytestmark = pytest.mark.gpu

PAD = _hip.TYPE_PAD256
TYPES = (T.Q4_0, T.IQ4_NL, T.Q4_1, T.Q5_0, T.Q5_1)
KS = (32, 224, 288, 2080, 4000, 8480)  # 1 and 7 valid blocks, a group + 1, a 5-block tail, a tail past 32 super-blocks (5 columns per launch)
TOL = 2e-6
SENT = 0x5A
DT = {"F32": (torch.float32, np.uint32), "F16": (torch.float16, np.uint16)}
tname = lambda t: T.NAMES[t]


def kp_of(k):
    return (k + 255) // 256 * 256


def weights(t, m, k, gen="plain", seed=41):
    if gen == "plain":
        return synth.random_weights(t, m, k, seed)
    return R.extreme_weights(m, k, seed) if t == T.IQ4_NL else extremes.extreme_weights(t, m, k, seed)


def extend_raw(t, raw, k):
    """The GGUF rows continued with all-zero-byte blocks to kp columns."""
    return np.concatenate([raw, np.zeros((raw.shape[0], (kp_of(k) - k) // 32 * T.TYPE_SIZE[t]), np.uint8)], axis=1)


def extend_x(x):
    n, k = x.shape
    return np.concatenate([x, np.zeros((n, kp_of(k) - k), np.float32)], axis=1)


def quantise(t, x):
    return synth.quantize_q8_1(x) if T.VEC_DOT[t] == T.Q8_1 else synth.quantize_q8_0(x)


def yardstick(oracle, t, raw, Bq, k):
    """[n, m] of the whole matrix against quantised rows Bq."""
    if t == T.IQ4_NL:
        return R.dot_ref(raw, Bq)
    ok, G = oracle.sgemm(t, np.ascontiguousarray(raw), T.VEC_DOT[t], np.ascontiguousarray(Bq), raw.shape[0], Bq.shape[0], k, nth=4)
    assert ok == 1
    return G


def dequant_bits(oracle, t, raw, k, dt):
    with np.errstate(over="ignore"):
        w = R.dequantize(raw) if t == T.IQ4_NL else oracle.dequantize(t, np.ascontiguousarray(raw), k)
        return w.view(np.uint32) if dt == "F32" else w.astype(np.float16).view(np.uint16)


def f32_rows(x, slack=True):
    """f32 rows on the device as the uint8 view mul_mat takes; slack: a row stride of (k + 40) floats, NaN behind column k."""
    n, k = x.shape
    if not slack:
        return torch.from_numpy(np.ascontiguousarray(x)).cuda().view(torch.uint8).view(n, -1)
    buf = np.full((n, k + 40), np.nan, dtype=np.float32)
    buf[:, :k] = x
    return torch.from_numpy(buf).cuda().view(torch.uint8).view(n, -1)


def q_rows(Bq, slack=True):
    """Q8_0 / Q8_1 rows with 36 bytes of 0xFF behind each (a block header read there is an f16 NaN)."""
    if not slack:
        return torch.from_numpy(np.ascontiguousarray(Bq)).cuda()
    buf = np.full((Bq.shape[0], Bq.shape[1] + 36), 0xFF, dtype=np.uint8)
    buf[:, :Bq.shape[1]] = Bq
    return torch.from_numpy(buf).cuda()


def run(gpu, W, B, bt, n, **kw):
    c = gpu.mul_mat(W, B, bt, n=n, **kw)
    torch.cuda.synchronize()
    return c.cpu().numpy()


def judge(Cm, G, what):
    assert np.isfinite(Cm).all(), (what, "non-finite: something behind column k was read")
    err = rel_err(Cm, G)
    frac, worst = elem_err(Cm, G, rtol=1e-5)
    print(f"{what}: normwise {err:.3e}, elements over rtol 1e-5: {frac}, worst {worst:.3e}")
    assert err <= TOL, (what, err)
    assert frac == 0.0, (what, frac, worst)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def pack_into(L, t, raw_dev, m, k, stride, fill):
    size = L.lfamd_packed_size(t, m, k)
    out = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lfamd_pack_weights(t, m, k, C.c_void_p(raw_dev.data_ptr()), stride, C.c_void_p(out.data_ptr()), st) == 0
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 1. pack / unpack

@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m,k", [(16, 32), (67, 224), (67, 288), (1030, 2080), (67, 4000), (16, 8480)], ids=str)
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_pack_is_the_image_of_the_zero_extended_rows(gpu, t, m, k, gen):
    L = _hip.lib()
    raw = weights(t, m, k, gen)
    rb = raw.shape[1]
    ext = extend_raw(t, raw, k)
    # the destination pre-filled with 0xA5: a tail the pack does not write shows
    img = pack_into(L, t | PAD, torch.from_numpy(raw).cuda(), m, k, rb, 0xA5)
    want = pack_into(L, t, torch.from_numpy(ext).cuda(), m, kp_of(k), ext.shape[1], 0x00)
    assert img.numel() == want.numel() == L.lfamd_packed_size(t, m, kp_of(k))
    assert torch.equal(img, want)
    W = PackedWeights(t | PAD, m, k, img)
    back = gpu.unpack_weights(W)
    assert np.array_equal(back.cpu().numpy(), raw)
    assert torch.equal(gpu.upload_weights(t | PAD, back, m, k).data, img)  # pack(unpack(pack)) = pack
    # strided raw rows in, strided rows out with sentinels behind each
    wide = np.full((m, rb + 30), SENT, dtype=np.uint8)
    wide[:, :rb] = raw
    assert torch.equal(pack_into(L, t | PAD, torch.from_numpy(wide).cuda(), m, k, rb + 30, 0xA5), img)
    out = torch.full((m, rb + 7), SENT, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lfamd_unpack_weights(t | PAD, m, k, C.c_void_p(img.data_ptr()), C.c_void_p(out.data_ptr()), rb + 7, st) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :rb], raw) and (o[:, rb:] == SENT).all()
    assert L.lfamd_pack_weights(t | PAD, m, k, C.c_void_p(img.data_ptr()), rb - 1, C.c_void_p(img.data_ptr()), st) == -2  # stride below a row


@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_whole_groups_the_modifier_changes_nothing(gpu, t):
    m, k = 67, 512
    raw = weights(t, m, k)
    W, Wp = gpu.upload_weights(t, raw, m, k), gpu.upload_weights(t | PAD, raw, m, k)
    assert torch.equal(W.data, Wp.data)
    x = synth.random_activations(40, k, 3)
    for n in (1, 5, 40):
        B = f32_rows(x[:n], slack=False)
        assert same_bits(run(gpu, W, B, T.F32, n), run(gpu, Wp, B, T.F32, n))
    assert torch.equal(gpu.dequantize(W), gpu.dequantize(Wp))


# ------------------------------------------------------------------------------------------------------------------------
# 2. get_rows

@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m,k", [(33, 32), (67, 224), (67, 2080), (40, 4000)], ids=str)
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_whole_matrix_read_back_bit_for_bit(gpu, oracle, t, m, k, gen, dt):
    raw = weights(t, m, k, gen)
    W = gpu.upload_weights(t | PAD, raw, m, k)
    got = gpu.dequantize(W, DT[dt][0]).cpu().numpy().view(DT[dt][1])
    want = dequant_bits(oracle, t, raw, k, dt)
    bad = int((got != want).sum())
    print(f"{tname(t)} get_rows {m} x {k} {gen} {dt}: {bad} of {want.size} differ")
    assert got.shape == want.shape and bad == 0


@pytest.mark.parametrize("dt", ["F32", "F16"])
@pytest.mark.parametrize("k", [288, 2080])
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_index_lists_ranges_and_padded_outputs(gpu, oracle, t, k, dt):
    rows = 67
    raw = weights(t, rows, k, "extreme")
    W = gpu.upload_weights(t | PAD, raw, rows, k)
    want = dequant_bits(oracle, t, raw, k, dt)
    tdt, ndt = DT[dt]
    esz = np.dtype(ndt).itemsize
    sent = int.from_bytes(bytes([SENT]) * esz, "little")
    idx = [66, 0, 5, 5, 64, -1, 31, 32, 65, rows, 0, 66, 17]  # repeats, the ragged last tile, two ids outside [0, rows)
    ids = torch.tensor(idx, dtype=torch.int32, device="cuda")
    pad = 24  # (a padded output narrower than the image's kp columns: nothing of the padded super-block may land in it)
    out = torch.full((len(idx), (k + pad) * esz), SENT, dtype=torch.uint8, device="cuda").view(tdt)
    gpu.get_rows(W, ids, tdt, out=out)
    got = out.cpu().numpy().view(ndt)
    for s, r in enumerate(idx):
        if 0 <= r < rows:
            assert (got[s, :k] == want[r]).all(), (s, r)
        else:
            assert (got[s, :k] == sent).all(), (s, r)
    assert (got[:, k:] == sent).all()
    for row0, n in ((29, rows - 29), (3, 5), (0, rows)):
        got = gpu.get_rows(W, None, tdt, row0=row0, n=n).cpu().numpy().view(ndt)
        assert (got == want[row0:row0 + n]).all(), (row0, n)
    flat = torch.full(((rows * (k + 1) + 1) * esz,), SENT, dtype=torch.uint8, device="cuda").view(tdt)  # unaligned base and stride
    gpu.get_rows(W, None, tdt, out=flat[1:].view(rows, k + 1))
    g2 = flat.cpu().numpy().view(ndt)
    assert (g2[1:].reshape(rows, k + 1)[:, :k] == want).all()
    assert g2[0] == sent and (g2[1:].reshape(rows, k + 1)[:, k] == sent).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. decode, n = 1 .. 8

@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m", [16, 67, 1030])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_decode_every_column_count(gpu, oracle, t, k, m, gen):
    L = _hip.lib()
    raw = weights(t, m, k, gen)
    Wp = gpu.upload_weights(t | PAD, raw, m, k)                      # the padded image
    We = gpu.upload_weights(t, extend_raw(t, raw, k), m, kp_of(k))   # the unmodified type on the zero-extended matrix
    Wr = gpu.upload_weights(t, raw, m, k)                            # RAW rows: the generic kernel
    assert Wr.data.numel() == m * raw.shape[1] and torch.equal(Wp.data, We.data)
    x8 = synth.random_activations(8, k, 42)
    q8 = quantise(t, x8)
    G8 = yardstick(oracle, t, raw, q8, k)
    xe, qe = extend_x(x8), quantise(t, extend_x(x8))
    bt = T.VEC_DOT[t]
    for n in range(1, 9):
        what = f"{tname(t)} decode {m} x {k} {gen} n={n}"
        assert L.lfamd_mul_mat_is_exact(t | PAD, m, k, n, 0) == 1
        c_f = run(gpu, Wp, f32_rows(x8[:n]), T.F32, n)
        c_q = run(gpu, Wp, q_rows(q8[:n]), bt, n)
        judge(c_f, G8[:n], what + " f32")                                                       # (a)
        judge(c_q, G8[:n], what + " quantised")
        assert rel_err(c_f, c_q) <= 1e-6, what                                                  # (b)
        assert same_bits(c_f, run(gpu, We, f32_rows(xe[:n], slack=False), T.F32, n)), what      # (c)
        assert same_bits(c_q, run(gpu, We, q_rows(qe[:n], slack=False), bt, n)), what
        assert rel_err(c_q, run(gpu, Wr, q_rows(q8[:n]), bt, n)) <= TOL, what                   # (d)
        assert rel_err(c_f, run(gpu, Wr, f32_rows(x8[:n]), T.F32, n)) <= TOL, what
        with pytest.raises(_hip.LfamdError):  # a packed image: not a layout the generic kernels read
            run(gpu, Wp, f32_rows(x8[:n]), T.F32, n, flags=_hip.FLAG_FORCE_GENERIC)


@pytest.mark.parametrize("k", [224, 4000])
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_decode_leaves_the_slack_of_a_wider_result_alone(gpu, oracle, t, k):
    m, n, ldc = 67, 3, 67 + 9
    raw = weights(t, m, k)
    W = gpu.upload_weights(t | PAD, raw, m, k)
    x = synth.random_activations(n, k, 43)
    q = quantise(t, x)
    G = yardstick(oracle, t, raw, q, k)
    for B, bt in ((f32_rows(x), T.F32), (q_rows(q), T.VEC_DOT[t])):
        out = torch.full((n, ldc), float("nan"), dtype=torch.float32, device="cuda")
        c = run(gpu, W, B, bt, n, ldc=ldc, out=out)
        assert np.isnan(c[:, m:]).all()
        judge(c[:, :m], G, f"{tname(t)} decode ldc {k}")


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("k", [288, 8480])
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_sibling_matrices_in_one_decode_launch(gpu, oracle, t, k, count):
    ms = [96, 40, 130][:count]
    raws = [weights(t, m, k, seed=60 + i) for i, m in enumerate(ms)]
    Ws = [gpu.upload_weights(t | PAD, r, m, k) for r, m in zip(raws, ms)]
    x = synth.random_activations(1, k, 44)
    q = quantise(t, x)
    for B, bt in ((f32_rows(x), T.F32), (q_rows(q), T.VEC_DOT[t])):
        fused = gpu.mul_mat_multi(Ws, B, bt, n=1)
        for W, r, f in zip(Ws, raws, fused):
            f = f.cpu().numpy()
            assert rel_err(f, run(gpu, W, B, bt, 1)) <= 1e-6  # (the fused launch's wave layout may differ from the lone matrix's)
            judge(f, yardstick(oracle, t, r, q, k), f"{tname(t)} siblings {count} k={k} m={W.rows}")


class Plan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("variant", "nc", "nw", "ch", "grid", "grid_b", "rows", "lds")]


def test_iq4nl_long_walk_of_32_row_items(gpu):
    """A matrix tall enough that the plan gives the decode launch the 32-row items on this device (k = 288: a few MB)."""
    L = C.CDLL(_hip.HIP_SO)
    L.lfamd_gemv_plan_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(Plan)]
    cus, k, t = torch.cuda.get_device_properties(0).multi_processor_count, 288, T.IQ4_NL
    m = None
    for cand in range(cus * 32, cus * 32 * 40, cus * 32):
        p = Plan()
        if _hip.lib().lfamd_packed_size(t | PAD, cand + 5, k) > 64 << 20:
            break
        if L.lfamd_gemv_plan_of(0, t, 1, (cand + 5 + 31) // 32 * 2, 0, k, 1, cus, C.byref(p)) == 0 and p.variant == 2:
            m = cand + 5  # (a ragged last tile)
            break
    if m is None:
        pytest.skip(f"no IQ4_NL shape under 64 MB takes the 32-row items on {cus} CUs")
    raw = synth.random_weights_torch(t, m, k, 5)
    W = gpu.upload_weights(t | PAD, raw, m, k)
    x = synth.random_activations(1, k, 45)
    q = quantise(t, x)
    c_f, c_q = run(gpu, W, f32_rows(x), T.F32, 1), run(gpu, W, q_rows(q), T.Q8_0, 1)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(64, m, 997), np.arange(m - 64, m)]))
    sub = raw[torch.from_numpy(rows).cuda()].cpu().numpy()
    G = R.dot_ref(sub, q)
    judge(c_f[:, rows], G, f"IQ4_NL 32-row items {m} x {k} f32")
    judge(c_q[:, rows], G, f"IQ4_NL 32-row items {m} x {k} q8_0")
    assert np.isfinite(c_f).all() and rel_err(c_f, c_q) <= 1e-6
    We = gpu.upload_weights(t, torch.cat([raw, torch.zeros((m, 7 * 18), dtype=torch.uint8, device="cuda")], dim=1), m, 512)
    assert same_bits(c_f, run(gpu, We, f32_rows(extend_x(x), slack=False), T.F32, 1))


# ------------------------------------------------------------------------------------------------------------------------
# 4. batches, n > 8

@pytest.mark.parametrize("gen", ["plain", "extreme"])
@pytest.mark.parametrize("m", [67, 300])
@pytest.mark.parametrize("k", [288, 2080, 4000])
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_batches_on_the_mfma_body(gpu, oracle, t, k, m, gen):
    L = _hip.lib()
    raw = weights(t, m, k, gen)
    Wp = gpu.upload_weights(t | PAD, raw, m, k)
    We = gpu.upload_weights(t, extend_raw(t, raw, k), m, kp_of(k))
    xa = synth.random_activations(130, k, 46)
    qa = quantise(t, xa)
    Ga = yardstick(oracle, t, raw, qa, k)
    xe, qe = extend_x(xa), quantise(t, extend_x(xa))
    bt = T.VEC_DOT[t]
    for n in (9, 40, 130):
        what = f"{tname(t)} batch {m} x {k} {gen} n={n}"
        assert L.lfamd_mul_mat_is_exact(t | PAD, m, k, n, 0) == 1
        c_f = run(gpu, Wp, f32_rows(xa[:n]), T.F32, n)
        c_q = run(gpu, Wp, q_rows(qa[:n]), bt, n)
        judge(c_f, Ga[:n], what + " f32")                                                       # (a)
        judge(c_q, Ga[:n], what + " quantised")
        assert same_bits(c_f, run(gpu, We, f32_rows(xe[:n], slack=False), T.F32, n)), what      # (c)
        assert same_bits(c_q, run(gpu, We, q_rows(qe[:n], slack=False), bt, n)), what
        with pytest.raises(_hip.LfamdError):
            run(gpu, Wp, f32_rows(xa[:n]), T.F32, n, flags=_hip.FLAG_FORCE_GENERIC)


@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_batch_workspace_is_exactly_what_the_query_says(gpu, t):
    L = _hip.lib()
    m, k, n = 67, 2080, 40
    W = gpu.upload_weights(t | PAD, weights(t, m, k), m, k)
    B = f32_rows(synth.random_activations(n, k, 47))
    need = L.lfamd_mul_mat_workspace(t | PAD, m, k, n)
    assert need == L.lfamd_mul_mat_workspace(t, m, kp_of(k), n) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, m), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda nbytes: L.lfamd_mul_mat(t | PAD, C.c_void_p(W.data.data_ptr()), m, k, T.F32, C.c_void_p(B.data_ptr()), B.stride(0), n,
                                          C.c_void_p(out.data_ptr()), m, C.c_void_p(ws.data_ptr()), nbytes, 0, st)
    assert call(need) == 0
    assert call(need - 1) == -4  # LFAMD_ERR_WORKSPACE
    assert call(need) == 0
    torch.cuda.synchronize()
    # a row stride below the row's k values is refused whatever the image's kp
    assert L.lfamd_mul_mat(t | PAD, C.c_void_p(W.data.data_ptr()), m, k, T.F32, C.c_void_p(B.data_ptr()), k * 4 - 16, n,
                           C.c_void_p(out.data_ptr()), m, C.c_void_p(ws.data_ptr()), need, 0, st) == -2
    # ... and a staged 32-block image, which the producers write for rows of whole groups only
    assert L.lfamd_mul_mat(t | PAD, C.c_void_p(W.data.data_ptr()), m, k, _hip.TYPE_STAGED_B32, C.c_void_p(ws.data_ptr()), 0, n,
                           C.c_void_p(out.data_ptr()), m, C.c_void_p(ws.data_ptr()), need, 0, st) == -1


# ------------------------------------------------------------------------------------------------------------------------
# 5. MUL_MAT_ID

@pytest.mark.parametrize("tokens_,tasks", [(1, 1), (1, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("t", TYPES, ids=tname)
def test_mul_mat_id_per_expert(gpu, oracle, t, tokens_, tasks):
    rows, cols, experts, thinkers = 96, 288, 4, 2
    Ws = [weights(t, rows, cols, seed=900 + e) for e in range(experts)]
    packed = torch.cat([gpu.upload_weights(t | PAD, W, rows, cols).data for W in Ws])
    assert packed.numel() == experts * _hip.lib().lfamd_packed_size(t, rows, 512)
    x = synth.random_activations(tokens_ * tasks, cols, 77)
    xq = quantise(t, x)
    plan = np.random.default_rng(5).integers(0, experts, size=(tokens_, thinkers)).astype(np.int32)
    if tokens_ > 1:
        plan[-1, -1] = experts + 3  # out of range: its result row stays untouched
    res = gpu.mul_mat_id(packed, t | PAD, rows, cols, experts, q_rows(xq), T.VEC_DOT[t], tasks, tokens_, torch.from_numpy(plan).cuda(),
                         thinkers, prefill=-7.0)
    torch.cuda.synchronize()
    res = res.cpu().numpy()
    for tok in range(tokens_):
        for th in range(thinkers):
            ex = int(plan[tok, th])
            if ex >= experts:
                assert (res[tok, th] == -7.0).all()
                continue
            row = tok * tasks + th % tasks
            judge(res[tok, th][None, :], yardstick(oracle, t, Ws[ex], xq[row:row + 1], cols), f"{tname(t)} mul_mat_id tok {tok} th {th}")


# ------------------------------------------------------------------------------------------------------------------------
# 6. the two integration layers keep their resident copies as the padded image (lfamd_resident_type)

@pytest.mark.parametrize("n", [1, 64])
def test_backend_mul_mat_node_on_a_ragged_q5_0_tensor(gpu, oracle, host_exe, tmp_path, n):
    """GGML_OP_MUL_MAT through the ggml backend interface, a Q5_0 tensor with ne[0] = 288 (f32 src1, quantised on the device)."""
    import subprocess
    t, m, k = T.Q5_0, 96, 288
    raw, x = weights(t, m, k, seed=7), synth.random_activations(n, k, 8)
    wp, xp, op = tmp_path / "w.bin", tmp_path / "x.bin", tmp_path / "o.bin"
    raw.tofile(wp)
    x.tofile(xp)
    r = subprocess.run([host_exe, _hip.HIP_SO, "mulmat", str(t), str(m), str(k), str(n), "1", str(wp), str(xp), str(op)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(op, dtype=np.float32).reshape(n, m)
    judge(got, yardstick(oracle, t, raw, quantise(t, x), k), f"backend Q5_0 {m} x {k} n={n}")
    # the bits of the padded image through the C ABI: the backend packs and calls with lfamd_resident_type's id
    W = gpu.upload_weights(t | PAD, raw, m, k)
    assert same_bits(got, run(gpu, W, f32_rows(x, slack=False), T.F32, n, flags=_hip.FLAG_Q0_VREGS32))


@pytest.mark.parametrize("n", [1, 64])
def test_host_plug_in_registered_ragged_q5_0_weights(gpu, oracle, n):
    """llamafile_sgemm on registered Q5_0 weights of 288 columns: the kept device copy is the padded image."""
    lib = C.CDLL(_hip.HOST_SO)
    lib.llamafile_sgemm.restype = C.c_bool
    lib.llamafile_sgemm.argtypes = [C.c_long] * 3 + [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long] + [C.c_int] * 5
    lib.llamafile_sgemm_amd_register_weights.argtypes = [C.c_void_p, C.c_size_t]
    lib.llamafile_sgemm_amd_unregister_weights.argtypes = [C.c_void_p]
    lib.llamafile_sgemm_amd_cached_bytes.restype = C.c_size_t
    t, m, k = T.Q5_0, 96, 288
    A, x = weights(t, m, k, seed=9), synth.random_activations(n, k, 10)
    B = quantise(t, x)
    G = yardstick(oracle, t, A, B, k)
    kb = k // 32
    base = lib.llamafile_sgemm_amd_cached_bytes()
    lib.llamafile_sgemm_amd_register_weights(A.ctypes.data, A.nbytes)
    try:
        for _ in range(2):  # packed, then served from the kept copy
            out = np.full((n, m), np.nan, dtype=np.float32)
            assert lib.llamafile_sgemm(m, n, kb, A.ctypes.data, kb, B.ctypes.data, kb, out.ctypes.data, m, 0, 1, t, T.Q8_0, T.F32)
            judge(out, G, f"host plug-in Q5_0 {m} x {k} n={n}")
            assert lib.llamafile_sgemm_amd_cached_bytes() - base == _hip.lib().lfamd_packed_size(t | PAD, m, k)
    finally:
        lib.llamafile_sgemm_amd_unregister_weights(A.ctypes.data)
    assert lib.llamafile_sgemm_amd_cached_bytes() == base
