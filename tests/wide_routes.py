"""What tests/test_gemm_wide_plan.py (no GPU) and tests/test_gpu_wide_routes.py share: the binding of the host-only export
lfamd_gemm_wide_plan_of (csrc/gemm_wide.hip), which of the library's own predicates send a call to wide_go on scaled operands,
the shapes whose forms the GPU file runs, their weights, and a NumPy restatement of the scaled arithmetic.

A form is chosen from the tile count alone: T = row blocks of 128 rows x token tiles of 128 (n_ct), k = 256 nb."""
import ctypes as C

import numpy as np

from llamafile_amd import _hip, ggml_types as T, synth
import extremes
import pack_ref
import producer_ref

FORMS = ("kr", "lw128", "lw128_then_lw64", "lw64", "ks", "lw64_ksplit")
KR, LW128, SPLIT, LW64, KS, KSPLIT = range(6)
MAX_MATS = 4
FLAG_GEMM_WIDE = _hip.FLAG_GEMM_WIDE


class Plan(C.Structure):
    _fields_ = [("form", C.c_int), ("rb_cut", C.c_int), ("ksp", C.c_int)]


_lib = None


def plan_lib():
    """The HIP module with the internal exports bound; loading it touches no device."""
    global _lib
    if _lib is None:
        L = C.CDLL(_hip.HIP_SO)
        L.lfamd_gemm_wide_plan_of.restype = C.c_int
        L.lfamd_gemm_wide_plan_of.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_long, C.c_long, C.c_size_t,
                                              C.POINTER(Plan), C.POINTER(C.c_long)]
        L.lfamd_gemm_i8_ok.restype, L.lfamd_gemm_i8_ok.argtypes = C.c_int, [C.c_int, C.c_long, C.c_long]
        L.lfamd_gemm_wide_dual_ok.restype, L.lfamd_gemm_wide_dual_ok.argtypes = C.c_int, [C.c_long, C.c_long, C.c_long]
        L.lfamd_gemm_lw_ksplit_bytes.restype, L.lfamd_gemm_lw_ksplit_bytes.argtypes = C.c_size_t, [C.c_long, C.c_long]
        L.lfamd_mul_mat_is_exact.restype, L.lfamd_mul_mat_is_exact.argtypes = C.c_int, [C.c_int, C.c_long, C.c_long, C.c_long, C.c_uint]
        _lib = L
    return _lib


def n_pad_of(n):
    return (n + 127) // 128 * 128


def row_blocks(ms):
    return sum((m + 127) // 128 for m in ms)


def plan_of(t, ms, nb, n, p_bytes=0, n_pad=None, parts=False):
    """(form, rb_cut, ksp) of a scaled wide launch; with parts also split_mats' two lists of (matrix, first row, rows, weight offset)."""
    p = Plan()
    arr = (C.c_long * len(ms))(*ms)
    out = (C.c_long * (2 * MAX_MATS * 4))() if parts else None
    rc = plan_lib().lfamd_gemm_wide_plan_of(t, len(ms), arr, nb, n, n_pad_of(n) if n_pad is None else n_pad, p_bytes, C.byref(p), out)
    assert rc == 0, (T.NAMES.get(t, t), ms, nb, n, n_pad, p_bytes)
    if not parts:
        return p.form, p.rb_cut, p.ksp
    halves = []
    for h in range(2):
        rows = [tuple(out[(h * MAX_MATS + i) * 4 + f] for f in range(4)) for i in range(MAX_MATS)]
        live = [r for r in rows if r[0] >= 0]
        assert rows[:len(live)] == live, "a list of parts has a hole"
        halves.append(live)
    return (p.form, p.rb_cut, p.ksp), halves[0], halves[1]


def call_form(t, ms, k, n, flags=0):
    """The form of a default lfamd_mul_mat (one matrix) / lfamd_mul_mat_multi (2 .. 4 of one type) call on f32 or Q8_K rows with a
    workspace of exactly the documented size — after asserting, with the library's own predicates, that the call reaches wide_go on
    scaled operands at all: not the int8 body (lfamd_gemm_i8_ok over the launch's row blocks, unless a testing flag keeps it away),
    not an exact body (lfamd_mul_mat_is_exact), more than 32 tokens (gemm_sb takes fewer), and for a fused launch the 192 tiles
    plan_group asks of `wide_multi` (api.hip: wide_group_ok) — fewer and it would be one call per matrix."""
    L = plan_lib()
    assert t in (T.Q4_K, T.Q5_K, T.Q6_K) and n > 32 and k % 256 == 0 and 1 <= len(ms) <= MAX_MATS
    rbs = row_blocks(ms)
    assert flags & FLAG_GEMM_WIDE or not L.lfamd_gemm_i8_ok(t, rbs, n), "the int8 body takes this grid"
    if len(ms) == 1:
        assert L.lfamd_mul_mat_is_exact(t, ms[0], k, n, flags) == 0, "an exact body takes this call"
        return plan_of(t, ms, k // 256, n, L.lfamd_gemm_lw_ksplit_bytes(ms[0], n))
    assert flags & FLAG_GEMM_WIDE or rbs * (n_pad_of(n) // 128) >= 192, "below 192 tiles the matrices run one call each"
    return plan_of(t, ms, k // 256, n, 0)  # (a fused launch has no K-split workspace)


# ---------------------------------------------------------------------------------------------------------------- the GPU cases
# name -> (form, types, rows of each matrix, n, nb, what).  A case with several types runs once per type.
CASES = {
    "kr-28-rows-nb1": (KR, (T.Q4_K,), (11036,), 300, 1, "T = 261; the last 256-row block has 28 rows; last token tile 44; 2 periods < 4 LDS stages"),
    "kr-one-row-one-token": (KR, (T.Q4_K,), (16641,), 129, 3, "T = 262; the last block has ONE row, the last token tile ONE token"),
    "kr-fused": (KR, (T.Q4_K,), (5000, 129, 12000), 200, 4, "T = 272; 256-row rebasing per matrix: a 136-row last block, a matrix below a block"),
    "split-one-matrix-nb1": (SPLIT, (T.Q6_K, T.Q5_K), (38350,), 100, 1, "T = 300, rem 44: cut inside the one matrix, ragged last block in hi"),
    "split-two-token-tiles": (SPLIT, (T.Q5_K,), (19199,), 200, 2, "n_ct = 2, rb_cut = 128"),
    "lw128-no-split": (LW128, (T.Q6_K,), (12800,), 300, 1, "T = 300, rem 44, 44 % 3 != 0: no split"),
    "split-fused-last": (SPLIT, (T.Q6_K,), (20000, 77, 18000), 100, 1, "299 blocks: the cut inside the LAST matrix, skip = 98"),
    "split-fused-boundary": (SPLIT, (T.Q5_K,), (32768, 5000), 100, 1, "the cut ON a matrix boundary: lo = matrix 0, hi = matrix 1"),
    "split-fused-first": (SPLIT, (T.Q6_K,), (40000, 300), 100, 2, "the cut inside matrix 0: hi = its rest + all of matrix 1"),
}
# the kr launch below 257 tiles: two Q4_K matrices on the STAGED_SCALED image.  Their grid is one the int8 body takes, which a
# staged-scaled call answers with LFAMD_ERR_UNSUPPORTED; LFAMD_FLAG_GEMM_WIDE keeps the int8 body away (api.hip: i8_takes).
KR_STAGED = (KR, T.Q4_K, (9000, 3333), 150, 2)  # 71 + 27 row blocks x 2 token tiles = 196
# two types in one launch (lfamd_lw_dual_go): 79 + 55 row blocks, one token tile = 134 tiles, both groups ragged
DUAL = ((T.Q4_K, T.Q6_K), (T.Q5_K, T.Q6_K)), (10001, 7000), 100, 3


def case_ids():
    return [f"{name}-{T.NAMES[t]}" for name, c in CASES.items() for t in c[1]]


def case_list():
    return [(name, t) for name, c in CASES.items() for t in c[1]]


# ---------------------------------------------------------------------------------------------------------------------- weights
def route_weights(t, m, k, seed, control=False):
    """extremes.extreme_weights (bands by row % 8: codes at minimum / maximum, sub-block scales at maximum / most negative) with block
    overrides that do not depend on the block index, so that they exist at one super-block too: over the LAST 40 rows of the matrix
    (the ragged tile of every case) and rows 120 .. 135 (a 128-row edge inside), row r gets d < 0 in every block when r % 4 = 1,
    dmin < 0 when r % 4 = 2 (Q4_K, Q5_K), and the last row but two is all zero (d = dmin = 0).  control: synth.random_weights.
    Both end in `representable`."""
    if control:
        return representable(t, synth.random_weights(t, m, k, seed).copy())
    raw = extremes.extreme_weights(t, m, k, seed)
    blk = extremes._blocks(raw, t)
    rows = np.array(sorted(set(range(max(0, m - 40), m)) | set(range(min(120, m), min(136, m)))))
    d = extremes._get_f16(blk, extremes.D_OFF[t])
    d[rows[rows % 4 == 1]] *= -1.0
    if m >= 3:
        d[m - 3] = 0.0
    extremes._put_f16(blk, extremes.D_OFF[t], d)
    if extremes.M_OFF[t] is not None:
        mm = extremes._get_f16(blk, extremes.M_OFF[t])
        mm[rows[rows % 4 == 2]] *= -1.0
        if m >= 3:
            mm[m - 3] = 0.0
        extremes._put_f16(blk, extremes.M_OFF[t], mm)
    return representable(t, raw)


def representable(t, raw):
    """Make the f16 operands of the scaled bodies exactly representable, so that the arithmetic's own rounding stays below half the
    project's bounds at k = 256 .. 1024 (profiles/wide_routes_model_error.txt has the figures before and after): d and dmin keep
    sign and exponent and lose their mantissa (a power of two, zero stays zero), so d sc q of Q4_K / Q5_K (at most 6 + 5 bits) and
    dmin m (6 bits) are exact in f16's 11; Q6_K's sc (q - 32) has up to 13 bits, so its codes lose their low bit (2 sc j with
    |sc j| <= 2048 is exact; the band of maximal codes holds 62, not 63)."""
    blk = extremes._blocks(raw, t)
    for off in (extremes.D_OFF[t], extremes.M_OFF[t]):
        if off is not None:
            v = extremes._get_f16(blk, off)
            _, e = np.frexp(np.abs(v))
            extremes._put_f16(blk, off, np.where(v != 0, np.sign(v) * np.ldexp(np.float32(0.5), e), 0).astype(np.float32))
    if t == T.Q6_K:
        blk[:, :, 0:128] &= 0xEE  # ql: bit 0 of both nibbles = the low bit of two codes
    return raw


def route_activations(n, k, seed):
    """f32 [n, k] whose Q8_K blocks and scaled image are exact: every 256-block holds one element of the token's largest magnitude,
    -2^s with s = token % 5 - 2, the rest stay below it, so d = 2^s / 128 and the staged f16(code d 2^-e) = 4 code."""
    x = np.clip(synth.random_activations(n, k, seed), -0.999, 0.999).astype(np.float32)
    xb = x.reshape(n, k // 256, 256)
    pos = np.random.default_rng(seed).integers(0, 256, (n, k // 256))
    np.put_along_axis(xb, pos[..., None], np.float32(-1.0), axis=2)
    return x * np.ldexp(np.float32(1.0), np.arange(n) % 5 - 2).astype(np.float32)[:, None]


# ------------------------------------------------------------------------------------------- the scaled arithmetic, restated
def _f16(blk, off):
    return np.ascontiguousarray(blk[..., off:off + 2]).view(np.float16)[..., 0].astype(np.float32)


def _scale_min_k4(sc12):
    q = sc12.astype(np.int32)
    sc = np.empty(q.shape[:-1] + (8,), np.int32)
    mn = np.empty_like(sc)
    sc[..., :4] = q[..., 0:4] & 63
    mn[..., :4] = q[..., 4:8] & 63
    sc[..., 4:] = (q[..., 8:12] & 0xF) | ((q[..., 0:4] >> 6) << 4)
    mn[..., 4:] = (q[..., 8:12] >> 4) | ((q[..., 4:8] >> 6) << 4)
    return sc, mn


def q5k_codes(raw, nb):
    """raw [rows, nb * 176] -> codes [rows, nb, 256] (0 .. 31) and headers [rows, nb, 16]."""
    rows = raw.shape[0]
    blk = raw.reshape(rows, nb, 176)
    qh = blk[:, :, 16:48]
    qs = blk[:, :, 48:].reshape(rows, nb, 4, 32)
    codes = np.empty((rows, nb, 4, 64), dtype=np.uint8)
    for j in range(4):
        codes[:, :, j, :32] = (qs[:, :, j] & 15) | (((qh >> (2 * j)) & 1) << 4)
        codes[:, :, j, 32:] = (qs[:, :, j] >> 4) | (((qh >> (2 * j + 1)) & 1) << 4)
    return codes.reshape(rows, nb, 256), blk[:, :, :16]


def scaled_weight_operands(t, raw, k):
    """The f16 operands the scaled bodies multiply: Wh = f16(d sc q) [rows, k] (Q6_K: q - 32) and, for Q4_K / Q5_K, the mins
    weights f16(-dmin m) [rows, nb, 8] (else None).  One f16 rounding of an f32 product each."""
    rows, nb, f = raw.shape[0], k // 256, np.float32
    if t == T.Q6_K:
        codes, sc, dd = pack_ref.q6k_codes(raw, nb)
        dl = (_f16(dd, 0)[..., None] * sc.view(np.int8).astype(f)).astype(f)  # [rows, nb, 16]
        q = (codes.astype(np.int32) - 32).reshape(rows, nb, 16, 16).astype(f)
        return (dl[..., None] * q).astype(f).astype(np.float16).reshape(rows, k), None
    codes, hdr = pack_ref.q4k_codes(raw, nb) if t == T.Q4_K else q5k_codes(raw, nb)
    d, dmin = _f16(hdr, 0), _f16(hdr, 2)
    sc, mn = _scale_min_k4(hdr[..., 4:16])
    dl = (d[..., None] * sc.astype(f)).astype(f)
    wh = (dl[..., None] * codes.reshape(rows, nb, 8, 32).astype(f)).astype(f).astype(np.float16).reshape(rows, k)
    wm = (-dmin[..., None] * mn.astype(f)).astype(f).astype(np.float16)
    return wh, wm


def scaled_model(t, raw, k, x, q8k_rows):
    """C[token, row] of the scaled bodies, restated: f16(d sc q) x f16(d8 code 2^-e) summed in f64, the mins as f16(-dmin m) x
    f16(d8 bsum 2^-e), times the token scale 2^e (producer_ref.scaled_image_model gives the activation side)."""
    xh, tok, xm = producer_ref.scaled_image_model(x, q8k_rows)
    wh, wm = scaled_weight_operands(t, raw, k)
    n = x.shape[0]
    acc = xh.reshape(n, k).astype(np.float64) @ wh.astype(np.float64).T
    if wm is not None:
        acc += xm[:, :, :8].reshape(n, -1).astype(np.float64) @ wm.reshape(raw.shape[0], -1).astype(np.float64).T
    return acc * tok.astype(np.float64)[:, None]


# ---------------------------------------------------------------------------------------------------------- inputs and figures
SCALED_TOL, ELEM_RTOL = 1e-3, 1.5e-3  # the project's bounds of the scaled bodies (tests/test_gpu_parity.py, test_gpu_full_size.py)


def inputs(ms, t_of, n, k, seed, control=False):
    """(raw GGUF rows per matrix, x f32 [n, k], its Q8_K rows): what the GPU test and tools/wide_routes_model_error.py both use.
    t_of: one type, or one per matrix."""
    ts = t_of if isinstance(t_of, (list, tuple)) else [t_of] * len(ms)
    raws = [route_weights(t, m, k, seed + 17 * j, control) for j, (t, m) in enumerate(zip(ts, ms))]
    x = route_activations(n, k, seed + 1000)
    return raws, x, synth.quantize_activations(T.Q8_K, x)


def seed_of(name):
    return 9000 + 100 * sorted(list(CASES) + ["kr-staged", "dual"]).index(name)


def figures(C, G):
    """(normwise error, fraction of elements beyond ELEM_RTOL (|G| + rms), worst element) of C against the oracle's G."""
    G = np.asarray(G, np.float64)
    C = np.asarray(C, np.float64)
    rms = float(np.sqrt(np.mean(G * G))) or 1e-30
    d = np.abs(C - G)
    return (float(d.max() / max(np.abs(G).max(), 1e-30)), float(np.mean(d > ELEM_RTOL * np.abs(G) + ELEM_RTOL * rms)),
            float((d / (np.abs(G) + rms)).max()))


# every run of the GPU file: (case, type, control weights?) — one synth.random_weights control per form
RUNS = [(name, t, False) for name, t in case_list()] + [("kr-28-rows-nb1", T.Q4_K, True), ("split-one-matrix-nb1", T.Q6_K, True),
                                                        ("lw128-no-split", T.Q6_K, True)]


def run_id(r):
    return f"{r[0]}-{T.NAMES[r[1]]}" + ("-control" if r[2] else "")
