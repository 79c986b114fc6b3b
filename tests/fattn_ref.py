"""References for lfamd_flash_attn (include/lfamd_hip.h): the f64 value of the call on the operands as each route sees them, a numpy
emulation of each route's arithmetic, the test inputs, and the per-row error measure

    err = ||dst - ref||_2 / ||a||_2,   a_l = sum_t p_t |V[t][l]| / sum_t p_t   (f64)

whose denominator does not collapse when the weighted V values cancel.

Shapes: Q f32 [ne3][n_head][n_q][D], K / V f16 [ne3][n_head_kv][n_kv][D], mask f32 [n_q][n_kv] (finite f16 values or -inf) or None,
results [ne3][n_q][n_head][D] (ggml's order: heads inside tokens)."""
import numpy as np

LOG2E = np.float32(1.44269504088896340736)
CHUNK = 256       # keys per work-group of the decode route (csrc/flash_attn.hip: LFAMD_FA_CHUNK)
TOL_MMA = 1e-3    # the n_q > 8 route: BASELINE's north-star tolerance, what this project holds its f16-operand bodies to
# The n_q <= 8 route: 4 x the f32 emulation's largest error against the f64 reference over decode_cases(), never below 2e-6
# (tests/test_fattn_ref.py computes it and compares; measured largest error 2.53e-06 -> 1.01e-05, rounded up).
TOL_F32 = 1.1e-5


def route_of(n_q):
    return "decode" if n_q <= 8 else "prefill"


def _expand(K, group):
    return np.repeat(K, group, axis=1)


def ref64(Q, K, V, mask, scale, route):
    """(value, a): the f64 value [ne3][n_q][n_head][D] of the call whose Q is the route's (rounded to f16 for 'prefill'), and the
    error measure's denominator vector a."""
    group = Q.shape[1] // K.shape[1]
    Qr = Q.astype(np.float16).astype(np.float64) if route == "prefill" else Q.astype(np.float64)
    Kx, Vx = _expand(K.astype(np.float64), group), _expand(V.astype(np.float64), group)
    s = np.float64(np.float32(scale)) * np.einsum("bhjd,bhtd->bhjt", Qr, Kx)
    if mask is not None:
        s = s + mask.astype(np.float64)[None, None]
    p = np.exp(s - s.max(-1, keepdims=True))
    l = p.sum(-1)[..., None]
    out = np.einsum("bhjt,bhtd->bhjd", p, Vx) / l
    a = np.einsum("bhjt,bhtd->bhjd", p, np.abs(Vx)) / l
    return out.transpose(0, 2, 1, 3), a.transpose(0, 2, 1, 3)


def emulate(Q, K, V, mask, scale, route):
    """The route's arithmetic in numpy: f32 sums and an f32 exp2 ('decode'); Q and p rounded once to f16, f32 sums, the row sum from
    the f32 p ('prefill').  Scores in log2 units, scale * log2 e folded into one factor, as the kernels do."""
    group = Q.shape[1] // K.shape[1]
    Qr = Q.astype(np.float16).astype(np.float32) if route == "prefill" else Q.astype(np.float32)
    Kx, Vx = _expand(K.astype(np.float32), group), _expand(V.astype(np.float32), group)
    c = np.float32(np.float32(scale) * LOG2E)
    s = np.einsum("bhjd,bhtd->bhjt", Qr, Kx, dtype=np.float32) * c
    if mask is not None:
        s = s + (mask.astype(np.float32) * LOG2E)[None, None]
    p = np.exp2((s - s.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
    l = p.sum(-1, dtype=np.float32)[..., None]
    pv = p.astype(np.float16).astype(np.float32) if route == "prefill" else p
    out = np.einsum("bhjt,bhtd->bhjd", pv, Vx, dtype=np.float32) / l
    return out.transpose(0, 2, 1, 3).astype(np.float32)


def row_err(dst, ref, a):
    """The largest per-(i3, j, h) error of dst against ref."""
    d = np.asarray(dst, np.float64) - ref
    return float((np.linalg.norm(d, axis=-1) / np.maximum(np.linalg.norm(a, axis=-1), 1e-300)).max())


# ---- test inputs
def onehot_keys(kind, n_q, n_kv):
    """The one live key t_j of every row of an 'onehot' / 'diag' mask.  'diag': t_j = j (n_q == n_kv).  'onehot' on the decode route
    (n_q <= 8): the first and the last key, both sides of the first chunk edge, the middle, and their neighbours; on the prefill route
    t_j = (7 j + 3) % n_kv, so that neighbouring rows land in different 32-key halves and tiles."""
    if kind == "diag":
        assert n_q == n_kv
        return np.arange(n_q)
    if n_q <= 8:
        picks = [0, n_kv - 1, CHUNK - 1, CHUNK, n_kv // 2, 1, n_kv - 2, CHUNK + 1]
        return np.minimum(np.array(picks[:n_q]), n_kv - 1)
    return (7 * np.arange(n_q) + 3) % n_kv


def make_mask(kind, n_q, n_kv, rng):
    """None / 'bias' (finite f16 values) / 'causal' (-inf above the diagonal, the diagonal offset by off = n_kv - n_q) / 'causal70'
    (causal, and the first 70 keys -inf for the odd rows that keep a live key behind them: a leading fully masked tile of the prefill
    route; a decode chunk has 256 keys, so these 70 kill none).  Masks of 0 and -inf that leave whole chunks, tiles and segments dead:
      'window:W'   key t is live for row j iff j + off - W < t <= j + off
      'causal0'    causal with off = 0, a prompt on an empty cache ('window' with W = n_kv and off = 0)
      'onehot', 'diag'  row j sees the one key onehot_keys()[j]
      'tiles:a,b,..'  only the keys of the listed 64-key tiles are live; the rows of wave 1 (32 .. 63 of each 128) are live only in
                   the second 32-key half of the second listed tile
      'head:N', 'tail:N'  only the first / the last N keys are live, for every row
    Every row keeps a live key."""
    if kind is None:
        return None
    if kind == "bias":
        return rng.standard_normal((n_q, n_kv)).astype(np.float16).astype(np.float32)
    name, _, arg = kind.partition(":")
    off = max(n_kv - n_q, 0)
    j, t = np.arange(n_q)[:, None], np.arange(n_kv)[None, :]
    if name in ("causal", "causal70"):
        live = t <= j + off
        if name == "causal70":
            live = live & ~((j % 2 == 1) & (j + off >= 70) & (t < 70))
    elif name == "window":
        live = (t > j + off - int(arg)) & (t <= j + off)
    elif name == "causal0":
        live = t <= j
    elif name in ("onehot", "diag"):
        live = t == onehot_keys(name, n_q, n_kv)[:, None]
    elif name == "tiles":
        tiles = sorted(int(x) for x in arg.split(","))
        live = np.isin(t // 64, tiles) & (j >= 0)
        wave1 = (j % 128) // 32 == 1
        live = np.where(wave1, (t // 64 == tiles[1]) & (t % 64 >= 32), live)
    elif name == "head":
        live = (t < int(arg)) & (j >= 0)
    elif name == "tail":
        live = (t >= n_kv - int(arg)) & (j >= 0)
    else:
        raise ValueError(kind)
    m = np.where(live, np.float32(0), np.float32(-np.inf)).astype(np.float32)
    assert np.isfinite(m).any(axis=1).all()
    return m


def make_inputs(D, kvh, group, ne3, n_q, n_kv, mask=None, extreme=None, seed=0, q_gain=4.0, scale=None):
    """extreme: 'first' / 'last' — one key whose score is about +60, at the start / the end (the late spike: the rescale path);
    'low' — every score near -60.  Built on component 0: Q[..., 0] = 8, K[t][0] = +-60 / (8 scale); the other components of Q then keep
    unit gain (an f32 score of magnitude 60 * log2 e carries an absolute error of 2^-18, which is what bounds TOL_F32 from below).
    scale: the call's scale in place of 1 / sqrt(D) (not with extreme)."""
    rng = np.random.default_rng(seed)
    Q = (rng.standard_normal((ne3, kvh * group, n_q, D)) * (1.0 if extreme else q_gain)).astype(np.float32)
    K = rng.standard_normal((ne3, kvh, n_kv, D)).astype(np.float16)
    V = rng.standard_normal((ne3, kvh, n_kv, D)).astype(np.float16)
    assert scale is None or not extreme
    scale = np.float32(1.0 / np.sqrt(D)) if scale is None else np.float32(scale)
    if extreme:
        Q[..., 0] = 8.0
        big = np.float16(60.0 / (8.0 * scale))
        if extreme == "first":
            K[:, :, 0, 0] = big
        elif extreme == "last":
            K[:, :, n_kv - 1, 0] = big
        else:
            K[:, :, :, 0] = (-big + K[:, :, :, 0].astype(np.float32)).astype(np.float16)
    return Q, K, V, make_mask(mask, n_q, n_kv, rng), scale


def decode_cases():
    """(D, kv heads, group, ne3, n_q, n_kv, mask, extreme): a pairwise subset.  n_kv crosses 1, a partial load, the chunk edge from
    both sides and several chunks; (2, 4) at n_q = 1 / 2 is the shared-read branch, at n_q = 8 the one-head-per-item branch."""
    C = CHUNK
    return [
        (128, 1, 1, 1, 1, 1, None, None), (64, 3, 1, 2, 2, 1, "bias", None),
        (128, 2, 4, 1, 1, 33, "bias", None), (64, 2, 4, 2, 2, 33, None, None),
        (64, 1, 1, 1, 8, C - 1, "causal", None), (128, 3, 1, 1, 2, C - 1, None, None),
        (128, 2, 4, 1, 2, C + 1, "causal", None), (64, 3, 1, 1, 1, C + 1, "bias", None),
        (128, 2, 4, 2, 1, 3 * C + 7, None, None), (64, 2, 4, 1, 8, 3 * C + 7, "causal70", None),
        (128, 1, 1, 1, 8, 3 * C + 7, "causal70", None), (64, 1, 1, 2, 1, 3 * C + 7, "bias", None),
        (128, 3, 1, 1, 8, 33, "causal", None), (128, 2, 4, 1, 8, C + 1, "bias", None),
        (128, 2, 4, 1, 1, 3 * C + 7, None, "first"), (64, 2, 4, 1, 2, 3 * C + 7, "bias", "last"),
        (128, 1, 1, 1, 8, C + 1, None, "low"), (64, 3, 1, 1, 1, 33, None, "last"),
    ]


def prefill_cases():
    """n_q crosses a wave's 32 rows, one wave with a ragged edge, two work-groups; n_kv a partial half tile, one and several tiles."""
    return [
        (128, 1, 1, 1, 9, 1, None, None), (64, 2, 4, 1, 9, 31, "bias", None),
        (64, 3, 1, 2, 16, 33, "causal", None), (128, 2, 4, 1, 16, 65, None, None),
        (128, 3, 1, 1, 17, 257, "causal70", None), (64, 1, 1, 2, 17, 1000, "bias", None),
        (64, 2, 4, 1, 33, 1, "bias", None), (128, 1, 1, 2, 33, 31, None, None),
        (128, 2, 4, 1, 33, 257, "causal", None), (64, 3, 1, 1, 33, 1000, "causal70", None),
        (128, 3, 1, 2, 65, 33, "causal", None), (64, 1, 1, 1, 65, 65, "causal", None),
        (64, 2, 4, 1, 65, 257, "causal70", None), (128, 1, 1, 1, 65, 1000, "causal", None),
        (64, 1, 1, 1, 130, 31, None, None), (128, 2, 4, 1, 130, 65, "bias", None),
        (128, 1, 1, 1, 130, 257, "causal70", None), (64, 2, 4, 2, 130, 1000, "causal", None),
        (128, 2, 4, 1, 130, 1000, "causal70", None),
        (128, 2, 4, 1, 33, 257, None, "first"), (64, 1, 1, 1, 65, 1000, "bias", "last"),
        (128, 3, 1, 1, 17, 257, None, "low"), (64, 2, 4, 1, 130, 65, None, "last"),
    ]


def decode_edge_cases():
    """The control paths decode_cases() leaves without an execution (its n_q is 1, 2 or 8 and its group 1 or 4, so the live column
    count always equals the kernel's NC and is a power of two; its longest n_kv has 4 chunks, none of them dead).
    Column counts 3, 5, 6, 7 on both branches and both D, 8 columns from one row, group 8 x 2 rows (one head per item); then 10
    chunks (more than the combine's G = 8 / 4 groups), 512 chunks (one full tile of the combine), 513 (a second tile of one chunk),
    dead chunks in front ('window:40'), behind ('head:5') and around single keys ('onehot')."""
    C = CHUNK
    cols = [
        (128, 2, 3, 1, 1, 33, "bias"), (64, 1, 3, 1, 2, C + 1, "causal"), (128, 1, 5, 1, 1, C - 1, None), (64, 2, 7, 1, 1, 3 * C + 7, "bias"),
        (128, 1, 8, 1, 1, 33, None), (64, 1, 8, 2, 2, C + 1, "bias"), (128, 2, 2, 1, 3, 33, "causal"), (64, 3, 1, 1, 3, 3 * C + 7, "causal70"),
        (128, 1, 4, 1, 5, C + 1, "bias"), (64, 2, 1, 1, 6, 33, None), (128, 1, 2, 1, 7, 3 * C + 7, "causal"),
    ]
    chunks = [
        (64, 1, 1, 1, 2, 9 * C + 1, "bias"), (128, 2, 4, 1, 1, 9 * C + 1, None), (128, 1, 1, 1, 2, 512 * C, None),
        (64, 1, 1, 1, 1, 513 * C + 5, "bias"), (128, 1, 1, 1, 2, 513 * C + 5, None), (64, 2, 4, 1, 2, 3 * C + 7, "window:40"),
        (128, 1, 1, 1, 8, 9 * C + 1, "head:5"), (64, 1, 1, 1, 8, 3 * C + 7, "onehot"),
    ]
    return [c + (None,) for c in cols + chunks]


def prefill_edge_cases():
    """The skip logic of the prefill route beyond a causal mask whose diagonal ends at the last key: trailing dead tiles ('causal0'),
    tiles that are dead for a work-group's last rows and live for earlier ones ('window'), runs of dead tiles between live ones and a
    tile that one wave sees half of ('tiles'), single keys ('onehot', 'diag'), one live tile at either end ('head', 'tail'; n_q = 129:
    a work-group of one row).  Then the 128-tile segments of the live flags (D = 64, one head, 9 rows): exactly one segment, a second
    segment of one tile with one key, and segments without a live tile in front ('tail'), behind ('head') and but for their last
    tile ('window:100' at 8257 keys: tile 127 of segment 0, tiles 0 and 1 of segment 1)."""
    skips = [
        (128, 1, 1, 1, 257, 257, "causal0"), (64, 2, 4, 1, 130, 130, "causal0"), (64, 2, 4, 1, 300, 300, "window:40"),
        (128, 1, 1, 1, 130, 1000, "window:40"), (64, 1, 1, 1, 130, 1000, "tiles:1,5,6,12"), (128, 2, 4, 1, 65, 1000, "tiles:0,15"),
        (64, 1, 1, 1, 200, 200, "diag"), (128, 2, 4, 1, 33, 257, "onehot"), (64, 1, 1, 1, 17, 1000, "head:5"),
        (128, 1, 1, 1, 129, 1000, "tail:3"),
    ]
    segments = [
        (64, 1, 1, 1, 9, 8192, None), (64, 1, 1, 1, 9, 8193, "bias"), (64, 1, 1, 1, 9, 16449, "tail:100"), (64, 1, 1, 1, 9, 16449, "head:100"),
        (64, 1, 1, 1, 9, 8257, "window:100"), (64, 1, 1, 1, 9, 16449, "tail:60"),
    ]
    return [c + (None,) for c in skips + segments]


def scale_cases():
    """(case, scale): a zero and a negative scale on either route."""
    return [(c, s) for c in ((64, 1, 1, 1, 2, CHUNK + 1, None, None), (64, 1, 1, 1, 17, 65, None, None)) for s in (0.0, -0.125)]


def case_id(c):
    D, kvh, group, ne3, n_q, n_kv, mask, extreme = c
    return f"D{D}-h{kvh}x{group}-b{ne3}-q{n_q}-kv{n_kv}-{mask or 'nomask'}" + (f"-{extreme}" if extreme else "")


def inputs_of(c, seed=0, scale=None):
    D, kvh, group, ne3, n_q, n_kv, mask, extreme = c
    return make_inputs(D, kvh, group, ne3, n_q, n_kv, mask, extreme, seed, scale=scale)
