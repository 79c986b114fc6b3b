"""lfamd_flash_attn without a device: the references the device tests rely on (tests/fattn_ref.py) against each other, the tolerance
of the n_q <= 8 route, and every refusal of the call in the order include/lfamd_hip.h states — with a NULL stream and bogus non-NULL
pointers, so a refusal that came after a device call would fault instead of answering."""
import numpy as np
import pytest

import fattn_ref as R
from llamafile_amd import _hip, ggml_types as T

OK, UNSUPPORTED, INVALID, WORKSPACE = 0, -1, -2, -4


# ---- the references
@pytest.fixture(scope="module")
def decode_figures():
    """Per decode case: the emulation's error against the f64 reference, and how far the two routes' f64 references lie apart."""
    out = []
    for c in R.decode_cases():
        Q, K, V, mask, scale = R.inputs_of(c)
        ref, a = R.ref64(Q, K, V, mask, scale, "decode")
        other, _ = R.ref64(Q, K, V, mask, scale, "prefill")
        out.append((c, R.row_err(R.emulate(Q, K, V, mask, scale, "decode"), ref, a), R.row_err(other, ref, a)))
    return out


def test_prefill_emulation_is_within_half_the_tolerance():
    """The route's own error: 2^-11 for the one rounding of p, plus about D * 2^-24 * scale * sum |q k| for the f32 score."""
    for c in R.prefill_cases():
        Q, K, V, mask, scale = R.inputs_of(c)
        ref, a = R.ref64(Q, K, V, mask, scale, "prefill")
        err = R.row_err(R.emulate(Q, K, V, mask, scale, "prefill"), ref, a)
        print(R.case_id(c), err)
        assert err < R.TOL_MMA / 2, R.case_id(c)


def test_decode_tolerance_is_four_times_the_emulations_error(decode_figures):
    worst = max(e for _, e, _ in decode_figures)
    want = max(4 * worst, 2e-6)
    print("largest emulation error", worst, "-> TOL_F32 >=", want)
    assert want <= R.TOL_F32 <= 1.25 * want  # the constant is this figure, rounded up
    assert R.TOL_F32 <= 2e-5


def test_the_two_routes_references_lie_apart(decode_figures):
    """A decode route that rounded Q to f16 would miss TOL_F32 by a factor of ten on every input that has more than one key to weigh
    (one key, or one key at +60, gets all the weight whatever Q is; scores near -60 are built on a component f16 holds exactly)."""
    seen = 0
    for c, _, apart in decode_figures:
        if c[5] >= 33 and c[7] is None:
            print(R.case_id(c), apart)
            assert apart >= 10 * R.TOL_F32, R.case_id(c)
            seen += 1
    assert seen >= 10


def test_masks_keep_a_live_key_in_every_row_and_a_dead_first_tile():
    m = R.make_mask("causal70", 17, 257, np.random.default_rng(0))
    assert np.isinf(m[1, :70]).all() and np.isfinite(m[0, 0]) and np.isfinite(m).any(axis=1).all()
    assert np.isinf(m[1, :R.CHUNK]).sum() >= 70


# ---- the edge cases (fattn_ref.decode_edge_cases / prefill_edge_cases / scale_cases)
def test_edge_case_ids_are_new_and_distinct():
    old = {R.case_id(c) for c in R.decode_cases() + R.prefill_cases()}
    new = [R.case_id(c) for c in R.decode_edge_cases() + R.prefill_edge_cases()]
    assert len(set(new)) == len(new) and not old & set(new)
    assert all(R.route_of(c[4]) == "decode" for c in R.decode_edge_cases())
    assert all(R.route_of(c[4]) == "prefill" for c in R.prefill_edge_cases())


def test_decode_edge_cases_keep_the_margin_the_tolerance_was_derived_with():
    """TOL_F32 is 4 x the emulation's largest error over decode_cases(); every new input stays within that figure."""
    for c, scale in [(c, None) for c in R.decode_edge_cases()] + [cs for cs in R.scale_cases() if R.route_of(cs[0][4]) == "decode"]:
        Q, K, V, mask, scale = R.inputs_of(c, scale=scale)
        ref, a = R.ref64(Q, K, V, mask, scale, "decode")
        err = R.row_err(R.emulate(Q, K, V, mask, scale, "decode"), ref, a)
        print(R.case_id(c), float(scale), err)
        assert err <= R.TOL_F32 / 4, R.case_id(c)


def test_prefill_edge_cases_emulate_within_half_the_tolerance():
    for c, scale in [(c, None) for c in R.prefill_edge_cases()] + [cs for cs in R.scale_cases() if R.route_of(cs[0][4]) == "prefill"]:
        Q, K, V, mask, scale = R.inputs_of(c, scale=scale)
        ref, a = R.ref64(Q, K, V, mask, scale, "prefill")
        err = R.row_err(R.emulate(Q, K, V, mask, scale, "prefill"), ref, a)
        print(R.case_id(c), float(scale), err)
        assert err < R.TOL_MMA / 2, R.case_id(c)


def edge_mask(kind, n_q, n_kv):
    return np.isfinite(R.make_mask(kind, n_q, n_kv, np.random.default_rng(0)))


def blocks(live, width):
    """live [n_q][n_kv] -> [n_q][blocks of `width` keys]: the row has a live key in the block."""
    n_q, n_kv = live.shape
    pad = np.zeros((n_q, -n_kv % width), bool)
    return np.concatenate([live, pad], axis=1).reshape(n_q, -1, width).any(axis=2)


def test_decode_edge_masks_have_the_dead_chunks_claimed():
    C = R.CHUNK
    w = blocks(edge_mask("window:40", 2, 3 * C + 7), C)
    assert not w[:, :2].any() and w[:, 2:].all()  # chunks 0 and 1 entirely -inf, 2 and 3 live for both rows
    h = blocks(edge_mask("head:5", 8, 9 * C + 1), C)
    assert h[:, 0].all() and not h[:, 1:].any() and h.shape[1] == 10
    o = edge_mask("onehot", 8, 3 * C + 7)
    assert (o.sum(axis=1) == 1).all()
    assert list(np.argmax(o, axis=1)) == [0, 3 * C + 6, C - 1, C, (3 * C + 7) // 2, 1, 3 * C + 5, C + 1]
    assert blocks(edge_mask("causal70", 8, 3 * C + 7), C)[:, 0].all()  # the 70 keys of 'causal70' kill no chunk of 256


def test_tiles_masks_have_dead_tiles_for_every_row_and_one_half_tile_for_wave_1():
    for n_q, tiles in ((130, [1, 5, 6, 12]), (65, [0, 15])):
        live = edge_mask("tiles:" + ",".join(map(str, tiles)), n_q, 1000)
        t64, t32 = blocks(live, 64), blocks(live, 32)
        dead = [t for t in range(16) if t not in tiles]
        assert not t64[:128, dead].any()                      # dead for all rows of the first work-group (and of the second)
        assert not t64[:, dead].any()
        for t in tiles:
            assert t64[:32, t].all() and t64[64:, t].all()    # waves 0, 2, 3 (and the second work-group): every listed tile
        w1 = t32[32:64]
        assert w1[:, 2 * tiles[1] + 1].all() and w1.sum(axis=1).max() == 1  # wave 1: one 32-key half of one tile


def test_window_and_causal0_masks_are_not_decided_by_a_work_groups_last_eight_rows():
    """A scan of the mask that looked at the last eight rows of a work-group alone would pass every causal mask whose diagonal ends
    at the last key.  'window': some tile is dead for those rows and live for an earlier one, and some tile the other way round.
    'causal0' (later rows see more keys, so no tile can be dead for the last rows and live before them): tiles live for the last
    rows and dead for the first row, and dead tiles behind the last live one for every work-group but the last."""
    for kind, n_q, n_kv in (("window:40", 300, 300), ("window:40", 130, 1000), ("causal0", 257, 257), ("causal0", 130, 130)):
        t64 = blocks(edge_mask(kind, n_q, n_kv), 64)
        wg = t64[:128]
        last8, earlier = wg[-8:].any(axis=0), wg[:-8].any(axis=0)
        assert (last8 & ~wg[0]).any(), kind
        if kind == "causal0":
            assert not wg[:, 2:].any() and t64.shape[1] > 2   # trailing dead tiles
        else:
            assert (~last8 & earlier).any(), (kind, n_q)
    # a tile that is live for the work-group and dead for three of its four waves: tile 12 of the 130 x 1000 window (row 0 alone)
    t64 = blocks(edge_mask("window:40", 130, 1000), 64)
    assert t64[0, 12] and not t64[32:128, 12].any()
    # a run of several dead tiles between two live ones
    assert "".join("x" if v else "." for v in blocks(edge_mask("tiles:1,5,6,12", 130, 1000), 64)[0]) == ".x...xx.....x..."


def test_segment_masks_have_the_dead_segments_claimed():
    """Tiles per segment of the live flags: 128.  16449 keys are 258 tiles: segments of 128, 128 and 2 tiles, the last tile of one key."""
    def segs(kind, n_kv):
        t64 = blocks(edge_mask(kind, 9, n_kv), 64).any(axis=0)
        return [t64[s:s + 128] for s in range(0, len(t64), 128)]
    s = segs("tail:60", 16449)
    assert len(s) == 3 and not s[0].any() and not s[1].any() and s[2].all() and len(s[2]) == 2
    s = segs("tail:100", 16449)  # the last 100 keys begin in tile 255: segment 0 is dead, segment 1 but for its last tile
    assert not s[0].any() and not s[1][:-1].any() and s[1][-1] and s[2].all()
    s = segs("head:100", 16449)
    assert s[0][:2].all() and not s[0][2:].any() and not s[1].any() and not s[2].any()
    s = segs("window:100", 8257)
    assert len(s) == 2 and not s[0][:-1].any() and s[0][-1] and s[1].all() and len(s[1]) == 2
    assert (8192 + 63) // 64 == 128 and (8193 + 63) // 64 == 129  # one full segment; a second segment of one tile with one key


# ---- the call's checks
PQ,PK, PV, PM, PD, PW = 0x10000, 0x20000, 0x30000, 0x40002, 0x50000, 0x60000  # never dereferenced
ORDER = ["Q", "q_nb1", "q_nb2", "q_nb3", "Ktype", "K", "k_nb1", "k_nb2", "k_nb3", "Vtype", "V", "v_nb1", "v_nb2", "v_nb3", "mask", "mask_nb1",
         "D", "n_q", "n_kv", "n_head", "n_head_kv", "ne3", "scale", "max_bias", "dst", "dst_nb1", "dst_nb2", "dst_nb3", "ws", "ws_bytes",
         "flags", "stream"]
# a GQA prefill call that passes every check: 8 heads on 2 KV heads, the permuted cache views
GOOD = dict(Q=PQ, q_nb1=512, q_nb2=512 * 17, q_nb3=512 * 17 * 8, Ktype=T.F16, K=PK, k_nb1=2 * 272, k_nb2=272, k_nb3=2 * 272 * 65,
            Vtype=T.F16, V=PV, v_nb1=2 * 272, v_nb2=272, v_nb3=2 * 272 * 65, mask=PM, mask_nb1=2 * 65, D=128, n_q=17, n_kv=65, n_head=8,
            n_head_kv=2, ne3=1, scale=0.088, max_bias=0.0, dst=PD, dst_nb1=512, dst_nb2=512 * 8, dst_nb3=512 * 8 * 17, ws=None, ws_bytes=0,
            flags=0, stream=None)
SPLIT = dict(n_q=1, n_kv=3 * R.CHUNK + 7, mask_nb1=2 * (3 * R.CHUNK + 7))  # the decode route with a KV split: needs a workspace


def call(**over):
    args = dict(GOOD, **over)
    return _hip.lib().lfamd_flash_attn(*[args[n] for n in ORDER])


def last_error():
    return _hip.lib().lfamd_last_error().decode()


def test_symbols_are_exported_and_listed():
    assert "lfamd_flash_attn" in _hip.EXPORTS and "lfamd_flash_attn_workspace" in _hip.EXPORTS
    assert _hip.lib().lfamd_abi_version() == 1


def test_workspace_is_zero_where_no_split_runs():
    ws = _hip.lib().lfamd_flash_attn_workspace
    assert ws(128, 17, 65, 8, 2, 1) == 0          # the n_q > 8 route
    assert ws(128, 130, 100000, 8, 2, 1) == 0
    assert ws(128, 1, R.CHUNK, 8, 2, 1) == 0      # one chunk
    assert ws(128, 1, R.CHUNK + 1, 8, 2, 1) == 2 * 8 * (128 + 2) * 4
    assert ws(64, 2, 3 * R.CHUNK + 7, 8, 2, 3) == 3 * 8 * 2 * 4 * (64 + 2) * 4
    assert ws(128, 1, -5, 8, 2, 1) == 0 and ws(128, 0, 4096, 8, 2, 1) == 0


@pytest.mark.parametrize("dim", ["D", "n_q", "n_kv", "n_head", "n_head_kv", "ne3"])
def test_1_negative_dimension_is_invalid_before_everything(dim):
    assert call(**{dim: -1}) == INVALID
    assert "lfamd_flash_attn" in last_error()
    assert call(**{dim: -1, "Ktype": T.Q4_0, "Q": None, "n_q": -1 if dim == "n_q" else 0}) == INVALID  # before the empty call and the types


@pytest.mark.parametrize("dim", ["n_q", "n_head", "ne3"])
def test_2_empty_calls_are_ok_and_look_at_nothing(dim):
    assert call(**{dim: 0}) == OK
    assert call(**{dim: 0, "Q": None, "K": None, "V": None, "dst": None, "Ktype": 99, "D": 96, "max_bias": 8.0, "flags": 7, "q_nb1": 3}) == OK


@pytest.mark.parametrize("over", [dict(Ktype=T.Q4_0), dict(Vtype=T.Q8_0), dict(Ktype=T.F32), dict(D=96), dict(D=256), dict(D=0), dict(max_bias=8.0),
                                  dict(n_head=65536, n_head_kv=1), dict(n_head=256, ne3=256), dict(n_kv=0)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_3_unsupported_comes_before_the_invalid_arguments(over):
    assert call(**over) == UNSUPPORTED
    assert "lfamd_flash_attn" in last_error()
    assert call(**dict(over, Q=None, flags=1, k_nb1=7)) == UNSUPPORTED  # before the pointers, the strides and the flags


@pytest.mark.parametrize("over", [dict(Q=None), dict(K=None), dict(V=None), dict(dst=None), dict(ws=None, ws_bytes=64), dict(n_head_kv=0),
                                  dict(n_head_kv=3), dict(Q=PQ + 4), dict(K=PK + 16 - 2), dict(V=PV + 8), dict(dst=PD + 4), dict(q_nb1=516),
                                  dict(q_nb2=512 * 17 + 8), dict(q_nb3=4), dict(k_nb1=2 * 272 + 2), dict(k_nb2=270), dict(k_nb3=8),
                                  dict(v_nb1=2 * 272 + 4), dict(v_nb2=264), dict(v_nb3=2), dict(dst_nb1=520), dict(dst_nb2=4), dict(dst_nb3=12),
                                  dict(mask=PM + 1), dict(mask_nb1=2 * 65 + 1), dict(mask_nb1=2 * 65 - 2), dict(k_nb1=240, k_nb2=16),
                                  dict(v_nb1=128), dict(q_nb1=496), dict(dst_nb1=256), dict(flags=1)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_4_invalid_arguments_are_refused_before_any_device_call(over):
    assert call(**over) == INVALID
    assert "lfamd_flash_attn" in last_error()
    assert call(**dict(SPLIT, **over)) == INVALID  # before the workspace is measured


def test_4_a_null_mask_and_a_null_zero_size_workspace_are_not_errors_of_their_own():
    # they pass check 4; what answers is check 5 (the split call has no workspace)
    assert call(**dict(SPLIT, mask=None, mask_nb1=0)) == WORKSPACE


def test_5_a_small_workspace_is_refused_last():
    need = _hip.lib().lfamd_flash_attn_workspace(128, 1, 3 * R.CHUNK + 7, 8, 2, 1)
    assert need > 0
    assert call(**SPLIT) == WORKSPACE
    assert call(**dict(SPLIT, ws=PW, ws_bytes=need - 1)) == WORKSPACE
    assert "lfamd_flash_attn" in last_error()
