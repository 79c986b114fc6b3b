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


# ---- the call's checks
PQ, PK, PV, PM, PD, PW = 0x10000, 0x20000, 0x30000, 0x40002, 0x50000, 0x60000  # never dereferenced
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
