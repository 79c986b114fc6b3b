"""lfamd_flash_attn_q without a device: the references of tests/fattn_q_ref.py against each other over the device suite's cases,
the properties of the quantised inputs the routes rely on, and the call's check table (include/lfamd_hip.h) through
lfamd_flash_attn_q_check with made-up addresses, in the style of tests/entry_checks_cases.py: nothing stands behind them, so a case
that passes is only ever sent to the check function."""
import numpy as np
import pytest

import entry_checks_cases as cases
import fattn_q_ref as QR
import fattn_ref as R
from llamafile_amd import _hip, ggml_types as T

DECODE_SUITE = R.decode_cases() + QR.decode_edge_cases()
PREFILL_SUITE = R.prefill_cases() + QR.prefill_edge_cases()


# ---- the references
@pytest.mark.parametrize("t", QR.TYPES, ids=QR.type_name)
def test_decode_emulation_keeps_the_margin_tol_f32_was_derived_with(t):
    """The route's operands are exact in f32 and everything behind them is the F16 call's n_q <= 8 route: the same error model, the
    same rule — 4 x the emulation's largest error <= TOL_F32."""
    worst = 0.0
    for c in DECODE_SUITE:
        Q, _, _, K, V, mask, scale = QR.inputs_of(c, t)
        ref, a = R.ref64(Q, K, V, mask, scale, "decode")
        err = R.row_err(R.emulate(Q, K, V, mask, scale, "decode"), ref, a)
        print(R.case_id(c), err)
        worst = max(worst, err)
    print(QR.type_name(t), "largest emulation error", worst)
    assert 4 * worst <= R.TOL_F32


@pytest.mark.parametrize("t", QR.TYPES, ids=QR.type_name)
def test_prefill_emulation_is_within_half_the_tolerance(t):
    worst = 0.0
    for c in PREFILL_SUITE:
        Q, _, _, K, V, mask, scale = QR.inputs_of(c, t)
        assert K.dtype == np.float16 and V.dtype == np.float16
        ref, a = R.ref64(Q, K, V, mask, scale, "prefill")
        err = R.row_err(R.emulate(Q, K, V, mask, scale, "prefill"), ref, a)
        print(R.case_id(c), err)
        worst = max(worst, err)
    print(QR.type_name(t), "largest emulation error", worst)
    assert worst < R.TOL_MMA / 2


@pytest.mark.parametrize("t", QR.TYPES, ids=QR.type_name)
def test_the_inputs_are_inside_the_domain_and_exact_in_f32(t):
    """Every f16(d * code) is finite (the n_q > 8 route's domain), and d * code is exactly representable in f32 (an 11-bit by an
    8-bit significand), so dequantise() loses nothing and the n_q <= 8 route's operands are the block values themselves."""
    for c in DECODE_SUITE + PREFILL_SUITE:
        _, K, V, _, _ = R.inputs_of(c)
        for X in (K, V):
            raw = QR.quantise(t, X)
            d, codes = QR.codes_and_d(t, raw)
            exact = d.astype(np.float64) * codes.astype(np.float64)
            x32 = QR.dequantise(t, raw)
            assert np.array_equal(x32.astype(np.float64).reshape(exact.shape), exact), R.case_id(c)
            assert np.array_equal(QR.dequantise(t, QR.quantise(t, X)), x32)
            with np.errstate(over="raise"):
                assert np.isfinite(x32.astype(np.float16)).all(), R.case_id(c)
            assert np.abs(codes).max() <= (127 if t == T.Q8_0 else 8)


def test_quantise_gives_the_block_layout_the_header_states():
    lo, hi = np.arange(16), np.arange(15, -1, -1)  # the codes of elements 0 .. 15 and 16 .. 31
    x = (2.0 * (np.concatenate([lo, hi]) - 8)).astype(np.float32)[None]  # vmax = -16 -> d = 2
    raw = QR.quantise(T.Q4_0, x)
    assert raw.shape == (1, 18) and raw[0, :2].view(np.float16)[0] == 2.0
    assert list(raw[0, 2:] & 15) == list(lo)   # elements 0 .. 15: the low nibbles of bytes 0 .. 15
    assert list(raw[0, 2:] >> 4) == list(hi)   # elements 16 .. 31: their high nibbles
    assert np.array_equal(QR.dequantise(T.Q4_0, raw), x)
    raw = QR.quantise(T.Q8_0, x)
    assert raw.shape == (1, 34) and raw[0, 2:].view(np.int8)[0] == -127  # d = 16 / 127, the first code its largest


# ---- the check table
Q8, Q4 = 4 * 34, 4 * 18  # a row of D = 128
D, N_Q, N_KV, HEADS, KVH = cases.D, cases.N_Q, cases.N_KV, cases.HEADS, cases.KVH
PAIR_Q8 = dict(Ktype=T.Q8_0, k_nb1=KVH * Q8, k_nb2=Q8, k_nb3=N_KV * KVH * Q8, Vtype=T.Q8_0, v_nb1=KVH * Q8, v_nb2=Q8, v_nb3=N_KV * KVH * Q8)
PAIR_Q4 = dict(Ktype=T.Q4_0, k_nb1=KVH * Q4, k_nb2=Q4, k_nb3=N_KV * KVH * Q4, Vtype=T.Q4_0, v_nb1=KVH * Q4, v_nb2=Q4, v_nb3=N_KV * KVH * Q4)
CONTROL = dict(cases.FA_CONTROL, **PAIR_Q8)
LONG = dict(n_kv=600, k_nb3=600 * KVH * Q8, v_nb3=600 * KVH * Q8, mask_nb1=1200)
SHORT_WS = dict(LONG, ws=cases.WS_AT, ws_bytes=cases.LONG_WS - 1)
K_AT, Q_AT = cases.K_AT, cases.Q_AT
UNSUPPORTED, INVALID, WORKSPACE = cases.ERR_UNSUPPORTED, cases.ERR_INVALID, cases.ERR_WORKSPACE
P = "lfamd_flash_attn_q: "
PAIR = (UNSUPPORTED, P + "the K / V types are not (Q8_0, Q8_0) or (Q4_0, Q4_0)")
KV2 = (INVALID, P + "a K / V base or stride is not a multiple of 2")
QD16 = (INVALID, P + "a Q / dst base or stride is not a multiple of 16")
ROWS = (INVALID, P + "a row stride is smaller than the row")
D96 = (UNSUPPORTED, P + "head size is not 64 or 128")
FLAGS = (INVALID, P + "flags are reserved (0)")
OK = (0, "")

# (name, changes to CONTROL, the answer)
TABLE = [
    ("control_q8_0", {}, OK),
    ("control_q4_0", PAIR_Q4, OK),
    ("control_nomask", dict(mask=None, mask_nb1=0), OK),
    ("control_long_with_its_workspace", dict(LONG, ws=cases.WS_AT, ws_bytes=cases.LONG_WS), OK),
    # steps 1 and 2 are lfamd_flash_attn's
    ("negative_D", dict(D=-128), (INVALID, P + "negative dimension")),
    ("n_q_0", dict(cases.NO_POINTERS, n_q=0, Ktype=T.F16), OK),
    # step 3, first clause: the pair
    ("f16_pair", dict(Ktype=T.F16, Vtype=T.F16), (UNSUPPORTED, P + "F16 K and V: that is lfamd_flash_attn")),
    ("q8_0_k_f16_v", dict(Vtype=T.F16), PAIR),
    ("f16_k_q8_0_v", dict(Ktype=T.F16), PAIR),
    ("q8_0_k_q4_0_v", dict(Vtype=T.Q4_0), PAIR),
    ("q4_0_k_q8_0_v", dict(Ktype=T.Q4_0), PAIR),
    ("q4_1_pair", dict(Ktype=T.Q4_1, Vtype=T.Q4_1), PAIR),
    ("q5_0_pair", dict(Ktype=T.Q5_0, Vtype=T.Q5_0), PAIR),
    ("q5_1_pair", dict(Ktype=T.Q5_1, Vtype=T.Q5_1), PAIR),
    ("iq4_nl_pair", dict(Ktype=T.IQ4_NL, Vtype=T.IQ4_NL), PAIR),
    ("q4_k_pair", dict(Ktype=T.Q4_K, Vtype=T.Q4_K), PAIR),
    ("f32_pair", dict(Ktype=T.F32, Vtype=T.F32), PAIR),
    ("d96", dict(D=96), D96),
    ("max_bias_1", dict(max_bias=1.0), (UNSUPPORTED, P + "max_bias != 0 (ALiBi)")),
    ("n_kv_0", dict(n_kv=0), (UNSUPPORTED, P + "n_kv == 0")),
    # step 4
    ("null_K", dict(K=None), (INVALID, P + "null pointer")),
    ("k_base_plus_1", dict(K=K_AT + 1), KV2),
    ("k_base_plus_2", dict(K=K_AT + 2), OK),
    ("k_base_plus_2_q4_0", dict(PAIR_Q4, K=K_AT + 2, V=cases.V_AT + 6), OK),
    ("v_nb2_odd", dict(v_nb2=Q8 + 1), KV2),
    ("k_nb1_plus_2", dict(k_nb1=KVH * Q8 + 2), OK),
    ("q_base_plus_8", dict(Q=Q_AT + 8), QD16),
    ("dst_nb3_plus_8", dict(dst_nb3=N_Q * HEADS * D * 4 + 8), QD16),
    ("k_nb1_one_block_short", dict(k_nb1=Q8 - 34), ROWS),
    ("v_nb1_one_block_short", dict(v_nb1=Q8 - 34), ROWS),
    ("k_nb1_one_block_short_q4_0", dict(PAIR_Q4, k_nb1=Q4 - 18), ROWS),
    ("q4_0_pair_with_q8_0_row_strides", dict(Ktype=T.Q4_0, Vtype=T.Q4_0), OK),
    ("q_nb1_short", dict(q_nb1=D * 4 - 16), ROWS),
    ("flags_1", dict(flags=1), FLAGS),
    # step 5
    ("workspace_one_byte_short", SHORT_WS, (WORKSPACE, P + "workspace smaller than lfamd_flash_attn_workspace()")),
    # the order of two violated clauses
    ("step_3_pair_before_d96", dict(Vtype=T.F16, D=96), PAIR),
    ("step_3_f16_pair_before_d96", dict(Ktype=T.F16, Vtype=T.F16, D=96), (UNSUPPORTED, P + "F16 K and V: that is lfamd_flash_attn")),
    ("steps_3_4_d96_and_k_base_plus_1", dict(D=96, K=K_AT + 1), D96),
    ("step_4_q_dst_16_before_k_v_2", dict(Q=Q_AT + 8, K=K_AT + 1), QD16),
    ("step_4_alignment_before_row_strides", dict(K=K_AT + 1, k_nb1=Q8 - 34), KV2),
    ("step_4_row_strides_before_flags", dict(k_nb1=Q8 - 34, flags=1), ROWS),
    ("steps_4_5_flags_1_and_short_workspace", dict(SHORT_WS, flags=1), FLAGS),
]

# under LFAMD_CHECK_UNPLACED
UNPLACED = [
    ("every_pointer_null", cases.NO_POINTERS, OK),
    ("every_pointer_null_q4_0", dict(cases.NO_POINTERS, **PAIR_Q4), OK),
    ("k_pointer_1", dict(cases.NO_POINTERS, K=1), KV2),
    ("k_pointer_2", dict(cases.NO_POINTERS, K=2), OK),
    ("k_pointer_34_a_view_one_block_in", dict(cases.NO_POINTERS, K=34), OK),
    ("q_pointer_8", dict(cases.NO_POINTERS, Q=8), QD16),
    ("workspace_one_byte_short", SHORT_WS, OK),
    ("null_workspace_with_a_size", dict(ws=None, ws_bytes=16), OK),
    ("d96", dict(cases.NO_POINTERS, D=96), D96),
    ("mixed_pair", dict(cases.NO_POINTERS, Vtype=T.F16), PAIR),
    ("k_nb1_one_block_short", dict(cases.NO_POINTERS, k_nb1=Q8 - 34), ROWS),
    ("flags_1_beside_it", dict(flags=1), FLAGS),
]


@pytest.fixture(scope="module")
def lib():
    lib = cases.bind(_hip.HIP_SO)
    types = [cases._ctype("lfamd_flash_attn", n) for n in cases.FA_ARGS]
    lib.lfamd_flash_attn_q.argtypes = types
    lib.lfamd_flash_attn_q_check.argtypes = [t for t, n in zip(types, cases.FA_ARGS) if n not in ("scale", "stream")]
    return lib


def ask(lib, fn, changes, flags=0):
    """(rc, message) of lfamd_flash_attn_q_check / lfamd_flash_attn_q / lfamd_flash_attn_check on CONTROL with `changes`."""
    a = dict(CONTROL, **changes)
    a["flags"] |= flags
    check = fn.endswith("_check")
    rc = getattr(lib, fn)(*[a[n] for n in cases.FA_ARGS if not (check and n in ("scale", "stream"))])
    return rc, (lib.lfamd_last_error().decode() if rc else "")


def leave_another_message(lib):
    rc, message = cases.call(lib, "lfamd_cpy", dict(flags=1), check=True)
    assert rc == INVALID and message.startswith("lfamd_cpy:")


def test_symbols_are_exported_and_listed():
    assert "lfamd_flash_attn_q" in _hip.EXPORTS and "lfamd_flash_attn_q_check" in _hip.EXPORTS


@pytest.mark.parametrize("name,changes,want", TABLE, ids=[r[0] for r in TABLE])
def test_the_check_table(lib, name, changes, want):
    leave_another_message(lib)
    assert ask(lib, "lfamd_flash_attn_q_check", changes) == want


@pytest.mark.parametrize("name,changes,want", UNPLACED, ids=[r[0] for r in UNPLACED])
def test_unplaced_operands(lib, name, changes, want):
    leave_another_message(lib)
    assert ask(lib, "lfamd_flash_attn_q_check", changes, flags=cases.CHECK_UNPLACED) == want


def test_lfamd_flash_attn_check_still_answers_f16_k_and_v_only(lib):
    """The controls of this table, sent to the F16 call's check: its answer and message are what they were."""
    for pair in ({}, PAIR_Q4):
        leave_another_message(lib)
        assert ask(lib, "lfamd_flash_attn_check", pair) == (UNSUPPORTED, "lfamd_flash_attn: F16 K and V only")
        assert ask(lib, "lfamd_flash_attn_check", pair, flags=cases.CHECK_UNPLACED) == (UNSUPPORTED, "lfamd_flash_attn: F16 K and V only")


def test_the_entry_point_answers_from_the_same_table(lib):
    """The refused and the empty cases through lfamd_flash_attn_q itself, where no GPU is present: a call that got past the checks
    after all would launch on the made-up addresses.  LFAMD_CHECK_UNPLACED is the check function's alone."""
    import torch
    if torch.cuda.is_available():
        return
    for name, changes, want in TABLE:
        if want == OK and changes.get("n_q") != 0:
            continue
        leave_another_message(lib)
        assert ask(lib, "lfamd_flash_attn_q", changes) == want, name
    leave_another_message(lib)
    assert ask(lib, "lfamd_flash_attn_q", {}, flags=cases.CHECK_UNPLACED) == FLAGS
