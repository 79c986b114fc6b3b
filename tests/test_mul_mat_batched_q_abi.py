"""lfamd_mul_mat_batched_q (include/lfamd_hip.h): the export and every refusal, in the order the header states.  The checks precede any
device call, so none of this needs a GPU: the pointers below are never dereferenced (a call that got as far as a launch would answer
LFAMD_ERR_HIP here, or write through them on a GPU box — either way not the code asserted)."""
import ctypes as C

import pytest

from llamafile_amd import _hip, ggml_types as T

OK, UNSUPPORTED, INVALID = 0, -1, -2
PA, PB, PC = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000  # 16-byte aligned, never read
ROW = 4 * 34  # a Q8_0 row of k = 128

# a KQ call that passes every check: m = 96 keys, k = 128, n = 2, 2 KV heads x 4 query heads each, the permuted K cache
GOOD = dict(Atype=T.Q8_0, A=PA, m=96, k=128, a_nb1=2 * ROW, a_nb2=ROW, a_nb3=96 * 2 * ROW, a_ne2=2, a_ne3=1,
            B=PB, n=2, b_nb1=8 * 512, b_nb2=512, b_nb3=2 * 8 * 512, ne2=8, ne3=1,
            C=PC, c_nb1=96 * 4, c_nb2=2 * 96 * 4, c_nb3=8 * 2 * 96 * 4, flags=0, stream=None)
ORDER = ["Atype", "A", "m", "k", "a_nb1", "a_nb2", "a_nb3", "a_ne2", "a_ne3", "B", "n", "b_nb1", "b_nb2", "b_nb3", "ne2", "ne3",
         "C", "c_nb1", "c_nb2", "c_nb3", "flags", "stream"]
SIX = [T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL]


def call(**over):
    a = {**GOOD, **over}
    return _hip.lib().lfamd_mul_mat_batched_q(*[a[name] for name in ORDER])


def last_error_names_the_call():
    return b"lfamd_mul_mat_batched_q" in _hip.lib().lfamd_last_error()


def test_symbol_is_exported_and_listed():
    assert "lfamd_mul_mat_batched_q" in _hip.EXPORTS
    assert hasattr(C.CDLL(_hip.HIP_SO), "lfamd_mul_mat_batched_q")
    assert len(_hip._SIGS["lfamd_mul_mat_batched_q"][1]) == len(ORDER)
    assert _hip._SIGS["lfamd_mul_mat_batched_q"] == _hip._SIGS["lfamd_mul_mat_batched"]  # one argument list
    assert _hip.lib().lfamd_abi_version() == 1  # additive


@pytest.mark.parametrize("name", ["m", "k", "n", "ne2", "ne3", "a_ne2", "a_ne3"])
def test_negative_dimension_is_invalid(name):
    assert call(**{name: -1}) == INVALID
    assert last_error_names_the_call()
    # the first check: it wins over the empty case and over the type
    if name != "m":
        assert call(**{name: -1, "m": 0}) == INVALID
    assert call(**{name: -1, "Atype": T.Q4_K}) == INVALID


@pytest.mark.parametrize("name", ["m", "n", "ne2", "ne3"])
def test_empty_calls_are_ok_with_null_pointers(name):
    assert call(**{name: 0, "A": None, "B": None, "C": None}) == OK
    # the second check: nothing behind it is looked at — not the type, k, the strides or the flags
    assert call(**{name: 0, "A": None, "B": None, "C": None, "Atype": T.Q4_K, "k": 48, "a_nb1": 1, "b_nb1": 2, "flags": 7, "a_ne2": 0}) == OK
    assert call(**{name: 0, "Atype": T.F16, "k": 4096}) == OK


@pytest.mark.parametrize("t", [T.F16, T.F32, T.BF16, T.Q4_K, T.Q8_1, 99, T.Q8_0 | _hip.TYPE_PAD256])
def test_other_weight_types_are_unsupported(t):
    assert call(Atype=t) == UNSUPPORTED
    assert last_error_names_the_call()
    assert call(Atype=t, A=None) == UNSUPPORTED  # the third check comes before the pointers


@pytest.mark.parametrize("t", SIX)
def test_k_above_the_cap_is_unsupported(t):
    row = T.row_size(t, 1056)
    assert call(Atype=t, k=1056, a_nb1=2 * row, a_nb2=row, a_nb3=96 * 2 * row, b_nb1=8 * 4 * 1056, b_nb2=4 * 1056, b_nb3=16 * 4 * 1056) == UNSUPPORTED
    assert last_error_names_the_call()
    assert call(Atype=t, k=1056, A=None, flags=1) == UNSUPPORTED  # before the pointers, the strides and the flags
    assert call(Atype=t, k=1040) == UNSUPPORTED  # ... and before k % 32


def test_more_slices_than_the_launch_indexes_is_unsupported():
    assert call(ne2=65536, a_ne2=65536) == UNSUPPORTED
    assert call(ne2=256, ne3=256, a_ne2=256, a_ne3=256) == UNSUPPORTED
    assert call(ne2=65536, a_ne2=65536, A=None, flags=1) == UNSUPPORTED
    assert call(n=65535 * 64 + 1) == UNSUPPORTED
    assert call(m=2 ** 32 + 1, c_nb1=4 * (2 ** 32 + 1)) == UNSUPPORTED
    assert last_error_names_the_call()


@pytest.mark.parametrize("over", [
    dict(A=None), dict(B=None), dict(C=None),
    dict(a_ne2=0), dict(a_ne3=0), dict(a_ne2=3), dict(ne3=3, a_ne3=2), dict(a_ne2=16),
    dict(k=48), dict(k=1),
    dict(a_nb1=ROW - 2), dict(b_nb1=4 * 128 - 4), dict(c_nb1=4 * 96 - 4),
    dict(A=PA + 1), dict(a_nb1=2 * ROW + 1), dict(a_nb2=ROW + 1), dict(a_nb3=96 * 2 * ROW + 1),
    dict(B=PB + 2), dict(b_nb1=8 * 512 + 2), dict(b_nb2=514), dict(b_nb3=2 * 8 * 512 + 1),
    dict(C=PC + 2), dict(c_nb1=96 * 4 + 2), dict(c_nb2=2 * 96 * 4 + 2), dict(c_nb3=8 * 2 * 96 * 4 + 1),
    dict(flags=1), dict(flags=0x80000000),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_invalid_arguments_are_refused_before_any_launch(over):
    assert call(**over) == INVALID
    assert last_error_names_the_call()


@pytest.mark.parametrize("t", SIX)
def test_row_stride_is_checked_against_the_types_row_size(t):
    row = T.row_size(t, 128)
    assert call(Atype=t, a_nb1=row - 2, a_nb2=2 * 96 * row, a_nb3=2 * 96 * row) == INVALID
    assert last_error_names_the_call()


def test_k_zero_is_not_an_empty_call():
    """k == 0 writes zeros, so it goes through every check: with a NULL result it is refused, not LFAMD_OK."""
    assert call(k=0, C=None) == INVALID
    assert call(k=0, Atype=T.F32) == UNSUPPORTED


def test_the_f16_call_still_refuses_block_types():
    """The feature is a new entry point: lfamd_mul_mat_batched answers a 32-block type as before."""
    args = [{**GOOD, "Atype": T.Q8_0}[name] for name in ORDER]
    assert _hip.lib().lfamd_mul_mat_batched(*args) == UNSUPPORTED
