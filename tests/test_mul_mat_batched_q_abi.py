"""lfamd_mul_mat_batched_q (include/lfamd_hip.h): the export and every refusal, in the order the header states.  The refusals it shares
with lfamd_mul_mat_batched are tests/batched_abi.py's, collected here on this call; the rest is what only a 32-block A decides: the six
types, the k cap, k % 32 and the row size per type."""
import pytest

from llamafile_amd import _hip, ggml_types as T
from batched_abi import (GOOD_BC, INVALID, INVALID_BC, ORDER, PA, UNSUPPORTED, Abi, invalid_argument_is_refused_before_any_launch,
                         other_weight_type_is_unsupported, over_id, test_empty_calls_are_ok_with_null_pointers,
                         test_k_zero_is_not_an_empty_call, test_more_slices_than_the_launch_indexes_is_unsupported,
                         test_negative_dimension_is_invalid, test_symbol_is_exported_and_listed)  # noqa: F401  (collected here)

ROW = 4 * 34  # a Q8_0 row of k = 128
# a KQ call that passes every check: the permuted Q8_0 K cache
GOOD = dict(GOOD_BC, Atype=T.Q8_0, A=PA, a_nb1=2 * ROW, a_nb2=ROW, a_nb3=96 * 2 * ROW)
SIX = [T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL]


@pytest.fixture
def abi():
    return Abi("lfamd_mul_mat_batched_q", GOOD)


@pytest.mark.parametrize("t", [T.F16, T.F32, T.BF16, T.Q4_K, T.Q8_1, 99, T.Q8_0 | _hip.TYPE_PAD256])
def test_other_weight_types_are_unsupported(abi, t):
    other_weight_type_is_unsupported(abi, t)


@pytest.mark.parametrize("t", SIX)
def test_k_above_the_cap_is_unsupported(abi, t):
    row = T.row_size(t, 1056)
    assert abi.call(Atype=t, k=1056, a_nb1=2 * row, a_nb2=row, a_nb3=96 * 2 * row, b_nb1=8 * 4 * 1056, b_nb2=4 * 1056, b_nb3=16 * 4 * 1056) == UNSUPPORTED
    assert abi.last_error_names_the_call()
    assert abi.call(Atype=t, k=1056, A=None, flags=1) == UNSUPPORTED  # before the pointers, the strides and the flags
    assert abi.call(Atype=t, k=1040) == UNSUPPORTED  # ... and before k % 32


@pytest.mark.parametrize("over", INVALID_BC + [dict(k=48), dict(k=1), dict(a_nb1=ROW - 2), dict(a_nb1=2 * ROW + 1), dict(a_nb2=ROW + 1),
                                               dict(a_nb3=96 * 2 * ROW + 1)], ids=over_id)
def test_invalid_arguments_are_refused_before_any_launch(abi, over):
    invalid_argument_is_refused_before_any_launch(abi, over)


@pytest.mark.parametrize("t", SIX)
def test_row_stride_is_checked_against_the_types_row_size(abi, t):
    row = T.row_size(t, 128)
    assert abi.call(Atype=t, a_nb1=row - 2, a_nb2=2 * 96 * row, a_nb3=2 * 96 * row) == INVALID
    assert abi.last_error_names_the_call()


def test_the_f16_call_still_refuses_block_types():
    """The feature is a new entry point: lfamd_mul_mat_batched answers a 32-block type as before."""
    args = [GOOD[name] for name in ORDER]
    assert _hip.lib().lfamd_mul_mat_batched(*args) == UNSUPPORTED
