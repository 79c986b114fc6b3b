"""lfamd_mul_mat_batched (include/lfamd_hip.h): the export and every refusal.  The refusals it shares with lfamd_mul_mat_batched_q are
tests/batched_abi.py's, collected here on this call; the rest is what only an F16 A decides."""
import pytest

from llamafile_amd import _hip, ggml_types as T
from batched_abi import (GOOD_BC, INVALID_BC, PA, Abi, invalid_argument_is_refused_before_any_launch, other_weight_type_is_unsupported,
                         over_id, test_empty_calls_are_ok_with_null_pointers, test_k_zero_is_not_an_empty_call,
                         test_more_slices_than_the_launch_indexes_is_unsupported, test_negative_dimension_is_invalid,
                         test_symbol_is_exported_and_listed)  # noqa: F401  (collected here)

# a KQ call that passes every check: the permuted F16 K cache
GOOD = dict(GOOD_BC, Atype=T.F16, A=PA, a_nb1=512, a_nb2=256, a_nb3=96 * 512)


@pytest.fixture
def abi():
    return Abi("lfamd_mul_mat_batched", GOOD)


@pytest.mark.parametrize("t", [T.F32, T.BF16, T.Q4_K, T.Q8_0, 99, T.F16 | _hip.TYPE_PAD256])
def test_other_weight_types_are_unsupported(abi, t):
    other_weight_type_is_unsupported(abi, t)


@pytest.mark.parametrize("over", INVALID_BC + [dict(a_nb1=2 * 128 - 2), dict(a_nb1=513), dict(a_nb2=257), dict(a_nb3=96 * 512 + 1)], ids=over_id)
def test_invalid_arguments_are_refused_before_any_launch(abi, over):
    invalid_argument_is_refused_before_any_launch(abi, over)
