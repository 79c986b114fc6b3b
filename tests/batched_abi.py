"""The refusals lfamd_mul_mat_batched and lfamd_mul_mat_batched_q share (include/lfamd_hip.h: one argument list, one check list,
csrc/mul_mat_batched_common.h).  tests/test_mul_mat_batched_abi.py and tests/test_mul_mat_batched_q_abi.py import these tests and
give each its call through their `abi` fixture: Abi(entry point, a call that passes every check).  The checks precede any device
call, so none of this needs a GPU: the pointers are never dereferenced (a call that got as far as a launch would answer LFAMD_ERR_HIP
here, or write through them on a GPU box — either way not the code asserted)."""
import ctypes as C

import pytest

from llamafile_amd import _hip, ggml_types as T

OK, UNSUPPORTED, INVALID = 0, -1, -2
PA, PB, PC = 0x7000_0000_1000, 0x7000_0100_0000, 0x7000_0200_0000  # 16-byte aligned, never read
ORDER = ["Atype", "A", "m", "k", "a_nb1", "a_nb2", "a_nb3", "a_ne2", "a_ne3", "B", "n", "b_nb1", "b_nb2", "b_nb3", "ne2", "ne3",
         "C", "c_nb1", "c_nb2", "c_nb3", "flags", "stream"]
# what every good call here has in common: m = 96 keys, k = 128, n = 2, 2 KV heads x 4 query heads each
GOOD_BC = dict(m=96, k=128, a_ne2=2, a_ne3=1, B=PB, n=2, b_nb1=8 * 512, b_nb2=512, b_nb3=2 * 8 * 512, ne2=8, ne3=1,
               C=PC, c_nb1=96 * 4, c_nb2=2 * 96 * 4, c_nb3=8 * 2 * 96 * 4, flags=0, stream=None)
# refused as LFAMD_ERR_INVALID by both calls, whatever A is
INVALID_BC = [
    dict(A=None), dict(B=None), dict(C=None),
    dict(a_ne2=0), dict(a_ne3=0), dict(a_ne2=3), dict(ne3=3, a_ne3=2), dict(a_ne2=16),
    dict(b_nb1=4 * 128 - 4), dict(c_nb1=4 * 96 - 4), dict(A=PA + 1),
    dict(B=PB + 2), dict(b_nb1=8 * 512 + 2), dict(b_nb2=514), dict(b_nb3=2 * 8 * 512 + 1),
    dict(C=PC + 2), dict(c_nb1=96 * 4 + 2), dict(c_nb2=2 * 96 * 4 + 2), dict(c_nb3=8 * 2 * 96 * 4 + 1),
    dict(flags=1), dict(flags=0x80000000),
]
over_id = lambda o: ",".join(f"{k}={v}" for k, v in o.items())


class Abi:
    def __init__(self, name, good):
        self.name, self.good = name, good

    def call(self, **over):
        a = {**self.good, **over}
        return getattr(_hip.lib(), self.name)(*[a[name] for name in ORDER])

    def last_error_names_the_call(self):
        return self.name.encode() in _hip.lib().lfamd_last_error()


def test_symbol_is_exported_and_listed(abi):
    assert abi.name in _hip.EXPORTS
    assert hasattr(C.CDLL(_hip.HIP_SO), abi.name)
    assert len(_hip._SIGS[abi.name][1]) == len(ORDER)
    assert _hip._SIGS["lfamd_mul_mat_batched_q"] == _hip._SIGS["lfamd_mul_mat_batched"]  # one argument list
    assert _hip.lib().lfamd_abi_version() == 1


@pytest.mark.parametrize("name", ["m", "k", "n", "ne2", "ne3", "a_ne2", "a_ne3"])
def test_negative_dimension_is_invalid(abi, name):
    assert abi.call(**{name: -1}) == INVALID
    assert abi.last_error_names_the_call()
    # the first check: it wins over the empty case and over the type
    if name != "m":
        assert abi.call(**{name: -1, "m": 0}) == INVALID
    assert abi.call(**{name: -1, "Atype": T.Q4_K}) == INVALID


@pytest.mark.parametrize("name", ["m", "n", "ne2", "ne3"])
def test_empty_calls_are_ok_with_null_pointers(abi, name):
    assert abi.call(**{name: 0, "A": None, "B": None, "C": None}) == OK
    # the second check: nothing behind it is looked at — not the type, k, the strides or the flags
    assert abi.call(**{name: 0, "A": None, "B": None, "C": None, "Atype": T.Q4_K, "k": 48, "a_nb1": 1, "b_nb1": 2, "flags": 7, "a_ne2": 0}) == OK
    assert abi.call(**{name: 0, "Atype": T.BF16, "k": 4096}) == OK


def other_weight_type_is_unsupported(abi, t):
    assert abi.call(Atype=t) == UNSUPPORTED
    assert abi.last_error_names_the_call()
    assert abi.call(Atype=t, A=None) == UNSUPPORTED  # the third check comes before the pointers


def test_more_slices_than_the_launch_indexes_is_unsupported(abi):
    assert abi.call(ne2=65536, a_ne2=65536) == UNSUPPORTED
    assert abi.call(ne2=256, ne3=256, a_ne2=256, a_ne3=256) == UNSUPPORTED
    assert abi.call(ne2=65536, a_ne2=65536, A=None, flags=1) == UNSUPPORTED
    assert abi.call(n=65535 * 64 + 1) == UNSUPPORTED
    assert abi.call(m=2 ** 32 + 1, c_nb1=4 * (2 ** 32 + 1)) == UNSUPPORTED
    assert abi.last_error_names_the_call()


def invalid_argument_is_refused_before_any_launch(abi, over):
    assert abi.call(**over) == INVALID
    assert abi.last_error_names_the_call()


def test_k_zero_is_not_an_empty_call(abi):
    """k == 0 writes zeros, so it goes through every check: with a NULL result it is refused, not LFAMD_OK."""
    assert abi.call(k=0, C=None) == INVALID
    assert abi.call(k=0, Atype=T.F32) == UNSUPPORTED
