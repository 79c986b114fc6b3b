"""The documented check order of lfamd_flash_attn, lfamd_flash_attn_q, lfamd_cpy, lfamd_mul_mat_batched and lfamd_mul_mat_batched_q
(include/lfamd_hip.h: "Checks, before any device call and in this order") without a GPU: lfamd_flash_attn_check,
lfamd_flash_attn_q_check and lfamd_cpy_check, which the entry points call first and the ggml backend's supports_op asks, give the
code and leave the message the entry points gave before the checks were moved into them; the two batched calls, which have no check
function, are held through the entry points themselves.

tests/golden/entry_checks_parent.json was recorded by tools/entry_checks_record.py from the library of commit 0bd7222 (the parent of
the change that introduced the check functions): lfamd_flash_attn and lfamd_cpy themselves were called, on a machine without a GPU, with
the refused and the empty cases of tests/entry_checks_cases.py — a refusal comes before any device call — and (rc, message) was kept
per case.  The controls, which pass every check, were not sent: they are held to LFAMD_OK here, through the check functions alone.
The answers of lfamd_flash_attn_q, lfamd_mul_mat_batched and lfamd_mul_mat_batched_q were recorded the same way from the library of
commit 541c006 (the parent of the change that gave the five calls one check runner); that library answers the cases of
lfamd_flash_attn and lfamd_cpy byte for byte as 0bd7222's did."""
import json
import os

import pytest

import entry_checks_cases as cases
from llamafile_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = json.load(open(os.path.join(ROOT, "tests", "golden", "entry_checks_parent.json")))
ALL = [(op, name, expectation, changes) for op, (_, _, table, _) in cases.OPERATORS.items() for name, expectation, changes in table]
CHECKED = [a for a in ALL if a[0] in cases.NOT_IN_CHECK]  # the operators that have a check function
UNPLACED = [(op, name, changes, same_as) for op, (_, _, _, table) in cases.OPERATORS.items() for name, changes, same_as in table]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_hip.HIP_SO), "run __graft_entry__.build() first"
    return cases.bind(_hip.HIP_SO)


def leave_another_message(lib, op):
    """lfamd_last_error() holds the OTHER operator's refusal, so a check that answers without setting its message shows."""
    other = "lfamd_flash_attn" if op == "lfamd_cpy" else "lfamd_cpy"
    rc, message = cases.call(lib, other, dict(flags=1), check=True)
    assert rc == cases.ERR_INVALID and message.startswith(other + ":")


def test_every_refused_and_empty_case_was_recorded():
    for op, name, expectation, _ in ALL:
        assert (name in PARENT[op]) == (expectation != cases.PASSES), (op, name)
    assert sum(len(v) for v in PARENT.values()) == sum(e != cases.PASSES for _, _, e, _ in ALL)
    for op, answers in PARENT.items():
        assert all(rc != cases.ERR_HIP for rc, _ in answers.values()), op


@pytest.mark.parametrize("op,name,expectation,changes", CHECKED, ids=[f"{a[0]}-{a[1]}" for a in CHECKED])
def test_the_check_function_gives_the_parents_answer(lib, op, name, expectation, changes):
    leave_another_message(lib, op)
    rc, message = cases.call(lib, op, changes, check=True)
    if expectation == cases.PASSES:
        assert rc == 0
        return
    want_rc, want_message = PARENT[op][name]
    assert (rc, message) == (want_rc, want_message)
    assert (rc == 0) == (expectation == cases.EMPTY)


@pytest.mark.parametrize("op,name,changes,same_as", UNPLACED, ids=[f"{a[0]}-{a[1]}" for a in UNPLACED])
def test_unplaced_operands(lib, op, name, changes, same_as):
    """LFAMD_CHECK_UNPLACED, what supports_op passes before tensors have addresses: a NULL pointer is no error, a pointer argument
    counts with its alignment bits, the workspace is not looked at; every other row answers as in the entry point."""
    leave_another_message(lib, op)
    rc, message = cases.call(lib, op, changes, check=True, flags=cases.CHECK_UNPLACED)
    assert (rc, message) == (tuple(PARENT[op][same_as]) if same_as else (0, ""))


def test_the_entry_points_answer_from_the_same_table(lib):
    """The refused and the empty cases through the five entry points themselves, where no GPU is present: a call that got past the
    checks after all would launch on the cases' made-up addresses."""
    import torch
    if torch.cuda.is_available():
        return
    for op, name, expectation, changes in ALL:
        if expectation == cases.PASSES:
            continue
        leave_another_message(lib, op)
        assert list(cases.call(lib, op, changes, check=False)) == PARENT[op][name], (op, name)
    for op in cases.OPERATORS:  # LFAMD_CHECK_UNPLACED is the check functions' alone: to an entry point it is a reserved flag like any other
        leave_another_message(lib, op)
        assert list(cases.call(lib, op, {}, check=False, flags=cases.CHECK_UNPLACED)) == PARENT[op]["flags_1"], op
