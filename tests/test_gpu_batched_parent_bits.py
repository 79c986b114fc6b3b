"""lfamd_mul_mat_batched and lfamd_mul_mat_batched_q give the bits of the commit before their common front end
(csrc/mul_mat_batched_common.h): tests/golden/mul_mat_batched_parent.json (tools/batched_record.py) holds, per case of
tests/batched_cases.py, the digests a library built at that commit produced — of the inputs, and of the whole sentinel-prefilled
result buffer after the call."""
import re
import subprocess

import pytest

import batched_cases as cases

CASES = cases.cases()


def test_the_fixture_has_exactly_the_cases():
    assert sorted(cases.golden()["cases"]) == sorted(cases.case_id(c) for c in CASES) and len(CASES) == len(set(CASES))


def test_the_cases_reach_every_kernel_of_the_library():
    """The 48 instantiations, read from the built library's symbols (a kernel keeps its name as a host-side stub)."""
    from llamafile_amd import _hip
    raw = subprocess.run(["nm", "--defined-only", _hip.HIP_SO], capture_output=True, text=True, check=True).stdout
    built = set(re.findall(r"_ZN12_GLOBAL__N_115(mm[bq]_(?:gemv|mfma)_kernelI\w+?E)EvNS_8mm[bq]_argsE", raw))
    reached = {cases.kernels_reached(c) for c in CASES}
    assert len(built) == 48 and reached == built, sorted(built ^ reached)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[cases.case_id(c) for c in CASES])
def test_bits_are_the_parents(gpu, case):
    from llamafile_amd import _hip
    import batched_case
    want = cases.golden()["cases"][cases.case_id(case)]
    got = cases.digest(batched_case.Dev(), cases.bind(_hip.HIP_SO), case)
    assert (got["A"], got["B"]) == (want["A"], want["B"]), "the generator changed: it no longer gives the recorded inputs"
    assert got["C"] == want["C"], "the kernel changed: the result buffer is not the parent's"
