"""Every weight image is the parent commit's, byte for byte: tests/golden/pack_images_parent.json (tools/pack_image_record.py) holds,
per case of tests/pack_image_cases.py, the digests a library built at the parent of the one-writer change produced — bytes the readers
ignore included, since the output buffer starts as 0xEE and is hashed whole."""
import pytest

import pack_image_cases as pic

pytestmark = pytest.mark.gpu

CASES = pic.cases()


def test_the_fixture_has_exactly_the_cases():
    assert sorted(pic.golden()["cases"]) == sorted(pic.case_id(*c) for c in CASES) and len(CASES) == len(set(CASES))


@pytest.mark.parametrize("case", CASES, ids=[pic.case_id(*c) for c in CASES])
def test_image_is_the_parents(gpu, case):
    from llamafile_amd import _hip
    want = pic.golden()["cases"][pic.case_id(*case)]
    got = pic.digest(pic.bind(_hip.HIP_SO), *case)
    assert got["raw"] == want["raw"], "synth.random_weights changed: the generator no longer gives the recorded input"
    assert got == want
