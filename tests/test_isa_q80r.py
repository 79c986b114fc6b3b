"""CPU: the ISA of the relaxed-order Q8_0 decode GEMV (gemv_q80r.hip: f32 rows, gemv_q80rb.hip: Q8_0 rows), cross-compiled for
gfx950 with the shipped flags (tools/isa_hazards.py): no FLAT access and no stack in any kernel of the two units — hipcc keeps
the counted weight prefetch only then — and the VALU wait-state rules."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazards  # noqa: E402

CSRC = os.path.join(ROOT, "llamafile_amd", "csrc")
SHIPPED_FLAGS = ("-mllvm", "-amdgpu-kernarg-preload-count=13")  # csrc/Makefile, the decode units

needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_hazards.HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module", params=["gemv_q80r.hip", "gemv_q80rb.hip"])
def unit_asm(request):
    return isa_hazards.shipped_asm(os.path.join(CSRC, request.param), SHIPPED_FLAGS)


@needs_hipcc
def test_kernels_have_no_flat_access_and_no_stack(unit_asm):
    res = isa_hazards.decode_hygiene(unit_asm)
    mine = {k: v for k, v in res.items() if "gemv_q80r_kernel" in k}
    assert len(mine) == 24, sorted(mine)  # 8 column counts x 3 chunk sizes
    for kernel, probs in mine.items():
        assert not probs, (kernel[:80], probs)


@needs_hipcc
def test_valu_wait_states(unit_asm):
    res = isa_hazards.check_valu_hazards(unit_asm)
    assert any("gemv_q80r_kernel" in k for k in res)
    for kernel, bad in res.items():
        assert not bad, (kernel, bad[:3])
