"""CPU: the ISA of the IQ4_NL kernels (tools/isa_hazards.py), cross-compiled for gfx950 here: the decode unit gemv_iq4nl.hip in its
shipped build, and the 128 x 128 batch body's IQ4_NL instantiation inside gemm_wide_l4.hip — test_isa_hazards.py walks that unit
too, and would pass just as well if the instantiation were not there."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazards  # noqa: E402

CSRC = os.path.join(ROOT, "llamafile_amd", "csrc")
SHIPPED_FLAGS = ("-mllvm", "-amdgpu-kernarg-preload-count=13")  # csrc/Makefile, the decode units
IQ4_NL = 20

needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_hazards.HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def decode_asm():
    return isa_hazards.shipped_asm(os.path.join(CSRC, "gemv_iq4nl.hip"), SHIPPED_FLAGS)


@needs_hipcc
def test_decode_kernels_have_no_flat_access_and_no_stack(decode_asm):
    res = isa_hazards.decode_hygiene(decode_asm)
    decode = {k: v for k, v in res.items() if "gemv_kq" in k and "iq4nl_traits" in k and "Li1ELi" in k}  # NC = 1 bodies
    assert len(decode) >= 12, sorted(decode)  # {8 x 2, 16 x 1, 16 x 2} x {plain, early} x {f32, Q8_0 rows}
    for kernel, probs in decode.items():
        assert not probs, (kernel[:80], probs)


@needs_hipcc
def test_valu_wait_states_in_the_decode_unit(decode_asm):
    res = isa_hazards.check_valu_hazards(decode_asm)
    assert any("iq4nl_traits" in k for k in res)
    for kernel, bad in res.items():
        assert not bad, (kernel, bad[:3])


@needs_hipcc
def test_the_decode_look_up_is_byte_permutes(decode_asm):
    """The codebook look-up is three v_perm_b32 per four indices on constants, not a table in memory: 16 dwords x 3 per 256 weights
    of a lane in the one-column kernels."""
    bodies = {k: b for k, b in re.findall(r"^(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end", decode_asm, re.S | re.M)
              if "iq4nl_traits" in k and "Li1ELi" in k}
    assert bodies
    for k, body in bodies.items():
        assert body.count("v_perm_b32") >= 48, (k[:80], body.count("v_perm_b32"))


@needs_hipcc
def test_the_batch_instantiation_exists_and_is_clean():
    res = isa_hazards.check_file(os.path.join(CSRC, "gemm_wide_l4.hip"))
    mine = {k: bad for k, bad in res.items() if f"gemm_wide_kernelILi{IQ4_NL}E" in k}
    assert mine, sorted(res)
    for kernel, bad in mine.items():
        assert not bad, (kernel, bad[:3])
