"""CPU: the early decode kernels issue their first item before they wait for the matrix table (tools/gemv_prologue_isa.py), in
the gfx950 ISA of the shipped build.  One unit per kind of body — Q4_K (three loads per super-block), Q6_K (five, and the
permuted item order), Q4_0 (a 32-block type, Q8_0 activations) and the two-type unit; the tool run by hand covers the rest.
hipcc cross-compiles here (device code only)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemv_prologue_isa as gp  # noqa: E402
import isa_hazards  # noqa: E402

UNITS = ["gemv_q4k.hip", "gemv_q6k.hip", "gemv_q40.hip", "gemv_dual.hip"]


@pytest.mark.skipif(not os.path.exists(isa_hazards.HIPCC), reason="needs hipcc")
def test_first_item_is_issued_ahead_of_the_table_wait():
    with ThreadPoolExecutor(max_workers=4) as ex:
        texts = list(ex.map(lambda f: isa_hazards.shipped_asm(os.path.join(gp.CSRC, f), gp.SHIPPED_FLAGS), UNITS))
    for unit, text in zip(UNITS, texts):
        res = gp.check_text(text)
        # {8 x 2, 16 x 1, 16 x 2} x {f32, pre-quantised}; the two-type unit: two pairs x {16 x 1, 16 x 2} x {f32, Q8_K}
        assert len(res) == (8 if unit == "gemv_dual.hip" else 6), (unit, list(res))
        for kernel, prob in res.items():
            assert prob is None, (unit, kernel[:90], prob)
        # no FLAT access and no stack in them either
        hygiene = {k: v for k, v in isa_hazards.decode_hygiene(text).items() if "early_kernel" in k}
        assert len(hygiene) == len(res)
        for kernel, probs in hygiene.items():
            assert not probs, (unit, kernel[:90], probs)


def test_checker_sees_a_load_behind_the_wait():
    asm = """
_Z20gemv_kq_early_kernelI10q4k_traitsLi1ELi0ELi16ELi1EEvPKhS2_S2_S2_iiiii9gemv_mats: ; @demo
	s_load_dwordx2 s[2:3], s[0:1], 0x0
	s_waitcnt lgkmcnt(0)
	s_branch .LBB0_0
	.p2align	8
.LBB0_0:
	buffer_load_dwordx4 v[14:17], v2, s[28:31], 0 offen
	s_load_dwordx16 s[52:67], s[0:1], 0x38
	buffer_load_dwordx4 v[2:5], v6, s[0:3], 0 offen nt
	buffer_load_dwordx4 v[6:9], v6, s[0:3], 0 offen offset:1024 nt
	s_waitcnt lgkmcnt(0)
	buffer_load_dwordx4 v[10:13], v10, s[0:3], 0 offen nt
	s_endpgm
.Lfunc_end0:
	.amdhsa_kernel _Z20gemv_kq_early_kernelI10q4k_traitsLi1ELi0ELi16ELi1EEvPKhS2_S2_S2_iiiii9gemv_mats
		.amdhsa_user_sgpr_kernarg_preload_length 13
	.end_amdhsa_kernel
"""
    (prob,) = gp.check_text(asm).values()
    assert prob is not None and "[3]" in prob
    ok = asm.replace("\ts_waitcnt lgkmcnt(0)\n\tbuffer_load_dwordx4 v[10:13], v10, s[0:3], 0 offen nt\n",
                     "\tbuffer_load_dwordx4 v[10:13], v10, s[0:3], 0 offen nt\n\ts_waitcnt lgkmcnt(0)\n")
    assert list(gp.check_text(ok).values()) == [None]
    few = ok.replace("preload_length 13", "preload_length 9")
    assert "preloaded" in list(gp.check_text(few).values())[0]
