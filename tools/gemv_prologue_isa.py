"""development / CPU test: the prologue of the decode GEMV's EARLY kernels in the gfx950 ISA of the shipped build.

A one-column launch of one to three matrices (gemv_kq_early_kernel) and the two-type launch (gemv_kq_dual_early_kernel) address
their first item from PRELOADED kernel arguments, so every load of that item, and the activation loads in front of it, must be
issued before the first `s_waitcnt lgkmcnt` — the wait for the scalar loads of the matrix table.  This walks every path from
the kernel's entry (behind the preload preamble) to its first such wait and counts the buffer loads on it.

usage: python3 tools/gemv_prologue_isa.py [gemv_q4k.hip ...]   (default: every decode unit)"""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hazards  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llamafile_amd", "csrc")
UNITS = ["gemv_q4k.hip", "gemv_q5k.hip", "gemv_q6k.hip", "gemv_q40.hip", "gemv_q41.hip", "gemv_q50.hip", "gemv_q51.hip", "gemv_q2k.hip",
         "gemv_q3k.hip", "gemv_iq4xs.hip", "gemv_iq4nl.hip", "gemv_dual.hip"]
SHIPPED_FLAGS = ("-mllvm", "-amdgpu-kernarg-preload-count=13")  # csrc/Makefile
PRELOAD_DWORDS = 13  # what the first item needs (the two-type kernel's fourteenth, grid_b, is granted as well)

# buffer loads of one super-block (TR::load of gemv_impl.h) and whether the type's activations are Q8_K, by mangled traits name
TRAITS = {"10q4k_traits": (3, True), "10q5k_traits": (4, True), "10q6k_traits": (5, True), "10q40_traits": (3, False),
          "12iq4nl_traits": (3, False), "11iq4c_traits": (3, True), "10pcl_traitsILi3EE": (4, False), "10pcl_traitsILi6EE": (4, False),
          "10pcl_traitsILi7EE": (5, False), "9pk_traitsILi10EE": (3, True), "9pk_traitsILi11EE": (4, True)}
F32, Q8_K = 0, 15


def expected_loads(traits, bt, nw, ch):
    """activation loads that go out ahead of the weights (gemv_kq_body1: JX float4 per lane, or the codes and the scale of a
    pre-quantised Q8_K block) + the first item's weight loads"""
    per_sb, act_q8k = TRAITS[traits]
    jx = 1 if ch == 1 else (2 if nw == 8 else 4)
    act = jx if bt == F32 else 2 if (bt == Q8_K and act_q8k and jx <= 2) else 0
    return act + ch * per_sb


def parse_name(name):
    m = re.match(r"_Z\d+gemv_kq_dual_early_kernelI(.+?)Li(\d+)ELi(\d+)ELi(\d+)EEv", name) or \
        re.match(r"_Z\d+gemv_kq_early_kernelI(.+?)Li1ELi(\d+)ELi(\d+)ELi(\d+)EEv", name)  # (one type: NC = 1 first)
    if not m:
        return None
    traits = re.findall(r"\d+(?:pcl|pk)_traitsILi\d+EE|\d+\w+?_traits", m.group(1))
    return traits, int(m.group(2)), int(m.group(3)), int(m.group(4))


def paths_to_table_wait(body):
    """buffer loads on every path from the entry to the first wait on lgkmcnt: [count, ...]; None where a path runs in a circle
    without one (paths that end the program are left out)"""
    lines = [ln.strip() for ln in body.split("\n")]
    start = next((i + 1 for i, ln in enumerate(lines[:40]) if ln.startswith(".p2align")), 0)  # behind the preload preamble
    labels = {ln[:-1]: i for i, ln in enumerate(lines) if re.match(r"\.LBB\w+:$", ln)}
    out, todo, seen = [], [(start, 0)], set()
    while todo:
        i, n = todo.pop()
        while True:
            if i >= len(lines) or (i, n) in seen:
                out.append(None)
                break
            seen.add((i, n))
            ln = lines[i]
            if ln.startswith("buffer_load"):
                n += 1
            elif ln.startswith("s_waitcnt") and "lgkmcnt" in ln:
                out.append(n)
                break
            elif ln.startswith("s_endpgm"):  # (a path that leaves without an item: the structuriser's exits)
                break
            elif ln.startswith("s_cbranch"):
                todo.append((labels[ln.split()[-1]], n))
            elif ln.startswith("s_branch"):
                i = labels[ln.split()[-1]]
                continue
            i += 1
    return out


def check_text(text):
    """{kernel: problem or None} for every early kernel of a unit's assembly"""
    res = {}
    granted = dict(re.findall(r"\.amdhsa_kernel (\S+).*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", text, re.S))
    for name, body in re.findall(r"^(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end", text, re.S | re.M):
        parsed = parse_name(name)
        if not parsed:
            continue
        traits, bt, nw, ch = parsed
        want = sorted(expected_loads(t, bt, nw, ch) for t in traits)
        got = paths_to_table_wait(body)
        prob = None
        if int(granted.get(name, -1)) < PRELOAD_DWORDS:
            prob = f"{granted.get(name)} dwords preloaded, fewer than {PRELOAD_DWORDS}"
        elif None in got or len(got) != len(want) or sorted(got) != want:
            prob = f"buffer loads ahead of the table wait per path: {got}, expected {want}"
        res[name] = prob
    return res


def check_unit(unit):
    return check_text(isa_hazards.shipped_asm(os.path.join(CSRC, unit), SHIPPED_FLAGS))


if __name__ == "__main__":
    units = sys.argv[1:] or UNITS
    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(check_unit, units))
    bad = 0
    for unit, res in zip(units, results):
        for kernel, prob in res.items():
            print(unit, kernel[:90], "ok" if prob is None else "BAD: " + prob)
            bad += prob is not None
        if not res:
            print(unit, "no early kernel found")
            bad += 1
    sys.exit(1 if bad else 0)
