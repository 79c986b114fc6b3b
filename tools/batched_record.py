"""Record the batched attention products of a library built at the parent commit: tests/golden/mul_mat_batched_parent.json, which
tests/test_gpu_batched_parent_bits.py holds this tree's lfamd_mul_mat_batched and lfamd_mul_mat_batched_q to, bit for bit (DESIGN.md
section 27).  Per case (tests/batched_cases.py): the SHA-256 of the A image, of the B image, and of the whole sentinel-prefilled result
buffer after the call.  Needs a GPU.

    python tools/batched_record.py PARENT_SO [OUT.json]     PARENT_SO: libllamafile_amd_hip.so built from the parent commit"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401  (first: its HIP runtime is the one the library must resolve to, as in llamafile_amd/_hip.py)
import batched_case  # noqa: E402
import batched_cases as cases  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "mul_mat_batched_parent.json")
P = cases.bind(os.path.abspath(sys.argv[1]))
assert P.lfamd_init(0) == 0
dev = batched_case.Dev()
doc = {"seed": cases.SEED, "cases": {cases.case_id(c): cases.digest(dev, P, c) for c in cases.cases()}}
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(doc['cases'])} cases -> {OUT}")
