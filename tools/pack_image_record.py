"""Record the weight images of a library built at the parent commit: tests/golden/pack_images_parent.json, which
tests/test_gpu_pack_images.py holds this tree's images to, byte for byte.  Per case (tests/pack_image_cases.py):
the SHA-256 of the raw rows, lfamd_packed_size, the SHA-256 of the 0xEE-prefilled output buffer after lfamd_pack_weights, and for
Q2_K / Q3_K / IQ4_XS the canonical builder's and the expander's outputs.  Needs a GPU; run without LFAMD_USE_BLASLT.

    python tools/pack_image_record.py PARENT_SO [OUT.json]     PARENT_SO: libllamafile_amd_hip.so built from the parent commit"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401  (first: its HIP runtime is the one the library must resolve to, as in llamafile_amd/_hip.py)
import pack_image_cases as pic  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "pack_images_parent.json")
P = pic.bind(os.path.abspath(sys.argv[1]))
assert P.lfamd_init(0) == 0 and not P.lfamd_vendor_gemm_available()
doc = {"seed": pic.SEED, "cases": {}, "sizes": {}}
for t, rows, cols in pic.cases():
    doc["cases"][pic.case_id(t, rows, cols)] = pic.digest(P, t, rows, cols)
for t, rows, cols in pic.size_only_cases():
    doc["sizes"][pic.case_id(t, rows, cols)] = P.lfamd_packed_size(t, rows, cols)
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(doc['cases'])} cases, {len(doc['sizes'])} sizes -> {OUT}")
