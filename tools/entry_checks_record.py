"""Record what the entry points of a library built at the parent commit (every operator of tests/entry_checks_cases.py: the two
flash-attention calls, lfamd_cpy, the two batched products) answer to the refused and the empty calls of that module:
tests/golden/entry_checks_parent.json, (rc, message) per case, which tests/test_entry_checks.py holds this tree's check functions
and entry points to.  The calls carry made-up addresses, so only cases their author marked
REFUSED or EMPTY are sent — a refusal comes before any device call — and never where a GPU is present: a call that passed the checks
after all would launch on those addresses.  Without a device such a call answers LFAMD_ERR_HIP, which fails the recording.

    python tools/entry_checks_record.py PARENT_SO [OUT.json]     PARENT_SO: libllamafile_amd_hip.so built from the parent commit"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (first: its HIP runtime is the one the library must resolve to, as in llamafile_amd/_hip.py)
import entry_checks_cases as cases  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
if torch.cuda.is_available():
    sys.exit("a GPU is present: the recorder sends made-up addresses to the entry points and runs on a machine without one only")
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "entry_checks_parent.json")
P = cases.bind(os.path.abspath(sys.argv[1]))
doc = {}
for op, (_, _, table, _) in cases.OPERATORS.items():
    doc[op] = {}
    for name, expectation, changes in table:
        if expectation not in (cases.REFUSED, cases.EMPTY):
            continue  # (a call that passes the checks is never sent)
        rc, message = cases.call(P, op, changes, check=False)
        assert rc != cases.ERR_HIP, (op, name, "passed the checks and reached the device layer", message)
        assert (rc == 0) == (expectation == cases.EMPTY), (op, name, expectation, rc, message)
        doc[op][name] = [rc, message]
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{sum(len(v) for v in doc.values())} cases -> {OUT}")
