"""lfamd_pack_weights, the model-load path, with a parent build's library and with this tree's: device events
around 20 back-to-back calls, the two libraries alternated window by window in one process, the median of 5 rounds.  The tree's median
may exceed the parent's by no more than the parent's own range (max - min) over its rounds; the script exits 1 otherwise.

    python tools/pack_image_bench.py PARENT_SO [OUT.txt]     PARENT_SO: libllamafile_amd_hip.so built from the parent commit"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import pack_image_cases as pic  # noqa: E402
from llamafile_amd import _hip, ggml_types as T, synth  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pack_images.txt")
LIBS = {"parent": pic.bind(os.path.abspath(sys.argv[1])), "tree": pic.bind(_hip.HIP_SO)}
CALLS, ROUNDS = 20, 5
SHAPES = [(T.Q4_K, 14336, 4096), (T.Q6_K, 128256, 4096), (T.Q5_1, 14336, 4096), (T.Q3_K, 14336, 4096), (T.IQ4_XS, 14336, 4096),
          (T.Q4_0 | pic.PAD, 14336, 4000)]
lines, ok = [], True


def say(s):
    print(s, flush=True)
    lines.append(s)


for L in LIBS.values():
    assert L.lfamd_init(0) == 0
say(f"# lfamd_pack_weights, us per call: {ROUNDS} rounds of {CALLS} back-to-back calls between device events, parent and tree alternated")
say(f"# device: {torch.cuda.get_device_name(0)}")
say(f"# {'type':14s} {'rows x cols':>14s}  {'parent median [min .. max]':>34s}  {'tree median [min .. max]':>34s}  tree - parent  allowed")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for t, rows, cols in SHAPES:
    raw = synth.random_weights(t & ~pic.PAD, 64, cols, 5)  # 64 distinct rows, repeated: the time does not depend on the values
    d_raw = torch.from_numpy(raw).cuda().repeat((rows + 63) // 64, 1)[:rows].contiguous()
    size = LIBS["parent"].lfamd_packed_size(t, rows, cols)
    assert size == LIBS["tree"].lfamd_packed_size(t, rows, cols) > 0
    outs = {k: torch.empty(size, dtype=torch.uint8, device="cuda") for k in LIBS}

    def run(k):
        assert LIBS[k].lfamd_pack_weights(t, rows, cols, C.c_void_p(d_raw.data_ptr()), raw.shape[1], C.c_void_p(outs[k].data_ptr()), st) == 0

    for k in LIBS:
        for _ in range(3):
            run(k)
    torch.cuda.synchronize()
    assert torch.equal(outs["parent"], outs["tree"])
    us = {k: [] for k in LIBS}
    for _ in range(ROUNDS):
        for k in LIBS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                run(k)
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1000.0 / CALLS)
    med = {k: statistics.median(v) for k, v in us.items()}
    allowed = max(us["parent"]) - min(us["parent"])
    good = med["tree"] - med["parent"] <= allowed
    ok = ok and good
    cell = {k: f"{med[k]:9.2f} [{min(v):9.2f} .. {max(v):9.2f}]" for k, v in us.items()}
    say(f"  {pic.type_name(t):14s} {rows:>7d} x {cols:<5d}  {cell['parent']:>34s}  {cell['tree']:>34s}  {med['tree'] - med['parent']:+12.2f}  "
        f"{allowed:7.2f}{'' if good else '  OVER'}")
    del d_raw, outs
    torch.cuda.empty_cache()
say("within the parent's range at every shape" if ok else "OVER the parent's range at a shape")
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
