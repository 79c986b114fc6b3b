#!/usr/bin/env python3
"""Q8_0 decode launches with and without LFAMD_FLAG_Q80_RELAXED on the GPU box (development tool): tools/kbench.py's measurement
(`--flags 0` against `--flags 128`) alternated in ONE process, f32 rows and pre-quantised rows, per shape.  One RESULT line per
shape and row format: {flags: (median, min, max)} in microseconds per launch over --repeats runs of each.
    python tools/q80_relaxed_kbench.py [--repeats 4] [--iters 20]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kbench  # noqa: E402
from llamafile_amd import _hip, sgemm  # noqa: E402

CASES = [(4096, 4096, 1), (14336, 4096, 1), (4096, 14336, 1), (4096, 4096, 4), (4096, 4096, 8), (1024, 4096, 1), (128256, 4096, 1)]

if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=4)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    sgemm.init(0)
    for m, k, n in CASES:
        for f32in in (True, False):
            us = {0: [], _hip.FLAG_Q80_RELAXED: []}
            for _ in range(a.repeats):
                for fl in us:
                    kbench.EXTRA_FLAGS = fl
                    us[fl].append(kbench.run("Q8_0", m, k, n, 0, a.iters, f32in=f32in))
            print("RESULT Q8_0", m, k, n, "f32" if f32in else "prequant",
                  {fl: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for fl, v in us.items()}, flush=True)
