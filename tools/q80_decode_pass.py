#!/usr/bin/env python3
"""Llama-3-8B Q8_0 decode pass (BASELINE config 3) with and without LFAMD_FLAG_Q80_RELAXED, on the GPU box (development tool).

Builds bench.Runner over llama_shapes.llama3_8b_q8_0(), captures the batch-1 pass twice — runner.flags (the bit-exact GEMV) and
runner.flags | FLAG_Q80_RELAXED — and times alternated replays of the two graphs with device events.  Prints one JSON line: the
two pass times (median of the repeats), GB/s over weight_bytes(), and the spread (min .. max) of the repeats of each.
    python tools/q80_decode_pass.py [--repeats 7] [--replays 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from llamafile_amd import _hip, llama_shapes as LS, sgemm  # noqa: E402


def capture(runner, flags, dev):
    runner.flags = flags
    runner.run_pass(1)  # warm: kernel attributes are set before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g.capture_begin(capture_error_mode="thread_local")
        runner.run_pass(1)
        g.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / replays


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--replays", type=int, default=10)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    sgemm.init(0)
    runner = bench.Runner(LS.llama3_8b_q8_0(), 0, 1, (1,), dev)
    base = runner.flags
    graphs = {"exact": capture(runner, base, dev), "relaxed": capture(runner, base | _hip.FLAG_Q80_RELAXED, dev)}
    ms = {name: [] for name in graphs}
    for _ in range(a.repeats):  # alternated: drift of the clocks lands on both
        for name, g in graphs.items():
            ms[name].append(timed(g, a.replays))
    wb = runner.weight_bytes()
    res = {"model": "llama3-8b-q8_0", "weight_bytes": wb, "repeats": a.repeats, "replays": a.replays}
    for name, v in ms.items():
        med = statistics.median(v)
        res[f"{name}_pass_ms"] = round(med, 4)
        res[f"{name}_GBps"] = round(wb / (med * 1e-3) / 1e9, 1)
        res[f"{name}_tokens_per_s"] = round(1e3 / med, 1)
        res[f"{name}_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
