"""What tools/attn_time.py and tools/attn_q_time.py share: the arguments, the timing loop and the output file.

Device events around back-to-back calls on the null stream, warm-up first, every window at least --window seconds, the routes
alternated round by round; per route the median of the rounds with their min and max."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEAD_DIM, HEADS, KV_HEADS = 128, 32, 8
SHAPES = [(512, 1), (4096, 1), (512, 512), (4096, 512)]


def parser(out_name):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", out_name))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="", help="n_kv:n,... (default: the four Llama-3-8B shapes)")
    return ap


def shapes_of(args):
    return [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")] if args.shapes else SHAPES


def time_routes(torch, runs, args):
    """{route: (median us per product, the JSON entry of the route)} for runs = {route: callable}."""
    def window(f, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per product

    reps = {}
    for v, f in runs.items():  # warm-up, and how many calls fill a window
        window(f, 3)
        reps[v] = max(3, math.ceil(args.window * 1e6 / window(f, 10)))
    times = {v: [] for v in runs}
    for _ in range(args.rounds):
        for v, f in runs.items():
            times[v].append(window(f, reps[v]))
    out = {}
    for v in runs:
        med = float(np.median(times[v]))
        out[v] = (med, {"us": round(med, 2), "us_min": round(min(times[v]), 2), "us_max": round(max(times[v]), 2),
                        "calls_per_window": reps[v]})
    return out


def write_doc(torch, args, routes, results):
    doc = {"device": torch.cuda.get_device_name(0), "heads": HEADS, "kv_heads": KV_HEADS, "head_dim": HEAD_DIM,
           "window_s": args.window, "rounds": args.rounds, "routes": routes, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
