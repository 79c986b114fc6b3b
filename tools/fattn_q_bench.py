#!/usr/bin/env python3
"""Device time of lfamd_flash_attn_q on Llama-3-8B attention (32 heads, 8 KV heads, D = 128) with a Q8_0 and with a Q4_0 K / V cache,
beside lfamd_flash_attn on an F16 cache of the same shape, timed in the same process: the yardstick (the code before
lfamd_flash_attn_q served these nodes on the CPU with cache copies around them, which is not a kernel time).

  decode   n_q = 1, n_kv in 512 / 4096 / 16384, no mask       -> TB/s of the K + V bytes each call reads
  prefill  n_q = n_kv in 512 / 2048, causal F16 mask           -> TFLOP/s of 4 * heads * n_q * n_kv * D / 2 (the causal half)

The method is tools/fattn_bench.py's: device events on the null stream around back-to-back calls, warm-up first, every window at
least --window seconds, the three paths alternated inside one process for --rounds rounds; median and min .. max of the rounds.  The
F16 cache holds f16(d * code) of the Q8_0 blocks, so the n_q > 8 results of the Q8_0 call must be the F16 call's bits, which is
checked before anything is timed.  The operands stay in place between calls: a decode figure is a rate of the call, not of HBM."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import fattn_q_ref as QR  # noqa: E402
from fattn_bench import D, HEADS, KV_HEADS, window  # noqa: E402
from llamafile_amd import _hip, ggml_types as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", choices=("all", "decode", "prefill"), default="all")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "fattn_q_bench.py measures on the GPU: there is no CPU fallback"
    lib = _hip.lib()
    _hip.check(lib.lfamd_init(0), "lfamd_init")
    rng = np.random.default_rng(1)
    scale = 1.0 / math.sqrt(D)
    lines = []
    for n_q, n_kv in [(1, 512), (1, 4096), (1, 16384), (512, 512), (2048, 2048)]:
        if args.shapes != "all" and (args.shapes == "decode") != (n_q == 1):
            continue
        Q = torch.from_numpy(rng.standard_normal((n_q, HEADS, D)).astype(np.float32)).cuda()  # memory [n_q][heads][D]
        kv = [rng.standard_normal((n_kv, KV_HEADS, D)).astype(np.float32) for _ in range(2)]  # the permuted -fa cache
        raw = {t: [QR.quantise(t, x) for x in kv] for t in QR.TYPES}
        caches = {t: [torch.from_numpy(r).cuda() for r in raw[t]] for t in QR.TYPES}
        caches[T.F16] = [torch.from_numpy(QR.dequantise(T.Q8_0, r).astype(np.float16)).cuda() for r in raw[T.Q8_0]]
        mask = None
        if n_q > 1:
            mask = torch.full((n_q, n_kv), float("-inf"), device="cuda").triu(1 + n_kv - n_q).half()
        out = {t: torch.empty((n_q, HEADS, D), device="cuda") for t in caches}
        ws_bytes = lib.lfamd_flash_attn_workspace(D, n_q, n_kv, HEADS, KV_HEADS, 1)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")

        def call(t):
            row = 2 * D if t == T.F16 else QR.row_bytes(t, D)
            fn = lib.lfamd_flash_attn if t == T.F16 else lib.lfamd_flash_attn_q
            K, V = caches[t]
            _hip.check(fn(Q.data_ptr(), HEADS * D * 4, D * 4, n_q * HEADS * D * 4, t, K.data_ptr(), KV_HEADS * row, row, n_kv * KV_HEADS * row,
                          t, V.data_ptr(), KV_HEADS * row, row, n_kv * KV_HEADS * row, mask.data_ptr() if mask is not None else None, n_kv * 2,
                          D, n_q, n_kv, HEADS, KV_HEADS, 1, scale, 0.0, out[t].data_ptr(), D * 4, HEADS * D * 4, n_q * HEADS * D * 4,
                          ws.data_ptr(), ws_bytes, 0, None), "lfamd_flash_attn" + ("" if t == T.F16 else "_q"))

        # agreement first: every path against torch in f64 on its own cache contents; Q8_0 against the F16 call's bits where n_q > 8
        diff = {}
        for t in caches:
            call(t)
            torch.cuda.synchronize()
            Kd, Vd = (c.double() if t == T.F16 else torch.from_numpy(QR.dequantise(t, r)).cuda().double() for c, r in zip(caches[t], raw.get(t, kv)))
            Kx, Vx = (x.permute(1, 0, 2).repeat_interleave(HEADS // KV_HEADS, 0) for x in (Kd, Vd))
            s = torch.einsum("jhd,htd->hjt", Q.double(), Kx) * scale
            if mask is not None:
                s = s + mask.double()[None]
            ref = torch.einsum("hjt,htd->jhd", torch.softmax(s, -1), Vx)
            diff[t] = float((out[t].double() - ref).abs().max() / ref.abs().max())
            del Kd, Vd, Kx, Vx, s, ref
        if n_q > 8:
            assert torch.equal(out[T.Q8_0].view(torch.int32), out[T.F16].view(torch.int32)), "Q8_0 is not the F16 call's bits"
        times = {t: [] for t in caches}
        for _ in range(args.rounds):
            for t in (T.F16, T.Q8_0, T.Q4_0):
                times[t].append(window(torch, lambda: call(t), args.window))
        row = {"n_q": n_q, "n_kv": n_kv}
        for t in (T.F16, T.Q8_0, T.Q4_0):
            name, med = T.NAMES[t].lower(), statistics.median(times[t])
            row[name + "_us"] = round(med, 2)
            row[name + "_min_max"] = [round(min(times[t]), 2), round(max(times[t]), 2)]
            row[name + "_max_rel_diff_vs_f64"] = diff[t]
            kv_bytes = 2 * n_kv * KV_HEADS * (2 * D if t == T.F16 else QR.row_bytes(t, D))
            if n_q == 1:
                row[name + "_kv_TB_per_s"] = round(kv_bytes / med * 1e-6, 3)
            else:
                row[name + "_causal_TFLOP_per_s"] = round(4 * HEADS * n_q * n_kv * D / 2 / med * 1e-6, 1)
            if t != T.F16:
                row[name + "_over_f16"] = round(med / statistics.median(times[T.F16]), 3)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del Q, caches, out, ws, mask
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/fattn_q_bench.py --window {args.window} --rounds {args.rounds} on {torch.cuda.get_device_name(0)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
