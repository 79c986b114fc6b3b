#!/usr/bin/env python3
"""Device time of lfamd_flash_attn on Llama-3-8B attention (32 heads, 8 KV heads, D = 128) beside the path a graph without -fa takes
for the same layer: lfamd_mul_mat_batched for KQ on the permuted K cache plus lfamd_mul_mat_batched for KQV on a transposed V cache.
The two products do strictly less arithmetic than the fused call (no scale, mask or softmax) and move strictly more bytes (the scores
out and back), so their sum is the yardstick: the fused call should not be slower at any shape.

  decode   n_q = 1, n_kv in 512 / 4096 / 16384, no mask       -> TB/s of the K + V bytes
  prefill  n_q = n_kv in 512 / 2048, causal F16 mask           -> TFLOP/s of 4 * heads * n_q * n_kv * D / 2 (the causal half)

Device events on the null stream around back-to-back calls, warm-up first, every window at least --window seconds, the two paths
alternated inside one process for --rounds rounds; median and min .. max of the rounds.  The operands stay in place between calls:
the 2 - 64 MB caches are served from the on-die caches and the MALL, so a decode figure is a rate of the call, not of HBM."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamafile_amd import _hip, ggml_types as T  # noqa: E402

HEADS, KV_HEADS, D = 32, 8, 128


def window(torch, fn, seconds):
    """Average device time (us) of fn over a window of at least `seconds`."""
    fn()
    torch.cuda.synchronize()
    iters, us = 4, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        us = ms * 1e3 / iters
        if ms >= seconds * 1e3:
            return us
        iters = max(iters * 2, int(iters * seconds * 1e3 / max(ms, 1e-3) * 1.2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", choices=("all", "decode", "prefill"), default="all")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "fattn_bench.py measures on the GPU: there is no CPU fallback"
    lib = _hip.lib()
    _hip.check(lib.lfamd_init(0), "lfamd_init")
    gen = torch.Generator(device="cuda").manual_seed(1)
    scale = 1.0 / math.sqrt(D)
    lines = []
    for n_q, n_kv in [(1, 512), (1, 4096), (1, 16384), (512, 512), (2048, 2048)]:
        if args.shapes != "all" and (args.shapes == "decode") != (n_q == 1):
            continue
        Q = torch.randn((n_q, HEADS, D), device="cuda", generator=gen)                 # memory [n_q][heads][D]
        K = torch.randn((n_kv, KV_HEADS, D), device="cuda", generator=gen).half()      # the permuted -fa / no -fa K cache
        V = torch.randn((n_kv, KV_HEADS, D), device="cuda", generator=gen).half()      # -fa: not transposed
        Vt = V.permute(1, 2, 0).contiguous()                                            # no -fa: [kv head][D][n_kv]
        mask = None
        if n_q > 1:
            mask = torch.full((n_q, n_kv), float("-inf"), device="cuda").triu(1 + n_kv - n_q).half()
        S = torch.empty((HEADS, n_q, n_kv), device="cuda")
        O1 = torch.empty((n_q, HEADS, D), device="cuda")
        O2 = torch.empty((HEADS, n_q, D), device="cuda")
        ws_bytes = lib.lfamd_flash_attn_workspace(D, n_q, n_kv, HEADS, KV_HEADS, 1)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")

        def fused():
            _hip.check(lib.lfamd_flash_attn(Q.data_ptr(), HEADS * D * 4, D * 4, n_q * HEADS * D * 4, T.F16, K.data_ptr(), KV_HEADS * D * 2, D * 2,
                                            n_kv * KV_HEADS * D * 2, T.F16, V.data_ptr(), KV_HEADS * D * 2, D * 2, n_kv * KV_HEADS * D * 2,
                                            mask.data_ptr() if mask is not None else None, n_kv * 2, D, n_q, n_kv, HEADS, KV_HEADS, 1, scale, 0.0,
                                            O1.data_ptr(), D * 4, HEADS * D * 4, n_q * HEADS * D * 4, ws.data_ptr(), ws_bytes, 0, None),
                       "lfamd_flash_attn")

        def two_products():
            _hip.check(lib.lfamd_mul_mat_batched(T.F16, K.data_ptr(), n_kv, D, KV_HEADS * D * 2, D * 2, n_kv * KV_HEADS * D * 2, KV_HEADS, 1,
                                                 Q.data_ptr(), n_q, HEADS * D * 4, D * 4, n_q * HEADS * D * 4, HEADS, 1, S.data_ptr(), n_kv * 4,
                                                 n_q * n_kv * 4, HEADS * n_q * n_kv * 4, 0, None), "lfamd_mul_mat_batched KQ")
            _hip.check(lib.lfamd_mul_mat_batched(T.F16, Vt.data_ptr(), D, n_kv, n_kv * 2, D * n_kv * 2, KV_HEADS * D * n_kv * 2, KV_HEADS, 1,
                                                 S.data_ptr(), n_q, n_kv * 4, n_q * n_kv * 4, HEADS * n_q * n_kv * 4, HEADS, 1, O2.data_ptr(), D * 4,
                                                 n_q * D * 4, HEADS * n_q * D * 4, 0, None), "lfamd_mul_mat_batched KQV")

        # agreement first: the fused call against torch in f64
        fused()
        torch.cuda.synchronize()
        Kx = K.double().permute(1, 0, 2).repeat_interleave(HEADS // KV_HEADS, 0)
        Vx = V.double().permute(1, 0, 2).repeat_interleave(HEADS // KV_HEADS, 0)
        s = torch.einsum("jhd,htd->hjt", Q.double(), Kx) * scale
        if mask is not None:
            s = s + mask.double()[None]
        ref = torch.einsum("hjt,htd->jhd", torch.softmax(s, -1), Vx)
        diff = float((O1.double() - ref).abs().max() / ref.abs().max())
        del Kx, Vx, s, ref
        t = {"fused": [], "two": []}
        for _ in range(args.rounds):
            t["fused"].append(window(torch, fused, args.window))
            t["two"].append(window(torch, two_products, args.window))
        mf, mt = statistics.median(t["fused"]), statistics.median(t["two"])
        row = {"n_q": n_q, "n_kv": n_kv, "fused_us": round(mf, 2), "fused_min_max": [round(min(t["fused"]), 2), round(max(t["fused"]), 2)],
               "two_products_us": round(mt, 2), "two_min_max": [round(min(t["two"]), 2), round(max(t["two"]), 2)],
               "two_over_fused": round(mt / mf, 2), "max_rel_diff_vs_f64": diff}
        if n_q == 1:
            row["kv_TB_per_s"] = round(2 * n_kv * KV_HEADS * D * 2 / mf * 1e-6, 3)
        else:
            row["causal_TFLOP_per_s"] = round(4 * HEADS * n_q * n_kv * D / 2 / mf * 1e-6, 1)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del Q, K, V, Vt, S, O1, O2, ws, mask
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/fattn_bench.py --window {args.window} --rounds {args.rounds} on {torch.cuda.get_device_name(0)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
