#!/usr/bin/env python3
"""Device time of lfamd_cpy on the K / V cache stores of Llama-3-8B (n_embd_k_gqa = n_embd_v_gqa = 1024, a cache of 4096 cells) beside
yardsticks measured in the same process:

  512-token stores, the 512-cell moves   hipMemcpyAsync device-to-device of (source bytes + destination bytes) / 2 bytes: the same
                                         traffic (a copy of n bytes reads n and writes n) without the conversion.  Both are streaming
                                         passes; the margin to allow is the spread of the copy's own windows.
  one-token stores (launch-bound)        lfamd_memset of the destination's bytes on the same stream: one launch
  transposed V store                     also the general route on the same operands, selected by describing them with a dimension of
                                         extent 1 between the two (a layout the transposed route does not take; the same bytes)

Device events around back-to-back calls, warm-up first, every window at least --window seconds, the call and its yardstick alternated
for --rounds rounds; median and min .. max of the rounds.  Two modes, because a call of a few microseconds is shorter than the host
takes to enqueue it:
  eager   calls issued one by one on the null stream: the rate at which this host enqueues the call (its checks included)
  graph   --chain calls captured as one chain of a graph and replayed: the device's time per call, launch to launch
The operands stay in place between calls: at these sizes (4 KB - 3 MB) they are served from the on-die caches, so a figure is a rate
of the call, not of HBM."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamafile_amd import _hip, ggml_types as T  # noqa: E402

WIDTH, N_CTX, HEAD = 1024, 4096, 1000


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


def loaded_hip_runtime():
    """The HIP runtime this process already runs on (torch's): a second one must not be loaded."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


def arr(ctype, v):
    return (ctype * 4)(*v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chain", type=int, default=32, help="calls per captured graph")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "cpy_bench.py measures on the GPU: there is no CPU fallback"
    lib = _hip.lib()
    _hip.check(lib.lfamd_init(0), "lfamd_init")
    hip = loaded_hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    gen = torch.Generator(device="cuda").manual_seed(1)
    scratch_a = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    scratch_b = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    lines = []

    def cpy(st, ps, s_ne, s_nb, dt, pd, d_ne, d_nb):
        a = (st, ps, arr(C.c_long, s_ne), arr(C.c_size_t, s_nb), dt, pd, arr(C.c_long, d_ne), arr(C.c_size_t, d_nb), 0)
        return lambda stream: _hip.check(lib.lfamd_cpy(*a, stream), "lfamd_cpy")

    cases, keep = [], []

    def measure(name, n_tok, fn, src_bytes, dst_bytes, pd, other=None):
        """Queue fn beside its yardstick (and `other`, a second route on the same operands)."""
        half = (src_bytes + dst_bytes) // 2
        if n_tok == 1:
            yard_name, yard = "memset_us", lambda stream: _hip.check(lib.lfamd_memset(pd, 0, dst_bytes, stream), "lfamd_memset")
        else:
            def yard(stream):
                assert hip.hipMemcpyAsync(scratch_b.data_ptr(), scratch_a.data_ptr(), half, 3, stream) == 0  # hipMemcpyDeviceToDevice
            yard_name = "memcpy_us"
        row = {"case": name, "n_tok": n_tok, "src_bytes": src_bytes, "dst_bytes": dst_bytes}
        if n_tok != 1:
            row["yard_bytes"] = half
        cases.append((row, yard_name, fn, yard, other))

    def graphed(fn):
        """args.chain calls of fn captured as one chain; a replay is args.chain calls without the host's enqueue between them."""
        fn(None)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            stream = torch.cuda.current_stream().cuda_stream
            for _ in range(args.chain):
                fn(stream)
        keep.append(g)
        return g.replay

    def run_all(mode):
        for row, yard_name, fn, yard, other in cases:
            if mode == "eager":
                f, y, o, per = (lambda: fn(None)), (lambda: yard(None)), ((lambda: other(None)) if other else None), 1
            else:
                f, y, o, per = graphed(fn), graphed(yard), (graphed(other) if other else None), args.chain
            t = {"call": [], "yard": [], "other": []}
            for _ in range(args.rounds):
                t["call"].append(window(torch, f, args.window) / per)
                t["yard"].append(window(torch, y, args.window) / per)
                if o:
                    t["other"].append(window(torch, o, args.window) / per)
            mc, my = statistics.median(t["call"]), statistics.median(t["yard"])
            out = dict(row, mode=mode)
            out.update({"cpy_us": round(mc, 2), "cpy_min_max": [round(min(t["call"]), 2), round(max(t["call"]), 2)], yard_name: round(my, 2),
                        "yard_min_max": [round(min(t["yard"]), 2), round(max(t["yard"]), 2)], "cpy_over_yard": round(mc / my, 2),
                        "GB_per_s": round((row["src_bytes"] + row["dst_bytes"]) / mc * 1e-3, 1)})
            if o:
                mo = statistics.median(t["other"])
                out.update({"general_us": round(mo, 2), "general_min_max": [round(min(t["other"]), 2), round(max(t["other"]), 2)],
                            "general_over_cpy": round(mo / mc, 2)})
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))

    for n_tok in (1, 512):
        n = WIDTH * n_tok
        src = torch.randn(n, device="cuda", generator=gen)
        for t in (T.F16, T.Q8_0, T.Q4_0):  # the K store (and the V store under -fa): contiguous F32 into a 1-D view at cell HEAD
            row = T.row_size(t, WIDTH)
            cache = torch.zeros(N_CTX * row, dtype=torch.uint8, device="cuda")
            pd = cache.data_ptr() + HEAD * row
            ne = (n, 1, 1, 1)
            nb = (T.TYPE_SIZE[t], row * n_tok, row * n_tok, row * n_tok)
            measure(f"{T.NAMES[t]} rows", n_tok, cpy(T.F32, src.data_ptr(), (WIDTH, n_tok, 1, 1), (4, 4 * WIDTH, 4 * n, 4 * n), t, pd, ne, nb), 4 * n,
                    row * n_tok, pd)
            keep.append(cache)
        # the V store without -fa: the transposed view of v_cur [WIDTH, n_tok] into [n_tok, WIDTH] F16 rows N_CTX elements apart
        cache = torch.zeros(N_CTX * WIDTH * 2, dtype=torch.uint8, device="cuda")
        pd = cache.data_ptr() + HEAD * 2
        d_nb = (2, N_CTX * 2, N_CTX * 2 * WIDTH, N_CTX * 2 * WIDTH)
        fn = cpy(T.F32, src.data_ptr(), (n_tok, WIDTH, 1, 1), (4 * WIDTH, 4, 4 * n, 4 * n), T.F16, pd, (n_tok, WIDTH, 1, 1), d_nb)
        general = cpy(T.F32, src.data_ptr(), (n_tok, 1, WIDTH, 1), (4 * WIDTH, 4, 4, 4 * n), T.F16, pd, (n_tok, 1, WIDTH, 1),
                      (2, N_CTX * 2, N_CTX * 2, N_CTX * 2 * WIDTH))
        measure("F16 transposed V", n_tok, fn, 4 * n, 2 * n, pd, other=general if n_tok > 1 else None)
        keep += [cache, src]
    for t in (T.F16, T.Q8_0):  # defragmentation: 512 cells moved inside one cache
        row = T.row_size(t, WIDTH)
        cache = torch.zeros(N_CTX * row, dtype=torch.uint8, device="cuda")
        ne = (WIDTH * 512, 1, 1, 1)
        nb = (T.TYPE_SIZE[t], row * 512, row * 512, row * 512)
        pd = cache.data_ptr() + 100 * row
        measure(f"{T.NAMES[t]} move of 512 cells", 512, cpy(t, cache.data_ptr() + 2000 * row, ne, nb, t, pd, ne, nb), row * 512, row * 512, pd)
        keep.append(cache)
    run_all("eager")  # every eager window before the first capture
    run_all("graph")
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# tools/cpy_bench.py --window {args.window} --rounds {args.rounds} --chain {args.chain} on {torch.cuda.get_device_name(0)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
