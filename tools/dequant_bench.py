#!/usr/bin/env python3
"""Timing of the weight read-back calls on the GPU box (development tool): lfamd_get_rows and lfamd_unpack_weights.

(i)   whole-matrix dequantisation to F16 and F32 of Q4_K 14336 x 4096, Q6_K 128256 x 4096, Q8_0 4096 x 4096;
(ii)  get_rows of 1 and of 512 random indices from Q6_K 128256 x 4096;
(iii) unpack of the first two.
Device events over `iters` back-to-back launches after a warm-up.  Beside each whole-matrix and unpack figure: a plain
device-to-device copy that moves the SAME total traffic (it copies (bytes read + bytes written) / 2 bytes, so it reads and writes
that many in all), timed in the same process, the two alternated `rounds` times; the median of each is printed with bytes moved,
microseconds, GB/s and the ratio to the copy.  Small tensors are visited round-robin over several copies, so they stream from HBM
and not from the 256 MiB Infinity Cache (cf. tools/kbench.py).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llamafile_amd import ggml_types as T, sgemm, synth  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def against_copy(label, fn, moved, iters, rounds):
    """fn(i) moves `moved` bytes (read + written); the copy moves the same."""
    half = (moved // 2 + 255) // 256 * 256
    ncp = max(2, min(8, int(1.2e9 // half) + 1))  # distinct buffers: the copy must not run out of the Infinity Cache either
    src = [torch.empty(half, dtype=torch.uint8, device="cuda").fill_(i) for i in range(ncp)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(ncp)]

    def cp(i):
        dst[i % ncp].copy_(src[i % ncp])

    for i in range(3):  # warm-up: both
        fn(i)
        cp(i)
    torch.cuda.synchronize()
    a, c = [], []
    for _ in range(rounds):  # alternated
        a.append(timed(fn, iters))
        c.append(timed(cp, iters))
    us, cus = statistics.median(a), statistics.median(c)
    print(f"{label:34s} {moved / 1e6:9.1f} MB {us:9.1f} us {moved / us / 1e3:8.1f} GB/s | copy {cus:9.1f} us {2 * half / cus / 1e3:8.1f} GB/s"
          f" | ratio {us / cus:5.2f}", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--small", action="store_true", help="1/8 of the rows (a quick look)")
    a = p.parse_args()
    sgemm.init(0)
    cases = [("Q4_K", 14336, 4096), ("Q6_K", 128256, 4096), ("Q8_0", 4096, 4096)]
    big = None
    for tname, rows, cols in cases:
        if a.small:
            rows //= 8
        t = T.BY_NAME[tname]
        raw = synth.random_weights_torch(t, rows, cols, 1)
        per = rows * T.row_size(t, cols)
        copies = max(1, min(16, int(600e6 // per) + 1))
        Ws = [sgemm.upload_weights(t, raw, rows, cols) for _ in range(copies)]
        del raw
        for dt, esz in ((torch.float16, 2), (torch.float32, 4)):
            outs = [torch.empty((rows, cols), dtype=dt, device="cuda") for _ in range(min(copies, 2))]
            against_copy(f"dequantize {tname} {rows}x{cols} -> {'F16' if esz == 2 else 'F32'}",
                         lambda i: sgemm.get_rows(Ws[i % copies], None, dt, 0, rows, out=outs[i % len(outs)]),
                         Ws[0].resident_bytes + rows * cols * esz, a.iters, a.rounds)
            del outs
        if tname != "Q8_0":
            rb = T.row_size(t, cols)
            raws = [torch.empty((rows, rb), dtype=torch.uint8, device="cuda") for _ in range(min(copies, 2))]
            L = sgemm._hip.lib()

            def unpack(i):
                W, r = Ws[i % copies], raws[i % len(raws)]
                rc = L.lfamd_unpack_weights(t, rows, cols, sgemm._ptr(W.data), sgemm._ptr(r), rb, sgemm._stream())
                assert rc == 0, L.lfamd_last_error()

            against_copy(f"unpack {tname} {rows}x{cols}", unpack, Ws[0].resident_bytes + rows * rb, a.iters, a.rounds)
            del raws
        if tname == "Q6_K":
            big = (Ws[0], rows, cols)
        del Ws
    W, rows, cols = big
    g = torch.Generator(device="cpu").manual_seed(5)
    for n in (1, 512):
        idsets = [torch.randint(0, rows, (n,), generator=g, dtype=torch.int32).cuda() for _ in range(64)]  # new rows every launch
        for dt, name, esz in ((torch.float16, "F16", 2), (torch.float32, "F32", 4)):
            out = torch.empty((n, cols), dtype=dt, device="cuda")
            fn = lambda i: sgemm.get_rows(W, idsets[i % 64], dt, out=out)  # noqa: E731
            for i in range(3):
                fn(i)
            torch.cuda.synchronize()
            us = statistics.median(timed(fn, max(a.iters, 64)) for _ in range(a.rounds))
            moved = n * (T.row_size(T.Q6_K, cols) + cols * esz)
            print(f"get_rows Q6_K {rows}x{cols} n={n:4d} -> {name}  {moved / 1e6:9.3f} MB {us:9.1f} us {moved / us / 1e3:8.1f} GB/s (algorithmic"
                  f" bytes: the rows' share of their tiles + the output)", flush=True)


if __name__ == "__main__":
    main()
