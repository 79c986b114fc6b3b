"""Config-3 (Llama-3-8B, Q8_0) prefill groups at 512 tokens: lfamd_mul_mat / _multi on f32 rows, with a parent build's library and
with this tree's, against the same call on the LFAMD_TYPE_STAGED_Q80 image; the producers with and without the image; and producer +
mat-mul back to back.  Device events around windows of back-to-back calls, the variants alternated window by
window; every call re-reads the same operands, so the weights of the 4096 x 4096 group may stay in the last-level cache.

    python tools/q80_image_record.py PARENT_SO [OUT.txt]     PARENT_SO: libllamafile_amd_hip.so built from the parent commit"""
import ctypes as C
import os
import sys
import statistics

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llamafile_amd import _hip, ggml_types as T, sgemm as gpu, synth  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
PARENT_SO = os.path.abspath(sys.argv[1])
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "q80_image_record.txt")
os.makedirs(os.path.dirname(OUT), exist_ok=True)
log = open(OUT, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


gpu.init(0)
L = _hip.lib()
P = C.CDLL(PARENT_SO)
for name in ("lfamd_init", "lfamd_mul_mat", "lfamd_mul_mat_multi", "lfamd_rms_norm_quantize_b32", "lfamd_swiglu_quantize_b32"):
    f = getattr(P, name)
    f.restype, f.argtypes = _hip._SIGS[name]
assert P.lfamd_init(0) == 0
assert not hasattr(P, "lfamd_staged_q80_size")
flags = gpu.host_variant_flags()
Q80I = _hip.TYPE_STAGED_Q80
N = 512
ITERS, WINDOWS, WARM = 200, 9, 20


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(variants):
    """variants: {name: fn}; returns {name: [us per call of each window]} with the windows alternated."""
    res = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) * 1000.0 / ITERS)
    return res


def report(title, res):
    say(f"## {title}  ({WINDOWS} windows of {ITERS} calls each, alternated; us per call: median [min .. max])")
    for name, v in res.items():
        say(f"  {name:58s} {statistics.median(v):8.2f}  [{min(v):8.2f} .. {max(v):8.2f}]")


def group(title, ms, k, producer):
    count = len(ms)
    Ws = [gpu.upload_weights(T.Q8_0, synth.random_weights(T.Q8_0, m, k, 500 + i), m, k) for i, m in enumerate(ms)]
    x = torch.from_numpy(synth.random_activations(N, k, 7)).cuda()
    g = torch.from_numpy((np.random.default_rng(8).standard_normal((N, k)) * 2).astype(np.float32)).cuda()
    wn = torch.ones(k, dtype=torch.float32, device="cuda")
    yf = torch.empty((N, k), dtype=torch.float32, device="cuda")
    image = torch.empty(L.lfamd_staged_q80_size(k, N), dtype=torch.uint8, device="cuda")
    need = max(L.lfamd_mul_mat_workspace(T.Q8_0, m, k, N) for m in ms)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = [torch.empty((N, m), dtype=torch.float32, device="cuda") for m in ms]
    outs2 = [torch.empty((N, m), dtype=torch.float32, device="cuda") for m in ms]
    A = (C.c_void_p * count)(*[w.data.data_ptr() for w in Ws])
    mm = (C.c_long * count)(*ms)
    Cs = (C.c_void_p * count)(*[o.data_ptr() for o in outs])
    Cs2 = (C.c_void_p * count)(*[o.data_ptr() for o in outs2])
    none = C.c_void_p(0)
    st = stream()

    def prod(lib, vdt, yq, f):
        if producer == "rms_norm":
            rc = lib.lfamd_rms_norm_quantize_b32(ptr(x), k * 4, ptr(wn), 1e-5, N, k, vdt, yq, 0, ptr(yf) if f else none, k * 4, st)
        else:
            rc = lib.lfamd_swiglu_quantize_b32(ptr(g), k * 4, ptr(x), k * 4, N, k, vdt, yq, 0, ptr(yf) if f else none, k * 4, st)
        assert rc == 0

    def mat(lib, Btype, B, brb, cs, with_ws=True):
        if count == 1:
            rc = lib.lfamd_mul_mat(T.Q8_0, A[0], ms[0], k, Btype, B, brb, N, cs[0], ms[0], ptr(ws) if with_ws else none, need if with_ws else 0, flags, st)
        else:
            rc = lib.lfamd_mul_mat_multi(T.Q8_0, count, A, mm, k, Btype, B, brb, N, cs, mm, ptr(ws) if with_ws else none, need if with_ws else 0, flags, st)
        assert rc == 0

    # the same bits first
    prod(L, Q80I, ptr(image), True)
    mat(L, Q80I, ptr(image), 0, Cs, with_ws=False)
    mat(P, T.F32, ptr(yf), k * 4, Cs2)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, outs2))
    say(f"# {title}: {count} x Q8_0 {ms} x {k}, {N} tokens, producer {producer}; image call == parent f32 call by bits: {same}")
    assert same
    report(title + ": the mat-mul call alone", timed({
        "parent build, f32 rows (tok_scale + prep + GEMM)": lambda: mat(P, T.F32, ptr(yf), k * 4, Cs2),
        "this build,   f32 rows (tok_scale + prep + GEMM)": lambda: mat(L, T.F32, ptr(yf), k * 4, Cs2),
        "this build,   the image (GEMM alone)": lambda: mat(L, Q80I, ptr(image), 0, Cs, with_ws=False),
    }))
    report(title + ": the producer alone", timed({
        "parent build, f32 rows only (Q8_0-format kernel, d_yq = NULL)": lambda: prod(P, T.Q8_0, none, True),
        "this build,   f32 rows only": lambda: prod(L, T.Q8_0, none, True),
        "this build,   the image only": lambda: prod(L, Q80I, ptr(image), False),
        "this build,   the image and f32 rows": lambda: prod(L, Q80I, ptr(image), True),
    }))

    def chain_parent():
        prod(P, T.Q8_0, none, True)
        mat(P, T.F32, ptr(yf), k * 4, Cs2)

    def chain_image():
        prod(L, Q80I, ptr(image), False)
        mat(L, Q80I, ptr(image), 0, Cs, with_ws=False)

    def chain_image_f32():
        prod(L, Q80I, ptr(image), True)
        mat(L, Q80I, ptr(image), 0, Cs, with_ws=False)

    report(title + ": producer + mat-mul in the stream", timed({
        "parent build: producer (f32) + f32 call, 4 launches": chain_parent,
        "this build:   producer (image) + image call, 2 launches": chain_image,
        "this build:   producer (image + f32) + image call, 2 launches": chain_image_f32,
    }))
    del Ws
    torch.cuda.empty_cache()


say("device:", torch.cuda.get_device_name(0))
group("attn_q / attn_output 4096 x 4096", [4096], 4096, "rms_norm")
group("ffn_gate + ffn_up 14336 x 4096 x 2", [14336, 14336], 4096, "rms_norm")
group("ffn_down 4096 x 14336", [4096], 14336, "swiglu")
say("done")
