"""development: in-kernel s_memrealtime stamps (10 ns ticks) of the decode GEMV (GEMV_DIAG build via LFAMD_HIP_SO).

  gemv_stamps.py [M K [TYPE]]             every stamp of work-groups 0 and GEMV_DIAG_WG (default 100) of an M x K launch
  gemv_stamps.py --fused CASE             the prologue of a FUSED launch: when the first weight loads of the oldest and of the
                                          youngest wave of those two work-groups are out, relative to the work-group's entry
                                          (a wave's first stamp is its entry, its second follows its first weight loads)
     CASE: gateup    2 x 14336 x 4096 Q4_K                       (tools/build_diag.sh gemv_q4k)
           qkv       4096 + 1024 + 1024 x 4096 Q4_K              (tools/build_diag.sh gemv_q4k)
           qkv_dual  4096 + 1024 Q4_K + 1024 Q6_K x 4096         (tools/build_diag.sh gemv_dual -DGEMV_DIAG=1 -DGEMV_DIAG_WG=200:
                                                                  work-group 200 is one of the Q6_K side's on 256 CUs)"""
import ctypes as C, sys, numpy as np, torch
sys.path.insert(0, ".")
from llamafile_amd import sgemm, synth, _hip, ggml_types as T


def read_stamps():
    buf = (C.c_ulonglong * 1024)()
    print("rc", _hip.lib().lfamd_debug_stamps(buf, C.c_size_t(len(buf))))
    return np.array(buf[:512], dtype=np.int64).reshape(2, 16, 16)


def fused(case):
    k = 4096
    spec, copies = {"gateup": (((T.Q4_K, 14336), (T.Q4_K, 14336)), 6),
                    "qkv": (((T.Q4_K, 4096), (T.Q4_K, 1024), (T.Q4_K, 1024)), 24),
                    "qkv_dual": (((T.Q4_K, 4096), (T.Q4_K, 1024), (T.Q6_K, 1024)), 24)}[case]
    # several sets of weights, so that the launch that leaves the stamps reads from HBM like a decode pass does
    sets = [[sgemm.upload_weights(t, synth.random_weights_torch(t, m, k, seed=s * 5 + i), m, k) for i, (t, m) in enumerate(spec)]
            for s in range(copies)]
    B = torch.randn(1, k, device="cuda").view(torch.uint8).view(1, k * 4)
    for rep in range(3):
        for Ws in sets:
            sgemm.mul_mat_multi(Ws, B, T.F32, n=1)
    torch.cuda.synchronize()
    a = read_stamps()
    print("case", case, "library", _hip.HIP_SO)
    for g in (0, 1):
        entry, first = a[g, :, 0], a[g, :, 1]
        waves = [w for w in range(16) if entry[w] > 0 and first[w] > 0]
        if not waves:
            print("wg", g, "no stamps")
            continue
        t0 = min(entry[w] for w in waves)
        old, young = min(waves, key=lambda w: entry[w]), max(waves, key=lambda w: entry[w])
        print(f"wg {g}: {len(waves)} waves; oldest wave {old}: entry +{entry[old] - t0}, first weight loads out +{first[old] - t0}; "
              f"youngest wave {young}: entry +{entry[young] - t0}, first weight loads out +{first[young] - t0}  (ticks of 10 ns since the "
              f"work-group's entry); entry -> first weight loads per wave: {[int(first[w] - entry[w]) for w in waves]}")


sgemm.init(0)
if len(sys.argv) > 2 and sys.argv[1] == "--fused":
    fused(sys.argv[2])
    sys.exit(0)
m, k = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4096, 4096)
WT = getattr(T, sys.argv[3]) if len(sys.argv) > 3 else T.Q4_K
Ws = [sgemm.upload_weights(WT, synth.random_weights_torch(WT, m, k, seed=s), m, k) for s in range(24)]
x = torch.randn(1, k, device="cuda")
B = x.view(torch.uint8).view(1, k * 4)
for W in Ws:
    out = sgemm.mul_mat(W, B, T.F32, n=1)
torch.cuda.synchronize()
a = read_stamps()
t0 = a[a > 0].min()
for g in (0, 1):
    for w in range(16):
        t = a[g, w]
        t = t[t > 0]
        print("wg", g, "wave", w, "ticks(10ns) since first stamp:", (t - t0).tolist())
