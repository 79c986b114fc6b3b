#!/usr/bin/env python3
"""Device time of the two attention products of a Llama-3-8B layer (head_dim 128, 32 query heads, 8 KV heads) through three routes:

  a  lfamd_mul_mat_batched: the whole product, all heads, one call on the strided operands
  b  the per-slice loop the ggml backend ran before that call existed, through the C ABI: per KV head one lfamd_pack_weights copy
     of the head's rows into a scratch image, per query head one lfamd_mul_mat (--pack-per-head: a copy in front of every head)
  c  lfamd_gemm_strided_batched_f16 on activations converted to f16 beforehand (the conversion is not timed): it has no broadcast, so
     one call per KV head with strideA = 0 and batch = the group's query heads

KQ: src0 = the K cache permuted, memory [n_kv][kv_head][128] (m = n_kv, k = 128); src1 = Q, memory [n][head][128].
KQV: src0 = the V cache, memory [kv_head][128][n_kv] (m = 128, k = n_kv); src1 = the soft-max rows, contiguous [head][n][n_kv].

Device events around back-to-back calls on the null stream, warm-up first, every window at least --window seconds, the variants
alternated inside one process for --rounds rounds; median and min .. max of the rounds.  The operands stay where they are between
calls, so an 8 MB cache is read from the on-die caches: these are times of the calls, not of HBM.  Bytes/s are the algorithmic bytes
(every K / V slice once, B, C) over the median."""
import json

from attn_common import HEAD_DIM, HEADS, KV_HEADS, parser, shapes_of, time_routes, write_doc

from llamafile_amd import _hip, ggml_types as T  # noqa: E402  (attn_common put the repository root on the path)


def main():
    ap = parser("attn_batched.json")
    ap.add_argument("--pack-per-head", action="store_true")
    args = ap.parse_args()
    import torch
    from llamafile_amd import sgemm

    assert torch.cuda.is_available(), "attn_time.py measures on the GPU: there is no CPU fallback"
    sgemm.init(0)
    lib = _hip.lib()
    shapes = shapes_of(args)
    group = HEADS // KV_HEADS
    gen = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for n_kv, n in shapes:
        for what in ("KQ", "KQV"):
            if what == "KQ":
                m, k = n_kv, HEAD_DIM
                a_nb = (KV_HEADS * k * 2, k * 2)          # nb1, nb2
                b_nb = (HEADS * k * 4, k * 4)
                A = (torch.rand((m, KV_HEADS, k), device="cuda", generator=gen) * 2 - 1).half()
                B = torch.rand((n, HEADS, k), device="cuda", generator=gen) * 2 - 1
            else:
                m, k = HEAD_DIM, n_kv
                a_nb = (k * 2, m * k * 2)
                b_nb = (k * 4, n * k * 4)
                A = (torch.rand((KV_HEADS, m, k), device="cuda", generator=gen) * 2 - 1).half()
                B = torch.rand((HEADS, n, k), device="cuda", generator=gen)  # (soft-max rows are positive)
            B16 = B.half()
            Cs = {v: torch.zeros((HEADS, n, m), device="cuda") for v in "abc"}
            scratch = torch.empty(lib.lfamd_packed_size(T.F16, m, k) + 256, dtype=torch.uint8, device="cuda")
            ws_bytes = lib.lfamd_mul_mat_workspace(T.F16, m, k, n)
            ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
            pA, pB, pB16 = A.data_ptr(), B.data_ptr(), B16.data_ptr()

            def run_a():
                _hip.check(lib.lfamd_mul_mat_batched(T.F16, pA, m, k, a_nb[0], a_nb[1], KV_HEADS * m * k * 2, KV_HEADS, 1, pB, n, b_nb[0],
                                                     b_nb[1], HEADS * n * k * 4, HEADS, 1, Cs["a"].data_ptr(), m * 4, n * m * 4,
                                                     HEADS * n * m * 4, 0, None), "lfamd_mul_mat_batched")

            def run_b():
                pc = Cs["b"].data_ptr()
                for h in range(HEADS):
                    if h % group == 0 or args.pack_per_head:
                        _hip.check(lib.lfamd_pack_weights(T.F16, m, k, pA + (h // group) * a_nb[1], a_nb[0], scratch.data_ptr(), None),
                                   "lfamd_pack_weights")
                    _hip.check(lib.lfamd_mul_mat(T.F16, scratch.data_ptr(), m, k, T.F32, pB + h * b_nb[1], b_nb[0], n, pc + h * n * m * 4, m,
                                                 ws.data_ptr(), ws_bytes, _hip.FLAG_Q0_VREGS32, None), "lfamd_mul_mat")

            def run_c():
                pc = Cs["c"].data_ptr()
                for g in range(KV_HEADS):
                    _hip.check(lib.lfamd_gemm_strided_batched_f16(m, n, k, 1.0, pA + g * a_nb[1], a_nb[0] // 2, 0, pB16 + g * group * (b_nb[1] // 2),
                                                                  b_nb[0] // 4, b_nb[1] // 4, 0.0, pc + g * group * n * m * 4, T.F32, m, n * m,
                                                                  group, None), "lfamd_gemm_strided_batched_f16")

            runs = {"a": run_a, "b": run_b, "c": run_c}
            # agreement first.  n <= 8: a and b are the same arithmetic in another order, c rounds the activations to f16 (~2e-4).
            # n > 8: a and c round them to f16; b does where lfamd_mul_mat runs its f16 MFMA body (rows of whole 256-element groups)
            # and keeps them f32 on the generic kernel otherwise (k = 128: a and b then lie that rounding apart)
            for f in runs.values():
                f()
            torch.cuda.synchronize()
            ref = Cs["b"].double()
            agree = {v: float((Cs[v].double() - ref).abs().max() / ref.abs().max()) for v in "ac"}
            if agree["a"] > 1e-3:
                print("WARNING: routes a and b disagree", what, n_kv, n, agree, flush=True)

            timed = time_routes(torch, runs, args)
            nbytes = KV_HEADS * m * k * 2 + HEADS * n * k * 4 + HEADS * n * m * 4
            row = {"product": what, "n_kv": n_kv, "n": n, "m": m, "k": k, "algorithmic_bytes": nbytes, "flop": 2 * HEADS * n * m * k,
                   "max_rel_diff_vs_b": agree, "pack_per_head": bool(args.pack_per_head)}
            for v, (med, entry) in timed.items():
                row[v] = dict(entry, GB_per_s=round(nbytes / med * 1e-3, 1))
            row["b_over_a"] = round(row["b"]["us"] / row["a"]["us"], 2)
            row["c_over_a"] = round(row["c"]["us"] / row["a"]["us"], 2)
            print(json.dumps(row), flush=True)
            results.append(row)
            del A, B, B16, Cs, scratch, ws
            torch.cuda.empty_cache()
    write_doc(torch, args, {"a": "lfamd_mul_mat_batched, one call",
                            "b": "lfamd_pack_weights per KV head + lfamd_mul_mat per head (the per-slice loop)",
                            "c": "lfamd_gemm_strided_batched_f16 per KV head on pre-converted f16 activations"}, results)


if __name__ == "__main__":
    main()
