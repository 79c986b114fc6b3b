#!/usr/bin/env python3
"""Device time of the KQ product of a Llama-3-8B layer (head_dim 128, 32 query heads, 8 KV heads) on a QUANTISED K cache (-ctk q8_0,
q4_0), through three routes:

  a  lfamd_mul_mat_batched_q: the whole product, all heads, one call on the cache's own rows
  b  the per-slice loop the ggml backend runs without that call, through the C ABI: per KV head one lfamd_pack_weights of the head's
     rows into a scratch image (lfamd_resident_type(t, 128): Q8_0's P80 image; for Q4_0 the padded 256-column tile image), per query
     head one lfamd_mul_mat
  c  lfamd_mul_mat_batched on an F16 K cache of the same shape — for context only: another cache type, not a bar

KQ: src0 = the K cache permuted, memory [n_kv][kv_head][row of 128 weights] (m = n_kv, k = 128); src1 = Q, memory [n][head][128].

Device events around back-to-back calls on the null stream, warm-up first, every window at least --window seconds, the routes
alternated inside one process for --rounds rounds; median and min .. max of the rounds.  The operands stay where they are between
calls, so the cache is read from the on-die caches: these are times of the calls, not of HBM."""
import json

from attn_common import HEAD_DIM, HEADS, KV_HEADS, parser, shapes_of, time_routes, write_doc

from llamafile_amd import _hip, ggml_types as T, synth  # noqa: E402  (attn_common put the repository root on the path)


def main():
    ap = parser("attn_batched_q.json")
    ap.add_argument("--types", default="Q8_0,Q4_0")
    args = ap.parse_args()
    import torch
    from llamafile_amd import sgemm

    assert torch.cuda.is_available(), "attn_q_time.py measures on the GPU: there is no CPU fallback"
    sgemm.init(0)
    lib = _hip.lib()
    shapes = shapes_of(args)
    types = [{v: key for key, v in T.NAMES.items()}[name] for name in args.types.split(",")]
    group = HEADS // KV_HEADS
    k = HEAD_DIM
    gen = torch.Generator(device="cuda").manual_seed(1)
    results = []
    for t in types:
        row_bytes = T.row_size(t, k)
        rt = t | _hip.TYPE_PAD256 if t != T.Q8_0 and k % 256 else t  # lfamd_resident_type(t, k)
        for n_kv, n in shapes:
            m = n_kv
            a_nb = (KV_HEADS * row_bytes, row_bytes)  # nb1, nb2
            f_nb = (KV_HEADS * k * 2, k * 2)
            b_nb = (HEADS * k * 4, k * 4)
            A = torch.from_numpy(synth.random_weights(t, m * KV_HEADS, k, 3)).cuda()
            A16 = (torch.rand((m, KV_HEADS, k), device="cuda", generator=gen) * 2 - 1).half()
            B = torch.rand((n, HEADS, k), device="cuda", generator=gen) * 2 - 1
            Cs = {v: torch.zeros((HEADS, n, m), device="cuda") for v in "abc"}
            scratch = torch.empty(lib.lfamd_packed_size(rt, m, k) + 256, dtype=torch.uint8, device="cuda")
            ws_bytes = lib.lfamd_mul_mat_workspace(rt, m, k, n)
            ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
            pA, pA16, pB = A.data_ptr(), A16.data_ptr(), B.data_ptr()

            def run_a():
                _hip.check(lib.lfamd_mul_mat_batched_q(t, pA, m, k, a_nb[0], a_nb[1], m * a_nb[0], KV_HEADS, 1, pB, n, b_nb[0], b_nb[1],
                                                       HEADS * n * k * 4, HEADS, 1, Cs["a"].data_ptr(), m * 4, n * m * 4, HEADS * n * m * 4,
                                                       0, None), "lfamd_mul_mat_batched_q")

            def run_b():
                pc = Cs["b"].data_ptr()
                for h in range(HEADS):
                    if h % group == 0:
                        _hip.check(lib.lfamd_pack_weights(rt, m, k, pA + (h // group) * a_nb[1], a_nb[0], scratch.data_ptr(), None),
                                   "lfamd_pack_weights")
                    _hip.check(lib.lfamd_mul_mat(rt, scratch.data_ptr(), m, k, T.F32, pB + h * b_nb[1], b_nb[0], n, pc + h * n * m * 4, m,
                                                 ws.data_ptr(), ws_bytes, _hip.FLAG_Q0_VREGS32, None), "lfamd_mul_mat")

            def run_c():
                _hip.check(lib.lfamd_mul_mat_batched(T.F16, pA16, m, k, f_nb[0], f_nb[1], m * f_nb[0], KV_HEADS, 1, pB, n, b_nb[0], b_nb[1],
                                                     HEADS * n * k * 4, HEADS, 1, Cs["c"].data_ptr(), m * 4, n * m * 4, HEADS * n * m * 4,
                                                     0, None), "lfamd_mul_mat_batched")

            runs = {"a": run_a, "b": run_b, "c": run_c}
            # agreement first: a and b compute the same product (b's batch bodies may round operands to f16: up to ~1e-3)
            for f in runs.values():
                f()
            torch.cuda.synchronize()
            ref = Cs["b"].double()
            agree = float((Cs["a"].double() - ref).abs().max() / ref.abs().max())
            if agree > 2e-3:
                print("WARNING: routes a and b disagree", T.NAMES[t], n_kv, n, agree, flush=True)

            timed = time_routes(torch, runs, args)
            nbytes = KV_HEADS * m * row_bytes + HEADS * n * k * 4 + HEADS * n * m * 4
            row = {"type": T.NAMES[t], "n_kv": n_kv, "n": n, "m": m, "k": k, "algorithmic_bytes": nbytes, "flop": 2 * HEADS * n * m * k,
                   "max_rel_diff_a_vs_b": agree}
            for v, (_, entry) in timed.items():
                row[v] = entry
            row["b_over_a"] = round(row["b"]["us"] / row["a"]["us"], 2)
            # the routing condition: a beats b by more than the two routes' run-to-run spread
            row["a_beats_b_beyond_spread"] = bool(row["a"]["us_max"] < row["b"]["us_min"])
            print(json.dumps(row), flush=True)
            results.append(row)
            del A, A16, B, Cs, scratch, ws
            torch.cuda.empty_cache()
    write_doc(torch, args, {"a": "lfamd_mul_mat_batched_q, one call",
                            "b": "lfamd_pack_weights(lfamd_resident_type) per KV head + lfamd_mul_mat per head (the per-slice loop)",
                            "c": "lfamd_mul_mat_batched on an F16 K cache of the same shape (context, not a bar)"}, results)


if __name__ == "__main__":
    main()
