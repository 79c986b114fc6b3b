#!/bin/bash
# Before / after record of a decode GEMV change: outputs of bench.py --dump-outputs (sha256), three bench runs,
# tools/kbench.py per shape, rocprofv3 --kernel-trace --stats of the bench command, then counters of the deep-row Q6_K / Q4_K
# launches (4096 x 14336) in runs of their own: FETCH_SIZE alone, the instruction counters, the L2 counters.
# usage (on the GPU host, from the repository root): bash tools/decode_q6k_profile.sh TAG [DIR]  ->  DIR/TAG/ (DIR: profile_out)
TAG=${1:-x}
DIR=${2:-profile_out}
O=$DIR/$TAG; rm -rf $O; mkdir -p $O
set -o pipefail
step() { local t=$1; shift; timeout -k 10 $t "$@"; local rc=$?; if [ $rc -ne 0 ]; then echo "STEP FAILED rc=$rc: $*"; exit $rc; fi; }
step 300 python3 bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs $O/dump > $O/dump_bench.json 2> $O/dump_bench.err
python3 - $O <<'PY'
import hashlib, glob, json, os, sys
o = sys.argv[1]
h = {os.path.basename(f): hashlib.sha256(open(f, 'rb').read()).hexdigest() for f in sorted(glob.glob(f"{o}/dump/*.npy"))}
json.dump(h, open(f"{o}/dump_sha.json", "w"), indent=1)
print(len(h), "dump files hashed")
PY
rm -rf $O/dump
for i in 1 2 3; do step 300 python3 bench.py --gpus 1 --steps 10 --warmup 3 > $O/bench$i.json 2> $O/bench$i.err; done
step 200 python3 tools/kbench.py --cases "Q6_K,4096,14336,1;Q4_K,4096,14336,1;Q6_K,1024,4096,1;Q6_K,128256,4096,1;Q4_K,4096,4096,1;Q4_K,14336,4096,1" --iters 50 > $O/kbench.txt 2>&1
step 200 python3 tools/kbench.py --prequant --cases "Q6_K,4096,14336,1;Q4_K,4096,14336,1" --iters 50 > $O/kbench_prequant.txt 2>&1
step 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 bench.py --gpus 1 --steps 3 --warmup 1 > $O/trace.log 2>&1
find $O/trace -name '*kernel_trace.csv' -delete
CASES="Q6_K,4096,14336,1;Q4_K,4096,14336,1"
step 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc1 -- python3 tools/kbench.py --cases "$CASES" --iters 2 --copies 8 > $O/pmc1.log 2>&1
step 200 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_WAIT_INST_ANY SQ_INSTS_LDS SQ_WAVE_CYCLES --output-format csv -d $O/pmc2 -- python3 tools/kbench.py --cases "$CASES" --iters 2 --copies 8 > $O/pmc2.log 2>&1
timeout -k 10 200 rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/pmc3 -- python3 tools/kbench.py --cases "$CASES" --iters 2 --copies 8 > $O/pmc3.log 2>&1 || echo "pmc3 set not available"
python3 - $O <<'PY'
import csv, glob, json, sys, collections
o = sys.argv[1]
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{o}/pmc*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"]
        if "gemv_kq_kernel" not in k:
            continue
        key = ("q6k" if "q6k" in k else "q4k" if "q4k" in k else k[:60])
        agg[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
res = {k: {n: sum(v) / len(v) for n, v in d.items()} for k, d in agg.items()}
for k, d in agg.items():
    res[k]["launches_sampled"] = len(next(iter(d.values())))
json.dump(res, open(f"{o}/pmc.json", "w"), indent=1)
print(json.dumps(res, indent=1))
PY
find $O -name '*counter_collection.csv' -size +2M -delete
echo ALL DONE
