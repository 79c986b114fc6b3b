#!/bin/bash
# Before / after record of the early first issue of the fused decode launches, ONE job on ONE machine: the parent
# commit's library and this tree's, picked by LFAMD_HIP_SO, alternated so that both see the same machine state.
#   1. bench.py --dump-outputs with each library, sha256 of every dump file (the two sets must be equal)
#   2. bench.py --steps 10 --warmup 3, three runs per library: parent / here / parent / here / parent / here
#   3. tools/kbench_dual.py (the three fused launches) per library, alternated, twice
#   4. rocprofv3 --kernel-trace --stats of the bench command, once per library, each a run of its own (no counters)
# Every GPU step runs under its own time limit, the script stops at the first failure and nothing is run twice.
# usage (on the GPU host, from the repository root): bash tools/decode_early_profile.sh PARENT_SO [HERE_SO] [DIR]
#   PARENT_SO: libllamafile_amd_hip.so built from the parent commit; HERE_SO: this tree's (default: the in-tree build)
#   -> DIR/early_multi_{parent,here}_*  (DIR: profile_out; the files kept in the repository: profiles/README.md)
PARENT_SO=${1:?usage: decode_early_profile.sh PARENT_SO [HERE_SO] [DIR]}
HERE_SO=${2:-llamafile_amd/libllamafile_amd_hip.so}
DIR=${3:-profile_out}
set -o pipefail
for f in "$PARENT_SO" "$HERE_SO"; do [ -f "$f" ] || { echo "no such library: $f"; exit 2; }; done
PARENT_SO=$(readlink -f "$PARENT_SO"); HERE_SO=$(readlink -f "$HERE_SO")
mkdir -p $DIR
so_of() { if [ "$1" = parent ]; then echo "$PARENT_SO"; else echo "$HERE_SO"; fi; }
# step SECONDS WHICH command...: the command under its time limit with WHICH's library; the first failure ends the script
step() {
    local t=$1 which=$2; shift 2
    LFAMD_HIP_SO=$(so_of $which) timeout -k 10 $t "$@"
    local rc=$?
    if [ $rc -ne 0 ]; then echo "STEP FAILED rc=$rc ($which): $*"; exit $rc; fi
}
P=$DIR/early_multi

for w in parent here; do
    step 300 $w python3 bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs $DIR/dump_$w > ${P}_${w}_dump_bench.json 2> ${P}_${w}_dump_bench.err
done
python3 - $DIR $P <<'PY' || exit 1
import glob, hashlib, json, os, sys
d, p = sys.argv[1:3]
sha = {}
for w in ("parent", "here"):
    sha[w] = {os.path.basename(f): hashlib.sha256(open(f, "rb").read()).hexdigest() for f in sorted(glob.glob(f"{d}/dump_{w}/*.npy"))}
    json.dump(sha[w], open(f"{p}_{w}_dump_sha.json", "w"), indent=1)
same = sha["parent"] == sha["here"] and len(sha["here"]) > 0
print(len(sha["here"]), "dump files per library;", "ALL EQUAL" if same else "DIFFERENT: " + str([k for k in sha["here"] if sha["parent"].get(k) != sha["here"][k]]))
sys.exit(0 if same else 1)
PY
rm -rf $DIR/dump_parent $DIR/dump_here

for i in 1 2 3; do
    for w in parent here; do
        step 300 $w python3 bench.py --gpus 1 --steps 10 --warmup 3 > ${P}_${w}_bench$i.json 2> ${P}_${w}_bench$i.err
    done
done
python3 - $P <<'PY'
import json, statistics, sys
p = sys.argv[1]
res = {}
for w in ("parent", "here"):
    runs = [json.loads(open(f"{p}_{w}_bench{i}.json").read().strip().splitlines()[-1]) for i in (1, 2, 3)]
    v = [r["value"] for r in runs]
    ms = [r.get("ms_per_step") for r in runs]
    res[w] = {"tokens_per_s": v, "ms_per_step": ms, "median": statistics.median(v), "spread": max(v) - min(v)}
gain = res["here"]["median"] - res["parent"]["median"]
bar = 3 * max(res["parent"]["spread"], res["here"]["spread"])
res["gain_tokens_per_s"] = gain
res["gain_percent"] = 100.0 * gain / res["parent"]["median"]
res["three_times_larger_spread"] = bar
res["gain_exceeds_noise"] = gain > bar
json.dump(res, open(f"{p}_bench_summary.json", "w"), indent=1)
print(json.dumps(res, indent=1))
PY

: > ${P}_parent_kbench_dual.txt; : > ${P}_here_kbench_dual.txt
for i in 1 2; do
    for w in parent here; do
        step 200 $w python3 tools/kbench_dual.py >> ${P}_${w}_kbench_dual.txt 2>&1
    done
done

for w in parent here; do
    step 400 $w rocprofv3 --kernel-trace --stats --output-format csv -d $DIR/trace_$w -- python3 bench.py --gpus 1 --steps 3 --warmup 1 > ${P}_${w}_trace.log 2>&1
    f=$(find $DIR/trace_$w -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] && cp "$f" ${P}_${w}_bench_kernel_stats.csv
    rm -rf $DIR/trace_$w
done
echo ALL DONE
