#!/bin/bash
# Instruction-fetch counters of the fleet kernel over one bench workload: two rocprofv3 --pmc passes of their own (counters are never
# mixed with a trace), summed per kernel family in the format of profiles/r03_pmc_summary_*.txt.
# usage on the GPU box:  bash tools/icache_pmc.sh <out.txt> [tree] [workload] [steps]
#   tree: the checkout whose bench.py is run (default: this one; a built checkout of the parent commit gives the "before" file)
# profiles/icache_pmc_parent.txt and profiles/icache_pmc_this.txt are this script's output for the two trees.
set -u
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:?output file}
TREE=${2:-$HERE}
WL=${3:-light_flat}
STEPS=${4:-60}
WORK=$(mktemp -d)
ARGS="--workload $WL --steps $STEPS --warmup 10"
cd "$WORK"
i=0
for set in "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQ_IFETCH SQ_IFETCH_LEVEL SQ_WAVES" \
           "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQC_ICACHE_INPUT_VALID_READYB"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d "$WORK/pass$i" -- python3 "$TREE/bench.py" $ARGS > "$WORK/pass$i.log" 2>&1 \
    || { echo "pmc pass $i failed"; tail -n 20 "$WORK/pass$i.log"; exit 1; }
done
python3 - "$WORK" "$OUT" "$ARGS" <<'PY'
import collections, csv, glob, sys
work, out, args = sys.argv[1:4]
def family(name):
    for f in ("env_fixup_kernel", "env_kernel"):
        if f in name:
            return f
    return None
tot = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.defaultdict(lambda: collections.defaultdict(int))
launches = collections.defaultdict(collections.Counter)
for f in glob.glob(work + "/pass*/*/*counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        fam = family(r["Kernel_Name"])
        if fam:
            tot[fam][r["Counter_Name"]] += float(r["Counter_Value"]); cnt[fam][r["Counter_Name"]] += 1
            if r["Counter_Name"] in ("SQ_WAVES", "SQ_WAVE_CYCLES"):
                launches[fam][r["Kernel_Name"]] += 1
with open(out, "w") as o:
    for fam in sorted(tot, key=lambda f: -tot[f].get("SQ_WAVE_CYCLES", 0)):
        o.write(f"per launch of cosim::{fam}, rocprofv3 --pmc passes over: bench.py {args}\n")
        # every instantiation of the family is averaged under this heading: the one reset launch of the general fleet kernel
        # goes in with the step launches
        for n, c in sorted(launches[fam].items(), key=lambda nc: -nc[1]):
            o.write(f"# averaged here: {c // 2} launches of {n}\n")
        for k in sorted(tot[fam]):
            o.write(f"{k:28s} per-launch {tot[fam][k]/cnt[fam][k]:16.1f}   launches {cnt[fam][k]}\n")
PY
cat "$OUT"
rm -rf "$WORK"
