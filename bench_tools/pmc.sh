#!/bin/bash
# quick SQ counters: bash bench_tools/pmc.sh <tag> [bench args]
TAG=${1:-t}; shift || true
HERE=$(cd "$(dirname "$0")/.." && pwd)   # the repository root, resolved before any cd
cd /tmp && export TMPDIR=/tmp; cd "$HERE"
OUT=gpurun_out/pmc_$TAG; mkdir -p $OUT
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU --kernel-trace --output-format csv -d $OUT -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline "$@" > $OUT/bench.json 2> $OUT/err.txt
python - <<PY
import csv,glob,collections
f=glob.glob("$OUT/*/*_counter_collection.csv")[0]
agg=collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(f)):
    k=r["Kernel_Name"].split("(")[0].replace("void ","").replace("lurk::","")[:36]
    agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
    agg[k]["dur_us"].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
for k,v in agg.items():
    if "msm" in k: print(k, {c: round(sum(x)/len(x)/ (1e6 if c!="dur_us" else 1),2) for c,x in v.items()})
PY
