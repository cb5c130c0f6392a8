#!/bin/bash
# A/B of two builds of the library on ONE box, alternating: surround360_amd/libs360_old.so against libs360_new.so (both
# built beforehand, untracked). Per build and round: the batch-alone kernel table (one context, 22 slots) and the headline.
#   usage (through gpurun, from the repo root): bash tools/ab_libs.sh <tag> [rounds]
cd "$(dirname "$0")/.."
TAG=${1:?tag}; R=${2:-2}
O=gpurun_out/$TAG; mkdir -p $O
cp surround360_amd/libs360.so $O/libs360_keep.so
for r in $(seq 1 $R); do
  for v in ${VARIANTS:-old new}; do   # a variant "<lib>:<ENV=value>" runs libs360_<lib>.so with that environment variable
    lib=${v%%:*}; envs=""; [ "$lib" != "$v" ] && envs=${v#*:}
    cp surround360_amd/libs360_$lib.so surround360_amd/libs360.so
    # (a run that fails, faults or meets its time limit ends the script: nothing more is started on that GPU)
    env $envs timeout -k 10 600 python bench.py --full --steps 12 --warmup 6 --no-extras --no-cpu-baseline > $O/${v//[:=]/_}_$r.json 2> $O/${v//[:=]/_}_$r.err \
      || { rc=$?; echo "$v round $r: bench.py ended with status $rc"; tail -5 $O/${v//[:=]/_}_$r.err; cp $O/libs360_keep.so surround360_amd/libs360.so; exit $rc; }
    python - $O/${v//[:=]/_}_$r.json $v $r <<'P'
import json, sys
d = json.load(open(sys.argv[1]))
k = d["roofline"]["batch_alone_kernel_ms_per_frame"]
f = d["kernel_ms_per_frame_in_flight"]
print("%s round %s: value %.2f checked %s  HBM %s GB  batch alone %.3f ms/frame  median %.3f (in flight %.3f)  sweep %.3f  finish %.3f (in flight %.3f)"
      "  flow_final %.3f (in flight %.3f)  flatten %.3f (in flight %.3f)  pole_warp %.3f (in flight %.3f)" % (
    sys.argv[2], sys.argv[3], d["value"], d["checked"], d.get("hbm_used_GB_in_timed_region"), d["roofline"]["batch_alone_ms_per_frame"],
    k["flow_median"], f["flow_median"], k["flow_sweep"], k["finish"], f["finish"],
    k["flow_final"], f["flow_final"], k["flatten"], f["flatten"], k["pole_warp"], f["pole_warp"]))
P
  done
done
cp $O/libs360_keep.so surround360_amd/libs360.so
