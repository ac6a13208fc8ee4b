#!/bin/bash
# Per-wave instruction and cycle counters of k_rx on the config-B bench (DESIGN.md §6 "The
# uniform-wave path"), the slab forced tight (under counter collection the automatic choice stays
# wide), one rocprofv3 run per pass and nothing else traced.
#   tools/pmc_wave.sh TAG [LIB]     LIB: another build's libemurx.so (EMURX_LIB), relative to the root
set -u
cd "$(dirname "$0")/.."
tag=$1; lib=${2:-}
[ -n "$lib" ] && export EMURX_LIB=$PWD/$lib
export EMURX_STAGE=tight TMPDIR=/tmp
out=${PMC_OUT:-bench_logs}/pmc_$tag; rm -rf $out; mkdir -p $out
i=0
while read -r set; do
  [ -z "$set" ] && continue
  i=$((i+1)); echo "== pass $i: $set"
  timeout -k 10 150 rocprofv3 --pmc $set -T --kernel-include-regex k_rx -d $out/p$i -o run --output-format csv \
      -- python bench.py --steps 30 --no-cpu-baseline --no-check > $out/p$i.log 2>&1
  rc=$?; echo "rc=$rc"; [ $rc -eq 0 ] || { tail -5 $out/p$i.log; exit $rc; }
  grep -h '"mpps"\|Mpkt' $out/p$i.log | tail -1 | cut -c1-300
done <<'EOF'
SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_BRANCH SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM GRBM_GUI_ACTIVE
SQ_WAVES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_SCA GRBM_GUI_ACTIVE
EOF
python - $out <<'PY' | tee $out/summary.txt
"""Mean per-dispatch counter values of the k_rx dispatches in a pmc_b.sh output directory,
per kernel name, and the dispatch duration where the CSV carries timestamps."""
import collections
import csv
import glob
import sys

out = sys.argv[1]
for f in sorted(glob.glob(out + "/p*/**/*counter_collection.csv", recursive=True)):
    per = collections.defaultdict(float)
    name = {}
    dur = {}
    for r in csv.DictReader(open(f)):
        d = int(r["Dispatch_Id"])
        per[(d, r["Counter_Name"])] += float(r["Counter_Value"])
        name[d] = r.get("Kernel_Name", "?")
        if "Start_Timestamp" in r and "End_Timestamp" in r:
            dur[d] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    by = collections.defaultdict(lambda: collections.defaultdict(list))
    for (d, c), v in per.items():
        by[name[d]][c].append((d, v))
    print("##", f)
    for k, cs in by.items():
        nd = len(next(iter(cs.values())))
        ds = sorted(dur[d] for d in name if name[d] == k and d in dur)
        print(f"  {k[:60]}  dispatches {nd}" + (f"  median duration {ds[len(ds)//2]/1e3:.2f} us" if ds else ""))
        for c, l in sorted(cs.items()):
            l.sort()
            v = [x[1] for x in l][3:] or [x[1] for x in l]
            print(f"    {c:26s} {sum(v)/len(v):16.1f}")
PY
