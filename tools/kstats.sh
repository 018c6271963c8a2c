#!/bin/bash
# usage: tools/kstats.sh [DIR]  -> per-kernel average durations of one bench run (rocprofv3 --kernel-trace --stats); raw output in DIR
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
D=${1:-build/kstats}
rm -rf $D; mkdir -p $D; rocprofv3 --kernel-trace --stats --output-format csv -d $D -o k -- python bench.py --steps 20 --warmup 3 --full --no-cpu --no-frame-loop > $D/bench.log 2>&1
python - <<PY
import csv
rows=list(csv.DictReader(open("$D/k_kernel_stats.csv")))
for r in rows[:7]: print(f"{r['Name'][:52]:52s} calls {r['Calls']:>5s} avg_us {float(r['AverageNs'])/1e3:8.2f} total_ms {float(r['TotalDurationNs'])/1e6:8.2f}")
PY
grep "^{" $D/bench.log | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['roofline']['stages_ms'])"
