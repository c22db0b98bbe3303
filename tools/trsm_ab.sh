#!/bin/bash
# GPU box: configs[1] with several builds of libpipship.so, alternating on one box (the parent commit's build against this tree's; for
# profiles/trsm_triangular_ab.txt also a build with the paired wave map of the triangular trsm).  Three short bench lines per build, interleaved; three --full
# lines per build (phase_ms.leaf_factor.tail_trsm / schur); kernel statistics per build (rocprofv3 --kernel-trace --stats, runs of their own); one pair of
# --dump-outputs in deterministic mode compared entry for entry (in the default mode two runs of ONE build differ in the last bits: the
# Schur complement is accumulated with atomics).  Every GPU step under its own time limit, the chain stops at the first failure.
# usage: trsm_ab.sh <output dir> <label>=<library> [<label>=<library> ...]     (the first label is the parent)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=$1; shift; mkdir -p $O
cd $R
run() {  # label=lib, then bench.py's arguments
   local label=${1%%=*} lib=${1#*=}; shift
   echo "== $label: python bench.py $*" | tee -a $O/lines.txt
   PIPS_HIP_LIBRARY=$lib timeout -k 10 240 python3 bench.py "$@" 2>>$O/err.txt | grep '^{' | tee -a $O/lines.txt | cut -c1-200
}
for rep in 1 2 3; do
   for b in "$@"; do run $b --steps 20 --warmup 2 || exit 1; done
done
for rep in 1 2 3; do
   for b in "$@"; do run $b --steps 20 --warmup 2 --full --no-cpu-baseline --no-ipm || exit 1; done
done
for b in "$@"; do   # kernel statistics: rocprofv3 in a run of its own per build, the 14 kernels with the largest totals (calls, total, average)
   K=$O/kstats_${b%%=*}; rm -rf $K; mkdir -p $K
   echo "== ${b%%=*}: rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 5 --warmup 1" | tee -a $O/kstats.txt
   PIPS_HIP_LIBRARY=${b#*=} timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $K -o t -- python3 bench.py --steps 5 --warmup 1 > $K/log.txt 2>&1 || exit 1
   python3 - $K <<'PY' | tee -a $O/kstats.txt || exit 1
import csv, glob, re, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)[0]
for r in list(csv.DictReader(open(f)))[:14]:
    m = re.search(r"k_[a-z_0-9]+(<[^>]*>)?", r["Name"])
    print((m.group(0) if m else r["Name"][:30]).ljust(36), r["Calls"].rjust(6), ("%.3f ms" % (int(r["TotalDurationNs"]) / 1e6)).rjust(12),
          ("%.1f us" % (float(r["AverageNs"]) / 1e3)).rjust(12))
PY
   find $K -name "*.csv" -delete
done
export PIPS_HIP_DETERMINISTIC=1
run $1 --steps 5 --warmup 1 --dump-outputs $O/det_a && run $1 --steps 5 --warmup 1 --dump-outputs $O/det_a2 && run $2 --steps 5 --warmup 1 --dump-outputs $O/det_b || exit 1
python3 - $O <<'PY' | tee -a $O/lines.txt
import sys, numpy as np
o = sys.argv[1]
for v, what in (("a2", "the parent twice"), ("b", "the parent against the second build")):
    for f in ("x0.npy", "x_leaf.npy"):
        a, b = np.load(f"{o}/det_a/{f}"), np.load(f"{o}/det_{v}/{f}")
        print("deterministic mode,", what, f, a.shape, "array_equal", np.array_equal(a, b), "max abs diff", float(np.abs(a - b).max()))
PY
