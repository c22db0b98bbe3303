"""digest of a rocprofv3 kernel trace (csv): per-kernel statistics of the tile kernels, launches per factorisation, per-group durations of
the panel and deep launches, and the launch-by-launch timeline of the last factorisation's tail (profiles/tail_panel_ab.txt).
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o LABEL -- python bench.py --gpus 1 --steps 6 --warmup 2
       python tools/tail_panel_digest.py DIR LABEL"""
import csv
import glob
import re
import sys
from collections import defaultdict

d, label = sys.argv[1], sys.argv[2]
files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
assert files, "no kernel trace under " + d
rows = []
for f in files:
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()


def short(n):
    n = re.sub(r"\(.*", "", n).replace("pips::", "").replace("void ", "")
    return n


stat = defaultdict(lambda: [0, 0])
for s, e, n in rows:
    st = stat[short(n)]
    st[0] += 1
    st[1] += e - s
print(f"== {label}: {len(rows)} kernel launches in the trace")
tot = sum(v[1] for v in stat.values())
for n, (c, t) in sorted(stat.items(), key=lambda kv: -kv[1][1])[:25]:
    print(f"{n:60s} calls {c:7d}  total {t / 1e6:10.3f} ms  mean {t / c / 1e3:9.1f} us  {100.0 * t / tot:5.1f} %")

# factorisations: split at k_arena_clear (once per factorisation, before the tails)
tile = [(s, e, short(n)) for s, e, n in rows if "k_tile_" in n]
marks = [s for s, e, n in rows if "k_arena_clear" in n]
facts = []
for i, m in enumerate(marks):
    hi = marks[i + 1] if i + 1 < len(marks) else 1 << 62
    facts.append([t for t in tile if m <= t[0] < hi])
facts = [f for f in facts if f]
assert len(facts) >= 2, "fewer than two factorisations (k_arena_clear launches) in the trace: nothing to average over"
print(f"factorisations in the trace: {len(facts)}; tile-kernel launches in each: {sorted(set(len(f) for f in facts))}")
per = defaultdict(lambda: defaultdict(list))
for f in facts[1:]:
    idx = defaultdict(int)
    for s, e, n in f:
        per[n][idx[n]].append((e - s) / 1e3)
        idx[n] += 1
for n in per:
    if "k_tile_panel" in n or "k_tile_gemm_bal<0>" in n:
        print(f"-- {n}: mean us per launch index (group) over {len(facts) - 1} factorisations")
        print("   " + " ".join(f"{sum(v) / len(v):.0f}" for _, v in sorted(per[n].items())))
last = facts[-1]
t0 = last[0][0]
print(f"-- timeline of the last factorisation's tile kernels (start us, duration us, gap to the latest end before it us, kernel)")
end = t0
busy = 0
for s, e, n in last:
    gap = (s - end) / 1e3
    print(f"{(s - t0) / 1e3:10.1f} {(e - s) / 1e3:9.1f} {gap:8.1f}  {n}")
    end = max(end, e)
span = (end - t0) / 1e3
# idle time: union of the intervals
iv = sorted((s, e) for s, e, _ in last)
cur_s, cur_e = iv[0]
for s, e in iv[1:]:
    if s > cur_e:
        busy += cur_e - cur_s
        cur_s, cur_e = s, e
    else:
        cur_e = max(cur_e, e)
busy += cur_e - cur_s
print(f"tile kernels of the last factorisation: span {span:.1f} us, device busy with them {busy / 1e3:.1f} us, idle {span - busy / 1e3:.1f} us")
