#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace CSV: per hardware queue, how many samples' chains it carried (scan launches), the streams that
fed it (when the trace names them), the sum of its kernels' time per sample and how much of the wall time it was busy -- is the
headline the length of one sample's chain on a queue two engines share?   tools/trace_queues.py kernel_trace.csv [warmup scans]"""
import csv, sys
from collections import defaultdict
rows = list(csv.DictReader(open(sys.argv[1])))
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void bk::", "").replace("bk::", ""),
       r.get("Queue_Id", "0"), r.get("Stream_Id", "")) for r in rows]
ev.sort()
scans = [e for e in ev if e[2].startswith(("scan_count", "scan_items"))]
warm = int(sys.argv[2]) if len(sys.argv) > 2 else len(scans) // 3   # (bench.py --steps 4 --warmup 2: a third of the launches warm up)
t_lo = scans[min(warm, len(scans) - 1)][0]
ev = [e for e in ev if e[0] >= t_lo]
wall = ev[-1][1] - ev[0][0]
n_scan = sum(1 for e in ev if e[2].startswith(("scan_count", "scan_items")))
print("window: %.3f ms, %d scan launches -> %.4f ms per sample; %d queues" % (wall / 1e6, n_scan, wall / 1e6 / max(n_scan, 1), len({e[3] for e in ev})))
by_q = defaultdict(list)
for e in ev: by_q[e[3]].append(e)
for q, es in sorted(by_q.items(), key=lambda kv: -len(kv[1])):
    ns = sum(1 for e in es if e[2].startswith(("scan_count", "scan_items")))
    tot = sum(e[1] - e[0] for e in es)
    busy, end = 0, 0
    for s, e2, *_ in es:   # union of the queue's kernel intervals (sorted by start)
        if e2 > end: busy += e2 - max(s, end); end = e2
    streams = sorted({e[4] for e in es if e[4] != ""})
    # how often the queue's next scan launch belongs to another stream than its last: two engines' chains taking turns
    sw = [e[4] for e in es if e[2].startswith(("scan_count", "scan_items"))]
    turns = sum(1 for a, b in zip(sw, sw[1:]) if a != b)
    print("queue %-4s kernels %5d  samples %4d  streams %-12s scan-to-scan stream changes %4d  kernel time %8.1f us per sample  busy %5.1f %% of the window" %
          (q, len(es), ns, ",".join(streams) or "?", turns, tot / 1e3 / max(ns, 1), 100.0 * busy / max(wall, 1)))
    per = defaultdict(int)
    for e in es: per[e[2]] += e[1] - e[0]
    print("           " + "  ".join("%s %.1f" % (n[:18], t / 1e3 / max(ns, 1)) for n, t in sorted(per.items(), key=lambda kv: -kv[1])[:9]))
