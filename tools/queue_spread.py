#!/usr/bin/env python3
"""How a run's kernels spread over the GPU's hardware queues: usage: python tools/queue_spread.py <kernel_trace.csv | trace dir>

Input is a `rocprofv3 --kernel-trace --output-format csv` trace (tools/prof_pipe.sh writes one).  Only the middle half of the run's
kernels (by start time) is counted, so start-up and drain do not dilute the steady state.  Printed for that window:
  per queue:  kernels, busy share (union of its kernels' intervals / window), distinct streams, kernels that overlap the one before
  per stream: its queue(s) and kernel count
A queue runs its kernels one after the other, so a queue whose busy share is near 1 is a serial lane that bounds the step."""
import collections
import csv
import glob
import os
import sys


def load(path):
    if os.path.isdir(path):
        found = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
        if not found:
            sys.exit("no *kernel_trace.csv under %s" % path)
        path = found[0]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), (r.get("Agent_Id", ""), r["Queue_Id"]),
                         r.get("Stream_Id", "?"), r["Kernel_Name"]))
    rows.sort()
    return rows


def busy_time(iv, t0, t1):
    """length of the union of the intervals, clipped to [t0, t1]"""
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        s, e = max(s, t0), min(e, t1)
        if e <= s:
            continue
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    if cur_e is not None:
        tot += cur_e - cur_s
    return tot


def spread(rows):
    mid = rows[len(rows) // 4: 3 * len(rows) // 4]
    if not mid:
        sys.exit("trace has too few kernels")
    t0, t1 = mid[0][0], max(r[1] for r in mid)
    win = t1 - t0
    per_q = collections.defaultdict(list)
    per_s = collections.defaultdict(collections.Counter)
    for s, e, q, st, _ in mid:
        per_q[q].append((s, e, st))
        per_s[st][q] += 1
    qname = {q: i + 1 for i, q in enumerate(sorted(per_q, key=lambda q: (q[0], int(q[1]) if q[1].isdigit() else q[1])))}
    out = ["window %.2f ms, %d kernels, %d queues, %d streams" % (win / 1e6, len(mid), len(per_q), len(per_s))]
    for q in sorted(per_q, key=qname.get):
        ks = per_q[q]
        overl = sum(1 for a, b in zip(ks, ks[1:]) if b[0] < a[1])
        out.append("queue %d (id %s): %5d kernels (%.3f of the window's), busy %.3f, streams %d, overlapping the previous kernel %d" % (
            qname[q], q[1], len(ks), len(ks) / len(mid), busy_time([(s, e) for s, e, _ in ks], t0, t1) / win,
            len({st for _, _, st in ks}), overl))
    for st in sorted(per_s, key=lambda x: (int(x) if x.isdigit() else 1 << 62, x)):
        qs = per_s[st]
        out.append("stream %s: queue %s, %d kernels" % (st, "+".join(str(qname[q]) for q in sorted(qs, key=qname.get)), sum(qs.values())))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print("\n".join(spread(load(sys.argv[1]))))
