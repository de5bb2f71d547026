#!/usr/bin/env python3
"""The premise of the pool's groups (profiles/pool_group.md): bench.py's pool on items of 256 and of 512 C4 blobs.

    python tools/pool_group_probe.py ab | one256 | one512        (STEPS=3000: 256-blob steps a run)
    python tools/pool_group_probe.py stats <trace dir> <label>

Pool([0], threads=5, depth=4), set_packed_host_blobs(True).  The 256-blob item is bench.load_blobs(0) in one pinned_host_arena; the 512-blob item
is load_blobs(0) + load_blobs(256) - seeds 0..511 - in ONE pinned_host_arena.  Each item is warmed with 8 x lanes + 400 steps.  `ab`: three
rounds, the two items alternating, STEPS x 256 blobs a run behind a warm-up of 8 x lanes steps; a line a run.  `one256` / `one512`: one such run
of one item and nothing else - what a `rocprofv3 --output-format csv --kernel-trace -d DIR -o t -- python tools/pool_group_probe.py one256` is
taken over (a pool with groups decodes that item two tickets a call).  `stats`: per-kernel count and average duration over the middle half of
that trace's kernels, the window tools/queue_spread.py uses for the queues."""
import collections
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def stats(path, label):
    f = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    mid = rows[len(rows) // 4: 3 * len(rows) // 4]
    t0, t1 = int(mid[0]["Start_Timestamp"]), max(int(r["End_Timestamp"]) for r in mid)
    acc = collections.defaultdict(list)
    for r in mid:
        acc[r["Kernel_Name"].split("(")[0].replace("corto_hip::", "")].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("%s: window %.2f ms, %d kernels, sum of durations %.1f ms" % (label, (t1 - t0) / 1e6, len(mid), sum(sum(v) for v in acc.values()) / 1e3))
    for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        print("%s: %-28s n=%5d avg %8.1f us max %8.1f" % (label, k, len(v), sum(v) / len(v), max(v)))


def main():
    mode = sys.argv[1]
    if mode == "stats":
        return stats(sys.argv[2], sys.argv[3])
    import bench
    import corto_amd as ca
    steps = int(os.environ.get("STEPS", "3000"))
    b0, _ = bench.load_blobs(0)
    items = {}
    if mode in ("ab", "one256"):
        items[256] = ca.pinned_host_arena(b0)
    if mode in ("ab", "one512"):
        b1, _ = bench.load_blobs(256)
        items[512] = ca.pinned_host_arena(list(b0) + list(b1))
    pool = ca.Pool([0], threads=5, depth=4)
    pool.set_packed_host_blobs(True)
    for n, (pin, views) in items.items():
        pool.run([views], steps=8 * pool.lanes, warmup=0)
        pool.run([views], steps=400, warmup=0)
    for rep_i in range(3 if mode == "ab" else 1):
        for n, (pin, views) in items.items():
            k = steps * 256 // n
            rep, st = pool.run([views], steps=k, warmup=8 * pool.lanes)
            assert rep.failed_blobs == 0 and rep.first_error == 0, (rep.failed_blobs, rep.first_error)
            print("PREMISE blobs/item %d run %d: %d steps %.4f ms/step %.4f ms/256blobs %.1f Mtri/s host_us_per_step %.0f plan %.0f wait %.0f finish %.0f grouped_steps %d" % (
                n, rep_i, k, rep.elapsed_s / k * 1e3, rep.elapsed_s / k * 1e3 * 256 / n, rep.triangles / rep.elapsed_s / 1e6,
                rep.host_us_per_step, rep.host_plan_us, rep.host_wait_us, rep.host_finish_us, rep.grouped_steps), flush=True)
    pool.close()


if __name__ == "__main__":
    main()
