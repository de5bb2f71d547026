"""crthip_encode_batch_attrs on a LiDAR-like cloud with and without its three generic attributes (int16 intensity, int8 class, double GPS
time): one JSON record per leg - the call's wall time (best of --reps), its stats and its per-kernel times, the blob size.

    python tools/encode_generic_rate.py [--points 1000003] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corto_amd as ca  # noqa: E402
from test_encode_generic_gpu import lidar  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000003)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m, attrs = lidar(a.points)
    ctx = ca.Context(0)
    ctx.set_profiling(True)
    recs = []
    for leg, extra in (("positions only", None), ("+ intensity, class, gps_time", attrs)):
        kw = dict(position_bits=0, position_q=0.001)
        if extra is not None:
            kw["attributes"] = extra
        ca.encode_batch([m], ctx, kw=[kw])                  # warm-up
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            blobs, st = ca.encode_batch([m], ctx, kw=[kw], with_stats=True)
            t = (time.perf_counter() - t0) * 1e3
            if best is None or t < best[0]:
                best = (t, st, len(blobs[0]))
        t, st, size = best
        rec = dict(leg=leg, points=m.nvert, wall_ms=round(t, 3), blob_bytes=size,
                   input_bytes=int(m.position.nbytes + sum(v.nbytes for _, v, _, _ in (extra or []))),
                   quantize_ms=st["kernel_times"].get("enc_quantize_batch", {}).get("ms"), stats=st)
        recs.append(rec)
        print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
