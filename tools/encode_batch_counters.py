"""What a batch encode does, counted, for comparing two builds of the library (CORTO_HIP_LIB_PATH selects one): every workload of
tools/encode_batch_rate.py x topology mode x host_threads (1, 16) through crthip_encode_batch and through crthip_encode_batch_to_device.

    python tools/encode_batch_counters.py [--out FILE]

One JSON record per call: the SHA-256 over all blobs (device output: over the arena copied back), bytes_to_device, bytes_from_device,
value_streams, the cloud and topology counters, the splice statistics (but its kernel time) and every kernel's launches.  Nothing in a
record is a time, so the records of two builds that do the same work are equal line by line.

    python tools/encode_batch_counters.py --trace

--trace: what a rocprofv3 run of each build is made over - a warm-up, then one crthip_encode_batch of the 256 x C4 unit workload in host
mode and one crthip_encode_batch_to_device of it in device mode."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import corto_amd as ca  # noqa: E402
from encode_batch_rate import workloads  # noqa: E402

COUNTERS = ("bytes_to_device", "bytes_from_device", "value_streams", "clouds_device_sorted", "clouds_host_sorted", "topology_device", "topology_lds")


def record(name, mode, threads, entry, sha, st):
    rec = dict(workload=name, mode=mode, host_threads=threads, entry=entry, sha256=sha)
    rec.update({k: st[k] for k in COUNTERS})
    rec["launches"] = {k: v["launches"] for k, v in sorted(st["kernel_times"].items())}
    if "splice" in st:
        rec["splice"] = {k: v for k, v in sorted(st["splice"].items()) if k != "splice_kernel_us"}
    return rec


def counters(out):
    recs = []
    for name, meshes, kw in workloads():
        for mode in ("host", "device", "split"):
            ctx = ca.Context(0)
            ctx.set_profiling(True)
            ctx.set_encode_topology(mode)
            for threads in (1, 16):
                blobs, st = ca.encode_batch(meshes, ctx, kw=kw, host_threads=threads, with_stats=True)
                h = hashlib.sha256()
                for b in blobs:
                    h.update(b.tobytes())
                recs.append(record(name, mode, threads, "encode_batch", h.hexdigest(), st))
                arena, _, _, st = ca.encode_batch_to_device(meshes, ctx, kw=kw, host_threads=threads, with_stats=True)
                sha = hashlib.sha256(arena[:st["total"]].cpu().numpy().tobytes()).hexdigest()
                recs.append(record(name, mode, threads, "encode_batch_to_device", sha, st))
                for r in recs[-2:]:
                    print(json.dumps(r), flush=True)
            ctx.close()
    if out:
        with open(out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


def trace():
    name, meshes, kw = next(workloads())
    ctx = ca.Context(0)
    ca.encode_batch(meshes[:2], ctx, kw=kw)
    ca.encode_batch_to_device(meshes[:2], ctx, kw=kw)
    ca.encode_batch(meshes, ctx, kw=kw)
    ctx.set_encode_topology("device")
    ca.encode_batch_to_device(meshes, ctx, kw=kw)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    trace() if a.trace else counters(a.out)
