"""Host create against resident create (crthip_batch_create_resident): what planning a batch costs when the blobs are host arrays and
the host walks them, and when they live only in device memory and the walk runs on the device (k_walk_blobs) with one copy of the records
back and one synchronisation.

    python tools/resident_walk_time.py [--reps 50] [--out DIR]

Three batches: 256 C4 blobs (c4_blobs16 x 16), 4 096 C4 blobs, 16 C2-class meshes (128 K vertices, BORDER normals: four seeds, each four
times).  One batch object per form, reset REPS times after a warm-up; per form the median and the spread of the call's wall time, the
host time inside it (crthip_batch_stats.host_create_us) and, for the resident form, the walk kernel's device time
(crthip_walk_stats.walk_kernel_us) and the bytes it copied back.  One JSON line per batch on stdout and in DIR/resident_walk.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402


def c4_blobs(n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "c4_blobs16.npz"))
    base = [np.ascontiguousarray(z["crt_%02d" % i], dtype=np.uint8) for i in range(16)]
    return [base[i % 16] for i in range(n)]


def c2_blobs():
    four = [ca.encode(synth.bumpy_sphere(512, 250, seed=s), normal_prediction=ca.BORDER) for s in range(1, 5)]
    return [four[i % 4] for i in range(16)]


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 2), p10=round(float(np.percentile(v, 10)), 2), p90=round(float(np.percentile(v, 90)), 2))


def measure(ctx, name, blobs, reps):
    host_blobs = [ca.aligned_blob(b) for b in blobs]
    offs, total = ca.arena_layout([len(b) for b in blobs])
    lens = np.array([len(b) for b in blobs], dtype=np.uint32)
    img = np.zeros(max(total, 16), dtype=np.uint8)
    for b, o in zip(blobs, offs):
        img[int(o):int(o) + len(b)] = b
    dev = torch.from_numpy(img).to("cuda:0")
    torch.cuda.synchronize()
    hb = ca.Batch(ctx, host_blobs)
    rb = ca.Batch.resident(ctx, dev, offs, lens)
    out = dict(batch=name, blobs=len(blobs), blob_bytes=int(lens.sum()))
    for form, reset in (("host", lambda: hb.reset(host_blobs)), ("resident", lambda: rb.reset_resident(dev, offs, lens))):
        b = hb if form == "host" else rb
        for _ in range(5):
            reset()
        ctx.sync()
        wall, host_us, walk_us = [], [], []
        for _ in range(reps):
            t = time.perf_counter()
            reset()
            wall.append((time.perf_counter() - t) * 1e6)
            host_us.append(b.stats().host_create_us)
            walk_us.append(b.walk_stats().walk_kernel_us)
            ctx.sync()                                   # (the host form's upload is not waited for by the call: drain it between calls)
        ws = b.walk_stats()
        out[form] = dict(wall_us=stats(wall), host_create_us=stats(host_us), device_walked=ws.device_walked, host_walked=ws.host_walked,
                         bytes_to_host=int(ws.bytes_to_host))
        if form == "resident":
            out[form]["walk_kernel_us"] = stats(walk_us)
    # the two forms planned the same thing
    assert [bytes(i) for i in hb.infos] == [bytes(i) for i in rb.infos]
    hb.close(); rb.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = ca.Context(0)
    rows = []
    for name, blobs in (("C4 x 256", c4_blobs(256)), ("C4 x 4096", c4_blobs(4096)), ("C2-class x 16", c2_blobs())):
        r = measure(ctx, name, blobs, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "resident_walk.jsonl"), "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
