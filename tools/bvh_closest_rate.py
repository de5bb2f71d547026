"""Closest-face queries (crthip_bvh_closest) on an MI355X: what profiles/bvh_closest.md records.

    python tools/bvh_closest_rate.py [--steps 20] [--warmup 3] [--units 256] [--points 4096] [--sample 1024] [--only near|far] [--out FILE]

`--units` C4 units (synth.bumpy_sphere(64, 32): 2 112 vertices, 4 096 faces, position + uv stored), every blob bound with bvh=True and a
quantised position, `--points` points a blob, all in ONE call, in two legs:
  near  the blob's own vertices (drawn with repetition) moved by up to 8 grid units a component: points at the surface;
  far   points drawn evenly from the blob's box grown by its own size on every side: most of them far from the surface.
Per leg, the plain call and CRTHIP_CLOSEST_WITHIN (radius 16 grid units in the near leg, a quarter of the box's longest side in the far
one) taken in turn within every repetition: the host clock round crthip_bvh_closest + crthip_ctx_sync, median (min - max) of --steps calls
after --warmup, and points a second from the median; the batch's decode step (decode + sync) the same way; a decode with the call enqueued
right behind it (the device transform record, no wait in between); the share of points with a face, by feature code; the nodes taken and
faces tested a point, counted by the host hook (crthip_bvh_closest_model_stats) in both child orders on a sample of the first blob's points,
whose records must equal the kernel's byte for byte.  One JSON record a line.  Needs a device: there is nothing to fall back to.
Under a profiler (rocprofv3 --kernel-trace --stats -- python tools/bvh_closest_rate.py --only near --steps 5) the kernel is k_bvh_closest."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def summary(ms):
    return dict(median_us=round(statistics.median(ms) * 1e3, 1), min_us=round(min(ms) * 1e3, 1), max_us=round(max(ms) * 1e3, 1))


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def leg(name, blobs, args, out):
    import torch
    dev = torch.device("cuda", 0)
    ctx = ca.Context(0)
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(index16=all(ca.probe(x).nvert < 65536 for x in blobs), bvh=True, quantized=("position",))
    records = torch.zeros(48 * sum(i.nattr for i in b.infos), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    b.bind_quant_transforms(records.data_ptr())
    b.decode()
    assert (b.sync() == 0).all()
    n = args.points
    rng = np.random.default_rng(1)
    pts = []
    for i in range(len(blobs)):
        t = b.quant_transform(i, "position")
        base = np.array([t.base[c] for c in range(3)], np.int64)
        span = np.array([t.span[c] for c in range(3)], np.int64)
        if name == "near":
            u16 = b.host_outputs(i)["position"].view(np.uint16).reshape(-1, 3).astype(np.int64)
            p, r = base + u16[rng.integers(0, len(u16), n)] + rng.integers(-8, 9, (n, 3)), 16
        else:
            p, r = rng.integers(base - span, base + 2 * span + 1, (n, 3)), int(span.max()) // 4
        pts.append(ca.make_points(p, r))
    dpt = torch.from_numpy(np.concatenate(pts).view(np.uint8).reshape(-1)).to(dev)
    dhit = torch.full((len(blobs) * n * 48,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    flagset = (0, ca.CLOSEST_WITHIN)
    sets = {fl: [b.closest_set(i, dpt.data_ptr() + i * n * 16, dhit.data_ptr() + i * n * 48, n, fl) for i in range(len(blobs))] for fl in flagset}
    ms = {0: [], ca.CLOSEST_WITHIN: [], "decode": [], "decode+closest": []}
    for k in range(args.warmup + args.steps):
        for fl in flagset:                                    # the two in turn
            t = timed(lambda: ctx.bvh_closest(sets[fl]), ctx.sync)
            if k >= args.warmup:
                ms[fl].append(t)
        t = timed(b.decode, b.sync)
        t2 = timed(lambda: (b.decode(), ctx.bvh_closest(sets[0])), lambda: (ctx.sync(), b.sync()))
        if k >= args.warmup:
            ms["decode"].append(t); ms["decode+closest"].append(t2)
    total = len(blobs) * n
    rec = dict(leg=name, blobs=len(blobs), faces=int(b.infos[0].nface), height=b.bvh(0)[3][3], points=total, steps=args.steps, warmup=args.warmup,
               decode=summary(ms["decode"]), decode_then_closest=summary(ms["decode+closest"]))
    # the host hook on a sample of the first blob's points: its counts in both child orders, and the kernel's bytes
    take = min(n, args.sample)
    nodes = b.bvh(0)[0]
    o = b.host_outputs(0)
    t0 = b.quant_transform(0, "position")
    base = [int(t0.base[c]) for c in range(3)]
    for fl, tag in zip(flagset, ("plain", "within")):
        ctx.bvh_closest(sets[fl])
        ctx.sync()
        res = dhit.cpu().numpy().view(ca.CLOSEST_HIT_DTYPE)
        hit = res["status"] == ca.CLOSEST_HIT
        stats = {}
        for order in (0, 1):
            got, stats[order] = ca.bvh_closest_model(nodes, o["position"].view(np.uint16), o["index"], pts[0][:take], base=base, flags=fl, with_stats=True, fill=0xFF, order=order)
            assert got.tobytes() == res[:take].tobytes(), "the kernel's records differ from the hook's"
        rec[tag] = dict(summary(ms[fl]), Mpoint_s=round(total / statistics.median(ms[fl]) / 1e3, 1), hit_share=round(float(hit.sum()) / total, 4),
                        status_counts=[int(x) for x in np.bincount(res["status"], minlength=4)], feature_counts=[int(x) for x in np.bincount(res["feature"][hit], minlength=7)],
                        wide_records=int(((res["num_hi"] > 0) | (res["den_hi"] > 0)).sum()), hook_sample=take,
                        nodes_a_point=round(stats[0][0] / take, 2), faces_a_point=round(stats[0][1] / take, 2),
                        nodes_a_point_own_order=round(stats[1][0] / take, 2), faces_a_point_own_order=round(stats[1][1] / take, 2))
    emit(rec, out)
    b.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", type=int, default=256)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=1024)
    ap.add_argument("--only", choices=("near", "far"))
    ap.add_argument("--out")
    args = ap.parse_args()
    if ca.lib().crthip_device_count() < 1:
        sys.exit("bvh_closest_rate: no HIP device")
    blobs = [ca.encode(synth.bumpy_sphere(64, 32, seed=i), position_bits=14, uv_bits=12, with_normal=False, with_color=False) for i in range(args.units)]
    for name in ("near", "far"):
        if args.only in (None, name):
            leg(name, blobs, args, args.out)


if __name__ == "__main__":
    main()
