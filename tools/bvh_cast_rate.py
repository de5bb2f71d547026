"""Segment casts (crthip_bvh_cast) on an MI355X: what profiles/bvh_cast.md records.

    python tools/bvh_cast_rate.py [--steps 20] [--warmup 3] [--units 256] [--grid 64] [--big 256] [--big-grid 1024] [--only c4|big] [--out FILE]

1. `--units` C4 units (synth.bumpy_sphere(64, 32): 2 112 vertices, 4 096 faces, position + uv stored), every blob bound with bvh=True and a
   quantised position, `--grid`^2 coherent segments a blob (a camera grid over the blob's box, along -z), all in ONE call.
2. One mesh of synth.bumpy_sphere(N, N + 1) with N = `--big` (256: 131 584 faces) with `--big-grid`^2 segments, coherent (the camera grid in
   row order) and incoherent (the same segments shuffled).
Per leg, nearest and any-hit taken in turn within every repetition: the host clock round crthip_bvh_cast + crthip_ctx_sync, median (min - max)
of --steps calls after --warmup, and segments a second from the median; the batch's decode step (decode + sync) the same way; a decode with
the cast enqueued right behind it (the device transform record, no wait in between) against the decode alone; the share of segments that
hit; the nodes taken and faces tested a segment, counted by the host hook (crthip_bvh_cast_model_stats) on a sample of the same segments,
whose records must equal the kernel's byte for byte.  One JSON record a line.  Needs a device: there is nothing to fall back to.
Under a profiler (rocprofv3 --kernel-trace --stats -- python tools/bvh_cast_rate.py --only big --steps 5) the kernel is k_bvh_cast."""
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


def camera_grid(t, n):
    """n*n segments along -z over the box of a transform record, from 4 steps above it to 4 below: SEGMENT_DTYPE, row order"""
    lo = np.array([t.base[c] for c in range(3)], np.int64)
    hi = lo + np.array([t.span[c] for c in range(3)], np.int64)
    xs = np.linspace(lo[0], hi[0], n).round().astype(np.int64)
    ys = np.linspace(lo[1], hi[1], n).round().astype(np.int64)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.full(n * n, hi[2] + 4)], axis=1)
    q = np.stack([x.ravel(), y.ravel(), np.full(n * n, lo[2] - 4)], axis=1)
    return ca.make_segments(p, q)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def leg(name, blobs, grid, args, out, shuffle=False):
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
    nseg = grid * grid
    rng = np.random.default_rng(1)
    segs = []
    for i in range(len(blobs)):
        s = camera_grid(b.quant_transform(i, "position"), grid)
        segs.append(s[rng.permutation(nseg)] if shuffle else s)
    dseg = torch.from_numpy(np.concatenate(segs).view(np.uint8).reshape(-1)).to(dev)
    dhit = torch.full((len(blobs) * nseg * 32,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sets = {fl: [b.cast_set(i, dseg.data_ptr() + i * nseg * 32, dhit.data_ptr() + i * nseg * 32, nseg, fl) for i in range(len(blobs))]
            for fl in (0, ca.CAST_ANY)}
    ms = {0: [], ca.CAST_ANY: [], "decode": [], "decode+cast": []}
    for k in range(args.warmup + args.steps):
        for fl in (0, ca.CAST_ANY):                           # the two in turn
            t = timed(lambda: ctx.bvh_cast(sets[fl]), ctx.sync)
            if k >= args.warmup:
                ms[fl].append(t)
        t = timed(b.decode, b.sync)
        t2 = timed(lambda: (b.decode(), ctx.bvh_cast(sets[0])), lambda: (ctx.sync(), b.sync()))
        if k >= args.warmup:
            ms["decode"].append(t); ms["decode+cast"].append(t2)
    ctx.bvh_cast(sets[0])
    ctx.sync()
    hits = dhit.cpu().numpy().view(ca.CAST_HIT_DTYPE)
    status = np.bincount(hits["status"], minlength=4)
    # the host hook on a sample of the same segments: its counts, and the kernel's bytes
    take = min(nseg, args.sample)
    nodes = b.bvh(0)[0]
    o = b.host_outputs(0)
    t0 = b.quant_transform(0, "position")
    base = [int(t0.base[c]) for c in range(3)]
    stats = {}
    for fl in (0, ca.CAST_ANY):
        got, (taken, tested) = ca.bvh_cast_model(nodes, o["position"].view(np.uint16), o["index"], segs[0][:take], base=base, flags=fl, with_stats=True)
        stats[fl] = (taken / take, tested / take)
        if fl == 0:
            assert got.tobytes() == hits[:take].tobytes(), "the kernel's records differ from the hook's"
    total = len(blobs) * nseg
    rec = dict(leg=name, blobs=len(blobs), faces=int(b.infos[0].nface), height=b.bvh(0)[3][3], segments=total, steps=args.steps, warmup=args.warmup,
               hit_share=round(float(status[1]) / total, 4), status_counts=[int(x) for x in status],
               nearest=summary(ms[0]), any=summary(ms[ca.CAST_ANY]), decode=summary(ms["decode"]), decode_then_cast=summary(ms["decode+cast"]),
               nearest_Mseg_s=round(total / statistics.median(ms[0]) / 1e3, 1), any_Mseg_s=round(total / statistics.median(ms[ca.CAST_ANY]) / 1e3, 1),
               hook_sample=take, nodes_a_segment_nearest=round(stats[0][0], 2), faces_a_segment_nearest=round(stats[0][1], 2),
               nodes_a_segment_any=round(stats[ca.CAST_ANY][0], 2), faces_a_segment_any=round(stats[ca.CAST_ANY][1], 2))
    emit(rec, out)
    b.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--big-grid", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--only", choices=("c4", "big"))
    ap.add_argument("--out")
    args = ap.parse_args()
    if ca.lib().crthip_device_count() < 1:
        sys.exit("bvh_cast_rate: no HIP device")
    if args.only != "big":
        blobs = [ca.encode(synth.bumpy_sphere(64, 32, seed=i), position_bits=14, uv_bits=12, with_normal=False, with_color=False) for i in range(args.units)]
        leg("c4 units, coherent", blobs, args.grid, args, args.out)
    if args.only != "c4":
        blob = [ca.encode(synth.bumpy_sphere(args.big, args.big + 1, seed=1), position_bits=14, with_normal=False, with_color=False, with_uv=False)]
        leg("big mesh, coherent", blob, args.big_grid, args, args.out)
        leg("big mesh, incoherent", blob, args.big_grid, args, args.out, shuffle=True)


if __name__ == "__main__":
    main()
