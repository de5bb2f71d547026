"""Box queries (crthip_bvh_query) on an MI355X: what profiles/bvh_query.md records.

    python tools/bvh_query_rate.py [--steps 20] [--warmup 3] [--units 256] [--grid 16] [--big 256] [--big-grid 100] [--only c4|big] [--out FILE]

1. `--units` C4 units (synth.bumpy_sphere(64, 32): 2 112 vertices, 4 096 faces, position + uv stored), every blob bound with bvh=True and a
   quantised position, `--grid`^3 coherent boxes a blob (a brick grid over the blob's box: 16^3 = 4 096 bricks), all in ONE call.
2. One mesh of synth.bumpy_sphere(N, N + 1) with N = `--big` (256: 131 584 faces) with `--big-grid`^3 bricks (100^3 = 1 M), coherent (the
   grid in row order) and incoherent (the same boxes shuffled).
Per leg, lists (at `--capacity` words a box) and CRTHIP_QUERY_COUNT taken in turn within every repetition: the host clock round
crthip_bvh_query + crthip_ctx_sync, median (min - max) of --steps calls after --warmup, and boxes a second from the median; the batch's
decode step (decode + sync) the same way; a decode with the query enqueued right behind it (the device transform record, no wait in
between) against the decode alone; the share of boxes that match a face and that are clipped; the nodes taken and faces tested a box,
counted by the host hook (crthip_bvh_query_model_stats) on a sample of the same boxes, whose records and lists must equal the kernel's byte
for byte.  One JSON record a line.  Needs a device: there is nothing to fall back to.
Under a profiler (rocprofv3 --kernel-trace --stats -- python tools/bvh_query_rate.py --only big --steps 5) the kernel is k_bvh_query."""
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


def brick_grid(t, n):
    """n*n*n boxes that tile the box of a transform record: BOX_DTYPE, row order; neighbours share their boundary planes"""
    lo = np.array([t.base[c] for c in range(3)], np.int64)
    hi = lo + np.array([t.span[c] for c in range(3)], np.int64)
    cuts = [np.linspace(lo[c], hi[c], n + 1).round().astype(np.int64) for c in range(3)]
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    return ca.make_boxes(np.stack([cuts[0][i], cuts[1][j], cuts[2][k]], axis=1), np.stack([cuts[0][i + 1], cuts[1][j + 1], cuts[2][k + 1]], axis=1))


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
    nbox, cap = grid ** 3, args.capacity
    rng = np.random.default_rng(1)
    boxes = []
    for i in range(len(blobs)):
        s = brick_grid(b.quant_transform(i, "position"), grid)
        boxes.append(s[rng.permutation(nbox)] if shuffle else s)
    dbox = torch.from_numpy(np.concatenate(boxes).view(np.uint8).reshape(-1)).to(dev)
    dres = torch.full((len(blobs) * nbox * 16,), 0xCD, dtype=torch.uint8, device=dev)
    dlist = torch.full((len(blobs) * nbox * cap,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sets = {fl: [b.query_set(i, dbox.data_ptr() + i * nbox * 32, dres.data_ptr() + i * nbox * 16, dlist.data_ptr() + i * nbox * cap * 4, nbox, cap, fl)
                 for i in range(len(blobs))] for fl in (0, ca.QUERY_COUNT)}
    ms = {0: [], ca.QUERY_COUNT: [], "decode": [], "decode+query": []}
    for k in range(args.warmup + args.steps):
        for fl in (0, ca.QUERY_COUNT):                        # the two in turn
            t = timed(lambda: ctx.bvh_query(sets[fl]), ctx.sync)
            if k >= args.warmup:
                ms[fl].append(t)
        t = timed(b.decode, b.sync)
        t2 = timed(lambda: (b.decode(), ctx.bvh_query(sets[0])), lambda: (ctx.sync(), b.sync()))
        if k >= args.warmup:
            ms["decode"].append(t); ms["decode+query"].append(t2)
    ctx.bvh_query(sets[0])
    ctx.sync()
    res = dres.cpu().numpy().view(ca.QUERY_RESULT_DTYPE)
    words = dlist.cpu().numpy().view(np.uint32).reshape(-1, cap)
    status = np.bincount(res["status"], minlength=4)
    # the host hook on a sample of the same boxes: its counts, and the kernel's bytes
    take = min(nbox, args.sample)
    nodes = b.bvh(0)[0]
    o = b.host_outputs(0)
    t0 = b.quant_transform(0, "position")
    base = [int(t0.base[c]) for c in range(3)]
    stats = {}
    for fl in (0, ca.QUERY_COUNT):
        got, lists, (taken, tested) = ca.bvh_query_model(nodes, o["position"].view(np.uint16), o["index"], boxes[0][:take], base=base, flags=fl, capacity=cap, with_stats=True,
                                                         fill=0xFF)
        stats[fl] = (taken / take, tested / take)
        if fl == 0:
            assert got.tobytes() == res[:take].tobytes(), "the kernel's records differ from the hook's"
            assert lists.tobytes() == words[:take].tobytes(), "the kernel's lists differ from the hook's"
    total = len(blobs) * nbox
    rec = dict(leg=name, blobs=len(blobs), faces=int(b.infos[0].nface), height=b.bvh(0)[3][3], boxes=total, capacity=cap, steps=args.steps, warmup=args.warmup,
               match_share=round(float((res["count"] > 0).sum()) / total, 4), faces_a_box=round(float(res["count"].sum()) / total, 2), max_count=int(res["count"].max()),
               status_counts=[int(x) for x in status],
               lists=summary(ms[0]), count=summary(ms[ca.QUERY_COUNT]), decode=summary(ms["decode"]), decode_then_query=summary(ms["decode+query"]),
               lists_Mbox_s=round(total / statistics.median(ms[0]) / 1e3, 1), count_Mbox_s=round(total / statistics.median(ms[ca.QUERY_COUNT]) / 1e3, 1),
               hook_sample=take, nodes_a_box=round(stats[0][0], 2), faces_tested_a_box=round(stats[0][1], 2))
    emit(rec, out)
    b.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", type=int, default=256)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--big-grid", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--only", choices=("c4", "big"))
    ap.add_argument("--out")
    args = ap.parse_args()
    if ca.lib().crthip_device_count() < 1:
        sys.exit("bvh_query_rate: no HIP device")
    if args.only != "big":
        blobs = [ca.encode(synth.bumpy_sphere(64, 32, seed=i), position_bits=14, uv_bits=12, with_normal=False, with_color=False) for i in range(args.units)]
        leg("c4 units, coherent", blobs, args.grid, args, args.out)
    if args.only != "c4":
        blob = [ca.encode(synth.bumpy_sphere(args.big, args.big + 1, seed=1), position_bits=14, with_normal=False, with_color=False, with_uv=False)]
        leg("big mesh, coherent", blob, args.big_grid, args, args.out)
        leg("big mesh, incoherent", blob, args.big_grid, args, args.out, shuffle=True)


if __name__ == "__main__":
    main()
