"""What crthip_pool_decode costs beside crthip_pool_run, on the batch and the pool shape bench.py uses.

    python tools/pool_decode_rate.py [--items 40] [--reps 5] [--host-threads 5] [--depth 4] [--distinct 1] [--out FILE]

The C4 batch (256 blobs x 4 096 triangles, bench.py: load_blobs) is handed over as --items items with a device block each, so a call writes
--items distinct output blocks where crthip_pool_run reuses its lanes' own.  --distinct K: the items cycle through K different batches (seeds 256 k ..
256 k + 255, a pinned buffer and a device arena each) instead of naming one - what a lane call that decodes a GROUP of items meets in real use: two
items' dictionaries, two uploads from two buffers (profiles/pool_group.md).  Measured, --reps times each on ONE pool, in turn:
    decode/host      crthip_pool_decode, blobs in one pinned host buffer (packed: uploaded inside the step)
    run/host         crthip_pool_run for --items steps (warmup 0) on the same items
    decode/resident  crthip_pool_decode, blobs resident in HBM (device arenas)
    run/resident     crthip_pool_run for --items steps on those
A line per leg: median and range of Gtri/s over the call's elapsed_s - both calls start with empty lanes and end drained, so both pay the
pipeline's filling and draining, which bench.py's long timed region does not - and the medians of the report's host_plan_us / host_wait_us /
host_finish_us (per step and worker thread).  The lines go to stdout and, with --out, are appended to FILE.
The driver around it (a shell script that runs every GPU step under its own time limit) adds bench.py's `value` of this branch and of its
parent: profiles/pool_decode_rate.md."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBLOBS = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=5)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--distinct", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import corto_amd as ca
    from corto_amd import synth
    from oracle import oracle as oc
    K = max(1, args.distinct)
    batches = [[ca.encode(synth.bumpy_sphere(64, 32, seed=k * NBLOBS + i), position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER)
                for i in range(NBLOBS)] for k in range(K)]
    blobs = batches[0]
    arena_k = [ca.upload_arena([ca.aligned_blob(b) for b in bl], 0) for bl in batches]
    pool = ca.Pool([0], threads=args.host_threads, depth=args.depth)
    lines = []
    try:
        pins = [ca.pinned_host_arena(bl) for bl in batches]
        views = pins[0][1]
        n = args.items
        its = [pins[j % K][1] for j in range(n)]
        legs = {"host": dict(items=its, arenas=None, packed=True),
                "resident": dict(items=its, arenas=[[arena_k[j % K]] for j in range(n)], packed=False)}
        total = ca.output_layout(views)[1]
        blocks = [torch.empty(total, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        torch.cuda.synchronize()
        tris = NBLOBS * 4096 * n
        # every context used and the GPU at its clocks before anything is timed (bench.py does the same)
        pool.set_packed_host_blobs(True)
        pool.run(legs["host"]["items"], steps=8 * pool.lanes, warmup=0)
        pool.decode(legs["host"]["items"], dest="device", blocks=blocks)
        samples = {}
        for _ in range(args.reps):
            for name, leg in legs.items():
                pool.set_packed_host_blobs(leg["packed"])
                res, rep = pool.decode(leg["items"], dest="device", arenas=leg["arenas"], blocks=blocks)
                assert rep.failed_blobs == 0 and rep.steps == n and rep.triangles == tris, (name, rep.failed_blobs)
                samples.setdefault("decode/" + name, []).append(rep)
                rep, _ = pool.run(leg["items"], steps=n, warmup=0, arenas=leg["arenas"])
                assert rep.failed_blobs == 0 and rep.triangles == tris, (name, rep.failed_blobs)
                samples.setdefault("run/" + name, []).append(rep)
        # the last call's blocks against the oracle: a sample of blobs of the first, a middle and the last item
        lay = ca.output_layout(views)[0]
        for j in (0, n // 2, n - 1):
            raw = res[j].block.cpu().numpy()
            for i in (0, 101, 255):
                ref = oc.decode(ca.aligned_blob(batches[j % K][i]))
                for name, (o, dt, shape) in lay[i].items():
                    assert raw[o:o + ref[name].nbytes].tobytes() == ref[name].tobytes(), (j, i, name)
        lines.append("pool %d x %d lanes (%d), %d items of %d blobs x 4096 triangles (%d distinct), %d repetitions, GPU_MAX_HW_QUEUES=%s" % (
            args.host_threads, args.depth, pool.lanes, n, NBLOBS, K, args.reps, os.environ.get("GPU_MAX_HW_QUEUES", "unset")))
        lines.append("| leg | Gtri/s median | range | ms a call | host_plan_us | host_wait_us | host_finish_us | host_us_per_step |")
        lines.append("|---|---|---|---|---|---|---|---|")
        for name in ("decode/host", "run/host", "decode/resident", "run/resident"):
            reps = samples[name]
            g = np.array([r.triangles / r.elapsed_s / 1e9 for r in reps])
            med = lambda f: float(np.median([getattr(r, f) for r in reps]))   # noqa: E731
            lines.append("| %s | %.2f | %.2f - %.2f | %.2f | %.0f | %.0f | %.0f | %.0f |" % (
                name, np.median(g), g.min(), g.max(), 1e3 * float(np.median([r.elapsed_s for r in reps])),
                med("host_plan_us"), med("host_wait_us"), med("host_finish_us"), med("host_us_per_step")))
    finally:
        pool.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
