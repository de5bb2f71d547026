"""crthip_encode_batch_layout against what a caller had to do without it: one JSON record per topology mode (INTEGRATION.md §3c,
profiles/encode_layout.md).

    python tools/encode_layout_rate.py [--out FILE] [--reps 9] [--units 256]

256 C4 units are encoded, decoded into interleaved render buffers (Batch.allocate_interleaved: position f32x3 | normal i16x3 + pad | uv f32x2
| rgba8 per vertex, a uint16 index) and encoded again from there, by two routes taken in turn within every repetition:
  (a) torch kernels de-interleave every array, widen the index and convert the normals into packed tensors (mesh by mesh: the buffers are
      per blob), then crthip_encode_batch_to_device on the packed tensors - the route open before crthip_mesh_layout;
  (b) crthip_encode_batch_layout on the buffers as they are.
Every repetition is recorded; the figures reported are medians.  Wall times are host clocks around calls that end with the device drained;
kernel times are the library's own events (crthip_kernel_times), taken in every repetition.  Whether
(b)'s arena equals (a)'s byte for byte is part of the record.  Needs a device: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402

KERNELS = ("enc_input_check", "enc_input_reduce", "enc_quantize_batch", "enc_topo_compact")


def pack(views, divisor):
    """route (a)'s first half: packed float / int32 tensors of every mesh's arrays"""
    out = []
    for v in views:
        out.append(ca.DeviceMesh(v.position.contiguous(), v.index.to(torch.int32) & 0xFFFF, v.normal.to(torch.float32) / divisor,
                                 v.color.contiguous(), v.uv.contiguous()))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--units", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encode_layout_rate: no device")
    meshes = [synth.bumpy_sphere(64, 32, seed=s) for s in range(a.units)]
    kw = dict(normal_prediction=ca.BORDER)
    blobs = [ca.aligned_blob(ca.encode(m, **kw)) for m in meshes]
    ctx = ca.Context(0)
    b = ca.Batch(ctx, blobs)
    b.allocate_interleaved(ca.FMT_INT16, index16=True)
    b.decode(); b.sync()
    views, layouts = zip(*b.interleaved_meshes())
    divisor = torch.full((), 32767.0, dtype=torch.float32, device="cuda:0")      # (a tensor: an elementwise IEEE division, as upstream's)
    bound = ca.encode_batch_bound(pack(views, divisor), kw=kw)
    out_a = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
    out_b = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
    recs = []
    for mode in ("host", "device", "split"):
        ctx.set_encode_topology(mode)
        for _ in range(2):                                                       # warm both routes
            ca.encode_batch_to_device(pack(views, divisor), ctx, kw=kw, resident=True, out=out_a)
            ca.encode_batch_layout(views, ctx, layouts, kw=kw, device_out=True, out=out_b)
        reps = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            packed = pack(views, divisor)
            t1 = time.perf_counter()
            _, offs_a, lens_a, st_a = ca.encode_batch_to_device(packed, ctx, kw=kw, resident=True, out=out_a, with_stats=True)
            t2 = time.perf_counter()
            _, offs_b, lens_b, st_b = ca.encode_batch_layout(views, ctx, layouts, kw=kw, device_out=True, out=out_b, with_stats=True)
            t3 = time.perf_counter()
            del packed
            reps.append(dict(a_pack_ms=(t1 - t0) * 1e3, a_encode_ms=(t2 - t1) * 1e3, a_ms=(t2 - t0) * 1e3, b_ms=(t3 - t2) * 1e3,
                             a_kernels={k: st_a["kernel_times"].get(k, {}).get("ms", 0.0) for k in KERNELS},
                             b_kernels={k: st_b["kernel_times"].get(k, {}).get("ms", 0.0) for k in KERNELS},
                             a_from_device=st_a["bytes_from_device"], b_from_device=st_b["bytes_from_device"]))
        total = int(st_b["total"])
        same = lens_a.tolist() == lens_b.tolist() and bool(torch.equal(out_a[:total], out_b[:total]))
        med = lambda f: round(statistics.median(f(r) for r in reps), 4)
        rec = dict(workload="%d x C4 unit, interleaved i16 / u16" % a.units, mode=mode, reps=a.reps, arena_bytes=total, identical=same,
                   a_pack_ms=med(lambda r: r["a_pack_ms"]), a_encode_ms=med(lambda r: r["a_encode_ms"]), a_ms=med(lambda r: r["a_ms"]),
                   b_ms=med(lambda r: r["b_ms"]),
                   a_ms_min_max=[round(min(r["a_ms"] for r in reps), 3), round(max(r["a_ms"] for r in reps), 3)],
                   b_ms_min_max=[round(min(r["b_ms"] for r in reps), 3), round(max(r["b_ms"] for r in reps), 3)],
                   a_kernel_ms={k: med(lambda r, k=k: r["a_kernels"][k]) for k in KERNELS},
                   b_kernel_ms={k: med(lambda r, k=k: r["b_kernels"][k]) for k in KERNELS},
                   a_bytes_from_device=reps[-1]["a_from_device"], b_bytes_from_device=reps[-1]["b_from_device"],
                   input_bytes=dict(interleaved=int(sum(v.position.shape[0] * 32 + v.index.numel() * 2 for v in views)),
                                    packed=int(sum(v.position.shape[0] * (12 + 12 + 8 + 4) + v.index.numel() * 4 for v in views))),
                   every_rep=[{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items() if not isinstance(v, dict)} for r in reps])
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    b.close(); ctx.close()


if __name__ == "__main__":
    main()
