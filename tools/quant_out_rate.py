"""Quantised vertex outputs (CRTHIP_BIND_QUANTIZED) against FLOAT ones: what profiles/quantized_outputs.md records.

    python tools/quant_out_rate.py [--steps 40] [--warmup 10] [--out FILE]

1. The C4 batch (256 blobs of 2 112 vertices / 4 096 triangles) on a lone context, render layouts (int16 normals, uint16 index), position + uv
   as FLOAT against position + uv quantised, the two taken in turn within every repetition:
     output bytes a step (crthip_batch_stats.output_bytes and the buffer allocated),
     kernel times of the finishers (Batch.kernel_times(), a profiled decode of their own),
     ms a step with the outputs left in HBM, and with ONE device-to-host copy of the output buffer into pinned memory behind the decode -
     each the median of --steps steps after --warmup.
2. One quantised job (a point cloud's position) of 1 024 ... 65 536 vertices through k_quant_out_blob and through
   k_quant_range + k_quant_store ($CORTO_QOUT_BLOB_MAX picks; a context reads it when it is made): the kernels' device times, median of --steps.
One JSON record a line.  Needs a device: there is nothing to fall back to."""
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

NBLOBS = 256


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def median_kernel_ms(b, steps, names):
    got = {n: [] for n in names}
    for _ in range(steps):
        b.decode()
        b.sync()
        kt = b.kernel_times()
        for n in names:
            if n in kt:
                got[n].append(kt[n]["ms"])
    return {n: round(statistics.median(v), 5) for n, v in got.items() if v}


def c4_batch(args, out):
    import torch
    blobs = [ca.encode(synth.bumpy_sphere(64, 32, seed=i), position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER) for i in range(NBLOBS)]
    ctx = ca.Context(0)
    legs = {}
    for name, quantized in (("float", ()), ("quantized", ("position", "uv"))):
        b = ca.Batch(ctx, blobs)
        b.allocate_outputs(normal_format=ca.FMT_INT16, index16=True, quantized=quantized)
        buf = b._keep[0]
        legs[name] = dict(batch=b, buf=buf, pinned=torch.empty(buf.numel(), dtype=torch.uint8).pin_memory(), hbm=[], d2h=[])
    for k in range(args.warmup + args.steps):
        for name, L in legs.items():                         # the two in turn
            b = L["batch"]
            t0 = time.perf_counter(); b.decode(); b.sync(); t1 = time.perf_counter()
            b.decode(); b.sync(); L["pinned"].copy_(L["buf"], non_blocking=True); torch.cuda.synchronize(); t2 = time.perf_counter()
            if k >= args.warmup:
                L["hbm"].append((t1 - t0) * 1e3); L["d2h"].append((t2 - t1) * 1e3)
    ctx.set_profiling(True)
    for name, L in legs.items():
        b = L["batch"]
        kt = median_kernel_ms(b, 10, ["delta_lds16", "normal_blob", "dequantize", "quant_out_blob", "quant_range", "quant_store"])
        emit(dict(leg="c4_batch", outputs=name, blobs=NBLOBS, output_bytes=int(b.stats().output_bytes), buffer_bytes=int(L["buf"].numel()),
                  ms_step_hbm_median=round(statistics.median(L["hbm"]), 4), ms_step_hbm_min=round(min(L["hbm"]), 4),
                  ms_step_d2h_median=round(statistics.median(L["d2h"]), 4), ms_step_d2h_min=round(min(L["d2h"]), 4),
                  steps=args.steps, warmup=args.warmup, kernel_ms_median=kt), out)
        b.close()
    ctx.close()
    # the same 512 quantised jobs through the two-kernel path
    os.environ["CORTO_QOUT_BLOB_MAX"] = "1"
    ctx = ca.Context(0)
    ctx.set_profiling(True)
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(normal_format=ca.FMT_INT16, index16=True, quantized=("position", "uv"))
    for _ in range(args.warmup):
        b.decode(); b.sync()
    emit(dict(leg="c4_batch", outputs="quantized, every job through quant_range + quant_store", blobs=NBLOBS,
              kernel_ms_median=median_kernel_ms(b, 10, ["quant_out_blob", "quant_range", "quant_store"])), out)
    b.close(); ctx.close()
    os.environ.pop("CORTO_QOUT_BLOB_MAX", None)


def size_class(args, out):
    for nv in (1024, 2048, 3072, 4096, 16384, 65536):
        j = np.arange(nv, dtype=np.float64)
        pos = np.stack([np.cos(0.01 * j), np.sin(0.017 * j), 0.001 * j], 1).astype(np.float32)
        blob = ca.encode(synth.Mesh(pos), with_normal=False, with_color=False, with_uv=False)
        rec = dict(leg="size_class", nvert=nv)
        for path, limit in (("blob", 1 << 30), ("range_store", 1)):
            os.environ["CORTO_QOUT_BLOB_MAX"] = str(limit)
            ctx = ca.Context(0)
            ctx.set_profiling(True)
            b = ca.Batch(ctx, [blob])
            b.allocate_outputs(quantized=("position",))
            for _ in range(args.warmup):
                b.decode(); b.sync()
            kt = median_kernel_ms(b, args.steps, ["quant_out_blob", "quant_range", "quant_store"])
            assert (set(kt) == {"quant_out_blob"}) == (path == "blob"), (path, kt)
            rec[path + "_ms"] = round(sum(kt.values()), 5)
            rec[path + "_kernels"] = kt
            b.close(); ctx.close()
        os.environ.pop("CORTO_QOUT_BLOB_MAX", None)
        emit(rec, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    if ca.lib().crthip_device_count() < 1:
        sys.exit("quant_out_rate: no HIP device")
    c4_batch(args, args.out)
    size_class(args, args.out)


if __name__ == "__main__":
    main()
