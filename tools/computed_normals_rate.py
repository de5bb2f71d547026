"""Computed normals against stored BORDER normals (crthip_batch_bind_computed_normals): what the normals kernel and the whole decode cost
when 256 C4 units (bumpy_sphere(64, 32, seed): 2 112 vertices / 4 096 triangles, positions 14 bits + uv 12 + rgba) are encoded WITHOUT
normals and decoded with computed ones, and when the same meshes are encoded with BORDER normals (10 bits) and decoded as ever.

    python tools/computed_normals_rate.py [--reps 15] [--out DIR]

On a two-stream context and on a single-stream one (the LDS-lean layout of the normals kernel).  The two batches are decoded in turn, A B A B,
in one process: REPS decodes each with the context's profiling off - the wall time of decode + sync - then REPS with it on - the normals
kernel's device time from crthip_batch_kernel_times (normal_blob_computed / normal_blob).  Median, minimum and maximum of each; one JSON line
per context on stdout and in DIR/computed_normals.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402

NBLOBS = 256


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2), runs=len(v))


def blobs():
    bare, border = [], []
    for i in range(NBLOBS):
        m = synth.bumpy_sphere(64, 32, seed=i)
        bare.append(ca.encode(m, position_bits=14, uv_bits=12, with_normal=False))
        border.append(ca.encode(m, position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER))
    return bare, border


def measure(single, bare, border, reps):
    ctx = ca.Context(0)
    if single:
        ctx.set_single_stream(True)
    forms = {"computed": (ca.Batch(ctx, bare), "normal_blob_computed"), "border": (ca.Batch(ctx, border), "normal_blob")}
    forms["computed"][0].allocate_outputs(computed_normals=True)
    forms["border"][0].allocate_outputs()

    def step(b):
        t = time.perf_counter()
        b.decode()
        st = b.sync()
        dt = (time.perf_counter() - t) * 1e6
        assert (st == 0).all(), st
        return dt

    for _ in range(5):
        for b, _k in forms.values():
            step(b)
    wall = {k: [] for k in forms}
    for _ in range(reps):
        for k, (b, _k) in forms.items():
            wall[k].append(step(b))
    ctx.set_profiling(True)
    kern, all_kernels = {k: [] for k in forms}, {}
    for _ in range(3):
        for b, _k in forms.values():
            step(b)
    for _ in range(reps):
        for k, (b, name) in forms.items():
            step(b)
            kt = b.kernel_times()
            assert kt[name]["launches"] == 1, (k, kt)
            kern[k].append(kt[name]["ms"] * 1000.0)
            all_kernels[k] = sorted(kt)
    ctx.set_profiling(False)
    # the two forms decode the same meshes
    for i in (0, NBLOBS // 2, NBLOBS - 1):
        a, c = forms["computed"][0].host_outputs(i), forms["border"][0].host_outputs(i)
        for key in ("position", "index", "uv", "color"):
            assert a[key].tobytes() == c[key].tobytes(), (i, key)
        assert a["normal"].shape == c["normal"].shape and np.isfinite(a["normal"]).all()
    out = dict(context="single_stream" if single else "two_stream", blobs=NBLOBS, triangles=NBLOBS * 4096,
               blob_bytes=dict(computed=int(sum(len(b) for b in bare)), border=int(sum(len(b) for b in border))))
    for k in forms:
        out[k] = dict(normals_kernel=forms[k][1], normals_kernel_us=stats(kern[k]), decode_wall_us=stats(wall[k]), kernels=all_kernels[k])
    for b, _k in forms.values():
        b.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit("at least 9 runs a form")
    bare, border = blobs()
    rows = []
    for single in (False, True):
        r = measure(single, bare, border, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "computed_normals.jsonl"), "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
