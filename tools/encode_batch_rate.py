"""crthip_encode_batch against the host encoder: one JSON record per workload.

    python tools/encode_batch_rate.py [--out FILE] [--reps 3]

    python tools/encode_batch_rate.py --topology [--out FILE] [--reps 3]

--topology: the mesh workloads alone, over where the CLERS topology pass runs (Context.set_encode_topology: host, device, split - host alone
where the library has no such switch) and host_threads (1, 4, 16); one record per combination with every repetition's time, the best one's
stats and kernel times, and whether the blobs equal the host mode's.

    python tools/encode_batch_rate.py --resident [--out FILE] [--reps 3]

--resident: what a producer whose meshes are in device memory pays, over the five workloads and under host and device topology, the legs
taken in turn within every repetition and every repetition recorded: (a) crthip_encode_batch from host arrays; (b)
crthip_encode_batch_resident on the same arrays in one device buffer; (c) what such a producer had to do before - one device-to-host
copy of all inputs, then (a), or then crthip_encode on 16 host threads.  With the device time of the input pass's kernels, both calls'
stats, and whether (b)'s blobs equal (a)'s.  Needs a device: there is nothing to fall back to.

    python tools/encode_batch_rate.py --device-out [--out FILE] [--reps 3]

--device-out: two routes from meshes in device memory to a decodable resident batch, over the five workloads and the three topology modes,
taken in turn within every repetition and every repetition recorded: (a) crthip_encode_batch_resident (blobs to the host), upload_arena,
Batch.resident - what such a producer had to do before; (b) crthip_encode_batch_to_device, Batch.resident.  With each route's parts, the
device time of enc_splice, the splice statistics, both calls' stats, and whether (b)'s arena holds (a)'s blobs.  Needs a device.

For each workload: the batch call's wall time, its stats and per-kernel times (of the same run), beside crthip_encode on one
host thread and on 16 (ctypes releases the GIL), crthip_encode_gpu mesh by mesh, and the reference encoder on one core when
oracle/_ref is present; every leg is the best of --reps runs.  Every batch blob is checked against crthip_encode's bytes."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402


def workloads():
    yield "256 x C4 unit", [synth.bumpy_sphere(64, 32, seed=s) for s in range(256)], dict(normal_prediction=ca.BORDER)
    yield "64 x 16K-triangle", [synth.bumpy_sphere(128, 64, seed=s) for s in range(64)], dict(normal_prediction=ca.BORDER)
    yield "16 x C2", [synth.bumpy_sphere(512, 250, seed=s) for s in range(16)], dict(normal_prediction=ca.BORDER)
    yield "C3 cloud", [synth.point_cloud()], dict(normal_prediction=ca.BORDER)
    yield "4M-point cloud", [synth.point_cloud(2048, 2048, seed=5)], dict(normal_prediction=ca.BORDER)


def best(f, reps):
    """the fastest of `reps` runs, and that run's result (its stats and kernel times belong to the time reported)"""
    bt, br = None, None
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); t = (time.perf_counter() - t0) * 1e3
        if bt is None or t < bt:
            bt, br = t, r
    return bt, br


def topology_axis(reps):
    modes = ["host"] + (["device", "split"] if hasattr(ca.Context, "set_encode_topology") else [])
    recs = []
    for name, meshes, kw in workloads():
        if meshes[0].nface == 0:
            continue
        want = None
        for mode in modes:
            ctx = ca.Context(0)
            ctx.set_profiling(True)
            if mode != "host":
                ctx.set_encode_topology(mode)
            ca.encode_batch(meshes[:2], ctx, kw=kw)                               # warm the context and the kernels
            for threads in (1, 4, 16):
                times, bt, br = [], None, None
                for _ in range(reps):
                    t0 = time.perf_counter(); r = ca.encode_batch(meshes, ctx, kw=kw, host_threads=threads, with_stats=True); t = (time.perf_counter() - t0) * 1e3
                    times.append(round(t, 3))
                    if bt is None or t < bt:
                        bt, br = t, r
                blobs, st = br
                if want is None:
                    want = [b.tobytes() for b in blobs]
                rec = dict(workload=name, mode=mode, host_threads=threads, batch_ms=round(bt, 3), reps_ms=times, wall_ms=round(st["wall_ms"], 3),
                           identical_to_host_mode=[b.tobytes() for b in blobs] == want,
                           stats={k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k != "kernel_times"},
                           kernel_times={k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in st["kernel_times"].items() if k.startswith("enc_topo")})
                print(json.dumps(rec), flush=True)
                recs.append(rec)
            ctx.close()
    return recs


def place_on_device(meshes):
    """Every data array of the meshes in ONE device byte tensor (16-byte aligned starts): (buffer, device meshes, rebuild), where
    rebuild(host_bytes) gives the meshes again as views of a host copy of the buffer."""
    import numpy as np
    import torch
    names = ("position", "index", "normal", "color", "uv", "radius")
    plan, pos = [], 0
    for m in meshes:
        d = {}
        for a in names:
            v = getattr(m, a)
            if v is not None:
                d[a] = (pos, v.dtype, v.shape, v.nbytes)
                pos += (v.nbytes + 15) // 16 * 16
        plan.append(d)
    host = np.zeros(pos + 16, dtype=np.uint8)
    for m, d in zip(meshes, plan):
        for a, (at, _, _, nb) in d.items():
            host[at:at + nb] = getattr(m, a).view(np.uint8).reshape(-1)
    buf = torch.from_numpy(host).to("cuda:0")
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint32): torch.int32, np.dtype(np.uint8): torch.uint8}
    dev = [ca.DeviceMesh(**{a: buf[at:at + nb].view(tdt[np.dtype(dt)]).reshape(shape) for a, (at, dt, shape, nb) in d.items()}, groups=m.groups,
                         group_props=getattr(m, "group_props", None)) for m, d in zip(meshes, plan)]
    torch.cuda.synchronize()

    def rebuild(h):
        out = []
        for m, d in zip(meshes, plan):
            r = synth.Mesh(**{a: h[at:at + nb].view(dt).reshape(shape) for a, (at, dt, shape, nb) in d.items()}, groups=m.groups)
            r.group_props = getattr(m, "group_props", None)
            out.append(r)
        return out
    return buf, dev, rebuild


def resident_axis(reps):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("encode_batch_rate.py --resident: no device (the resident encoder has no CPU fallback)")
    recs = []
    clock = time.perf_counter

    def timed(f):
        t0 = clock(); r = f(); return (clock() - t0) * 1e3, r

    for name, meshes, kw in workloads():
        buf, dev, rebuild = place_on_device(meshes)
        input_bytes = int(buf.numel())
        for mode in ("host", "device"):
            ctx = ca.Context(0)
            ctx.set_profiling(True)
            ctx.set_encode_topology(mode)
            ca.encode_batch(meshes[:1], ctx, kw=kw); ca.encode_batch_resident(dev[:1], ctx, kw=kw)      # warm the context and the kernels
            legs = {k: [] for k in ("a_host_arrays", "b_resident", "c_copy_then_batch", "c_copy_then_16_threads", "c_copy_alone")}
            best_a = best_b = None
            identical = True
            with ThreadPoolExecutor(16) as ex:
                for _ in range(reps):
                    t, (blobs_a, st_a) = timed(lambda: ca.encode_batch(meshes, ctx, kw=kw, with_stats=True))
                    legs["a_host_arrays"].append(round(t, 3))
                    if best_a is None or t < best_a[0]:
                        best_a = (t, st_a)
                    t, (blobs_b, st_b) = timed(lambda: ca.encode_batch_resident(dev, ctx, kw=kw, with_stats=True))
                    legs["b_resident"].append(round(t, 3))
                    if best_b is None or t < best_b[0]:
                        best_b = (t, st_b)
                    identical = identical and [b.tobytes() for b in blobs_a] == [b.tobytes() for b in blobs_b]
                    t0 = clock(); back = rebuild(buf.cpu().numpy()); t_copy = (clock() - t0) * 1e3
                    t, _ = timed(lambda: ca.encode_batch(back, ctx, kw=kw))
                    legs["c_copy_then_batch"].append(round(t_copy + t, 3)); legs["c_copy_alone"].append(round(t_copy, 3))
                    t0 = clock(); back = rebuild(buf.cpu().numpy()); t_copy = (clock() - t0) * 1e3
                    t, _ = timed(lambda: list(ex.map(lambda m: ca.encode(m, **kw), back)))
                    legs["c_copy_then_16_threads"].append(round(t_copy + t, 3))
            pick = lambda st: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k != "kernel_times"}
            rec = dict(workload=name, mode=mode, items=len(meshes), input_bytes=input_bytes, reps_ms=legs, best_ms={k: min(v) for k, v in legs.items()},
                       resident_identical_to_host_arrays=identical, stats_host_arrays=pick(best_a[1]), stats_resident=pick(best_b[1]),
                       input_kernels={k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in best_b[1]["kernel_times"].items() if k.startswith("enc_input")})
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            ctx.close()
        del buf, dev
    return recs


def device_out_axis(reps):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("encode_batch_rate.py --device-out: no device (the device encoder has no CPU fallback)")
    recs = []
    clock = time.perf_counter
    for name, meshes, kw in workloads():
        buf, dev, _ = place_on_device(meshes)
        out = torch.empty(max(ca.encode_batch_bound(dev, kw=kw), 16), dtype=torch.uint8, device="cuda:0")   # allocated once: a producer reuses its arena
        for mode in ("host", "device", "split"):
            ctx = ca.Context(0)
            ctx.set_profiling(True)
            ctx.set_encode_topology(mode)
            ca.encode_batch_resident(dev[:1], ctx, kw=kw); ca.encode_batch_to_device(dev[:1], ctx, kw=kw, out=out)      # warm the context and the kernels
            legs = {k: [] for k in ("a_total", "a_encode_resident", "a_upload_arena", "a_batch_resident", "b_total", "b_encode_to_device", "b_batch_resident")}
            best_a = best_b = None
            identical = True
            for _ in range(reps):
                t0 = clock()
                blobs, st_a = ca.encode_batch_resident(dev, ctx, kw=kw, with_stats=True)
                t1 = clock()
                arena = ca.upload_arena(blobs)
                t2 = clock()
                offs_a, _ = ca.arena_layout([len(b) for b in blobs])
                ba = ca.Batch.resident(ctx, arena, offs_a, [len(b) for b in blobs])
                t3 = clock()
                ba.close()
                for k, v in (("a_total", t3 - t0), ("a_encode_resident", t1 - t0), ("a_upload_arena", t2 - t1), ("a_batch_resident", t3 - t2)):
                    legs[k].append(round(v * 1e3, 3))
                if best_a is None or t3 - t0 < best_a[0]:
                    best_a = (t3 - t0, st_a)
                t0 = clock()
                o, offs, lens, st_b = ca.encode_batch_to_device(dev, ctx, kw=kw, out=out, with_stats=True)
                t1 = clock()
                bb = ca.Batch.resident(ctx, o, offs, lens)
                t2 = clock()
                bb.close()
                for k, v in (("b_total", t2 - t0), ("b_encode_to_device", t1 - t0), ("b_batch_resident", t2 - t1)):
                    legs[k].append(round(v * 1e3, 3))
                if best_b is None or t2 - t0 < best_b[0]:
                    best_b = (t2 - t0, st_b)
                identical = identical and offs.tolist() == offs_a.tolist() and bool(torch.equal(o[:st_b["total"]], arena[:st_b["total"]]))
            pick = lambda st: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k not in ("kernel_times", "splice")}
            sb = best_b[1]
            rec = dict(workload=name, mode=mode, items=len(meshes), arena_bytes=sb["total"], reps_ms=legs, best_ms={k: min(v) for k, v in legs.items()},
                       a_spread_ms=round(max(legs["a_total"]) - min(legs["a_total"]), 3), b_minus_a_ms=round(min(legs["b_total"]) - min(legs["a_total"]), 3),
                       arena_identical_to_route_a=identical, enc_splice=sb["kernel_times"].get("enc_splice"),
                       splice={k: (round(v, 3) if isinstance(v, float) else v) for k, v in sb["splice"].items()},
                       stats_resident=pick(best_a[1]), stats_to_device=pick(sb))
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            ctx.close()
        del buf, dev, out
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--topology", action="store_true", help="the topology mode x host_threads table of the mesh workloads")
    ap.add_argument("--resident", action="store_true", help="host arrays against arrays in device memory against copying those back first")
    ap.add_argument("--device-out", action="store_true", help="blobs to the host and back up against blobs spliced on the device, up to a resident batch")
    a = ap.parse_args()
    if a.topology or a.resident or a.device_out:
        recs = device_out_axis(a.reps) if a.device_out else resident_axis(a.reps) if a.resident else topology_axis(a.reps)
        if a.out:
            with open(a.out, "w") as f:
                for r in recs:
                    f.write(json.dumps(r) + "\n")
        return
    from oracle import refcodec as rc
    ctx = ca.Context(0)
    ctx.set_profiling(True)
    ca.encode_batch([synth.bumpy_sphere(16, 8)], ctx)                       # warm the context and the kernels
    recs = []
    for name, meshes, kw in workloads():
        ms, (blobs, st) = best(lambda: ca.encode_batch(meshes, ctx, kw=kw, with_stats=True), a.reps)
        host1, ref = best(lambda: [ca.encode(m, **kw) for m in meshes], a.reps)
        identical = all(b.tobytes() == r.tobytes() for b, r in zip(blobs, ref))
        with ThreadPoolExecutor(16) as ex:
            host16, _ = best(lambda: list(ex.map(lambda m: ca.encode(m, **kw), meshes)), a.reps)
        gpu1, _ = best(lambda: [ca.encode(m, ctx=ctx, **kw) for m in meshes], a.reps)
        rec = dict(workload=name, items=len(meshes), triangles=int(sum(m.nface for m in meshes)), vertices=int(sum(m.nvert for m in meshes)),
                   batch_ms=round(ms, 3), host_1thread_ms=round(host1, 3), host_16threads_ms=round(host16, 3), encode_gpu_per_mesh_ms=round(gpu1, 3),
                   identical=identical, stats={k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k != "kernel_times"},
                   kernel_times={k: dict(ms=round(v["ms"], 4), launches=v["launches"]) for k, v in st["kernel_times"].items()})
        if rc.available():
            rec["reference_1core_ms"] = round(best(lambda: [rc.encode(m, **kw) for m in meshes], a.reps)[0], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
