"""A context's second HIP stream is made by the first decode that forks onto it (csrc/batch.cpp ctx_stream2), not when the context is
made: a single-stream context decodes and is destroyed with one stream, one switched back to two streams makes the second on its next
forking decode, and the pool's 5 x 4 single-stream lanes decode bench.py's C4 batch.  GPU cases are bit-exact against the oracle and
the goldens; the CPU case checks tools/queue_spread.py on a hand-made trace."""
import csv
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import corto_amd as ca
from conftest import GOLDEN, MESH_CASES, ROOT, aligned, load_golden
from oracle import oracle as oc

KEYS = ("position", "normal", "color", "uv", "radius", "index")


def decode(ctx, blobs):
    b = ca.Batch(ctx, blobs)
    try:
        b.allocate_outputs(fill=0)
        b.decode()
        st = b.sync()
        assert (st == 0).all(), st
        return [b.host_outputs(i) for i in range(len(blobs))]
    finally:
        b.close()


def assert_same(outs, refs, tag):
    for i, (o, r) in enumerate(zip(outs, refs)):
        for k in KEYS:
            if k not in r:
                continue
            assert k in o, (tag, i, k)
            assert o[k].dtype == r[k].dtype and o[k].shape == r[k].shape, (tag, i, k)
            assert o[k].tobytes() == r[k].tobytes(), (tag, i, k)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_single_stream_context_decodes_goldens_and_is_destroyed():
    """switched to one stream before its first decode, the context never makes its second stream; destroying it must not wait on or
    destroy a stream it does not have"""
    gs = [load_golden(n) for n in MESH_CASES]
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        assert_same(decode(c, [g["crt"] for g in gs]), gs, "golden batch")
        for n, g in zip(MESH_CASES, gs):
            assert_same(decode(c, [g["crt"]]), [g], n)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_single_stream_context_switched_back_forks():
    """a context that has decoded on one stream is switched back to two: its next forking decode makes the second stream - the
    attribute-stream fork of a batch of C4 blobs with a wide-alphabet mesh, and a C2-class mesh whose delta tiles run beside its automaton"""
    from corto_amd import synth
    z = np.load(os.path.join(GOLDEN, "c4_blobs16.npz"))
    c4 = [aligned(z["crt_%02d" % s]) for s in range(16)]
    wide = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32, seed=5, noise=0.2), position_bits=20, uv_bits=16, normal_bits=12,
                                     normal_prediction=ca.BORDER))
    c2 = ca.aligned_blob(ca.encode(synth.bumpy_sphere(512, 250, seed=1), normal_prediction=ca.BORDER))
    g = load_golden("c4_unit")
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        assert_same(decode(c, [g["crt"]]), [g], "single")
        c.set_single_stream(False)
        for tag, blobs in (("fork", c4 + [wide]), ("c2", [c2]), ("fork again", c4)):
            assert_same(decode(c, blobs), [oc.decode(b) for b in blobs], tag)
        c.set_single_stream(True)                               # (the second stream, made now, stays unused until the context goes)
        assert_same(decode(c, [g["crt"]]), [g], "single again")
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_pool_of_five_by_four_lanes_runs_the_c4_batch():
    """bench.py's shape: 5 host threads x 4 batches in flight = 20 single-stream contexts on one GPU, the 256-blob C4 batch from a
    device arena; a sample of every lane's last outputs against the oracle, and seeds 0..15 against their goldens"""
    from corto_amd import synth
    blobs = [ca.encode(synth.bumpy_sphere(64, 32, seed=i), position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER)
             for i in range(256)]
    pool = ca.Pool([0], threads=5, depth=4)
    try:
        assert pool.lanes == 20
        rep, stamps = pool.run([blobs], steps=80, warmup=20, arenas=[[ca.upload_arena(blobs, 0)]])
        assert rep.steps == 80 and rep.failed_blobs == 0 and rep.first_error == 0 and len(stamps) == 80
        z = np.load(os.path.join(GOLDEN, "c4_blobs16.npz"))
        dts = {"position": (np.float32, 3), "normal": (np.float32, 3), "color": (np.uint8, 4), "uv": (np.float32, 2), "index": (np.uint32, 3)}
        for lane in range(pool.lanes):
            it, slot = pool.lane_item(lane)
            assert it == 0 and slot == 0
            for i in (lane, 255 - lane, 100 + 7 * lane):
                ref = oc.decode(blobs[i])
                for k, (dt, w) in dts.items():
                    got = pool.lane_read(lane, i, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                    assert got.tobytes() == ref[k].tobytes(), (lane, i, k)
        for s in range(16):                                      # seeds 0..15: their outputs' hashes came from the reference
            assert bytes(z["crt_%02d" % s]) == bytes(blobs[s]), s
            ref = oc.decode(blobs[s])
            for k, (dt, w) in dts.items():
                got = pool.lane_read(s, s, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                assert hashlib.sha256(got.tobytes()).hexdigest() == z["%s_sha256_%02d" % (k, s)].tobytes().decode(), (s, k)
    finally:
        pool.close()


def test_queue_spread_on_a_hand_made_trace(tmp_path):
    """tools/queue_spread.py: two queues, three streams; the first and last quarter of the kernels are left out of the window"""
    rows = []
    # 16 kernels, 100 ns apart, 50 ns long; stream 1 and 3 on queue 7, stream 2 on queue 9
    for i in range(16):
        st = (1, 2, 3, 2)[i % 4]
        rows.append({"Kind": "KERNEL_DISPATCH", "Agent_Id": "1", "Queue_Id": "7" if st != 2 else "9", "Stream_Id": str(st),
                     "Kernel_Name": "k_%d" % i, "Start_Timestamp": str(1000 + 100 * i), "End_Timestamp": str(1050 + 100 * i)})
    f = tmp_path / "x_kernel_trace.csv"
    with open(f, "w", newline="") as h:
        w = csv.DictWriter(h, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "queue_spread.py"), str(tmp_path)], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    # window: kernels 4..11 = 1400 .. 2150 ns
    assert out[0] == "window 0.00 ms, 8 kernels, 2 queues, 3 streams"
    assert out[1].startswith("queue 1 (id 7):     4 kernels (0.500 of the window's), busy 0.267, streams 2"), out[1]
    assert out[2].startswith("queue 2 (id 9):     4 kernels (0.500 of the window's), busy 0.267, streams 1"), out[2]
    assert out[3:] == ["stream 1: queue 1, 2 kernels", "stream 2: queue 2, 4 kernels", "stream 3: queue 1, 2 kernels"]
