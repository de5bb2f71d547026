"""crthip_pool_decode: the pool decodes every item exactly once into a block the caller owns.  Everything here is raw-byte equality with the
oracle (tolerance 0), on items that DIFFER in size and content - with equal items a mix-up of two blocks would be invisible.  Blocks are
pre-filled with 0xA5: a device block keeps that byte everywhere outside its arrays, any block from the layout's total on."""
import gc
import threading

import numpy as np
import pytest
import torch

import corto_amd as ca
from conftest import aligned
from corto_amd import synth
from oracle import oracle as oc

pytestmark = pytest.mark.gpu

E_MAGIC, E_ARGUMENT = -2, -8
FILL, SPARE = 0xA5, 512


def enc(mesh, **kw):
    kw.setdefault("normal_prediction", ca.BORDER)
    return ca.aligned_blob(ca.encode(mesh, **kw))


def c4_item(n, seed0):
    return [enc(synth.bumpy_sphere(64, 32, seed=seed0 + i), position_bits=14, uv_bits=12, normal_bits=10) for i in range(n)]


def flipped_item(n, seed0):
    return [enc(synth.bumpy_sphere_flipped(40, 20, seed=seed0 + i), position_bits=14, uv_bits=12, normal_bits=10) for i in range(n)]


def small_item(n, seed0):
    return [enc(synth.bumpy_sphere(40, 20, seed=seed0 + i), position_bits=13, uv_bits=11, normal_bits=9) for i in range(n)]


def tiny_item(n, seed0):
    return [enc(synth.bumpy_sphere(24, 12, seed=seed0 + i), position_bits=12, uv_bits=10, normal_bits=9) for i in range(n)]


def cloud_item(seed):
    return [enc(synth.point_cloud(90, 45, seed=seed), normal_prediction=ca.DIFF)]


_refs = {}


def ref_of(blob, render=False):
    k = (blob.tobytes(), render)
    if k not in _refs:
        if render:
            _refs[k] = oc.decode(blob, normal_format=oc.FMT_INT16, index16=ca.probe(blob).nvert < 65536)
        else:
            _refs[k] = oc.decode(blob)
    return _refs[k]


@pytest.fixture(scope="module")
def items():
    """eleven items: three kinds of 64-80-blob items (sixty-four blobs is the smallest item a lane carries), a 34K-vertex mesh, three point
    clouds, a five-blob item, an empty one, two more carried items"""
    return [c4_item(64, 100), flipped_item(72, 200), small_item(80, 300),
            [enc(synth.bumpy_sphere(264, 130, seed=3))],
            cloud_item(2), cloud_item(5), cloud_item(9),
            c4_item(5, 600), [],
            tiny_item(64, 700), tiny_item(70, 800)]


def make_blocks(pool, item_list, kinds, slots=None, render=False):
    """one block per item: the layout's bytes + SPARE, every byte 0xA5"""
    blocks = []
    for j, blobs in enumerate(item_list):
        n = ca.output_layout(blobs, render)[1] + SPARE
        if kinds[j] == "device":
            slot = slots[j] if slots is not None else j % len(pool.devices)
            blocks.append(torch.full((n,), FILL, dtype=torch.uint8, device=torch.device("cuda", pool.devices[slot])))
        elif kinds[j] == "host":
            t = torch.empty(n, dtype=torch.uint8).pin_memory()
            t.fill_(FILL)
            blocks.append(t)
        else:
            raw = np.full(n + 256, FILL, dtype=np.uint8)
            blocks.append(raw[(-raw.ctypes.data) % 256:][:n])
    return blocks


def own_allocation(n):
    """a device tensor of n bytes, every byte 0xA5, that is an allocation of its own to the runtime.  torch's cache serves a request from the
    smallest free block that holds it, and a segment that a live tensor shares - a block that the pool keeps from its last call, say - can have
    one: such a tensor lies in an allocation larger than itself.  Each one found so is held, so that it fills its hole, until the request
    reaches the runtime"""
    plugs = []
    for _ in range(16):
        t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0")
        if any(s["address"] == t.data_ptr() and s["total_size"] == n for s in torch.cuda.memory_snapshot()):
            return t
        plugs.append(t)
    raise AssertionError("no allocation of exactly %d bytes after %d tries" % (n, len(plugs)))


def block_bytes(block):
    if isinstance(block, np.ndarray):
        return block
    return block.cpu().numpy()


def check_item(r, blobs, tag, render=False, strict_gaps=True, only=None):
    """every array of every blob (of the blobs `only`) is the oracle's; outside the arrays the block is still 0xA5 - everywhere for a device
    block, from the layout's total on for a host block.  Returns the arrays' bytes."""
    lay, total = ca.output_layout(blobs, render)
    assert r.total == total and len(r.outputs) == len(blobs), tag
    raw = block_bytes(r.block)
    covered = np.zeros(len(raw), dtype=bool)
    got = {}
    for i, blob in enumerate(blobs):
        for name, (o, dt, shape) in lay[i].items():
            covered[o:o + int(np.prod(shape)) * dt.itemsize] = True
        if only is not None and i not in only:
            continue
        ref = ref_of(blob, render)
        assert set(lay[i]) == {k for k in ("position", "normal", "color", "uv", "radius", "index") if k in ref}, (tag, i)
        for name, (o, dt, shape) in lay[i].items():
            nbytes = int(np.prod(shape)) * dt.itemsize
            assert ref[name].dtype == dt and ref[name].shape == shape, (tag, i, name, ref[name].dtype, dt)
            view = r.outputs[i][name]
            host = view.cpu().numpy().view(dt) if isinstance(view, torch.Tensor) else view
            assert host.dtype == dt and host.shape == shape, (tag, i, name)
            assert host.tobytes() == raw[o:o + nbytes].tobytes(), (tag, i, name, "the view is not the block's bytes")
            assert host.tobytes() == ref[name].tobytes(), (tag, i, name)
            got[(i, name)] = host.tobytes()
    assert covered[total:].sum() == 0
    if strict_gaps:
        assert (raw[~covered] == FILL).all(), (tag, "bytes outside the arrays were written", np.flatnonzero(raw[~covered] != FILL)[:8])
    else:
        assert (raw[total:] == FILL).all(), (tag, "bytes behind the layout's total were written")
    return got


def decode_round(pool, item_list, kind, tag, render=False, slots=None, arenas=None):
    kinds = [kind] * len(item_list) if isinstance(kind, str) else list(kind)
    blocks = make_blocks(pool, item_list, kinds, slots, render)
    calls, lock = [], threading.Lock()

    def on_done(item, slot, status):
        with lock:
            calls.append((item, slot, status.copy()))
    res, rep = pool.decode(item_list, dest=kinds, slots=slots, arenas=arenas, on_done=on_done, blocks=blocks)
    assert len(res) == len(item_list)
    assert sorted(c[0] for c in calls) == list(range(len(item_list))), (tag, sorted(c[0] for c in calls))    # each item exactly once
    for item, slot, status in calls:
        assert (status == res[item].status).all() and len(status) == len(item_list[item]), (tag, item)
    assert rep.steps == len(item_list) and rep.poisoned_lanes == 0, tag
    assert sum(rep.steps_per_device) == len(item_list), tag
    assert rep.triangles == sum(ca.probe(b).nface for it in item_list for b in it), tag
    assert rep.elapsed_s > 0
    return res, rep, calls, kinds


def test_device_destinations_every_item_once(items, monkeypatch):
    """eleven items (more than 2 x lanes, no multiple of lanes) on four single-stream, pipelined lanes, into device blocks: the oracle's bytes,
    nothing written outside the arrays (gaps and spare included), every status 0, every item reported once - with the carry on and with
    $CORTO_CARRY=0, bit-identical"""
    assert len(items) == 11 and len({len(it) for it in items}) > 5
    seen = {}
    for carry in ("1", "0"):
        monkeypatch.setenv("CORTO_CARRY", carry)
        pool = ca.Pool([0], threads=2, depth=2)
        try:
            assert pool.lanes == 4
            res, rep, calls, _ = decode_round(pool, items, "device", "carry=" + carry)
            assert rep.failed_blobs == 0 and rep.first_error == 0
            assert all(slot == 0 for _, slot, _ in calls)
            for j, r in enumerate(res):
                assert r.block.is_cuda and (r.status == 0).all() and len(r.status) == len(items[j]), (carry, j)
                for key, val in check_item(r, items[j], (carry, j)).items():
                    assert seen.setdefault((j,) + key, val) == val, (carry, j, key)
            with pytest.raises(ca.CortoError):
                pool.lane_read(0, 0, "position", np.float32, 3)
            assert pool.lane_item(0)[0] == -1
        finally:
            pool.close()


@pytest.mark.parametrize("kind", ["host", "pageable"])
def test_host_destinations(items, kind):
    """the same items into pinned blocks (the D2H copy lands in them) and into pageable ones (through the lane's pinned mirror)"""
    pool = ca.Pool([0], threads=2, depth=2)
    try:
        res, rep, calls, _ = decode_round(pool, items, kind, kind)
        assert rep.failed_blobs == 0
        for j, r in enumerate(res):
            assert isinstance(r.block, np.ndarray) == (kind == "pageable") and (r.status == 0).all()
            if kind == "host":
                assert r.block.is_pinned()
            check_item(r, items[j], (kind, j), strict_gaps=False)
    finally:
        pool.close()


def test_render_layouts(items):
    """int16 normals and a 16-bit index (the 34K-vertex mesh among the items), device and host blocks; the dtypes are output_layout's"""
    sub = [items[3], items[0], items[4], items[7], items[9]]
    pool = ca.Pool([0], threads=2, depth=2)
    try:
        pool.set_render_layouts(True)
        for kind in ("device", "host"):
            res, rep, _, _ = decode_round(pool, sub, kind, "render " + kind, render=True)
            assert rep.failed_blobs == 0
            for j, r in enumerate(res):
                lay = ca.output_layout(sub[j], render=True)[0]
                assert lay[0]["normal"][1] == np.int16 and ("index" not in lay[0] or lay[0]["index"][1] == np.uint16)
                assert r.outputs[0]["normal"].dtype in (torch.int16, np.dtype(np.int16))
                check_item(r, sub[j], ("render", kind, j), render=True, strict_gaps=kind == "device")
        pool.set_render_layouts(False)
        res, _, _, _ = decode_round(pool, sub, "device", "render off again")
        for j, r in enumerate(res):
            check_item(r, sub[j], ("render off", j))
    finally:
        pool.close()


def test_layout_is_allocate_outputs(items):
    """ca.output_layout names the dtypes, shapes and offsets Batch.allocate_outputs gives the same blobs"""
    blobs = items[7] + items[4]
    c = ca.Context(0)
    try:
        for render in (False, True):
            b = ca.Batch(c, blobs)
            outs = b.allocate_outputs(normal_format=ca.FMT_INT16 if render else ca.FMT_FLOAT, color_components=4, index16=render)
            lay, total = ca.output_layout(blobs, render)
            base = b._keep[0].data_ptr()
            assert total == (b._keep[0].numel() + 255) // 256 * 256       # (allocate_outputs' block ends with its last array)
            for i, d in enumerate(lay):
                assert list(d) == list(outs[i])
                for name, (o, dt, shape) in d.items():
                    t, tag = outs[i][name]
                    assert np.dtype(ca._DT[tag]) == dt and tuple(t.shape) == shape and t.data_ptr() - base == o, (render, i, name)
            b.close()
    finally:
        c.close()


def test_two_slots_on_one_gpu(items):
    """two pool devices on one GPU, nine items: device destinations pinned alternately to slot 0 and 1, three host items among them,
    resident arenas for the even items - each device item is decoded by ITS slot"""
    sub = [items[k] for k in (0, 4, 1, 7, 2, 5, 9, 3, 10)]
    kinds = ["device", "device", "host", "device", "device", "pageable", "device", "host", "device"]
    slots, nxt = [], 0
    for k in kinds:
        slots.append(nxt if k == "device" else -1)
        nxt ^= 1 if k == "device" else 0
    assert {s for s in slots if s >= 0} == {0, 1}
    pool = ca.Pool([0, 0], threads=2, depth=2)
    try:
        arenas = [[ca.upload_arena(sub[j], 0), ca.upload_arena(sub[j], 0)] if j % 2 == 0 else None for j in range(len(sub))]
        res, rep, calls, _ = decode_round(pool, sub, kinds, "two slots", slots=slots, arenas=arenas)
        assert rep.failed_blobs == 0 and sum(rep.steps_per_device) == 9
        for item, slot, _ in calls:
            if kinds[item] == "device":
                assert slot == slots[item], (item, slot)
            else:
                assert slot in (0, 1)
        for j, r in enumerate(res):
            assert (r.status == 0).all()
            check_item(r, sub[j], ("two slots", j), strict_gaps=kinds[j] == "device")
    finally:
        pool.close()


def corrupt_item(rng):
    """the fuzz tests' recipe on C4 blobs (byte flips, a burst, a garbage tail, a zeroed window), intact ones in between; only what the host
    walk accepts (tests/test_pool_carry_gpu.py: corrupt_item)"""
    blobs, intact = [], []
    for i in range(100):
        b = enc(synth.bumpy_sphere(64, 32, seed=9000 + i), position_bits=14, uv_bits=12, normal_bits=10).copy()
        body = oc.parse_header(b)["body_offset"]
        mode = i % 5
        if mode == 0:
            for p in rng.integers(body, len(b), 6):
                b[p] ^= rng.integers(1, 256)
        elif mode == 1:
            p = int(rng.integers(body, max(body + 1, len(b) - 64))); b[p:p + 48] ^= 0xA5
        elif mode == 2:
            p = int(rng.integers(body, len(b))); b[p:] = rng.integers(0, 256, len(b) - p, dtype=np.uint8)
        elif mode == 3:
            p = int(rng.integers(body, max(body + 1, len(b) - 200))); b[p:p + 160] = 0
        blobs.append(aligned(b)); intact.append(mode == 4)
    return blobs, intact


def test_failures_stay_local(items):
    """an intact item, one with corrupted blobs (the recipe the suite already decodes: reported by status, nothing here is meant to fault) and
    one whose second blob is no .crt file: the call returns OK, the corrupt item's statuses are those of a plain Batch, its intact blobs and
    the intact item are the oracle's, the third item's block is untouched"""
    blobs, intact = corrupt_item(np.random.default_rng(11))
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        keep = []
        for i, b in enumerate(blobs):
            try:
                ca.Batch(c, [b]).close(); keep.append(i)
            except ca.CortoError:
                assert not intact[i]
        assert len(keep) >= 64
        bad = [blobs[i] for i in keep]
        plain = ca.Batch(c, bad)
        plain.allocate_outputs(fill=0)
        plain.decode()
        st_plain = plain.sync(raise_on_error=False).copy()
        plain.close()
    finally:
        c.close()
    assert set(np.unique(st_plain)) <= {0, -5}
    no_crt = [b.copy() for b in items[7][:3]]
    no_crt = [ca.aligned_blob(b) for b in no_crt]
    no_crt[1][:4] = 0x5A
    three = [items[2], bad, no_crt]
    pool = ca.Pool([0], threads=2, depth=2)
    try:
        blocks = make_blocks(pool, [three[0], three[1], items[7][:3]], ["device"] * 3)
        calls, lock = [], threading.Lock()

        def on_done(item, slot, status):
            with lock:
                calls.append(item)
        res, rep = pool.decode(three, dest="device", blocks=blocks, on_done=on_done)       # returns: the call is OK
        assert sorted(calls) == [0, 1, 2]
        assert (res[0].status == 0).all()
        check_item(res[0], three[0], "intact item")
        assert (res[1].status == st_plain).all(), (res[1].status, st_plain)
        ok = {j for j, i in enumerate(keep) if intact[i]}
        assert all(res[1].status[j] == 0 for j in ok)
        check_item(res[1], bad, "intact among corrupt", strict_gaps=False, only=ok)
        assert (res[2].status == E_MAGIC).all() and len(res[2].status) == 3
        assert (block_bytes(res[2].block) == FILL).all()
        nonzero = int((res[1].status != 0).sum()) + 3
        assert rep.failed_blobs == nonzero and rep.first_error != 0 and rep.steps == 3
        with pytest.raises(ca.CortoError):
            pool.decode(three, dest="device", blocks=make_blocks(pool, [three[0], three[1], items[7][:3]], ["device"] * 3), raise_on_error=True)
    finally:
        pool.close()


def test_argument_errors_before_any_launch(items):
    """a refused call has written nothing, and the pool decodes afterwards"""
    sub = [items[7], items[0] + items[1] + items[2], items[9]]
    pool = ca.Pool([0], threads=2, depth=2)
    try:
        totals = [ca.output_layout(b)[1] for b in sub]

        def refused(blocks, tag, kinds="device", slots=None, caps=None, outs=None):
            with pytest.raises(ca.CortoError) as e:
                pool.decode(sub, dest=kinds, slots=slots, blocks=outs if outs is not None else blocks, caps=caps)
            assert e.value.code == E_ARGUMENT and "item 1" in str(e.value), (tag, str(e.value))
            for b in blocks:
                assert (block_bytes(b) == FILL).all(), tag
        blocks = make_blocks(pool, sub, ["device"] * 3)
        refused(blocks, "cap = total - 1", caps=[None, totals[1] - 1, None])
        refused(blocks, "out off by 16", outs=[blocks[0], blocks[1][16:], blocks[2]])
        refused(blocks, "slot 1 on a one-device pool", slots=[0, 1, 0])
        pinned = make_blocks(pool, sub, ["device", "host", "device"])
        refused(pinned, "a pinned host tensor as a device destination", slots=[0, 0, 0])
        del pinned
        # a device tensor too short for the layout, its size overstated.  The runtime's pointer queries see ALLOCATIONS: torch gives a tensor of
        # 10 MiB or more, a multiple of 2 MiB, an allocation of exactly its size once its cache holds no larger free block - which own_allocation
        # sees to, whatever this process allocated before
        short = list(blocks)
        short[1] = None
        del blocks
        gc.collect()                                                                 # (the refusals' tracebacks are cycles that hold the blocks)
        torch.cuda.empty_cache()
        n_short = totals[1] // (2 << 20) * (2 << 20)
        assert 10 << 20 <= n_short < totals[1]
        short[1] = own_allocation(n_short)
        refused(short, "a device tensor too short for the layout", caps=[None, totals[1] + SPARE, None])
        del short
        res, rep, _, _ = decode_round(pool, sub, "device", "after the refusals")
        assert rep.failed_blobs == 0
        for j, r in enumerate(res):
            check_item(r, sub[j], ("after the refusals", j))
    finally:
        pool.close()


DTS = {"position": (np.float32, 3), "normal": (np.float32, 3), "color": (np.uint8, 4), "uv": (np.float32, 2), "index": (np.uint32, 3)}


def run_round(pool, item_list, steps, tag):
    """crthip_pool_run, checked with the lane-read loop: every lane's every blob against the oracle, the block's tail still poisoned"""
    rep, stamps = pool.run(item_list, steps=steps, warmup=0)
    assert rep.steps == steps and rep.failed_blobs == 0 and rep.poisoned_lanes == pool.lanes and len(stamps) == steps, tag
    for lane in range(pool.lanes):
        it, slot = pool.lane_item(lane)
        assert 0 <= it < len(item_list) and slot == 0, (tag, lane, it)
        for i, blob in enumerate(item_list[it]):
            ref = ref_of(blob)
            for k, (dt, w) in DTS.items():
                got = pool.lane_read(lane, i, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                assert got.tobytes() == ref[k].tobytes(), (tag, lane, it, i, k)
        assert (pool.lane_read(lane, 0, "#tail", np.uint8, 256) == 0xA5).all(), (tag, lane)


def test_run_and_decode_alternate(items):
    sub = [items[9], items[2], items[7]]
    pool = ca.Pool([0], threads=2, depth=2)
    try:
        run_round(pool, sub, 9, "run before")
        for kind in ("device", "pageable"):
            res, _, _, _ = decode_round(pool, sub, kind, "decode between")
            for j, r in enumerate(res):
                check_item(r, sub[j], ("decode between", kind, j), strict_gaps=kind == "device")
            for lane in range(pool.lanes):
                assert pool.lane_item(lane)[0] == -1
                with pytest.raises(ca.CortoError) as e:
                    pool.lane_read(lane, 0, "position", np.float32, 3)
                assert e.value.code == E_ARGUMENT
        run_round(pool, sub, 5, "run after")
    finally:
        pool.close()
