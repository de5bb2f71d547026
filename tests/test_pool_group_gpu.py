"""The pool's groups: a lane call decodes up to G items as ONE batch object where the lanes share hardware queues (corto_hip.h, "Groups").
Six single-stream lanes (G = 2), items of six mixed tiny blobs that all DIFFER, so that a mix-up of two members' blocks, statuses or
bindings cannot hide.  Host items are views of a pinned buffer each and packed host blobs are on: items whose blobs would have to be
gathered are not grouped (the last test).  Everything is raw-byte equality with the oracle (tolerance 0)."""
import threading

import numpy as np
import pytest
import torch

import corto_amd as ca
from corto_amd import synth
from oracle import oracle as oc

pytestmark = pytest.mark.gpu

FILL, SPARE = 0xA5, 512
LANES, G = 6, 2
DTS = {"position": (np.float32, 3), "normal": (np.float32, 3), "color": (np.uint8, 4), "uv": (np.float32, 2), "index": (np.uint32, 3)}
NAMES = ("position", "normal", "color", "uv", "radius", "index")


def enc(mesh, **kw):
    kw.setdefault("normal_prediction", ca.BORDER)
    return ca.aligned_blob(ca.encode(mesh, position_bits=12, uv_bits=10, normal_bits=9, **kw))


def mixed_item(seed):
    """six blobs: five small meshes of three sizes and a point cloud of a few hundred points"""
    s = 10 * seed
    return [enc(synth.bumpy_sphere(8, 4, seed=s)), enc(synth.bumpy_sphere(8, 4, seed=s + 1)), enc(synth.bumpy_sphere(10, 5, seed=s + 2)),
            enc(synth.point_cloud(20, 12 + seed % 5, seed=s + 3), normal_prediction=ca.DIFF), enc(synth.bumpy_sphere(12, 4, seed=s + 4)),
            enc(synth.bumpy_sphere(8, 4, seed=s + 5))]


_refs = {}
_pins = []


def ref_of(blob):
    k = blob.tobytes()
    if k not in _refs:
        _refs[k] = oc.decode(blob)
    return _refs[k]


@pytest.fixture(scope="module")
def items():
    """sixty-one distinct items, an odd number: a crthip_pool_decode draws extra tickets while 2 x lanes x G = 24 items are undrawn, so about
    half of these are decoded in groups and the last two dozen one item a call"""
    global _pins
    _pins = [ca.pinned_host_arena(mixed_item(j)) for j in range(61)]      # (the pinned buffers stay alive with the module)
    return [views for _, views in _pins]


@pytest.fixture()
def pool():
    p = ca.Pool([0], threads=2, depth=3)
    assert p.lanes == LANES
    p.set_packed_host_blobs(True)
    yield p
    p.close()


def make_blocks(item_list, kinds):
    blocks = []
    for j, blobs in enumerate(item_list):
        n = ca.output_layout(blobs)[1] + SPARE
        if kinds[j] == "device":
            blocks.append(torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0"))
        elif kinds[j] == "host":
            t = torch.empty(n, dtype=torch.uint8).pin_memory()
            t.fill_(FILL)
            blocks.append(t)
        else:
            raw = np.full(n + 256, FILL, dtype=np.uint8)
            blocks.append(raw[(-raw.ctypes.data) % 256:][:n])
    torch.cuda.synchronize()
    return blocks


def raw_of(block):
    return block if isinstance(block, np.ndarray) else block.cpu().numpy()


def check_block(block, blobs, device, tag, skip=()):
    """every array of every blob is the oracle's; a device block is 0xA5 everywhere outside the arrays, any block from the layout's total on"""
    lay, total = ca.output_layout(blobs)
    raw = raw_of(block)
    covered = np.zeros(len(raw), dtype=bool)
    for i, blob in enumerate(blobs):
        for name, (o, dt, shape) in lay[i].items():
            covered[o:o + int(np.prod(shape)) * dt.itemsize] = True
        if i in skip:
            continue
        ref = ref_of(blob)
        assert set(lay[i]) == {k for k in NAMES if k in ref}, (tag, i)
        for name, (o, dt, shape) in lay[i].items():
            assert raw[o:o + ref[name].nbytes].tobytes() == ref[name].tobytes(), (tag, i, name)
    assert (raw[total:] == FILL).all(), (tag, "bytes behind the layout's total were written")
    if device:
        assert (raw[~covered] == FILL).all(), (tag, "a gap between two arrays was written")


def decode_all(pool, item_list, kinds):
    blocks = make_blocks(item_list, kinds)
    calls, lock = [], threading.Lock()

    def on_done(item, slot, status):
        with lock:
            calls.append((item, status.copy()))
    res, rep = pool.decode(item_list, dest=kinds, on_done=on_done, blocks=blocks)
    assert sorted(c[0] for c in calls) == list(range(len(item_list)))           # `done` exactly once per item
    for item, status in calls:
        assert len(status) == len(item_list[item]) and (status == res[item].status).all(), item
    assert rep.steps == len(item_list) and sum(rep.steps_per_device) == len(item_list)
    return res, rep


def kinds_for(n):
    return [("device", "host", "pageable")[j % 3] for j in range(n)]


def test_run_counts_every_member_as_a_step(pool, items):
    """61 steps (odd, above 4 x lanes x G = 48) on three items: groups form, and the report, the stamps and the lanes' outputs are those of
    61 steps of one item each"""
    sub = items[:3]
    steps, warmup = 61, 5
    assert steps % 2 == 1 and steps > 4 * LANES * G
    rep, stamps = pool.run(sub, steps=steps, warmup=warmup)
    assert rep.steps == steps and len(stamps) == steps and rep.failed_blobs == 0 and rep.first_error == 0
    assert sum(rep.steps_per_device) == steps
    assert (np.diff(stamps) >= 0).all() and stamps[0] >= 0
    assert rep.grouped_steps >= G and rep.grouped_steps % G == 0                  # lane calls of two items happened
    assert rep.triangles > 0 and rep.vertices > 0
    assert rep.poisoned_lanes == pool.lanes
    seen = set()
    for lane in range(pool.lanes):
        it, slot = pool.lane_item(lane)
        assert 0 <= it < len(sub) and slot == 0, (lane, it)
        seen.add(it)
        for i, blob in enumerate(sub[it]):
            ref = ref_of(blob)
            for k, (dt, w) in DTS.items():
                if k not in ref:
                    continue
                got = pool.lane_read(lane, i, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                assert got.tobytes() == ref[k].tobytes(), (lane, it, i, k)
        assert (pool.lane_read(lane, 0, "#tail", np.uint8, 256) == 0xA5).all(), lane
    # triangles and vertices are the timed steps' own: whichever items they were, a multiple-free sum of the three items' counts
    per_item = [sum(ca.probe(b).nface for b in it) for it in sub]
    assert min(per_item) * steps <= rep.triangles <= max(per_item) * steps


def test_resident_items_in_separate_allocations(pool, items):
    """device arenas: a group's members lie in two allocations and the batch object reads both from the lower one's address - a decode of
    all items into device blocks (what a group wrote stays to be read), then a run whose lanes end as ever"""
    arenas = [[ca.upload_arena(it, 0)] for it in items]
    kinds = ["device"] * len(items)
    blocks = make_blocks(items, kinds)
    res, rep = pool.decode(items, dest=kinds, arenas=arenas, blocks=blocks)
    assert rep.failed_blobs == 0 and rep.grouped_steps >= G
    for j, r in enumerate(res):
        assert (r.status == 0).all()
        check_block(r.block, items[j], True, ("resident", j))
    sub = items[3:6]
    rep, stamps = pool.run(sub, steps=61, warmup=0, arenas=arenas[3:6])
    assert rep.steps == 61 and rep.failed_blobs == 0 and rep.grouped_steps >= G and rep.poisoned_lanes == pool.lanes
    for lane in range(pool.lanes):
        it, _ = pool.lane_item(lane)
        for i, blob in enumerate(sub[it]):
            ref = ref_of(blob)
            got = pool.lane_read(lane, i, "position", np.float32, ref["nvert"] * 3)
            assert got.tobytes() == ref["position"].tobytes(), (lane, it, i)


def test_decode_seven_items_mixed_destinations(pool, items):
    """seven distinct items (odd on purpose) into device, pinned and pageable blocks: fewer than 2 x lanes x G, so one item a call"""
    sub = items[:7]
    kinds = kinds_for(7)
    res, rep = decode_all(pool, sub, kinds)
    assert rep.failed_blobs == 0 and rep.grouped_steps == 0
    for j, r in enumerate(res):
        assert (r.status == 0).all()
        check_block(r.block, sub[j], kinds[j] == "device", ("seven", j))


def test_decode_sixty_one_items_in_groups(pool, items):
    """... and sixty-one: groups of two with destinations of different kinds side by side, every block its own item's"""
    kinds = kinds_for(len(items))
    res, rep = decode_all(pool, items, kinds)
    assert rep.failed_blobs == 0 and rep.grouped_steps >= G
    assert rep.triangles == sum(ca.probe(b).nface for it in items for b in it)
    for j, r in enumerate(res):
        assert (r.status == 0).all()
        check_block(r.block, items[j], kinds[j] == "device", ("sixty-one", j))


def test_a_bad_member_fails_alone(pool, items):
    """item 14 holds a truncated blob (the host walk refuses it: every entry carries the code, the block is untouched), item 21 a blob whose
    CLERS table names a symbol no automaton accepts (the recipe of test_gpu_parity.py: reported by status, that blob alone); all other
    items are exact - also the ones drawn into a group with either"""
    its = [list(it) for it in items]
    A, B = 14, 21                                            # (both drawn while groups are formed: behind the lanes' first calls, 24 before the end)
    cut = its[A][2]
    its[A][2] = ca.aligned_blob(cut[:len(cut) - 24].copy())
    bad = its[B][4].copy()
    probs = int(ca.probe(bad).body_offset) + 9 + 4 + 1
    bad[probs:probs + 2] = (7, 255)
    its[B][4] = ca.aligned_blob(bad)
    kinds = ["device"] * len(its)
    blocks = make_blocks(items, kinds)                       # (sized by the intact items' layouts: the headers are unchanged)
    calls, lock = [], threading.Lock()

    def on_done(item, slot, status):
        with lock:
            calls.append(item)
    res, rep = pool.decode(its, dest=kinds, on_done=on_done, blocks=blocks)
    assert sorted(calls) == list(range(len(its)))
    code = int(res[A].status[0])
    assert code < 0 and (res[A].status == code).all() and len(res[A].status) == 6
    assert (raw_of(res[A].block) == FILL).all()
    assert res[B].status[4] == -5 and (np.delete(res[B].status, 4) == 0).all()
    check_block(res[B].block, items[B], False, "the corrupt item's intact blobs", skip={4})
    for j, r in enumerate(res):
        if j in (A, B):
            continue
        assert (r.status == 0).all(), j
        check_block(r.block, items[j], True, ("beside the bad ones", j))
    assert rep.failed_blobs == 6 + 1 and rep.first_error != 0 and rep.steps == len(its) and rep.grouped_steps >= G


@pytest.mark.parametrize("n", [7, 61])
def test_group_size_does_not_change_a_byte(items, monkeypatch, n):
    """the decodes above under $CORTO_POOL_GROUP = 1 and = 2: byte-identical blocks"""
    sub = items[:n]
    kinds = kinds_for(n)
    seen = {}
    for g in ("1", "2"):
        monkeypatch.setenv("CORTO_POOL_GROUP", g)
        p = ca.Pool([0], threads=2, depth=3)
        try:
            p.set_packed_host_blobs(True)
            res, rep = decode_all(p, sub, kinds)
            assert rep.failed_blobs == 0
            assert (rep.grouped_steps > 0) == (g == "2" and n >= 2 * LANES * G)
            lay = [ca.output_layout(b) for b in sub]
            for j, r in enumerate(res):
                raw = raw_of(r.block)
                # a host block's bytes between the arrays are unspecified (the copy moves [0, total)): compare the arrays, and whole device blocks
                if kinds[j] == "device":
                    assert seen.setdefault(j, raw.tobytes()) == raw.tobytes(), (g, j)
                else:
                    arrays = b"".join(raw[o:o + int(np.prod(shape)) * dt.itemsize].tobytes() for d in lay[j][0] for (o, dt, shape) in d.values())
                    assert seen.setdefault(j, arrays) == arrays, (g, j)
                check_block(r.block, sub[j], kinds[j] == "device", (g, j))
        finally:
            p.close()


def test_items_that_must_be_gathered_are_not_grouped(pool, items):
    """the same items as separate pageable arrays, and as pinned views with packed host blobs off: one item a call, every block exact"""
    kinds = kinds_for(len(items))
    scattered = [[ca.aligned_blob(b.copy()) for b in it] for it in items]
    res, rep = decode_all(pool, scattered, kinds)
    assert rep.failed_blobs == 0 and rep.grouped_steps == 0
    for j in (0, 17, 60):
        check_block(res[j].block, items[j], kinds[j] == "device", ("scattered", j))
    pool.set_packed_host_blobs(False)
    res, rep = decode_all(pool, items, kinds)
    assert rep.failed_blobs == 0 and rep.grouped_steps == 0
    for j in (1, 30, 59):
        check_block(res[j].block, items[j], kinds[j] == "device", ("switch off", j))
