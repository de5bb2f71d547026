"""GPU (-m gpu): crthip_bvh_query through the C ABI - the kernel against the sequential model of the contract (tests/bvh_query.py: every face,
no tree), raw bytes.  Small blobs are decoded with allocate_outputs(bvh=True, quantized=("position",)); the model runs on the buffers read
back - the uint16 positions, the index, the transform's base - and the read-back positions are held to the oracle's integers.  Every set's
result records and face lists live in one device buffer pre-filled with 0xCD, each at exactly its size with poisoned gaps between them:
nothing but the records and the first `written` words of each box's slice may change.  No corrupt tree and no bad pointer reaches the GPU:
the call refuses them first (the corrupt trees: tests/test_bvh_query_cpu.py)."""
import functools

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_query as bq
import meshlet_edges as me

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = 0xCD
A = -8                                                      # CRTHIP_E_ARGUMENT

HANDMADE = {
    "one": lambda: bvh.strip(1, seed=1), "two": lambda: bvh.lattice(1), "lattice": lambda: bvh.lattice(12, step=6),
    "f4096": lambda: bvh.lattice(32, m=64),                 # bvh_blob's last face count ...
    "f4097": lambda: bvh.lattice(32, m=64, extra=1),        # ... and the other partition's first
}
NAMES = ["one", "two", "f4096", "f4097", "lattice"]
TOUCHING = 14                                               # the boxes that crates() puts first: seven touching pairs
REFERENCE = 16                                              # the first centroid box: the capacities "c - 1", "c", "c + 1" are about its count


@functools.lru_cache(maxsize=None)
def case(name):
    return me.Case(me.encode_exact(*HANDMADE[name]()))


@functools.lru_cache(maxsize=None)
def crates(name, n, seed=0):
    """n boxes for a case, computed once: seven touching pairs (a box, then its twin one unit away: against the mesh's +x side, at three
    vertices, three faces' own corner boxes), the whole mesh's box, an empty box, n // 3 boxes around face centroids that hold their face,
    then random ones, every seventh of those moved out of the range"""
    c = case(name)
    rng = np.random.default_rng(seed + n)
    bx = np.concatenate([bq.side_touches(c.P), bq.vertex_touches(c.P, rng.integers(0, c.nvert, 3)), bq.face_box_touches(c.P, c.index, rng.integers(0, c.nface, 3)),
                         bq.whole_box(c.P), bq.empty_boxes(c.P, 1), bq.centroid_boxes(c.P, c.index, rng.integers(0, c.nface, n // 3), half=12),
                         bq.out_of_range(bq.random_boxes(c.P, n, seed=seed + n))])[:n]
    bx.flags.writeable = False
    return bx


@functools.lru_cache(maxsize=None)
def answer(name, n, seed, flags, base=None):
    """the model on a case's own integers, computed once: ((status, count) a box, every box's whole list in rank order).  base: the
    position's base as a tuple, or None: the minimum a component, where CRTHIP_BIND_QUANTIZED puts it"""
    c = case(name)
    base = c.P.min(axis=0).astype(np.int64) if base is None else np.asarray(base, np.int64)
    u16 = (c.P.astype(np.int64) - base).astype(np.uint16)
    assert (u16.astype(np.int64) + base == c.P).all()
    rec, lists = bq.query_fast(u16, c.index, crates(name, n, seed), bq.order_of(c.P, c.index), base=base, flags=flags)
    return [(bq.RANGE if r["status"] == bq.RANGE else bq.OK, int(r["count"])) for r in rec], lists


def capacity_of(name, n, seed, flags, cap):
    """a set's face_capacity: a number, or "c-1" / "c" / "c+1" about the model's count of the reference box"""
    if not isinstance(cap, str):
        return cap
    c = answer(name, n, seed, flags)[0][REFERENCE][1]
    assert c >= 2, (name, n, flags, c)
    return c + {"c-1": -1, "c": 0, "c+1": 1}[cap]


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.close()


def device_bytes(a):
    import torch
    t = torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


class Out:
    """the result records and the face lists of some sets in one poisoned device buffer, each at exactly its size, poisoned gaps between
    them; shapes: (nbox, capacity) a set - capacity 0 (or a COUNT set): no list, a NULL pointer"""

    def __init__(self, shapes, fill=FILL):
        import torch
        self.at, off = [], 256
        for n, cap in shapes:
            off = (off + 255) & ~255
            r = (off, n * 16)
            off = (off + n * 16 + 255 + 64) & ~255
            self.at.append((r, (off, n * cap * 4), n, cap))
            off += n * cap * 4
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill

    def results(self, k):
        return self.buf.data_ptr() + self.at[k][0][0] if self.at[k][2] else None

    def faces(self, k):
        return self.buf.data_ptr() + self.at[k][1][0] if self.at[k][1][1] else None

    def read(self):
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        out = []
        for (ro, rn), (fo, fn), n, cap in self.at:
            untouched[ro:ro + rn] = False
            untouched[fo:fo + fn] = False
            out.append((host[ro:ro + rn].view(bq.RESULT).copy(), host[fo:fo + fn].view(np.uint32).reshape(n, cap).copy()))
        assert (host[untouched] == self.fill).all(), "bytes outside the records and the lists were written"
        return out


def bound(ctx, names, index16=False, records=False):
    import torch
    b = ca.Batch(ctx, [case(n).blob for n in names])
    b.allocate_outputs(fill=FILL, bvh=True, quantized=("position",), index16=index16)
    rec = None
    if records:
        rec = torch.full((48 * sum(i.nattr for i in b.infos) + 16,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        b.bind_quant_transforms(rec.data_ptr() + (-rec.data_ptr()) % 16)
    return b, rec


def expected(b, i, name, n, seed, flags, cap):
    """the model on what the decode left in blob i's buffers: they are held equal to the case's own integers, on which answer() ran"""
    out = b.host_outputs(i)
    t = b.quant_transform(i, "position")
    assert t.written == 1
    base = [int(t.base[c]) for c in range(3)]
    u16 = out["position"].view(np.uint16).reshape(-1, 3)
    assert (u16.astype(np.int64) + base == case(name).P).all(), name
    assert (out["index"].astype(np.uint32) == case(name).index).all(), name
    heads, lists = answer(name, n, seed, flags, None if base == case(name).P.min(axis=0).tolist() else tuple(base))
    want = bq.records(heads, flags, cap)
    return want, bq.expected_faces(want, lists, 0 if flags & bq.COUNT else cap, FILL)


def inputs_hold(want, tag):
    """the conditions on a set of at least 63 boxes, asserted on the MODEL's answer before the kernel's is looked at"""
    assert (want["count"] >= 1).sum() * 4 >= len(want), tag
    assert (want["status"] == bq.CLIPPED).any(), tag
    assert (want["status"] == bq.RANGE).any(), tag
    first, twin = want[0:TOUCHING:2], want[1:TOUCHING:2]
    assert ((first["count"] >= 1) & (twin["count"] == 0) & (twin["status"] != bq.RANGE)).any(), tag   # a match by touching alone


def compare(got, want, tag):
    rec, words = got
    wrec, wwords = want
    if rec.tobytes() != wrec.tobytes():
        bad = int(np.flatnonzero(rec != wrec)[0])
        raise AssertionError("%s: box %d: got %s expected %s" % (tag, bad, rec[bad], wrec[bad]))
    if words.tobytes() != wwords.tobytes():
        bad = int(np.flatnonzero((words != wwords).any(axis=1))[0])
        raise AssertionError("%s: box %d: list %s expected %s" % (tag, bad, words[bad], wwords[bad]))


def run(ctx, b, names, plan, seed, out=None, mutate=None):
    """the sets of one call from `plan` ((blob, boxes, flags, capacity) each); returns (out, device boxes, capacities, sets)"""
    caps = [capacity_of(names[i], n, seed, fl, cap) for (i, n, fl, cap) in plan]
    dbox = [device_bytes(crates(names[i], n, seed)) if n else None for (i, n, _, _) in plan]
    out = out or Out([(n, 0 if fl & bq.COUNT else cap) for (_, n, fl, _), cap in zip(plan, caps)])
    sets = [b.query_set(i, dbox[k].data_ptr() if n else None, out.results(k), out.faces(k), n, caps[k], fl) for k, (i, n, fl, _) in enumerate(plan)]
    if mutate:
        mutate(sets)
    return out, dbox, caps, sets


# ---- 1. one call, many sets, right behind the decode ----

#        blob, boxes, flags, capacity: 1, 63, 64, 65 and 257 boxes, a set without any, every legal flag combination, blobs twice, capacities
#        at the reference box's count - 1, at it, at it + 1 and 0.  (CLIPPED cannot happen under COUNT: those sets stay below 63 boxes.)
SETS = [(0, 1, bq.COUNT, 0), (1, 63, 0, "c-1"), (2, 64, bq.BOXES, "c+1"), (3, 65, bq.INSIDE, "c"), (4, 0, 0, 3), (4, 257, 0, "c-1"), (1, 33, bq.COUNT | bq.BOXES, 5),
        (3, 40, bq.COUNT | bq.INSIDE, 0), (0, 65, bq.BOXES, 0), (2, 257, bq.INSIDE, "c+1"), (4, 64, 0, 0), (3, 64, 0, "c")]


def test_sets_behind_the_decode_with_the_device_record(ctx):
    """the transform is the device record the decode writes: the query is enqueued right behind crthip_batch_decode, no wait in between"""
    b, rec = bound(ctx, NAMES, records=True)
    assert [i.nface for i in b.infos] == [1, 2, 4096, 4097, 288]
    out, dbox, caps, sets = run(ctx, b, NAMES, SETS, 0)
    assert all(s.transform for s in sets) and sorted({fl for (_, _, fl, _) in SETS}) == sorted(bq.FLAGS)
    b.decode()
    ctx.bvh_query(sets)
    ctx.sync()
    assert (b.sync() == 0).all()
    want = [expected(b, i, NAMES[i], n, 0, fl, caps[k]) for k, (i, n, fl, _) in enumerate(SETS)]
    for k, (i, n, fl, cap) in enumerate(SETS):
        if n >= 63:
            inputs_hold(want[k][0], ("set", k))
        if isinstance(cap, str):                                          # the reference box at its count - 1, its count, its count + 1
            r = want[k][0][REFERENCE]
            assert (r["status"], r["written"]) == ((bq.CLIPPED, r["count"] - 1) if cap == "c-1" else (bq.OK, r["count"])), (k, r)
    got = out.read()
    for k in range(len(SETS)):                                            # no box is left out
        compare(got[k], want[k], ("set", k))
    # the whole mesh's box lists every face in rank order where the capacity allows it: blob 4 through Batch.query
    res, lists = b.query(4, crates("lattice", 257)[TOUCHING:TOUCHING + 1])
    assert tuple(res[0]) == (bq.OK, 288, 288, 0) and lists[0].tolist() == bq.order_of(case("lattice").P, case("lattice").index).tolist()
    b.close()


# ---- 2. base[] on the host, a uint16 index, calls back to back ----

def test_host_base_u16_index_and_calls_back_to_back(ctx):
    names = ["lattice", "f4097", "two"]
    b, _ = bound(ctx, names, index16=True)
    b.decode()
    assert (b.sync() == 0).all()
    plan = [(0, 257, 0, "c-1"), (1, 65, bq.INSIDE, "c+1"), (2, 63, bq.BOXES, 1)]
    rounds = [0, bq.COUNT, 0]                                             # two calls back to back take the two slots; the third waits for the first's
    runs = []
    for r, extra in enumerate(rounds):
        p = [(i, n, fl | extra, cap) for (i, n, fl, cap) in plan]
        out, dbox, caps, sets = run(ctx, b, names, p, 3)
        assert not any(s.transform for s in sets) and sets[0].index_format == ca.FMT_UINT16
        ctx.bvh_query(sets)
        runs.append((p, out, dbox, caps))
    ctx.sync()
    for r, (p, out, _, caps) in enumerate(runs):
        got = out.read()
        for k, (i, n, fl, _) in enumerate(p):
            want = expected(b, i, names[i], n, 3, fl, caps[k])
            if not fl & bq.COUNT:
                inputs_hold(want[0], ("round", r, "set", k))
            compare(got[k], want, ("round", r, "set", k))
    assert runs[0][1].buf.cpu().numpy().tobytes() == runs[2][1].buf.cpu().numpy().tobytes()
    # Batch.query: upload, count, query at the largest count, download
    bx = crates("lattice", 257, 3)
    res, lists = b.query(0, bx, bq.BOXES)
    heads, full = answer("lattice", 257, 3, bq.BOXES)
    assert res.dtype == ca.QUERY_RESULT_DTYPE and res.tobytes() == bq.records(heads, bq.BOXES, max(c for _, c in heads)).tobytes()
    assert [l.tolist() for l in lists] == full and (res["status"] != bq.CLIPPED).all()
    res, lists = b.query(0, bx, 0, capacity=2)
    heads, full = answer("lattice", 257, 3, 0)
    assert res.tobytes() == bq.records(heads, 0, 2).tobytes() and [l.tolist() for l in lists] == [l[:2] for l in full]
    res, lists = b.query(0, bx, bq.COUNT)
    assert res.tobytes() == bq.records(heads, bq.COUNT, 0).tobytes() and all(len(l) == 0 for l in lists)
    assert len(b.query(0, bx[:0])[0]) == 0
    b.close()


# ---- 3. an interleaved position buffer ----

def test_interleaved_position(ctx):
    import torch
    names = ["lattice", "f4097"]
    b, _ = bound(ctx, names)
    bufs = []
    for i, name in enumerate(names):
        nv = b.infos[i].nvert
        assert b.infos[i].nattr == 1
        rec = torch.full((nv * 8 + 6,), 0x77, dtype=torch.uint8, device="cuda:0")    # records of 8 bytes from byte 6 on: 2-byte aligned, not 4
        torch.cuda.synchronize()
        at = rec.data_ptr() + 6
        index, _ = b.outputs[i]["index"]
        binding, keep = b._bvh[i]
        b.bind(i, [ca.AttrBinding(at, ca.FMT_UINT16, 0, 8, ca.BIND_QUANTIZED)], index.data_ptr(), ca.FMT_UINT32)
        b.bind_bvh(i, binding, keep)                                                  # (a bind drops the blob's derived bindings)
        bufs.append((rec, at))
    b.decode()
    assert (b.sync() == 0).all()
    plan = [(0, 65, 0, "c"), (1, 64, bq.INSIDE, "c-1")]

    def strided(sets):
        for cs, (i, _, _, _) in zip(sets, plan):
            cs.position, cs.pos_stride = bufs[i][1], 8
    out, dbox, caps, sets = run(ctx, b, names, plan, 5, mutate=strided)
    ctx.bvh_query(sets)
    ctx.sync()
    got = out.read()
    for k, (i, n, fl, _) in enumerate(plan):
        raw = bufs[i][0].cpu().numpy()[6:]
        nv = b.infos[i].nvert
        rows = raw.reshape(nv, 8)
        assert (rows[:, 6:] == 0x77).all()
        u16 = np.ascontiguousarray(rows[:, :6]).view(np.uint16)
        t = b.quant_transform(i, "position")
        base = [int(t.base[c]) for c in range(3)]
        assert (u16.astype(np.int64) + base == case(names[i]).P).all()
        heads, lists = answer(names[i], n, 5, fl)
        want = bq.records(heads, fl, caps[k])
        inputs_hold(want, ("strided", k))
        compare(got[k], (want, bq.expected_faces(want, lists, caps[k], FILL)), ("strided", k))
    # the packed buffer of the same blob with its stride spelt out: 6
    b2, _ = bound(ctx, names[:1])
    b2.decode()
    assert (b2.sync() == 0).all()

    def six(sets):
        sets[0].pos_stride = 6
    out2, _, _, sets = run(ctx, b2, names, plan[:1], 5, mutate=six)
    ctx.bvh_query(sets)
    ctx.sync()
    compare(out2.read()[0], got[0], "stride 6")
    b.close(); b2.close()


# ---- 4. every argument error, in the header's order; nothing is enqueued ----

def test_argument_errors(ctx):
    names = ["lattice", "two"]
    b, rec = bound(ctx, names, records=True)
    b.decode()
    assert (b.sync() == 0).all()
    dbox = device_bytes(crates("lattice", 64))
    out = Out([(64, 4), (64, 4)])
    L = ca.lib()

    def fresh():
        return [b.query_set(0, dbox.data_ptr(), out.results(0), out.faces(0), 64, 4, 0), b.query_set(1, dbox.data_ptr(), out.results(1), out.faces(1), 64, 4, 0)]

    def code(sets, n=None):
        arr = (ca.QuerySet * len(sets))(*sets)
        return L.crthip_bvh_query(ctx.handle, len(sets) if n is None else n, arr), L.crthip_last_error().decode()

    assert L.crthip_bvh_query(None, 0, None) == A
    assert L.crthip_bvh_query(ctx.handle, 1, None) == A and "sets" in L.crthip_last_error().decode()
    assert L.crthip_bvh_query(ctx.handle, 0, None) == 0
    host = np.zeros(4096, np.uint8)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    cases = [("nodes", None), ("nodes", lambda p: p + 8), ("position", None), ("position", lambda p: p + 1), ("index", None), ("index", lambda p: p + 2),
             ("transform", lambda p: p + 8), ("boxes", None), ("boxes", lambda p: p + 4), ("results", None), ("results", lambda p: p + 8),
             ("faces", None), ("faces", lambda p: p + 2),
             ("nface", 0), ("nface", 2**31), ("index_format", ca.FMT_INT32), ("pos_stride", 4), ("pos_stride", 7), ("flags", 8), ("flags", bq.BOXES | bq.INSIDE),
             ("reserved", 0), ("reserved", 1),
             # not device memory, or beyond the allocation
             ("nodes", hp), ("position", hp), ("index", hp), ("transform", hp), ("boxes", hp), ("results", hp), ("faces", hp), ("nbox", 2**27), ("face_capacity", 2**28)]
    for which in (0, 1):
        for field, v in cases:
            sets = fresh()
            if field == "reserved":
                sets[which].reserved[v] = 9
            else:
                setattr(sets[which], field, v(getattr(sets[which], field)) if callable(v) else v)
            c, msg = code(sets)
            word = {"nbox": "boxes", "face_capacity": "faces"}.get(field, field)
            assert c == A and "set %d" % which in msg and word in msg, (which, field, c, msg)
    # the first error of a set wins, and the first set's
    sets = fresh()
    sets[0].reserved[1], sets[0].flags, sets[0].pos_stride, sets[1].nodes = 1, 8, 7, None
    c, msg = code(sets)
    assert c == A and "set 0" in msg and "pos_stride" in msg, msg
    sets = fresh()
    sets[0].nface, sets[0].faces = 0, out.faces(0) + 2
    c, msg = code(sets)
    assert c == A and "faces" in msg, msg
    sets = fresh()
    sets[0].flags, sets[0].nodes = 8, hp                                  # a set's own fields come before where its memory is
    c, msg = code(sets)
    assert c == A and "flags" in msg, msg
    # faces is not looked at under COUNT or at capacity 0; a set without boxes: its arrays are not looked at
    sets = [fresh()[0], fresh()[0]]
    sets[0].flags, sets[0].faces = bq.COUNT, 2
    sets[1].face_capacity, sets[1].faces = 0, hp
    probe = Out([(64, 0), (64, 0)])
    sets[0].results, sets[1].results = probe.results(0), probe.results(1)
    assert code(sets)[0] == 0
    ctx.sync()
    r0, r1 = probe.read()
    assert (r0[0]["status"] != bq.CLIPPED).all() and (r0[0]["count"] == r1[0]["count"]).all() and (r1[0]["written"] == 0).all()
    sets = fresh()
    sets[0].nbox, sets[0].nodes, sets[0].results = 0, 8, None
    sets[1].nbox = 0
    assert code(sets)[0] == 0
    ctx.sync()
    assert (out.buf.cpu().numpy() == FILL).all(), "a refused call wrote"
    b.close()


# ---- 5. a batch that never queries keeps its bytes ----

def test_decode_without_a_query_is_unchanged(ctx):
    names = ["two", "lattice", "f4097"]
    a, _ = bound(ctx, names)
    a.decode()
    assert (a.sync() == 0).all()
    plain = a._keep[0].cpu().numpy().copy()
    a.close()
    b, _ = bound(ctx, names)
    b.decode()
    assert (b.sync() == 0).all()
    res, lists = b.query(1, crates("lattice", 257), 0)
    heads, full = answer("lattice", 257, 0, 0)
    assert res.tobytes() == bq.records(heads, 0, max(c for _, c in heads)).tobytes() and [l.tolist() for l in lists] == full
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()          # the query wrote nothing into the batch's outputs
    b.decode()                                                            # ... and a decode after a query leaves the same bytes again
    assert (b.sync() == 0).all()
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()
    b.close()
