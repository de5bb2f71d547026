"""GPU (-m gpu): crthip_bvh_cast through the C ABI - the kernel against the sequential model of the contract (tests/bvh_cast.py: every face,
no tree), raw bytes.  Small blobs are decoded with allocate_outputs(bvh=True, quantized=("position",)); the model runs on the buffers read
back - the uint16 positions, the index, the transform's base - and the read-back positions are held to the oracle's integers.  Every set's hit
records live in one device buffer pre-filled with 0xCD, each at exactly nseg records with poisoned gaps between them: nothing but the records
may change.  No corrupt tree and no bad pointer reaches the GPU: the call refuses them first (the corrupt trees: tests/test_bvh_cast_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_cast as bc
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


@functools.lru_cache(maxsize=None)
def case(name):
    return me.Case(me.encode_exact(*HANDMADE[name]()))


@functools.lru_cache(maxsize=None)
def shots(name, n, seed=0):
    """n segments for a case, computed once: shots through vertices and edge midpoints first (the watertight ones), then random ones, every
    seventh of those moved out of the range"""
    c = case(name)
    rng = np.random.default_rng(seed + n)
    nv = min(c.nvert, max(1, n // 6))
    vs = bc.vertex_shots(c.P, rng.choice(c.nvert, nv, replace=False))
    es = bc.edge_midpoint_shots(c.P, c.index, rng.choice(c.nface, min(c.nface, max(1, n // 18)), replace=False))
    rs = bc.random_segments(c.P, n, seed=seed + n)
    far = np.arange(len(rs)) % 7 == 3
    rs["q"][far, 0] += 1 << 20
    segs = np.concatenate([vs, es, rs])[:n]
    segs.flags.writeable = False
    return segs, min(n, len(vs) + len(es))


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


class Hits:
    """the hit arrays of some sets in one poisoned device buffer, each at exactly nseg records, poisoned gaps between them"""

    def __init__(self, counts, fill=FILL):
        import torch
        self.at, off = [], 256
        for n in counts:
            off = (off + 255) & ~255
            self.at.append((off, n * 32))
            off += n * 32
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill

    def ptr(self, k):
        return self.buf.data_ptr() + self.at[k][0]

    def read(self):
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        out = []
        for (o, n) in self.at:
            untouched[o:o + n] = False
            out.append(host[o:o + n].view(bc.HITREC).copy())
        assert (host[untouched] == self.fill).all(), "bytes outside the hit records were written"
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


def expected(b, i, name, segs, flags):
    """the model on what the decode left in blob i's buffers"""
    out = b.host_outputs(i)
    t = b.quant_transform(i, "position")
    assert t.written == 1
    base = [int(t.base[c]) for c in range(3)]
    u16 = out["position"].view(np.uint16).reshape(-1, 3)
    assert (u16.astype(np.int64) + base == case(name).P).all(), name
    assert (out["index"].astype(np.uint32) == case(name).index).all(), name
    return bc.cast_fast(u16, out["index"], segs, base=base, flags=flags)


def compare(got, want, tag):
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: segment %d: got %s expected %s" % (tag, bad, got[bad], want[bad]))


# ---- 1. one call, many sets, right behind the decode ----

#        blob, segments, flags: 1, 63, 64, 65 and 257 segments, a set without any, every flag combination, a blob twice
SETS = [(0, 1, 0), (1, 63, bc.ANY), (2, 64, bc.FRONT), (3, 65, 0), (4, 0, 0), (4, 257, 0), (1, 64, bc.ANY | bc.FRONT), (3, 257, bc.ANY), (0, 65, bc.FRONT)]


def test_sets_behind_the_decode_with_the_device_record(ctx):
    """the transform is the device record the decode writes: the cast is enqueued right behind crthip_batch_decode, no wait in between"""
    b, rec = bound(ctx, NAMES, records=True)
    assert [i.nface for i in b.infos] == [1, 2, 4096, 4097, 288]
    segs = [shots(NAMES[i], n)[0] for (i, n, _) in SETS]
    dsegs = [device_bytes(s) if len(s) else None for s in segs]
    hits = Hits([n for (_, n, _) in SETS])
    sets = [b.cast_set(i, dsegs[k].data_ptr() if n else None, hits.ptr(k) if n else None, n, fl) for k, (i, n, fl) in enumerate(SETS)]
    assert all(s.transform for s in sets)
    b.decode()
    ctx.bvh_cast(sets)
    ctx.sync()
    assert (b.sync() == 0).all()
    got = hits.read()
    for k, (i, n, fl) in enumerate(SETS):
        compare(got[k], expected(b, i, NAMES[i], segs[k], fl), ("set", k))
    # the watertight shots: through vertices and edge midpoints of a gap-free patch, nothing slips through
    k = 5
    tight = shots("lattice", 257)[1]
    assert tight > 40 and (got[k]["status"][:tight] == bc.HIT).all()
    assert (got[k]["status"] == bc.RANGE).sum() >= 8 and (got[k]["status"] == bc.MISS).any()
    # the device records are the host's
    host = rec.cpu().numpy()
    o = (-rec.data_ptr()) % 16
    first = np.cumsum([0] + [i.nattr for i in b.infos])
    for i in range(len(NAMES)):
        assert host[o + 48 * first[i]:o + 48 * first[i] + 48].tobytes() == bytes(b.quant_transform(i, "position"))
    b.close()


# ---- 2. base[] on the host, a uint16 index, casts back to back ----

def test_host_base_u16_index_and_casts_back_to_back(ctx):
    names = ["lattice", "f4097", "two"]
    b, _ = bound(ctx, names, index16=True)
    b.decode()
    assert (b.sync() == 0).all()
    plan = [(0, 257, 0), (1, 65, bc.FRONT), (2, 63, 0)]
    segs = [shots(names[i], n, seed=3)[0] for (i, n, _) in plan]
    dsegs = [device_bytes(s) for s in segs]
    rounds = [0, bc.ANY, bc.FRONT, 0]                                   # four calls before one sync: the job table's two blocks each come round again
    hits = [Hits([n for (_, n, _) in plan]) for _ in rounds]
    for r, extra in enumerate(rounds):
        sets = [b.cast_set(i, dsegs[k].data_ptr(), hits[r].ptr(k), n, fl | extra) for k, (i, n, fl) in enumerate(plan)]
        assert not any(s.transform for s in sets) and sets[0].index_format == ca.FMT_UINT16
        ctx.bvh_cast(sets)
    ctx.sync()
    for r, extra in enumerate(rounds):
        got = hits[r].read()
        for k, (i, n, fl) in enumerate(plan):
            compare(got[k], expected(b, i, names[i], segs[k], fl | extra), ("round", r, "set", k))
    assert hits[0].buf.cpu().numpy().tobytes() == hits[3].buf.cpu().numpy().tobytes()
    # Batch.cast: upload, cast, sync, download
    mine = b.cast(0, segs[0], bc.FRONT)
    assert mine.dtype == ca.CAST_HIT_DTYPE
    compare(mine.view(bc.HITREC), expected(b, 0, "lattice", segs[0], bc.FRONT), "Batch.cast")
    assert len(b.cast(0, segs[0][:0])) == 0
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
    plan = [(0, 65, 0), (1, 64, bc.FRONT)]
    segs = [shots(names[i], n, seed=5)[0] for (i, n, _) in plan]
    dsegs = [device_bytes(s) for s in segs]
    hits = Hits([n for (_, n, _) in plan])
    sets = []
    for k, (i, n, fl) in enumerate(plan):
        cs = b.cast_set(i, dsegs[k].data_ptr(), hits.ptr(k), n, fl)
        cs.position, cs.pos_stride = bufs[i][1], 8
        sets.append(cs)
    ctx.bvh_cast(sets)
    ctx.sync()
    got = hits.read()
    for k, (i, n, fl) in enumerate(plan):
        raw = bufs[i][0].cpu().numpy()[6:]
        nv = b.infos[i].nvert
        rows = raw.reshape(nv, 8)
        assert (rows[:, 6:] == 0x77).all()
        u16 = np.ascontiguousarray(rows[:, :6]).view(np.uint16)
        t = b.quant_transform(i, "position")
        base = [int(t.base[c]) for c in range(3)]
        assert (u16.astype(np.int64) + base == case(names[i]).P).all()
        compare(got[k], bc.cast_fast(u16, case(names[i]).index, segs[k], base=base, flags=fl), ("strided", k))
    # the packed buffer of the same blob with its stride spelt out: 6
    b2, _ = bound(ctx, names[:1])
    b2.decode()
    assert (b2.sync() == 0).all()
    h2 = Hits([65])
    cs = b2.cast_set(0, dsegs[0].data_ptr(), h2.ptr(0), 65, 0)
    cs.pos_stride = 6
    ctx.bvh_cast([cs])
    ctx.sync()
    assert h2.read()[0].tobytes() == got[0].tobytes()
    b.close(); b2.close()


# ---- 4. every argument error, in the header's order; nothing is enqueued ----

def test_argument_errors(ctx):
    names = ["lattice", "two"]
    b, rec = bound(ctx, names, records=True)
    b.decode()
    assert (b.sync() == 0).all()
    segs = shots("lattice", 64)[0]
    dseg = device_bytes(segs)
    hits = Hits([64, 64])
    L = ca.lib()

    def fresh():
        return [b.cast_set(0, dseg.data_ptr(), hits.ptr(0), 64, 0), b.cast_set(1, dseg.data_ptr(), hits.ptr(1), 64, 0)]

    def code(sets, n=None):
        arr = (ca.CastSet * len(sets))(*sets)
        return L.crthip_bvh_cast(ctx.handle, len(sets) if n is None else n, arr), L.crthip_last_error().decode()

    assert L.crthip_bvh_cast(None, 0, None) == A
    assert L.crthip_bvh_cast(ctx.handle, 1, None) == A and "sets" in L.crthip_last_error().decode()
    assert L.crthip_bvh_cast(ctx.handle, 0, None) == 0
    host = np.zeros(4096, np.uint8)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    cases = [("nodes", None), ("nodes", lambda p: p + 8), ("position", None), ("position", lambda p: p + 1), ("index", None), ("index", lambda p: p + 2),
             ("transform", lambda p: p + 8), ("segments", None), ("segments", lambda p: p + 4), ("hits", None), ("hits", lambda p: p + 8),
             ("nface", 0), ("nface", 2**31), ("index_format", ca.FMT_INT32), ("pos_stride", 4), ("pos_stride", 7), ("flags", 4), ("reserved", 9),
             # not device memory, or beyond the allocation
             ("nodes", hp), ("position", hp), ("index", hp), ("transform", hp), ("segments", hp), ("hits", hp), ("nseg", 2**27)]
    for which in (0, 1):
        for field, v in cases:
            sets = fresh()
            setattr(sets[which], field, v(getattr(sets[which], field)) if callable(v) else v)
            c, msg = code(sets)
            assert c == A and "set %d" % which in msg and ("segments" if field == "nseg" else field) in msg, (which, field, c, msg)
    # the first error of a set wins, and the first set's
    sets = fresh()
    sets[0].reserved, sets[0].flags, sets[0].pos_stride, sets[1].nodes = 1, 8, 7, None
    c, msg = code(sets)
    assert c == A and "set 0" in msg and "pos_stride" in msg, msg
    sets = fresh()
    sets[0].nface, sets[0].hits = 0, hits.ptr(0) + 8
    c, msg = code(sets)
    assert c == A and "hits" in msg, msg
    sets = fresh()
    sets[0].flags, sets[0].nodes = 4, hp                                  # a set's own fields come before where its memory is
    c, msg = code(sets)
    assert c == A and "flags" in msg, msg
    # a set without segments: its arrays are not looked at
    sets = fresh()
    sets[0].nseg, sets[0].nodes, sets[0].hits = 0, 8, None
    sets[1].nseg = 0
    assert code(sets)[0] == 0
    ctx.sync()
    assert (hits.buf.cpu().numpy() == FILL).all(), "a refused call wrote"
    b.close()


# ---- 5. a batch that never casts keeps its bytes ----

def test_decode_without_a_cast_is_unchanged(ctx):
    names = ["two", "lattice", "f4097"]
    a, _ = bound(ctx, names)
    a.decode()
    assert (a.sync() == 0).all()
    plain = a._keep[0].cpu().numpy().copy()
    a.close()
    b, _ = bound(ctx, names)
    b.decode()
    assert (b.sync() == 0).all()
    segs = shots("lattice", 257)[0]
    got = b.cast(1, segs, 0)
    compare(got.view(bc.HITREC), expected(b, 1, "lattice", segs, 0), "cast")
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()          # the cast wrote nothing into the batch's outputs
    b.decode()                                                            # ... and a decode after a cast leaves the same bytes again
    assert (b.sync() == 0).all()
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()
    b.close()
