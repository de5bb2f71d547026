"""GPU (-m gpu): crthip_bvh_closest through the C ABI - the kernel against the sequential model of the contract (tests/bvh_closest.py: every
face, no tree, distances in rationals), raw bytes.  Small blobs are decoded with allocate_outputs(bvh=True, quantized=("position",)); the
model runs on the case's own integers, and the buffers read back - the uint16 positions, the index, the transform's base - are held equal
to them.  Every set's hit records live in one device buffer pre-filled with 0xCD, each at exactly its size with poisoned gaps between them:
nothing but the records may change.  No corrupt tree and no bad pointer reaches the GPU: the call refuses them first (the corrupt trees:
tests/test_bvh_closest_cpu.py)."""
import functools
import math

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_closest as bc
import meshlet_edges as me

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = 0xCD
A = -8                                                      # CRTHIP_E_ARGUMENT


def wide():
    """corners at 0 and 65 535 on every axis: products beyond 128 bits (tests/test_bvh_closest_cpu.py holds that on the model)"""
    c = [0, 65535]
    pos = np.array([(x, y, z) for x in c for y in c for z in c], np.int32) + 12345
    return pos, np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [7, 0, 6], [1, 2, 4], [7, 4, 2], [0, 5, 6], [3, 6, 5]], np.uint32)


HANDMADE = {
    "one": lambda: bvh.strip(1, seed=1), "two": lambda: bvh.lattice(1), "lattice": lambda: bvh.lattice(12, step=6),
    "f4096": lambda: bvh.lattice(32, m=64),                 # bvh_blob's last face count ...
    "f4097": lambda: bvh.lattice(32, m=64, extra=1),        # ... and the other partition's first
    "wide": wide,
}
NAMES = ["one", "two", "f4096", "f4097", "lattice", "wide"]
BESIDE, VERTICES = 0, 3                                     # where clouds() puts beside()'s three copies and the three vertices


@functools.lru_cache(maxsize=None)
def case(name):
    return me.Case(me.encode_exact(*HANDMADE[name]()))


@functools.lru_cache(maxsize=None)
def cover(name):
    return bc.feature_cover(case(name).P, case(name).index)


@functools.lru_cache(maxsize=None)
def clouds(name, n, seed=0):
    """n points for a case, computed once: beside()'s three copies (at exactly r = 17 from a vertex: radius r, r - 1, 0), three vertices, seven
    points that cover the feature codes, a face's edge midpoints, two corners of the range, points off n // 4 faces' centroids along the
    normal, then random ones, every seventh of those moved out of the range.  The wide case's random points reach far into the range and
    carry radii to match"""
    c = case(name)
    rng = np.random.default_rng(seed + n)
    far = name == "wide"
    fs = rng.integers(0, c.nface, max(n // 4, 1))
    base = c.P.min(axis=0).astype(np.int64)
    pts = np.concatenate([bc.beside(c.P, c.index, 17), bc.on_vertices(c.P, rng.integers(0, c.nvert, 3)), cover(name), bc.edge_midpoints(c.P, c.index, fs[:1]),
                          bc.range_corners(base)[[0, 7]], bc.off_centroids(c.P, c.index, fs, heights=(0, 3) if not far else (0, 400)),
                          bc.out_of_range(bc.random_points(c.P, n, seed=seed + n, margin=400000 if far else 40, radius=500000 if far else 30), base)])[:n]
    pts.flags.writeable = False
    return pts


@functools.lru_cache(maxsize=None)
def faces_of(name, n, seed, base=None):
    """every point's faces with their distances, which all three flag combinations share, computed once on a case's own integers.  base: the
    position's base as a tuple, or None: the minimum a component, where CRTHIP_BIND_QUANTIZED puts it.  The rational form over all faces
    where they are few (the wide case among them), else the form that runs it on the faces a float64 pass cannot tell from the nearest"""
    c = case(name)
    base = c.P.min(axis=0).astype(np.int64) if base is None else np.asarray(base, np.int64)
    u16 = (c.P.astype(np.int64) - base).astype(np.uint16)
    assert (u16.astype(np.int64) + base == c.P).all()
    return (bc.candidates if c.nface <= 8 else bc.candidates_fast)(u16, c.index, clouds(name, n, seed), base=base), base


@functools.lru_cache(maxsize=None)
def answer(name, n, seed, flags, base=None):
    """the model's records of a set, computed once"""
    cands, base = faces_of(name, n, seed, base)
    rec = bc.closest(None, None, clouds(name, n, seed), base=base, flags=flags, cands=cands)
    rec.flags.writeable = False
    return rec


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
    """the hit records of some sets in one poisoned device buffer, each at exactly its size, poisoned gaps between them; counts: npoint a set"""

    def __init__(self, counts, fill=FILL):
        import torch
        self.at, off = [], 256
        for n in counts:
            off = (off + 255 + 64) & ~255
            self.at.append((off, n * 48))
            off += n * 48
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill

    def hits(self, k):
        return self.buf.data_ptr() + self.at[k][0] if self.at[k][1] else None

    def read(self):
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        out = []
        for o, n in self.at:
            untouched[o:o + n] = False
            out.append(host[o:o + n].view(bc.HITREC).copy())
        assert (host[untouched] == self.fill).all(), "bytes outside the records were written"
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


def expected(b, i, name, n, seed, flags):
    """the model on what the decode left in blob i's buffers: they are held equal to the case's own integers, on which answer() ran"""
    out = b.host_outputs(i)
    t = b.quant_transform(i, "position")
    assert t.written == 1
    base = [int(t.base[c]) for c in range(3)]
    u16 = out["position"].view(np.uint16).reshape(-1, 3)
    assert (u16.astype(np.int64) + base == case(name).P).all(), name
    assert (out["index"].astype(np.uint32) == case(name).index).all(), name
    return answer(name, n, seed, flags, None if base == case(name).P.min(axis=0).tolist() else tuple(base))


def inputs_hold(name, n, seed, tag):
    """the conditions on a set of at least 63 points, asserted on the MODEL's answers - under all three flag combinations, whichever the set
    runs with - before the kernel's is looked at"""
    c = case(name)
    plain, within, anyhit = (answer(name, n, seed, fl) for fl in bc.FLAGS)
    hit = plain["status"] == bc.HIT
    assert set(range(7)) <= set(plain["feature"][hit].tolist()), (tag, np.bincount(plain["feature"][hit], minlength=7))
    assert (plain["status"] == bc.RANGE).any() and hit.sum() * 2 >= n, tag
    # the radius is inclusive: at exactly r = 17 a hit, the same record as without the limit; at r - 1 and at 0 none
    assert bc.fractions_of(plain[BESIDE:BESIDE + 1]) == [(17 * 17, 1)] and plain[BESIDE].tobytes() == plain[BESIDE + 1].tobytes() == plain[BESIDE + 2].tobytes(), tag
    assert within[BESIDE].tobytes() == plain[BESIDE].tobytes() and tuple(within[BESIDE + 1]) == tuple(within[BESIDE + 2]) == bc.record(bc.MISS), tag
    assert tuple(anyhit[BESIDE]) == bc.record(bc.HIT) and tuple(anyhit[BESIDE + 1]) == bc.record(bc.MISS), tag
    assert ((within["status"] == bc.HIT) == (anyhit["status"] == bc.HIT)).all() and (anyhit["face"] == bc.NO_FACE).all(), tag
    # a vertex is at distance 0 from every face around it: the least id among them
    ties = 0
    for k in range(VERTICES, VERTICES + 3):
        around = np.flatnonzero((c.P[c.index] == clouds(name, n, seed)["p"][k]).all(axis=2).any(axis=1))
        assert bc.fractions_of(plain[k:k + 1])[0][0] == 0 and plain["face"][k] == around.min() and plain["feature"][k] < 3, (tag, k)
        ties += len(around) >= 2
    assert ties >= 1 or c.nface == 1, tag


def compare(got, want, tag):
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: point %d: got %s expected %s" % (tag, bad, got[bad], want[bad]))


def run(ctx, b, names, plan, seed, out=None, mutate=None):
    """the sets of one call from `plan` ((blob, points, flags) each); returns (out, device points, sets)"""
    dpt = [device_bytes(clouds(names[i], n, seed)) if n else None for (i, n, _) in plan]
    out = out or Out([n for (_, n, _) in plan])
    sets = [b.closest_set(i, dpt[k].data_ptr() if n else None, out.hits(k), n, fl) for k, (i, n, fl) in enumerate(plan)]
    if mutate:
        mutate(sets)
    return out, dpt, sets


# ---- 1. one call, many sets, right behind the decode ----

W, WA = bc.WITHIN, bc.WITHIN | bc.ANY
#        blob, points, flags: 1, 63, 64, 65 and 257 points, a set without any, every legal flag combination, every blob, some twice
SETS = [(0, 1, 0), (1, 63, 0), (2, 64, W), (3, 65, WA), (4, 0, 0), (4, 257, 0), (5, 65, 0), (1, 33, WA), (3, 40, W), (0, 65, W), (2, 257, 0), (5, 64, W), (4, 64, WA), (5, 63, WA)]


def test_sets_behind_the_decode_with_the_device_record(ctx):
    """the transform is the device record the decode writes: the call is enqueued right behind crthip_batch_decode, no wait in between"""
    b, rec = bound(ctx, NAMES, records=True)
    assert [i.nface for i in b.infos] == [1, 2, 4096, 4097, 288, 8]
    out, dpt, sets = run(ctx, b, NAMES, SETS, 0)
    assert all(s.transform for s in sets) and sorted({fl for (_, _, fl) in SETS}) == sorted(bc.FLAGS) and {i for (i, _, _) in SETS} == set(range(len(NAMES)))
    b.decode()
    ctx.bvh_closest(sets)
    ctx.sync()
    assert (b.sync() == 0).all()
    want = [expected(b, i, NAMES[i], n, 0, fl) for (i, n, fl) in SETS]
    for k, (i, n, fl) in enumerate(SETS):
        if n >= 63:
            inputs_hold(NAMES[i], n, 0, ("set", k))
    wide = want[6]
    assert (wide["num_hi"] > 0).any() and (wide["den_hi"] > 0).any()      # records that do not fit 64 bits
    got = out.read()
    for k in range(len(SETS)):                                            # no point is left out
        compare(got[k], want[k], ("set", k))
    b.close()


# ---- 2. base[] on the host, a uint16 index, calls back to back ----

def test_host_base_u16_index_and_calls_back_to_back(ctx):
    names = ["lattice", "f4097", "two"]
    b, _ = bound(ctx, names, index16=True)
    b.decode()
    assert (b.sync() == 0).all()
    plan = [(0, 257, 0), (1, 65, W), (2, 63, WA)]
    rounds = [0, W, 0]                                                    # two calls back to back take the two slots; the third waits for the first's
    runs = []
    for r, extra in enumerate(rounds):
        p = [(i, n, fl | extra) for (i, n, fl) in plan]
        out, dpt, sets = run(ctx, b, names, p, 3)
        assert not any(s.transform for s in sets) and sets[0].index_format == ca.FMT_UINT16
        ctx.bvh_closest(sets)
        runs.append((p, out, dpt))
    ctx.sync()
    for r, (p, out, _) in enumerate(runs):
        got = out.read()
        for k, (i, n, fl) in enumerate(p):
            inputs_hold(names[i], n, 3, ("round", r, "set", k))
            compare(got[k], expected(b, i, names[i], n, 3, fl), ("round", r, "set", k))
    assert runs[0][1].buf.cpu().numpy().tobytes() == runs[2][1].buf.cpu().numpy().tobytes()
    # Batch.closest: upload, call, download, and the float beside the records
    pts = clouds("lattice", 257, 3)
    for fl in bc.FLAGS:
        hits, dist = b.closest(0, pts, fl)
        want = answer("lattice", 257, 3, fl)
        assert hits.dtype == ca.CLOSEST_HIT_DTYPE and hits.tobytes() == want.tobytes()
        for k, (num, den) in enumerate(bc.fractions_of(want)):
            assert (math.isnan(dist[k]) and den == 0) or abs(dist[k] - math.sqrt(num / den)) <= 1e-12 * max(1.0, dist[k]), (fl, k)
    hits, dist = b.closest(0, pts[:0])
    assert len(hits) == 0 and len(dist) == 0 and hits.dtype == ca.CLOSEST_HIT_DTYPE
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
    plan = [(0, 65, 0), (1, 64, W)]

    def strided(sets):
        for cs, (i, _, _) in zip(sets, plan):
            cs.position, cs.pos_stride = bufs[i][1], 8
    out, dpt, sets = run(ctx, b, names, plan, 5, mutate=strided)
    ctx.bvh_closest(sets)
    ctx.sync()
    got = out.read()
    for k, (i, n, fl) in enumerate(plan):
        raw = bufs[i][0].cpu().numpy()[6:]
        nv = b.infos[i].nvert
        rows = raw.reshape(nv, 8)
        assert (rows[:, 6:] == 0x77).all()
        u16 = np.ascontiguousarray(rows[:, :6]).view(np.uint16)
        t = b.quant_transform(i, "position")
        base = [int(t.base[c]) for c in range(3)]
        assert (u16.astype(np.int64) + base == case(names[i]).P).all()
        inputs_hold(names[i], n, 5, ("strided", k))
        compare(got[k], answer(names[i], n, 5, fl), ("strided", k))
    # the packed buffer of the same blob with its stride spelt out: 6
    b2, _ = bound(ctx, names[:1])
    b2.decode()
    assert (b2.sync() == 0).all()

    def six(sets):
        sets[0].pos_stride = 6
    out2, _, sets = run(ctx, b2, names, plan[:1], 5, mutate=six)
    ctx.bvh_closest(sets)
    ctx.sync()
    compare(out2.read()[0], got[0], "stride 6")
    b.close(); b2.close()


# ---- 4. every argument error, in the header's order; nothing is enqueued ----

def test_argument_errors(ctx):
    names = ["lattice", "two"]
    b, rec = bound(ctx, names, records=True)
    b.decode()
    assert (b.sync() == 0).all()
    dpt = device_bytes(clouds("lattice", 64))
    out = Out([64, 64])
    L = ca.lib()

    def fresh():
        return [b.closest_set(0, dpt.data_ptr(), out.hits(0), 64, W), b.closest_set(1, dpt.data_ptr(), out.hits(1), 64, 0)]

    def code(sets, n=None):
        arr = (ca.ClosestSet * len(sets))(*sets)
        return L.crthip_bvh_closest(ctx.handle, len(sets) if n is None else n, arr), L.crthip_last_error().decode()

    assert L.crthip_bvh_closest(None, 0, None) == A
    assert L.crthip_bvh_closest(ctx.handle, 1, None) == A and "sets" in L.crthip_last_error().decode()
    assert L.crthip_bvh_closest(ctx.handle, 0, None) == 0
    host = np.zeros(4096, np.uint8)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    cases = [("nodes", None), ("nodes", lambda p: p + 8), ("position", None), ("position", lambda p: p + 1), ("index", None), ("index", lambda p: p + 2),
             ("transform", lambda p: p + 8), ("points", None), ("points", lambda p: p + 4), ("hits", None), ("hits", lambda p: p + 8),
             ("nface", 0), ("nface", 2**31), ("index_format", ca.FMT_INT32), ("pos_stride", 4), ("pos_stride", 7), ("flags", 4), ("flags", bc.ANY), ("reserved", 1),
             # not device memory, or beyond the allocation
             ("nodes", hp), ("position", hp), ("index", hp), ("transform", hp), ("points", hp), ("hits", hp), ("npoint", 2**27)]
    for which in (0, 1):
        for field, v in cases:
            sets = fresh()
            setattr(sets[which], field, v(getattr(sets[which], field)) if callable(v) else v)
            c, msg = code(sets)
            word = {"npoint": "points"}.get(field, field)
            assert c == A and "set %d" % which in msg and word in msg, (which, field, c, msg)
    # the first error of a set wins, and the first set's
    sets = fresh()
    sets[0].reserved, sets[0].flags, sets[0].pos_stride, sets[1].nodes = 1, 4, 7, None
    c, msg = code(sets)
    assert c == A and "set 0" in msg and "pos_stride" in msg, msg
    sets = fresh()
    sets[0].nface, sets[0].hits = 0, out.hits(0) + 8
    c, msg = code(sets)
    assert c == A and "hits" in msg, msg
    sets = fresh()
    sets[0].flags, sets[0].nodes = bc.ANY, hp                             # a set's own fields come before where its memory is
    c, msg = code(sets)
    assert c == A and "CRTHIP_CLOSEST_ANY" in msg, msg
    # a set without points: its arrays are not looked at
    sets = fresh()
    sets[0].npoint, sets[0].nodes, sets[0].hits = 0, 8, None
    sets[1].npoint = 0
    assert code(sets)[0] == 0
    ctx.sync()
    assert (out.buf.cpu().numpy() == FILL).all(), "a refused call wrote"
    b.close()


# ---- 5. a batch that never asks keeps its bytes ----

def test_decode_without_a_closest_call_is_unchanged(ctx):
    names = ["two", "lattice", "f4097"]
    a, _ = bound(ctx, names)
    a.decode()
    assert (a.sync() == 0).all()
    plain = a._keep[0].cpu().numpy().copy()
    a.close()
    b, _ = bound(ctx, names)
    b.decode()
    assert (b.sync() == 0).all()
    hits, _ = b.closest(1, clouds("lattice", 257), 0)
    assert hits.tobytes() == answer("lattice", 257, 0, 0).tobytes()
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()          # the call wrote nothing into the batch's outputs
    b.decode()                                                            # ... and a decode after it leaves the same bytes again
    assert (b.sync() == 0).all()
    assert b._keep[0].cpu().numpy().tobytes() == plain.tobytes()
    b.close()
