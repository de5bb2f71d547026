"""GPU (-m gpu): crthip_batch_bind_cloud_lod through the C ABI - the kernels against the sequential model of the contract (tests/cloud_lod.py),
raw bytes.  Every blob's arrays live in one device buffer pre-filled with 0xCD, a level's remap, points and weight at exactly nvert words and
its chunks at exactly ceil(nvert / K) records, with poisoned gaps between the arrays: nothing but remap, the first `cells` words of points and
weight, the first ceil(cells / K) chunk records and the 16-byte records may change.  The model runs on what the oracle decodes of the blob;
which path ran is read from Batch.kernel_times() (cloud batches, or clouds and plain meshes: under the 32 names it holds)."""
import ctypes as C

import numpy as np
import pytest

import cloud_lod as cl
import corto_amd as ca
import lod as ld
from test_lod_gpu import Bound as MeshBound
from test_lod_gpu import check as mesh_check

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = cl.FILL
A = cl.E_ARGUMENT
E_NEEDS_POSITION = -6                                       # CRTHIP_E_NORMAL_NEEDS_POSITION
BLOB = "cloud_lod_blob"
FIVE = ("cloud_lod_insert", "cloud_lod_lookup", "cloud_lod_offsets", "cloud_lod_scatter", "cloud_lod_chunks")
ALL = [(n, cl.SHIFTS[n]) for n in cl.NAMED]
EVERY = ("weight", "chunks", "record")


def make_ctx(single=False):
    c = ca.Context(0)
    if single:
        c.set_single_stream(True)
    c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def run(b):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return st


def blob_of(name):
    return cl.case(name).blob if name in cl.SHIFTS else ld.case(name).blob


class Bound:
    """cloud level-of-detail bindings of some blobs of a batch: one poisoned device buffer, every level's remap, points and weight at exactly nvert
    words and its chunks at exactly ceil(nvert / K) records, with poisoned gaps between them.  shifts: {blob: the shifts of its levels}; K: {blob:
    chunk_points}; has: {(blob, level): which of "weight", "chunks", "record" the level gets} (default: all three)"""

    def __init__(self, b, shifts, K, has=None, fill=FILL, bind=True):
        import torch
        self.b, self.shifts, self.K, self.has, self.at, off = b, dict(shifts), dict(K), dict(has or {}), {}, 0
        for i, ss in self.shifts.items():
            nv = b.infos[i].nvert
            self.at[i] = []
            for k in range(len(ss)):
                o = []
                for n in (nv * 4, nv * 4, nv * 4, cl.nchunks(nv, self.K[i]) * 32, 16):
                    off = (off + 255) & ~255
                    o.append((off, n))
                    off += n
                self.at[i].append(o)
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill
        if bind:
            self.bind()

    def wants(self, i, k):
        return self.has.get((i, k), EVERY)

    def binding(self, i):
        base = self.buf.data_ptr()
        nv = self.b.infos[i].nvert
        cb = ca.CloudLodBinding()
        cb.levels, cb.chunk_points = len(self.shifts[i]), self.K[i]
        for k, (s, o) in enumerate(zip(self.shifts[i], self.at[i])):
            w = self.wants(i, k)
            cb.level[k] = ca.CloudLodLevel(base + o[0][0], base + o[1][0], base + o[2][0] if "weight" in w else None, base + o[3][0] if "chunks" in w else None,
                                           base + o[4][0] if "record" in w else None, nv, cl.nchunks(nv, self.K[i]), s, 0)
        return cb

    def bind(self):
        for i in self.shifts:
            self.b.bind_cloud_lod(i, self.binding(i))

    def read(self, counts_of):
        """after sync: {blob: [(remap, points, weight or None, chunks or None, counts or None) a level]} cut to the written words; asserts that
        nothing but the bound arrays' written words and the records changed.  counts_of(blob, level): the counts of a level without a record"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, levels in self.at.items():
            res[i] = []
            for k, o in enumerate(levels):
                w = self.wants(i, k)
                counts = None
                if "record" in w:
                    untouched[o[4][0]:o[4][0] + 16] = False
                    counts = tuple(int(x) for x in host[o[4][0]:o[4][0] + 16].view(np.uint32))
                _, cells, nch, _ = counts or counts_of(i, k)
                if "chunks" not in w:
                    nch = 0
                assert 4 * cells <= o[1][1] and 32 * nch <= o[3][1], (i, k, counts)
                cut = lambda j, n: host[o[j][0]:o[j][0] + n].copy()                  # noqa: E731
                for j, n in ((0, o[0][1]), (1, 4 * cells), (2, 4 * cells if "weight" in w else 0), (3, 32 * nch)):
                    untouched[o[j][0]:o[j][0] + n] = False
                res[i].append((cut(0, o[0][1]).view(np.uint32), cut(1, 4 * cells).view(np.uint32), cut(2, 4 * cells).view(np.uint32) if "weight" in w else None,
                               cut(3, 32 * nch).view(ca.CLOUD_CHUNK_DTYPE) if "chunks" in w else None, counts))
        assert (host[untouched] == self.fill).all(), "bytes outside remap, the kept points, their weights, the chunks and the records were written"
        return res


def check(wb, names, tag):
    """every bound blob's levels against the model; names: {blob: case}"""
    K_at = lambda i, k: wb.K[i] if "chunks" in wb.wants(i, k) else 0                 # noqa: E731
    got = wb.read(lambda i, k: cl.model(names[i], wb.shifts[i][k], K_at(i, k))[4])
    for i, levels in got.items():
        seen = []
        for k, (remap, points, weight, chunks, counts) in enumerate(levels):
            shift = wb.shifts[i][k]
            exp = cl.model(names[i], shift, K_at(i, k))
            cl.assert_same((remap, points, weight, chunks, exp[4] if counts is None else counts), exp, (tag, names[i], shift))
            seen.append((shift, remap, points))
        cl.check_levels(seen, (tag, names[i]))
    return got


def expect_ran(b, blob, five):
    ran = set(k for k in b.kernel_times() if k.startswith("cloud_lod"))
    want = ({BLOB} if blob else set()) | (set(FIVE) if five else set())
    assert ran == want, (sorted(ran), sorted(want))


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


# ---- 1. the kernels equal the model: every named input at its shifts; with records, weights and chunks, without any, and level by level ----

def flavour_has(flavour, shifts):
    if flavour == "all":
        return {}
    if flavour == "bare":
        return {(i, k): () for i, ss in shifts.items() for k in range(len(ss))}
    sets = [("chunks",), ("weight", "record"), ("weight", "chunks"), ("record",), ("chunks", "record"), ("weight",)]
    return {(i, k): sets[(i + 2 * k) % len(sets)] for i, ss in shifts.items() for k in range(len(ss))}   # a level without chunks beside one with them


@pytest.mark.parametrize("flavour", ["all", "bare", "by_level"])
def test_kernels_equal_model(ctx, flavour):
    b = ca.Batch(ctx, [blob_of(n) for n, _ in ALL])
    b.allocate_outputs(fill=FILL)
    n = len(ALL)
    shifts = {i: ALL[i][1] for i in range(n)}
    K = {i: 0 if flavour == "bare" and i % 2 else cl.K_of(ALL[i][0]) for i in range(n)}          # (chunk_points 0, or in range and not read)
    wb = Bound(b, shifts, K, flavour_has(flavour, shifts))
    run(b)
    for i, (name, _) in enumerate(ALL):
        c = cl.case(name)
        assert (b.infos[i].nvert, b.infos[i].nface) == (c.nvert, 0), name
        if name in cl.HANDMADE:                                                     # (q = 1: the floats are the integers, exact below 2^24 and for `wide`'s multiples of 128)
            assert (b.host_outputs(i)["position"].astype(np.int64) == c.P).all(), name
    check(wb, {i: ALL[i][0] for i in range(n)}, flavour)
    ran = set(k for k in b.kernel_times() if k.startswith("cloud_lod"))
    assert ran == {BLOB} | set(FIVE[:4] if flavour == "bare" else FIVE), sorted(ran)   # (no level with chunks: no cloud_lod_chunks)
    b.close()


# ---- 2. both sides of the limit: 8 192 points are cloud_lod_blob's, one more the five kernels'; with and without records ----

@pytest.mark.parametrize("name,blob", [("n1", True), ("lattice_8192", True), ("lattice_8193", False), ("onecell_8193", False), ("plane_257", False),
                                       ("onecell_300", True), ("cloud_diff", True)])
@pytest.mark.parametrize("record", [True, False])
def test_paths(ctx, name, blob, record):
    b = ca.Batch(ctx, [blob_of(name)])
    b.allocate_outputs(fill=FILL)
    assert cl.in_blob(b.infos[0].nvert) == blob
    ss = cl.SHIFTS[name]
    wb = Bound(b, {0: ss}, {0: cl.K_of(name)}, {} if record else {(0, k): ("weight", "chunks") for k in range(len(ss))})
    run(b)
    got = check(wb, {0: name}, (name, record))
    assert len(got[0]) == len(ss)
    expect_ran(b, blob, not blob)
    b.close()


def test_no_chunks_launches_no_chunk_kernel(ctx):
    b = ca.Batch(ctx, [blob_of("lattice_8193")])
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, {0: (4, 6)}, {0: 0}, {(0, 0): ("weight", "record"), (0, 1): ()})
    run(b)
    check(wb, {0: "lattice_8193"}, "no chunks")
    assert set(k for k in b.kernel_times() if k.startswith("cloud_lod")) == set(FIVE[:4])
    b.close()


def test_one_level_and_four_levels_of_one_blob(ctx):
    b = ca.Batch(ctx, [blob_of("n257"), blob_of("n257"), blob_of("cloud_border")])
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, {0: (6,), 1: (0, 5, 6, 7), 2: (11,)}, {0: 32, 1: 32, 2: 65536})
    run(b)
    got = check(wb, {0: "n257", 1: "n257", 2: "cloud_border"}, "levels")
    assert [l[4][1:3] for l in got[1]] == [(257, 9), (55, 2), (8, 1), (8, 1)] and got[0][0][4] == got[1][2][4]
    assert got[0][0][1].tobytes() == got[1][2][1].tobytes() and got[2][0][4] == (800, 227, 1, 0)
    b.close()


# ---- 3. the position's own output, whatever its form, and every other output are those of a batch without the binding ----

FORMS = ["cloud_diff", "cloud_border", "straddle", "n257", "lattice_8193", "wide"]


def allocate(b, form):
    if form == "strided":
        b.allocate_interleaved(fill=FILL)
    else:
        b.allocate_outputs(fill=FILL, quantized={"position"} if form == "quantized" else ())


@pytest.mark.parametrize("form", ["packed", "strided", "quantized"])
def test_position_forms(ctx, form):
    # (`wide`'s span does not fit uint16 grid values: CRTHIP_BIND_QUANTIZED refuses it, with or without the binding)
    names = [n for n in FORMS if form != "quantized" or n != "wide"]
    blobs = [blob_of(n) for n in names]
    p = ca.Batch(ctx, blobs)
    allocate(p, form)
    run(p)
    assert not any(k.startswith("cloud_lod") for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(names))]
    transforms = [p.quant_transform(i, "position") for i in range(len(names))] if form == "quantized" else None
    p.close()
    b = ca.Batch(ctx, blobs)
    allocate(b, form)
    wb = Bound(b, {i: cl.SHIFTS[n] for i, n in enumerate(names)}, {i: cl.K_of(n) for i, n in enumerate(names)})
    run(b)
    check(wb, dict(enumerate(names)), form)
    for i in range(len(names)):
        same_outputs(b.host_outputs(i), plain[i], (form, names[i]))
        if transforms:
            assert bytes(b.quant_transform(i, "position")) == bytes(transforms[i]), names[i]
    expect_ran(b, True, True)
    b.close()


# ---- 4. a mixed batch: meshes (some with levels of their own) and clouds (some bound, some not), both paths; decoded twice; remove, rebind, reset ----

MIX = ["two_groups", "cloud_diff", "c4_unit", "lattice_8193", "cloud_border", "n257", "grid_64_64"]
MIX_CLOUD_SHIFTS = {1: (9, 11), 3: (4, 6), 5: (0, 5, 6, 7)}
MIX_K = {1: 64, 3: 100, 5: 32}
MIX_HAS = {(1, 1): ("weight",), (3, 0): ("chunks",), (5, 2): ()}
MIX_MESH_SHIFTS = {0: (9, 11), 6: (1, 2, 5)}
MIX_NAMES = dict(enumerate(MIX))


def mix_blobs():
    return [blob_of(n) for n in MIX]


def check_mix(b, wb, mb, plain, tag):
    check(wb, MIX_NAMES, tag)
    if mb is not None:
        mesh_check(mb, MIX_NAMES, tag)
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), plain[i], (tag, i))


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st = run(p)
    assert not any("lod" in k for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    return ref, st


def bound_mix(b, fill=FILL):
    return Bound(b, MIX_CLOUD_SHIFTS, MIX_K, MIX_HAS, fill=fill), MeshBound(b, MIX_MESH_SHIFTS)


def test_mixed_batch(ctx, mix_plain):
    import torch
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb, mb = bound_mix(b)
    st = run(b)
    assert (st == mix_plain[1]).all()
    check_mix(b, wb, mb, mix_plain[0], "first")
    first = wb.buf.cpu().numpy().copy()
    # decoded twice in a row: the same bytes over the old ones (the tables and the weight words are started again by the schedule), and over fresh poison
    run(b)
    check_mix(b, wb, mb, mix_plain[0], "again")
    assert wb.buf.cpu().numpy().tobytes() == first.tobytes()
    wb2 = Bound(b, MIX_CLOUD_SHIFTS, MIX_K, MIX_HAS, fill=0x3C)
    run(b)
    check_mix(b, wb2, mb, mix_plain[0], "other buffers")
    # NULL removes one blob's binding: the others stay, its bytes stay as they are
    b.bind_cloud_lod(3, None)
    o = wb2.at[3][0][0][0]
    wb2.buf[o:o + 64] = 0x11
    torch.cuda.synchronize()                                                        # (torch's stream; the decode runs on the context's own)
    run(b)
    assert (wb2.buf.cpu().numpy()[o:o + 64] == 0x11).all()
    expect_ran(b, True, False)                                                      # (lattice_8193 was the one job beyond cloud_lod_blob; names that fell off the 32 are not asked for)
    # ... bound again
    wb3, mb3 = bound_mix(b)
    run(b)
    check_mix(b, wb3, mb3, mix_plain[0], "bound again")
    # ... re-planned for other blobs, and back
    b.reset([blob_of("torus"), blob_of("onecell_300")])
    b.allocate_outputs(fill=FILL)
    wo = Bound(b, {1: cl.SHIFTS["onecell_300"]}, {1: 32})
    run(b)
    check(wo, {1: "onecell_300"}, "reset")
    expect_ran(b, True, False)
    b.reset(mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb4, mb4 = bound_mix(b)
    run(b)
    check_mix(b, wb4, mb4, mix_plain[0], "back")
    b.close()


def test_allocate_outputs_binds_every_cloud_and_no_mesh(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, cloud_lod=((9, 11), 64))
    assert sorted(b._cloud_lod) == [1, 3, 4, 5] and not b._lod
    run(b)

    def look(i, tag):
        levels = b.cloud_lod(i)
        assert len(levels) == 2
        for shift, got in zip((9, 11), levels):
            cl.assert_same(got, cl.model(MIX[i], shift, 64), (tag, MIX[i], shift))
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), mix_plain[0][i], i)
        if i in b._cloud_lod:
            look(i, "allocate")
    expect_ran(b, True, True)
    b.rebind()                                                                      # (rebind applies the bindings again)
    run(b)
    look(3, "rebind")
    expect_ran(b, True, True)
    # the arrays lie behind all others: the buffer without them is a prefix
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    run(p)
    small, big = p._keep[0].cpu().numpy(), b._keep[0].cpu().numpy()
    assert len(big) > len(small) and big[:len(small)].tobytes() == small.tobytes()
    p.close()
    b.close()


def test_decode_with_next_parity_1(mix_plain):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["cloud_border", "straddle", "onecell_8193"]
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        w0 = Bound(objs[0], MIX_CLOUD_SHIFTS, MIX_K, MIX_HAS)
        objs[1].reset([blob_of(n) for n in other])
        objs[1].allocate_outputs(fill=FILL)
        w1 = Bound(objs[1], {i: cl.SHIFTS[n] for i, n in enumerate(other)}, {i: 32 for i in range(len(other))}, {(1, 0): ("weight",)})
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_plain[1]).all() and (st1 == 0).all()
        check_mix(objs[0], w0, None, mix_plain[0], "cur")
        check(w1, dict(enumerate(other)), "next")
        for i, n in enumerate(other):
            if n in cl.HANDMADE:                                                    # (q = 1: the floats are the integers)
                assert (objs[1].host_outputs(i)["position"].astype(np.int64) == cl.case(n).P).all()
    finally:
        for o in objs:
            o.close()
        c.close()


# ---- 5. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    L = ca.lib()
    b = ca.Batch(ctx, [blob_of("n257"), blob_of("torus"), blob_of("cloud_border"), blob_of("cloud_diff")])
    b.allocate_outputs(fill=FILL, only={"position"})
    wb = Bound(b, {0: (5, 6), 2: (9, 11)}, {0: 32, 2: 32}, bind=False)
    good = wb.binding(0)

    def call(i, l):
        return L.crthip_batch_bind_cloud_lod(b.handle, i, C.byref(l) if l is not None else None)

    def variant(level=None, top=None, **kw):
        l = ca.CloudLodBinding.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(l.level[0 if level is None else level], k, v)
        for k, v in (top or {}).items():
            setattr(l, k, v)
        return l

    def refused(i, l, word, who=None):
        assert call(i, l) == A, word
        msg = L.crthip_last_error()
        assert word in msg and (b"blob %d" % i if who is None else who) in msg, (word, msg)
    g0, g1 = good.level[0], good.level[1]
    assert L.crthip_batch_bind_cloud_lod(None, 0, C.byref(good)) == A
    refused(4, good, b"no such blob", b"")
    refused(1, good, b"not a point cloud")
    # (a cloud without points: a batch of its own, bound and never decoded)
    nothing = ca.Batch(ctx, [ca.aligned_blob(ca.encode(ca.synth.Mesh(np.zeros((0, 3), np.float32)), with_normal=False, with_color=False, with_uv=False))])
    assert (nothing.infos[0].nvert, nothing.infos[0].nface) == (0, 0)
    for l in (good, variant(remap=None, top=dict(levels=0, chunk_points=1))):
        assert L.crthip_batch_bind_cloud_lod(nothing.handle, 0, C.byref(l)) == A and b"no points" in L.crthip_last_error() and b"blob 0" in L.crthip_last_error()
    nothing.close()
    for top in (dict(levels=0), dict(levels=5)):
        refused(0, variant(top=top), b"levels")
    for K in (1, 31, 65537, 0xFFFFFFFF):
        refused(0, variant(top=dict(chunk_points=K)), b"neither 0 nor in 32..65536")
    refused(0, variant(top=dict(chunk_points=0)), b"chunk_points is 0 and a level has chunks")
    for level in (0, 1):
        g = good.level[level]
        for kw, word in ((dict(remap=None), b"remap or points is NULL"), (dict(remap=g.remap + 2), b"not 4-byte aligned"), (dict(points=None), b"remap or points is NULL"),
                         (dict(points=g.points + 2), b"not 4-byte aligned"), (dict(weight=g.weight + 2), b"weight is not 4-byte aligned"),
                         (dict(chunks=g.chunks + 8), b"chunks or counts is not 16-byte aligned"), (dict(counts=g.counts + 8), b"chunks or counts is not 16-byte aligned"),
                         (dict(capacity=g.capacity - 1), b"capacity is below nvert"), (dict(chunks_capacity=g.chunks_capacity - 1), b"chunks_capacity is below"),
                         (dict(shift=32), b"above 31"), (dict(reserved=1), b"a level's reserved")):
            refused(0, variant(level, **kw), word)
    refused(0, variant(1, shift=5), b"not above")                                              # equal to the level's before
    refused(0, variant(1, shift=4), b"not above")
    refused(0, variant(top=dict(flags=1)), b"flag")
    refused(0, variant(top=dict(reserved=1)), b"reserved is not 0")
    # the errors come in the header's order: the mesh, no points, levels, chunk_points, then level by level the pointers, weight, chunks and counts,
    # capacity, chunks_capacity, shift, order, reserved, then the flags and the reserved word
    refused(1, variant(remap=None, top=dict(levels=0, chunk_points=1)), b"not a point cloud")
    refused(0, variant(remap=None, top=dict(levels=0, chunk_points=1)), b"levels")
    refused(0, variant(remap=None, top=dict(chunk_points=1)), b"neither 0 nor")
    refused(0, variant(remap=None, top=dict(chunk_points=0)), b"chunk_points is 0")
    refused(0, variant(remap=g0.remap + 2, weight=g0.weight + 2, counts=g0.counts + 4, capacity=0, shift=32, reserved=1), b"remap or points")
    refused(0, variant(weight=g0.weight + 2, counts=g0.counts + 4, capacity=0, shift=32, reserved=1), b"weight is not")
    refused(0, variant(counts=g0.counts + 4, capacity=0, shift=32, reserved=1), b"chunks or counts")
    refused(0, variant(capacity=0, chunks_capacity=0, shift=32, reserved=1), b"capacity is below nvert")
    refused(0, variant(chunks_capacity=0, shift=32, reserved=1), b"chunks_capacity")
    refused(0, variant(shift=32, reserved=1), b"above 31")
    refused(0, variant(1, shift=5, reserved=1), b"not above")
    refused(0, variant(1, reserved=1, top=dict(flags=1)), b"a level's reserved")
    l = variant(1, remap=None)
    l.level[0].reserved = 1
    refused(0, l, b"a level's reserved")                                                       # (level 0 is looked at whole before level 1)
    refused(0, variant(top=dict(flags=1, reserved=1)), b"flag")
    # levels beyond `levels` are not looked at; chunks_capacity is not looked at without chunks; chunk_points may be 0 without chunks
    assert call(0, variant(1, remap=None, top=dict(levels=1))) == 0
    l = variant(chunks=None, chunks_capacity=0)
    l.level[1].chunks, l.level[1].chunks_capacity, l.chunk_points = None, 0, 0
    assert call(0, l) == 0
    # every blob is held to its OWN sizes
    assert b.infos[2].nvert > g0.capacity
    refused(2, good, b"capacity is below nvert")
    roomy = wb.binding(2)
    assert b.infos[0].nvert < roomy.level[0].capacity and call(0, roomy) == 0
    # the weld's position rule: blob 3's position is not bound
    b.bind(3, [ca.AttrBinding() for _ in range(b.infos[3].nattr)])
    for k in (0, 1):
        roomy.level[k].capacity = roomy.level[k].chunks_capacity = 0xFFFFFFFF
    assert call(3, roomy) == E_NEEDS_POSITION and b"blob 3" in L.crthip_last_error() and b"position" in L.crthip_last_error()
    roomy.reserved = 1
    assert call(3, roomy) == A                                                                 # (the arguments come first)
    for l in (variant(counts=None), variant(weight=None), variant(capacity=g0.capacity + 5), variant(chunks_capacity=0xFFFFFFFF), variant(shift=0), variant(1, shift=31),
              variant(top=dict(chunk_points=65536))):
        assert call(0, l) == 0
    assert g1.shift == 6
    # crthip_batch_bind_lod keeps refusing the cloud
    ml = ca.LodBinding()
    assert L.crthip_batch_bind_lod(b.handle, 0, C.byref(ml)) == A and b"point cloud" in L.crthip_last_error()
    wb.bind()
    run(b)
    check(wb, {0: "n257", 2: "cloud_border"}, "bound")
    expect_ran(b, True, False)
    # a later bind of the blob drops it ...
    b._cloud_lod = {}
    b.rebind()                                                                      # (crthip_batch_bind_all: every blob bound again)
    run(b)
    expect_ran(b, False, False)
    # ... and so does a reset
    wb.bind()
    b.reset([blob_of("n257")])
    b.allocate_outputs(fill=FILL)
    run(b)
    expect_ran(b, False, False)
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """seven decodes on a single-stream context of 256 clouds of 2 048 points (cloud_lod_blob) and of one cloud of BASELINE config C3's size
    (578 x 289 = 167 042 points: the five kernels), with the binding and without it: the kernels' times and the batch's step time"""
    import time
    from corto_amd import synth
    c = make_ctx(True)
    small = ca.aligned_blob(ca.encode(synth.point_cloud(64, 32)))
    big = ca.aligned_blob(ca.encode(synth.point_cloud()))
    for what, blobs in (("256 clouds", [small] * 256), ("1 cloud", [big])):
        for on in (True, False):
            b = ca.Batch(c, blobs)
            b.allocate_outputs(cloud_lod=((9, 11), 64) if on else None)
            rows, steps = {}, []
            for _ in range(7):
                t0 = time.perf_counter()
                run(b)
                steps.append(round(1e6 * (time.perf_counter() - t0), 1))
                for k, v in b.kernel_times().items():
                    if k.startswith("cloud_lod") or k == "fill":
                        rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
            print("\nkernel times (us), 7 decodes of %s of %d points, cloud_lod %s:" % (what, b.infos[0].nvert, on), rows)
            print("  step (us, decode + sync, profiling on):", steps)
            if on:
                print("  counts of blob 0:", [l[4] for l in b.cloud_lod(0)])
            assert any(k.startswith("cloud_lod") for k in rows) == on
            b.close()
    c.close()
