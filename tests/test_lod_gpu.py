"""GPU (-m gpu): crthip_batch_bind_lod through the C ABI - the kernels against the sequential model of the contract (tests/lod.py), raw bytes.
Every blob's arrays live in one device buffer pre-filled with 0xCD, a level's remap at exactly nvert words and its index at exactly 3*nface
words, with poisoned gaps between the arrays: nothing but remap, the first 3*faces words of the index and the 16-byte records may change.  The
model runs on what the oracle decodes of the blob (the decode's own index is checked against it where it is bound); which path ran is read
from Batch.kernel_times()."""
import ctypes as C

import numpy as np
import pytest

import corto_amd as ca
import lod as ld
from conftest import CLOUD_CASES, MESH_CASES, load_golden
from test_launch_schedule_gpu import B_EST, B_NONORMAL, EVERYTHING, corpus

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = ld.FILL
A = ld.E_ARGUMENT
E_NEEDS_POSITION = -6                                       # CRTHIP_E_NORMAL_NEEDS_POSITION
BLOB = "lod_blob"
SIX = ("lod_insert", "lod_lookup", "lod_faces", "lod_keep", "lod_offsets", "lod_scatter")
GOLDEN_SHIFTS = (9, 11)
# (case, shifts): every golden mesh at (9, 11), then the named cases at theirs
ALL = [(n, GOLDEN_SHIFTS) for n in MESH_CASES] + [(n, ld.SHIFTS[n]) for n in ld.NAMED]


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
    return ld.case(name).blob


class Bound:
    """level-of-detail bindings of some blobs of a batch: one poisoned device buffer, every level's remap at exactly nvert words and its index at
    exactly 3*nface words with poisoned gaps between them; the blobs in `records` (default: all) get a device counts record a level, the
    others none.  shifts: {blob: the shifts of its levels}"""

    def __init__(self, b, shifts, records=None, fill=FILL, bind=True):
        import torch
        self.b, self.shifts, self.at, off = b, dict(shifts), {}, 0
        self.records = set(self.shifts if records is None else records)
        for i, ss in self.shifts.items():
            self.at[i] = []
            for _ in ss:
                o = []
                for n in (b.infos[i].nvert * 4, b.infos[i].nface * 12, 16):
                    off = (off + 255) & ~255
                    o.append((off, n))
                    off += n
                self.at[i].append(o)
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill
        if bind:
            self.bind()

    def binding(self, i):
        base = self.buf.data_ptr()
        lb = ca.LodBinding()
        lb.levels = len(self.shifts[i])
        for k, (s, o) in enumerate(zip(self.shifts[i], self.at[i])):
            lb.level[k] = ca.LodLevel(base + o[0][0], base + o[1][0], base + o[2][0] if i in self.records else None, self.b.infos[i].nvert,
                                      self.b.infos[i].nface * 3, s, 0)
        return lb

    def bind(self):
        for i in self.shifts:
            self.b.bind_lod(i, self.binding(i))

    def read(self, faces_of):
        """after sync: {blob: [(remap, the written index words, counts or None) a level]}; asserts that nothing but the bound arrays' written
        words and the records changed.  faces_of(blob, level): the kept faces of a level without a record (the model's)"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, levels in self.at.items():
            res[i] = []
            for k, o in enumerate(levels):
                untouched[o[0][0]:o[0][0] + o[0][1]] = False
                counts = None
                if i in self.records:
                    untouched[o[2][0]:o[2][0] + 16] = False
                    counts = tuple(int(x) for x in host[o[2][0]:o[2][0] + 16].view(np.uint32))
                faces = counts[1] if counts else faces_of(i, k)
                assert 12 * faces <= o[1][1], (i, k, counts)
                untouched[o[1][0]:o[1][0] + 12 * faces] = False
                res[i].append((host[o[0][0]:o[0][0] + o[0][1]].view(np.uint32).copy(), host[o[1][0]:o[1][0] + 12 * faces].view(np.uint32).copy(), counts))
        assert (host[untouched] == self.fill).all(), "bytes outside remap, the kept faces and the records were written"
        return res


def check(wb, names, tag):
    """every bound blob's levels against the model; names: {blob: case}"""
    got = wb.read(lambda i, k: ld.model(names[i], wb.shifts[i][k])[2][1])
    for i, levels in got.items():
        seen = []
        for k, (remap, index, counts) in enumerate(levels):
            shift = wb.shifts[i][k]
            exp = ld.model(names[i], shift)
            ld.assert_same((remap, index, exp[2] if counts is None else counts), exp, (tag, names[i], shift))
            seen.append((shift, remap, exp[2]))
        ld.check_levels(seen, (tag, names[i]))
    return got


def index_kw(mode):
    return {"u32": dict(index16=False), "u16": dict(index16=True), "unbound": dict(only={"position"})}[mode]


def expect_ran(b, blob, six):
    ran = set(k for k in b.kernel_times() if k.startswith("lod"))
    want = ({BLOB} if blob else set()) | (set(SIX) if six else set())
    assert ran == want, (sorted(ran), sorted(want))


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


# ---- 1. the kernels equal the model: every golden mesh at (9, 11), every named case at its shifts, every index form ----

@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernels_equal_model(ctx, mode):
    b = ca.Batch(ctx, [blob_of(n) for n, _ in ALL])
    b.allocate_outputs(fill=FILL, **index_kw(mode))
    n = len(ALL)
    wb = Bound(b, {i: ALL[i][1] for i in range(n)}, records=range(0, n, 2))
    run(b)
    for i, (name, _) in enumerate(ALL):
        c = ld.case(name)
        assert (b.infos[i].nvert, b.infos[i].nface) == (c.nvert, c.nface), name
        if mode != "unbound":                                                       # (the model's index is the one this decode left)
            assert (b.host_outputs(i)["index"].astype(np.uint32) == c.index).all(), name
    check(wb, {i: ALL[i][0] for i in range(n)}, mode)
    expect_ran(b, True, True)
    b.close()


# ---- 2. both sides of both limits: 8 192 faces and 8 192 vertices are lod_blob's, one more the six kernels'; with and without records;
#         one level (the strips, `twice`) and four (c4_unit) ----

@pytest.mark.parametrize("name,blob", [("grid_64_64", True), ("grid_17_241", False), ("grid_8192", True), ("grid_8193", False), ("c4_unit", True),
                                       ("twice", False), ("strip_257", True)])
@pytest.mark.parametrize("record", [True, False])
def test_paths(ctx, name, blob, record):
    b = ca.Batch(ctx, [blob_of(name)])
    b.allocate_outputs(fill=FILL)
    assert ld.in_blob(b.infos[0].nvert, b.infos[0].nface) == blob
    wb = Bound(b, {0: ld.SHIFTS[name]}, records=[0] if record else [])
    run(b)
    got = check(wb, {0: name}, (name, record))
    assert len(got[0]) == len(ld.SHIFTS[name])
    expect_ran(b, blob, not blob)
    b.close()


def test_one_level_and_four_levels_of_one_blob(ctx):
    b = ca.Batch(ctx, [blob_of("c4_unit"), blob_of("c4_unit"), blob_of("grid_90_91")])
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, {0: (11,), 1: (0, 9, 11, 13), 2: (3,)})
    run(b)
    got = check(wb, {0: "c4_unit", 1: "c4_unit", 2: "grid_90_91"}, "levels")
    assert [l[2][:2] for l in got[1]] == [(2112, 4096), (1902, 3746), (237, 470), (11, 14)] and got[0][0][2] == got[1][2][2]
    assert got[0][0][1].tobytes() == got[1][2][1].tobytes() and got[2][0][2][1] == 2244
    b.close()


# ---- 3. the position's own output, whatever its form, is that of a batch without the binding ----

FORMS = ["c4_unit", "confetti", "fields32", "straddle", "grid_17_241"]


def allocate(b, form):
    if form == "strided":
        b.allocate_interleaved(fill=FILL)
    else:
        b.allocate_outputs(fill=FILL, quantized={"position"} if form == "quantized" else ())


@pytest.mark.parametrize("form", ["packed", "strided", "quantized"])
def test_position_forms(ctx, form):
    # (the wide fixture's span does not fit uint16 grid values: CRTHIP_BIND_QUANTIZED refuses it, with or without the binding)
    names = [n for n in FORMS if form != "quantized" or n != "fields32"]
    blobs = [blob_of(n) for n in names]
    p = ca.Batch(ctx, blobs)
    allocate(p, form)
    run(p)
    assert not any(k.startswith("lod") for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(names))]
    transforms = [p.quant_transform(i, "position") for i in range(len(names))] if form == "quantized" else None
    p.close()
    b = ca.Batch(ctx, blobs)
    allocate(b, form)
    wb = Bound(b, {i: ld.SHIFTS[n] for i, n in enumerate(names)})
    run(b)
    check(wb, dict(enumerate(names)), form)
    for i in range(len(names)):
        same_outputs(b.host_outputs(i), plain[i], (form, names[i]))
        if transforms:
            assert bytes(b.quant_transform(i, "position")) == bytes(transforms[i]), names[i]
    expect_ran(b, True, True)
    b.close()


# ---- 4. a mixed batch: bound and unbound blobs, a cloud, both paths; every other output as without the binding; decoded twice; remove, rebind ----

MIX = ["two_groups", "cloud_diff", "c4_unit", "nonmanifold_fins", "confetti", "grid_8193", "strip_256", "grid_64_64"]
MIX_SHIFTS = {0: GOLDEN_SHIFTS, 2: (0, 9, 11, 13), 4: (9, 11, 13), 5: (1, 2), 7: (1, 2, 5)}
MIX_RECORDS = [0, 5, 7]
MIX_NAMES = dict(enumerate(MIX))


def mix_blobs():
    return [load_golden(n)["crt"] if n in CLOUD_CASES else blob_of(n) for n in MIX]


def check_mix(b, wb, plain, tag):
    check(wb, MIX_NAMES, tag)
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), plain[i], (tag, i))


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st = run(p)
    assert not any(k.startswith("lod") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    return ref, st


def test_mixed_batch(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, MIX_SHIFTS, MIX_RECORDS)
    st = run(b)
    assert (st == mix_plain[1]).all()
    expect_ran(b, True, True)
    check_mix(b, wb, mix_plain[0], "first")
    first = wb.buf.cpu().numpy().copy()
    # decoded twice in a row: the same bytes over the old ones (the tables and the records are started again by the schedule), and over fresh poison
    run(b)
    check_mix(b, wb, mix_plain[0], "again")
    assert wb.buf.cpu().numpy().tobytes() == first.tobytes()
    wb2 = Bound(b, MIX_SHIFTS, MIX_RECORDS, fill=0x3C)
    run(b)
    check_mix(b, wb2, mix_plain[0], "other buffers")
    # NULL removes one blob's binding: the others stay, its bytes stay as they are
    import torch
    b.bind_lod(5, None)
    o = wb2.at[5][0][0][0]
    wb2.buf[o:o + 64] = 0x11
    torch.cuda.synchronize()                                                        # (torch's stream; the decode runs on the context's own)
    run(b)
    assert (wb2.buf.cpu().numpy()[o:o + 64] == 0x11).all()
    expect_ran(b, True, False)                                                      # (grid_8193 was the one job beyond lod_blob)
    # ... bound again
    wb3 = Bound(b, MIX_SHIFTS, MIX_RECORDS)
    run(b)
    check_mix(b, wb3, mix_plain[0], "bound again")
    expect_ran(b, True, True)
    # ... re-planned for other blobs, and back
    b.reset([blob_of("torus"), blob_of("strip_255")])
    b.allocate_outputs(fill=FILL)
    wo = Bound(b, {1: ld.SHIFTS["strip_255"]})
    run(b)
    check(wo, {1: "strip_255"}, "reset")
    expect_ran(b, True, False)
    b.reset(mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb4 = Bound(b, MIX_SHIFTS, MIX_RECORDS)
    run(b)
    check_mix(b, wb4, mix_plain[0], "back")
    b.close()


def test_allocate_outputs_binds_every_mesh(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, lod=GOLDEN_SHIFTS)
    run(b)

    def look(i, tag):
        levels = b.lod(i)
        assert len(levels) == 2
        for shift, got in zip(GOLDEN_SHIFTS, levels):
            ld.assert_same(got, ld.model(MIX[i], shift), (tag, MIX[i], shift))
    for i, name in enumerate(MIX):
        same_outputs(b.host_outputs(i), mix_plain[0][i], i)
        if name in CLOUD_CASES:
            assert i not in b._lod
            continue
        look(i, "allocate")
    expect_ran(b, True, True)
    b.rebind()                                                                      # (rebind applies the bindings again)
    run(b)
    look(2, "rebind")
    expect_ran(b, True, True)
    b.close()


def test_everything_plus_the_levels(ctx):
    """the schedule test's EVERYTHING with and without the levels: every other output - attributes, index, computed normals and tangents,
    meshlets, bounds, adjacency, weld - has the bytes it has without them (allocate_outputs places the levels' arrays behind all others)"""
    blobs = [corpus()[B_EST], corpus()[B_NONORMAL], blob_of("c4_unit")]
    bufs = []
    for lod in (None, GOLDEN_SHIFTS):
        b = ca.Batch(ctx, blobs)
        b.allocate_outputs(fill=FILL, meshlets=(64, 124, 0), lod=lod, **EVERYTHING)
        run(b)
        assert any(k.startswith("lod") for k in b.kernel_times()) == (lod is not None)
        bufs.append(b._keep[0].cpu().numpy().copy())
        if lod:
            for shift, got in zip(GOLDEN_SHIFTS, b.lod(2)):
                ld.assert_same(got, ld.model("c4_unit", shift), ("everything", shift))
            for i in (0, 1):
                for remap, index, counts in b.lod(i):
                    assert sum(counts[1:]) == b.infos[i].nface and len(index) == 3 * counts[1] and (remap <= np.arange(len(remap))).all()
        b.close()
    assert len(bufs[1]) > len(bufs[0]) and bufs[1][:len(bufs[0])].tobytes() == bufs[0].tobytes()


def test_decode_with_next_parity_1(mix_plain):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["c4_unit", "straddle", "grid_17_241"]
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        w0 = Bound(objs[0], MIX_SHIFTS, MIX_RECORDS)
        objs[1].reset([blob_of(n) for n in other])
        objs[1].allocate_outputs(fill=FILL)
        w1 = Bound(objs[1], {i: ld.SHIFTS[n] for i, n in enumerate(other)}, [0, 2])
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_plain[1]).all() and (st1 == 0).all()
        check_mix(objs[0], w0, mix_plain[0], "cur")
        check(w1, dict(enumerate(other)), "next")
        for i, n in enumerate(other):
            assert (objs[1].host_outputs(i)["index"] == ld.case(n).index).all()
    finally:
        for o in objs:
            o.close()
        c.close()


# ---- 5. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    L = ca.lib()
    b = ca.Batch(ctx, [blob_of("torus"), load_golden("cloud_diff")["crt"], blob_of("two_groups"), blob_of("c4_unit")])
    b.allocate_outputs(fill=FILL, only={"position"})                                  # (neither the index nor every attribute is bound)
    wb = Bound(b, {0: (9, 11), 2: (9, 11)}, bind=False)
    good = wb.binding(0)

    def call(i, l):
        return L.crthip_batch_bind_lod(b.handle, i, C.byref(l) if l is not None else None)

    def variant(level=None, top=None, **kw):
        l = ca.LodBinding.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(l.level[0 if level is None else level], k, v)
        for k, v in (top or {}).items():
            if k == "reserved":
                l.reserved[v] = 1
            else:
                setattr(l, k, v)
        return l
    g0, g1 = good.level[0], good.level[1]
    assert L.crthip_batch_bind_lod(None, 0, C.byref(good)) == A
    assert call(4, good) == A and b"no such blob" in L.crthip_last_error()
    assert call(1, good) == A and b"point cloud" in L.crthip_last_error() and b"blob 1" in L.crthip_last_error()
    for top in (dict(levels=0), dict(levels=5)):
        assert call(0, variant(top=top)) == A and b"levels" in L.crthip_last_error() and b"blob 0" in L.crthip_last_error()
    for level in (0, 1):
        g = good.level[level]
        for kw, word in ((dict(remap=None), b"remap or index is NULL"), (dict(remap=g.remap + 2), b"not 4-byte aligned"), (dict(index=None), b"remap or index is NULL"),
                         (dict(index=g.index + 2), b"not 4-byte aligned"), (dict(counts=g.counts + 8), b"counts is not 16-byte aligned"),
                         (dict(remap_capacity=g.remap_capacity - 1), b"remap_capacity"), (dict(index_capacity=g.index_capacity - 1), b"index_capacity"),
                         (dict(shift=32), b"above 31"), (dict(reserved=1), b"reserved")):
            assert call(0, variant(level, **kw)) == A, (level, kw)
            assert b"blob 0" in L.crthip_last_error() and word in L.crthip_last_error(), (level, kw, L.crthip_last_error())
    assert call(0, variant(1, shift=9)) == A and b"not above" in L.crthip_last_error()          # equal to the level's before
    assert call(0, variant(1, shift=8)) == A and b"not above" in L.crthip_last_error()
    assert call(0, variant(top=dict(flags=1))) == A and b"flag" in L.crthip_last_error()
    for w in (0, 1):
        assert call(0, variant(top=dict(reserved=w))) == A and b"reserved" in L.crthip_last_error()
    # the errors come in the header's order: the point cloud, levels, then level by level pointers, counts, capacities, shift, order, reserved, then the flags
    assert call(1, variant(remap=None, top=dict(levels=0))) == A and b"point cloud" in L.crthip_last_error()
    assert call(0, variant(remap=None, top=dict(levels=0))) == A and b"levels" in L.crthip_last_error()
    assert call(0, variant(remap=g0.remap + 2, counts=g0.counts + 4, remap_capacity=0, shift=32, reserved=1)) == A and b"remap or index" in L.crthip_last_error()
    assert call(0, variant(counts=g0.counts + 4, remap_capacity=0, shift=32, reserved=1)) == A and b"counts is not" in L.crthip_last_error()
    assert call(0, variant(index_capacity=0, shift=32, reserved=1)) == A and b"index_capacity" in L.crthip_last_error()
    assert call(0, variant(shift=32, reserved=1)) == A and b"above 31" in L.crthip_last_error()
    assert call(0, variant(1, shift=9, reserved=1)) == A and b"not above" in L.crthip_last_error()
    assert call(0, variant(1, reserved=1, top=dict(flags=1))) == A and b"a level's reserved" in L.crthip_last_error()
    assert call(0, variant(0, reserved=1, top=dict(flags=1))) == A and b"a level's reserved" in L.crthip_last_error()
    l = variant(1, remap=None)
    l.level[0].reserved = 1
    assert call(0, l) == A and b"a level's reserved" in L.crthip_last_error()                  # (level 0 is looked at whole before level 1)
    assert call(0, variant(top=dict(flags=1, reserved=1))) == A and b"flag" in L.crthip_last_error()
    # levels beyond `levels` are not looked at
    assert call(0, variant(1, remap=None, top=dict(levels=1))) == 0
    # every blob is held to its OWN sizes
    assert b.infos[2].nvert < g0.remap_capacity and call(2, variant(remap_capacity=b.infos[2].nvert - 1)) == A and b"blob 2" in L.crthip_last_error()
    # the weld's position rule: blob 3's position is not bound
    b.bind(3, [ca.AttrBinding() for _ in range(b.infos[3].nattr)])
    roomy = ca.LodBinding.from_buffer_copy(good)
    for k in (0, 1):
        roomy.level[k].remap_capacity = roomy.level[k].index_capacity = 0xFFFFFFFF
    assert call(3, roomy) == E_NEEDS_POSITION and b"blob 3" in L.crthip_last_error() and b"position" in L.crthip_last_error()
    roomy.reserved[1] = 1
    assert call(3, roomy) == A                                                                 # (the arguments come first)
    for l in (variant(counts=None), variant(remap_capacity=g0.remap_capacity + 5), variant(index_capacity=0xFFFFFFFF), variant(shift=0), variant(1, shift=31)):
        assert call(0, l) == 0
    assert g1.shift == 11
    wb.bind()
    run(b)
    check(wb, {0: "torus", 2: "two_groups"}, "bound")
    expect_ran(b, True, False)
    # a later bind of the blob drops it ...
    b._lod = {}
    b.rebind()                                                                      # (crthip_batch_bind_all: every blob bound again)
    run(b)
    expect_ran(b, False, False)
    # ... and so does a reset
    wb.bind()
    b.reset([blob_of("torus")])
    b.allocate_outputs(fill=FILL)
    run(b)
    expect_ran(b, False, False)
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """seven decodes on a single-stream context of 256 C4 units (2 112 vertices each: lod_blob) and of the 131 584-face mesh (the six kernels),
    with the binding and without it: the kernels' times and the batch's step time"""
    import time
    from corto_amd import synth
    c = make_ctx(True)
    c4 = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32), with_color=False, with_normal=False))
    big = ca.aligned_blob(ca.encode(synth.bumpy_sphere(256, 257), with_normal=False, with_color=False, with_uv=False))
    for what, blobs in (("256 x 2112 vertices", [c4] * 256), ("1 x 131584 faces", [big])):
        for on in (True, False):
            b = ca.Batch(c, blobs)
            b.allocate_outputs(index16=len(blobs) > 1, lod=GOLDEN_SHIFTS if on else None)
            rows, steps = {}, []
            for _ in range(7):
                t0 = time.perf_counter()
                run(b)
                steps.append(round(1e6 * (time.perf_counter() - t0), 1))
                for k, v in b.kernel_times().items():
                    if k.startswith("lod") or k == "fill":
                        rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
            print("\nkernel times (us), 7 decodes of %s, lod %s:" % (what, on), rows)
            print("  step (us, decode + sync, profiling on):", steps)
            if on:
                print("  counts of blob 0:", [l[2] for l in b.lod(0)])
            assert any(k.startswith("lod") for k in rows) == on
            b.close()
    c.close()
