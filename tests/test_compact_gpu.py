"""GPU (-m gpu): crthip_batch_bind_compact through the C ABI - the kernels against the sequential model of the contract (tests/compact.py), raw
bytes.  Every set's arrays live in one device buffer pre-filled with 0xCD, newid at exactly nvert words, order and the gathered arrays at
exactly vertex_capacity records and the index at exactly index_capacity words, with poisoned gaps between them: nothing but newid, the first
min(used, vertex_capacity) words of order and records of a gathered array (their E bytes alone where it has a stride), the first
min(3*F, index_capacity) words of the index and the 16-byte records may change.  The model runs on the id list the set names as the decode
itself left it (the blob's index, its welded index, a level's index or points, each checked by its own tests) and on the blob's own final
vertex outputs; which path ran is read from Batch.kernel_times()."""
import ctypes as C

import numpy as np
import pytest

import cloud_lod as cl
import compact as cp
import corto_amd as ca
import lod as ld
import table_edges as te
from conftest import load_golden
from test_cloud_lod_gpu import Bound as CloudBound
from test_lod_gpu import Bound as MeshBound

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = cp.FILL
A, F_ = cp.E_ARGUMENT, cp.E_FORMAT
BLOB = "compact_blob"
FIVE = ("compact_mark", "compact_count", "compact_offsets", "compact_place", "compact_index")
GATHER = "compact_gather"
EVERY = ("newid", "order", "index", "record")


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


def golden(name):
    return ca.aligned_blob(load_golden(name)["crt"])


def attr_no(b, i, name):
    return [a["name"] for a in b.infos[i].attrs()].index(name)


class Compacted:
    """compaction bindings of some blobs of a batch in one poisoned device buffer.  sets: {blob: [dict(source=, level=0, has=EVERY, vcap=None,
    icap=None, gathers=[(source number, name of the host output it equals, dst_stride, group)])]} - capacities default to nvert and 3*nface;
    gathers of one `group` (not None) share one destination region at the byte offsets given as group = (key, offset)"""

    def __init__(self, b, sets, fill=FILL, bind=True):
        import torch
        self.b, self.sets, self.at, self.fill, off = b, sets, {}, fill, 0

        def take(n):
            nonlocal off
            off = (off + 255) & ~255
            r = off
            off += n
            return r
        for i, ss in sets.items():
            nv, nf = b.infos[i].nvert, b.infos[i].nface
            self.at[i] = []
            for s in ss:
                s.setdefault("level", 0); s.setdefault("has", EVERY); s.setdefault("gathers", [])
                s["vcap"] = nv if s.get("vcap") is None else s["vcap"]
                s["icap"] = 3 * nf if s.get("icap") is None else s["icap"]
                o = dict(newid=take(nv * 4), order=take(s["vcap"] * 4), index=take(s["icap"] * 4), record=take(16), gathers=[], groups={})
                for (src, name, stride, group) in s["gathers"]:
                    E = self.element(i, name)[0]
                    if group is None:
                        o["gathers"].append(take(s["vcap"] * (stride or E)))
                    else:
                        if group[0] not in o["groups"]:
                            o["groups"][group[0]] = take(s["vcap"] * stride)
                        o["gathers"].append(o["groups"][group[0]] + group[1])
                self.at[i].append(o)
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        if bind:
            self.bind()

    def element(self, i, name):
        """(E, the host output's array) of a gathered output: what Batch.host_outputs gives under that name, a record a vertex"""
        if isinstance(name, tuple):                                  # (E, a function that gives the (nvert, E) bytes)
            return name[0], None
        view, dt = self.b.outputs[i][name]
        return int(view.shape[1]) * np.dtype(ca._DT[dt]).itemsize, None

    def binding(self, i):
        base = self.buf.data_ptr()
        kb = ca.CompactBinding()
        kb.sets = len(self.sets[i])
        for k, (s, o) in enumerate(zip(self.sets[i], self.at[i])):
            t = kb.set[k]
            t.source, t.level, t.vertex_capacity, t.index_capacity, t.newid_capacity = s["source"], s["level"], s["vcap"], s["icap"], self.b.infos[i].nvert
            for f in ("newid", "order", "index"):
                if f in s["has"]:
                    setattr(t, f, base + o[f])
            if "record" in s["has"]:
                t.counts = base + o["record"]
            t.ngather = len(s["gathers"])
            for q, ((src, name, stride, group), go) in enumerate(zip(s["gathers"], o["gathers"])):
                t.gather[q] = ca.CompactGather(base + go, src, stride)
        return kb

    def bind(self):
        for i in self.sets:
            self.b.bind_compact(i, self.binding(i))

    def check(self, src_of, tag, sources=None):
        """after sync: every set against the model, and nothing written but what the contract names.  src_of(blob, set) -> (the id list as the
        decode left it, F or None); sources: {(blob, name): (nvert, E) bytes} for gathered outputs host_outputs does not give as they are"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        outs = {i: self.b.host_outputs(i) for i in self.sets}
        for i, ss in self.sets.items():
            nv = self.b.infos[i].nvert
            res[i] = []
            for k, (s, o) in enumerate(zip(ss, self.at[i])):
                cloud = s["source"] == ca.COMPACT_CLOUD_LOD
                src, F = src_of(i, k)
                if cloud:
                    order_full = np.asarray(src, np.uint32)
                    exp_counts = (nv, len(order_full), 0, int(bool(s["gathers"]) and len(order_full) > s["vcap"]))
                    exp = (None, order_full[:s["vcap"]], None, exp_counts, order_full)
                else:
                    exp = cp.build(src, nv, faces=F, vertex_capacity=s["vcap"], index_capacity=s["icap"], has_order="order" in s["has"],
                                   has_index="index" in s["has"], ngather=len(s["gathers"]))
                cut = lambda f, n: host[o[f]:o[f] + n].copy()                        # noqa: E731
                if "record" in s["has"]:
                    untouched[o["record"]:o["record"] + 16] = False
                    counts = tuple(int(x) for x in cut("record", 16).view(np.uint32))
                    assert counts == tuple(exp[3]), (tag, i, k, counts, exp[3])
                n = min(exp[3][1], s["vcap"])
                if not cloud:
                    got = []
                    for f, words in (("newid", nv), ("order", n), ("index", min(3 * exp[3][2], s["icap"]))):
                        if f in s["has"]:
                            untouched[o[f]:o[f] + 4 * words] = False
                            got.append(cut(f, 4 * words).view(np.uint32))
                        else:
                            got.append(None)
                    cp.assert_same(got + [exp[3]], exp, (tag, i, k))
                    if got[1] is not None and got[2] is not None:
                        cp.check_properties(np.asarray(src).reshape(-1)[:3 * exp[3][2]], nv, got[0], got[1], got[2], exp[3], tag=(tag, i, k))
                for (gsrc, name, stride, group), go in zip(s["gathers"], o["gathers"]):
                    E = self.element(i, name)[0]
                    S = stride or E
                    rows = (sources or {}).get((i, name))
                    if rows is None:
                        rows = np.ascontiguousarray(outs[i][name]).view(np.uint8).reshape(nv, E)
                    want = rows[exp[4][:n].astype(np.int64)]
                    at = go + np.arange(n)[:, None] * S + np.arange(E)[None, :]
                    assert host[at].tobytes() == want.tobytes(), (tag, i, k, name, "gathered bytes differ")
                    untouched[at.reshape(-1)] = False
                res[i].append(exp)
        assert (host[untouched] == self.fill).all(), (tag, "bytes outside what the contract names were written")
        return res


def expect_ran(b, blob, five, gather):
    ran = set(k for k in b.kernel_times() if k.startswith("compact"))
    want = ({BLOB} if blob else set()) | (set(FIVE) if five else set()) | ({GATHER} if gather else set())
    assert ran == want, (sorted(ran), sorted(want))


def mesh_case(name):
    if name in te.BIG_STRIPS:
        return te.big_strip(name)
    if name in te.ADJ_STRIPS:
        return te.adj_strip(te.ADJ_STRIPS[name])
    return ld.case(name)


# ---- 1. every mesh source, both sides of 8 192, one and two rounds of compact_offsets, the blocks' ends; levels with and without a record ----

@pytest.mark.parametrize("name,blob", [("c4_unit", True), ("grid_8192", True), ("grid_8193", False), ("nvert_255", True), ("nvert_256", True), ("nvert_257", True),
                                       ("strip_65536", False), ("strip_65537", False)])
@pytest.mark.parametrize("record", [True, False])
def test_mesh_sources(ctx, name, blob, record):
    c = mesh_case(name)
    b = ca.Batch(ctx, [c.blob])
    b.allocate_outputs(fill=FILL, weld=True)
    assert cp.in_blob(b.infos[0].nvert, b.infos[0].nface) == blob
    shifts = (te.BIG_SHIFTS[1], 31) if name in te.BIG_STRIPS else (2, 5) if name in te.ADJ_STRIPS else ld.SHIFTS[name][-2:]
    mb = MeshBound(b, {0: shifts}, records=None if record else [])
    pos = attr_no(b, 0, "position")
    sets = [dict(source=ca.COMPACT_INDEX, gathers=[(pos, "position", 0, None)]), dict(source=ca.COMPACT_WELD),
            dict(source=ca.COMPACT_LOD, level=0, gathers=[(pos, "position", 16, None)]),
            dict(source=ca.COMPACT_LOD, level=len(shifts) - 1, has=("order", "index", "record"))]
    kb = Compacted(b, {0: sets})
    run(b)
    assert (b.host_outputs(0)["index"] == c.index).all()
    lod_host = mb.buf.cpu().numpy()

    def lod_list(k):
        o = mb.at[0][k][1]
        words = lod_host[o[0]:o[0] + o[1]].view(np.uint32)
        F = int((words != cp.FILL32).sum()) // 3                                     # (a level's ids are below nvert: never the fill)
        assert (words[3 * F:] == cp.FILL32).all()
        return words, F

    def src_of(i, k):
        if k == 0:
            return c.index, None
        if k == 1:
            return b.weld(0)[1], None
        return lod_list(sets[k]["level"])
    got = kb.check(src_of, (name, record))
    assert got[0][0][3][1] == c.nvert and got[0][1][3][1] == b.weld(0)[2][1]        # (every vertex used; the welded index uses the weld's `unique`)
    assert got[0][2][3][2] == lod_list(0)[1]
    expect_ran(b, blob, not blob, True)
    b.close()


# ---- 2. the cloud source: the level's points are the order; levels with and without a record, both of the levels' paths ----

@pytest.mark.parametrize("name", ["cloud_diff", "lattice_8193", "n257"])
@pytest.mark.parametrize("record", [True, False])
def test_cloud_source(ctx, name, record):
    c = cl.case(name)
    b = ca.Batch(ctx, [c.blob])
    b.allocate_outputs(fill=FILL)
    ss = cl.SHIFTS[name][:2]
    wb = CloudBound(b, {0: ss}, {0: cl.K_of(name)}, {} if record else {(0, k): ("weight",) for k in range(len(ss))})
    pos = attr_no(b, 0, "position")
    sets = [dict(source=ca.COMPACT_CLOUD_LOD, level=k, has=("record",), gathers=[(pos, "position", 0, None)]) for k in range(len(ss))]
    sets.append(dict(source=ca.COMPACT_CLOUD_LOD, level=0, has=("record",), vcap=3, gathers=[(pos, "position", 12, None)]))
    sets.append(dict(source=ca.COMPACT_CLOUD_LOD, level=0, has=("record",), vcap=0))            # (the record alone)
    kb = Compacted(b, {0: sets})
    run(b)
    got = kb.check(lambda i, k: (cl.model(name, ss[sets[k]["level"]], 0)[1], None), (name, record))
    assert got[0][2][3][3] == int(got[0][2][3][1] > 3) and got[0][3][3][3] == 0
    expect_ran(b, False, False, True)
    b.close()


# ---- 3. clipping at used - 1 and at 0, the words behind the capacities untouched ----

@pytest.mark.parametrize("name", ["c4_unit", "grid_8193"])
def test_clipping(ctx, name):
    c = ld.case(name)
    b = ca.Batch(ctx, [c.blob])
    b.allocate_outputs(fill=FILL)
    pos = attr_no(b, 0, "position")
    used, words = c.nvert, 3 * c.nface
    sets = [dict(source=ca.COMPACT_INDEX, vcap=used - 1, gathers=[(pos, "position", 0, None)]), dict(source=ca.COMPACT_INDEX, vcap=0, gathers=[(pos, "position", 0, None)]),
            dict(source=ca.COMPACT_INDEX, icap=words - 1), dict(source=ca.COMPACT_INDEX, icap=0, vcap=used + 1, has=("index", "record"))]
    kb = Compacted(b, {0: sets})
    run(b)
    got = kb.check(lambda i, k: (c.index, None), name)
    assert [g[3] for g in got[0]] == [(c.nvert, used, c.nface, 1)] * 4
    b.close()


# ---- 4. the gathers: the position's forms; INT16 normals at stride 8; colours; computed normals; FLOAT tangents; an interleaved destination ----

@pytest.mark.parametrize("form", ["packed", "strided", "quantized"])
def test_position_forms(ctx, form):
    names = ["c4_unit", "grid_8193"]
    b = ca.Batch(ctx, [ld.case(n).blob for n in names])
    if form == "strided":
        b.allocate_interleaved(fill=FILL, normal_format=ca.FMT_FLOAT, index16=False)
    else:
        b.allocate_outputs(fill=FILL, quantized={"position"} if form == "quantized" else ())
    E = 6 if form == "quantized" else 12
    kb = Compacted(b, {i: [dict(source=ca.COMPACT_INDEX, has=("record",), gathers=[(attr_no(b, i, "position"), (E, None), 0, None)])] for i in range(2)})
    run(b)
    rows = {(i, (E, None)): np.ascontiguousarray(b.host_outputs(i)["position"]).view(np.uint8).reshape(-1, E) for i in range(2)}
    kb.check(lambda i, k: (ld.case(names[i]).index, None), form, sources=rows)
    expect_ran(b, True, True, True)
    b.close()


def test_int16_normals_at_stride_8_and_an_interleaved_destination(ctx):
    import torch
    b = ca.Batch(ctx, [golden("c4_unit")])
    b.allocate_outputs(fill=FILL)
    nv = b.infos[0].nvert
    nrm = torch.full((nv * 8,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    binds = [ca.AttrBinding.from_buffer_copy(b._keep[1][k]) for k in range(b.infos[0].nattr)]
    kn, kp, kc = (attr_no(b, 0, n) for n in ("normal", "position", "color"))
    binds[kn] = ca.AttrBinding(nrm.data_ptr(), ca.FMT_INT16, 0, 8, 0)
    b.bind(0, binds, b._keep[2][0], ca.FMT_UINT32)
    # a 24-byte compact record: position at 0, the normal at 12, the colour at 20; and the normal once more, packed
    sets = [dict(source=ca.COMPACT_INDEX, has=("record",), gathers=[(kp, "position", 24, ("rec", 0)), (kn, (6, "n"), 24, ("rec", 12)), (kc, "color", 24, ("rec", 20)),
                                                                   (kn, (6, "n"), 0, None)])]
    kb = Compacted(b, {0: sets})
    run(b)
    rows = nrm.cpu().numpy().reshape(nv, 8)
    assert (rows[:, 6:] == FILL).all()                                              # (a strided binding: its six bytes alone)
    assert (rows[:, :6] != FILL).any()
    kb.check(lambda i, k: (b.host_outputs(0)["index"], None), "interleaved", sources={(0, (6, "n")): np.ascontiguousarray(rows[:, :6])})
    expect_ran(b, True, False, True)
    b.close()


@pytest.mark.parametrize("oc", [3, 4])
def test_colour_components(ctx, oc):
    b = ca.Batch(ctx, [golden("group_props")])
    b.allocate_outputs(fill=FILL, color_components=oc)
    kb = Compacted(b, {0: [dict(source=ca.COMPACT_INDEX, has=("record",), gathers=[(attr_no(b, 0, "color"), "color", 0, None), (attr_no(b, 0, "color"), "color", 7, None)])]})
    run(b)
    assert b.host_outputs(0)["color"].shape[1] == oc
    kb.check(lambda i, k: (b.host_outputs(0)["index"], None), oc)
    b.close()


def test_computed_normals_and_float_tangents(ctx):
    """computed normals of a blob that stores none; FLOAT tangents, packed: 16 bytes a vertex from a 256-byte-aligned array to one, the 16-byte unit"""
    b = ca.Batch(ctx, [golden("pos_only"), golden("c4_unit")])
    b.allocate_outputs(fill=FILL, computed_normals=True, computed_tangents=True)
    assert "normal" in b.outputs[0] and "tangent" in b.outputs[1]
    kb = Compacted(b, {0: [dict(source=ca.COMPACT_INDEX, has=("record",), gathers=[(ca.COMPACT_COMPUTED_NORMALS, "normal", 0, None)])],
                       1: [dict(source=ca.COMPACT_INDEX, has=("record",), vcap=1000, gathers=[(ca.COMPACT_COMPUTED_TANGENTS, "tangent", 0, None),
                                                                                              (ca.COMPACT_COMPUTED_TANGENTS, "tangent", 32, None)])]})
    run(b)
    got = kb.check(lambda i, k: (b.host_outputs(i)["index"], None), "computed")
    assert got[1][0][3][3] == 1
    b.close()


# ---- 5. a mixed batch of bound and unbound meshes and clouds; decoded twice; the unbound blobs and an unbound batch are untouched ----

MIX = ["two_groups", "cloud_diff", "c4_unit", "grid_8193", "cloud_border", "grid_64_64"]
MIX_LOD = {2: (9, 11), 3: (1, 2)}
MIX_CLOUD = {1: (9, 11)}


def mix_blobs():
    return [cl.case(n).blob if n in cl.SHIFTS else ld.case(n).blob for n in MIX]


def bind_mix(b):
    b.allocate_outputs(fill=FILL, lod=None)
    mb = MeshBound(b, MIX_LOD, records=[3])
    wb = CloudBound(b, MIX_CLOUD, {1: 64})
    p = lambda i: attr_no(b, i, "position")                                          # noqa: E731
    sets = {1: [dict(source=ca.COMPACT_CLOUD_LOD, level=1, has=("record",), gathers=[(p(1), "position", 0, None), (attr_no(b, 1, "color"), "color", 0, None)])],
            2: [dict(source=ca.COMPACT_LOD, level=k, gathers=[(p(2), "position", 0, None), (attr_no(b, 2, "normal"), "normal", 0, None)]) for k in (0, 1)],
            3: [dict(source=ca.COMPACT_LOD, level=1, gathers=[(p(3), "position", 0, None)]), dict(source=ca.COMPACT_INDEX, has=("newid",))]}
    return mb, wb, Compacted(b, sets)


def mix_src(b, mb):
    lod_host = mb.buf.cpu().numpy()

    def src_of(i, k):
        if i == 1:
            return cl.model(MIX[1], MIX_CLOUD[1][1], 0)[1], None
        if i == 3 and k == 1:
            return ld.case(MIX[3]).index, None
        level = k if i == 2 else 1
        exp = ld.model(MIX[i], MIX_LOD[i][level])
        o = mb.at[i][level][1]
        assert lod_host[o[0]:o[0] + 12 * exp[2][1]].tobytes() == exp[1].tobytes()
        return exp[1], None
    return src_of


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    run(p)
    assert not any(k.startswith("compact") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX))], p.stats().descriptor_bytes
    p.close()
    return ref


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


def test_mixed_batch(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    mb, wb, kb = bind_mix(b)
    run(b)
    kb.check(mix_src(b, mb), "first")
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), mix_plain[0][i], ("first", i))
    first = kb.buf.cpu().numpy().copy()
    assert b.stats().descriptor_bytes > mix_plain[1]
    # decoded twice: the same bytes over the old ones - the mask was zeroed again - and over fresh poison
    run(b)
    assert kb.buf.cpu().numpy().tobytes() == first.tobytes()
    kb2 = Compacted(b, kb.sets, fill=0x3C)
    run(b)
    kb2.check(mix_src(b, mb), "other buffers")
    # (which kernels ran is asked of the small batches above: kernel_times holds 32 names and this batch has more)
    # the binding removed from every blob: the batch is the plain one again, descriptor bytes and kernels (the levels' own arrays aside)
    for i in kb.sets:
        b.bind_compact(i, None)
    b._lod, b._cloud_lod = {}, {}
    b.rebind()
    run(b)
    assert not any(k.startswith("compact") for k in b.kernel_times()) and b.stats().descriptor_bytes == mix_plain[1]
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), mix_plain[0][i], ("unbound", i))
    b.close()


def test_allocate_outputs_and_compact(ctx):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, lod=(9, 11), cloud_lod=((9, 11), 64), compact=True)
    run(b)
    for i, name in enumerate(MIX):
        sets, outs = b.compact(i), b.host_outputs(i)
        assert len(sets) == 2
        for k, s in enumerate(sets):
            nv, used, faces, clipped = s["counts"]
            assert clipped == 0 and nv == b.infos[i].nvert
            if b.infos[i].nface:
                src = b.lod(i)[k][1]
                exp = cp.build(src, nv)
                cp.assert_same((s["newid"], s["order"], s["index"], s["counts"]), exp, (name, k))
                order = exp[4]
            else:
                order = b.cloud_lod(i)[k][1]
                assert used == len(order)
            for attr in ("position", "normal", "color", "uv"):
                if attr in outs:
                    assert s[attr].tobytes() == np.ascontiguousarray(outs[attr][order.astype(np.int64)]).tobytes(), (name, k, attr)
    b.close()


# ---- 6. crthip_batch_decode_with_next on parity 1 of a single-stream context ----

def test_decode_with_next_parity_1(mix_plain):
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        objs[0].reset([ld.case("c4_unit").blob])
        objs[0].allocate_outputs(fill=FILL)
        k0 = Compacted(objs[0], {0: [dict(source=ca.COMPACT_INDEX, gathers=[(attr_no(objs[0], 0, "position"), "position", 0, None)])]})
        objs[1].reset(mix_blobs())
        mb, wb, k1 = bind_mix(objs[1])
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == 0).all() and (st1 == 0).all()
        k0.check(lambda i, k: (ld.case("c4_unit").index, None), "cur")
        k1.check(mix_src(objs[1], mb), "next")
        for i in range(len(MIX)):
            same_outputs(objs[1].host_outputs(i), mix_plain[0][i], ("next", i))
    finally:
        for o in objs:
            o.close()
        c.close()


# ---- 7. bind-time errors in the stated order, and the lifetime rules ----

def test_errors_in_order(ctx):
    L = ca.lib()
    b = ca.Batch(ctx, [golden("c4_unit"), cl.case("cloud_diff").blob, golden("pos_only")])
    b.allocate_outputs(fill=FILL, lod=(9, 11), cloud_lod=((9, 11), 64), weld=True, computed_normals=True)
    kp, kn, kc = (attr_no(b, 0, n) for n in ("position", "normal", "color"))
    kb = Compacted(b, {0: [dict(source=ca.COMPACT_LOD, level=1, gathers=[(kp, "position", 0, None), (kn, "normal", 0, None)]), dict(source=ca.COMPACT_WELD)],
                       1: [dict(source=ca.COMPACT_CLOUD_LOD, level=1, has=("record",), gathers=[(attr_no(b, 1, "position"), "position", 0, None)])]}, bind=False)
    good, cgood = kb.binding(0), kb.binding(1)
    err = L.crthip_last_error

    def call(i, k):
        return L.crthip_batch_bind_compact(b.handle, i, C.byref(k) if k is not None else None)

    def variant(base=good, s=0, g=None, top=None, **kw):
        k = ca.CompactBinding.from_buffer_copy(base)
        for f, v in kw.items():
            setattr(k.set[s].gather[g] if g is not None else k.set[s], f, v)
        for f, v in (top or {}).items():
            if f == "reserved":
                k.reserved[v] = 1
            else:
                setattr(k, f, v)
        return k
    assert call(0, good) == 0 and call(1, cgood) == 0
    # 1. the binding as a whole
    assert L.crthip_batch_bind_compact(None, 0, C.byref(good)) == A
    assert call(3, good) == A and b"no such blob" in err()
    for top in (dict(sets=0), dict(sets=5)):
        assert call(0, variant(top=top)) == A and b"sets" in err() and b"blob 0" in err()
    assert call(0, variant(top=dict(flags=1))) == A and b"flag" in err()
    for w in (0, 1):
        assert call(0, variant(top=dict(reserved=w))) == A and b"reserved" in err()
    # 2. set by set
    g0 = good.set[0]
    for s in (0, 1):
        assert call(0, variant(s=s, source=4)) == A and b"unknown source" in err() and ("set %d" % s).encode() in err()
    assert call(0, variant(source=ca.COMPACT_CLOUD_LOD)) == A and b"cloud source on a mesh" in err()
    assert call(1, variant(cgood, source=ca.COMPACT_INDEX)) == A and b"mesh source on a point cloud" in err() and b"blob 1" in err()
    assert call(0, variant(level=2)) == A and b"no such level" in err()
    assert call(1, variant(cgood, level=2)) == A and b"no such level" in err()
    for f in ("newid", "order", "index"):
        assert call(1, variant(cgood, **{f: g0.newid})) == A and b"takes no newid" in err()
        assert call(0, variant(**{f: getattr(g0, f) + 2})) == A and b"not 4-byte aligned" in err()
    assert call(0, variant(counts=g0.counts + 8)) == A and b"counts is not 16-byte aligned" in err()
    assert call(0, variant(newid_capacity=b.infos[0].nvert - 1)) == A and b"newid_capacity" in err()
    assert call(0, variant(newid=None, newid_capacity=0)) == 0
    assert call(0, variant(ngather=9)) == A and b"ngather" in err()
    # 3. gather by gather
    assert call(0, variant(g=1, source=b.infos[0].nattr)) == A and b"out of range" in err() and b"gather 1" in err() and b"set 0" in err()
    assert call(0, variant(g=0, source=ca.COMPACT_COMPUTED_NORMALS)) == A and b"no computed normals" in err()      # (c4_unit's stored normals are bound)
    assert call(0, variant(g=0, source=ca.COMPACT_COMPUTED_TANGENTS)) == A and b"no computed tangents" in err()
    assert call(0, variant(g=0, dst=None)) == A and b"dst is NULL" in err()
    assert call(0, variant(g=0, dst=good.set[0].gather[0].dst + 2)) == A and b"not aligned" in err()
    assert call(0, variant(g=0, dst_stride=8)) == A and b"dst_stride" in err()
    assert call(0, variant(g=0, dst_stride=14)) == A and b"dst_stride" in err()
    assert call(0, variant(g=0, dst_stride=16)) == 0
    # the order: the whole binding, then set 0 whole (its gathers too) before set 1, a set's own words before its gathers, a gather's source before its dst
    assert call(0, variant(source=4, top=dict(sets=0))) == A and b"sets" in err()
    k = variant(s=1, source=4)
    k.set[0].gather[1].dst = None
    assert call(0, k) == A and b"set 0" in err() and b"gather 1" in err()
    k = variant(ngather=9)
    k.set[0].gather[0].dst = None
    assert call(0, k) == A and b"ngather" in err()
    k = variant(g=0, source=99)
    k.set[0].gather[0].dst = None
    assert call(0, k) == A and b"out of range" in err()
    k = variant(source=4, newid=g0.newid + 2)
    assert call(0, k) == A and b"unknown source" in err()
    k = variant(counts=g0.counts + 8, newid_capacity=0)
    assert call(0, k) == A and b"counts" in err()
    # the bindings a set names: missing, or a weld without an index
    w = ca.WeldBinding.from_buffer_copy(b._weld[0][0])
    keep = b._weld[0][1]
    b.bind_weld(0, None)
    assert call(0, good) == A and b"no weld binding" in err() and b"set 1" in err()
    w.index, w.index_capacity = None, 0
    b.bind_weld(0, w, keep)
    assert call(0, good) == A and b"no weld binding with an index" in err()
    assert call(0, variant(top=dict(sets=1))) == 0                                   # (set 1 is not looked at)
    b.bind_lod(0, None)
    assert call(0, good) == A and b"no such level" in err() and b"set 0" in err()
    b.bind_cloud_lod(1, None)
    assert call(1, cgood) == A and b"no such level" in err() and b"blob 1" in err()
    b.close()


def test_refused_formats(ctx):
    """a generic attribute in an integer format, as DOUBLE or as stream values is CRTHIP_E_FORMAT: a work array, not vertex records; unbound: ARGUMENT"""
    import torch
    L = ca.lib()
    b = ca.Batch(ctx, [golden("c4_unit")])
    b.allocate_outputs(fill=FILL)
    nv = b.infos[0].nvert
    kp = attr_no(b, 0, "position")
    spare = torch.zeros(nv * 24 + 256, dtype=torch.uint8, device="cuda:0")
    for fmt, flags, want in ((ca.FMT_INT32, 0, F_), (ca.FMT_DOUBLE, 0, F_), (ca.FMT_INT32, ca.BIND_STREAM_VALUES, F_), (ca.FMT_FLOAT, 0, 0), (None, 0, A)):
        binds = [ca.AttrBinding.from_buffer_copy(b._keep[1][k]) for k in range(b.infos[0].nattr)]
        binds[kp] = ca.AttrBinding(spare.data_ptr(), fmt, 0, 0, flags) if fmt is not None else ca.AttrBinding()
        b.bind(0, binds, b._keep[2][0], ca.FMT_UINT32)
        kb = Compacted(b, {0: [dict(source=ca.COMPACT_INDEX, gathers=[(kp, (12, None), 0, None)])]}, bind=False)
        k = kb.binding(0)
        assert L.crthip_batch_bind_compact(b.handle, 0, C.byref(k)) == want, (fmt, flags, L.crthip_last_error())
        if want:
            assert b"gather 0" in L.crthip_last_error() and b"blob 0" in L.crthip_last_error()
    b.close()


def test_lifetime(ctx):
    """the whole binding is dropped by a later bind of the blob, by a reset, and by any later call that sets, replaces or removes a binding it names"""
    b = ca.Batch(ctx, [golden("c4_unit"), cl.case("cloud_diff").blob, golden("pos_only")])

    def fresh():
        b.allocate_outputs(fill=FILL, lod=(9, 11), cloud_lod=((9, 11), 64), weld=True, computed_normals=True, computed_tangents=True)
        p = lambda i: attr_no(b, i, "position")                                      # noqa: E731
        return Compacted(b, {0: [dict(source=ca.COMPACT_LOD, level=1, has=("record",), gathers=[(ca.COMPACT_COMPUTED_TANGENTS, "tangent", 0, None)]),
                                 dict(source=ca.COMPACT_WELD, has=("record",))],
                             1: [dict(source=ca.COMPACT_CLOUD_LOD, level=0, has=("record",), gathers=[(p(1), "position", 0, None)])],
                             2: [dict(source=ca.COMPACT_INDEX, has=("record",), gathers=[(ca.COMPACT_COMPUTED_NORMALS, "normal", 0, None)])]})

    def bound():
        """which blobs' compaction ran: their records were written"""
        kb.buf[:] = FILL
        import torch
        torch.cuda.synchronize()
        run(b)
        host = kb.buf.cpu().numpy()
        return [i for i in kb.sets if (host[kb.at[i][0]["record"]:kb.at[i][0]["record"] + 16] != FILL).any()]
    kb = fresh()
    assert "tangent" in b.outputs[0] and "normal" in b.outputs[2]
    assert bound() == [0, 1, 2]
    L = ca.lib()
    saved = (dict(b._weld), dict(b._lod), dict(b._cloud_lod))

    def restore():
        """everything allocate_outputs bound, bound again, and the compaction behind it"""
        b._weld, b._lod, b._cloud_lod = (dict(d) for d in saved)
        b._compact = {}
        b.rebind()
        kb.bind()
    steps = [
        (lambda: b.bind_weld(0, b._weld[0][0], b._weld[0][1]), [1, 2]),                                   # the weld set again: blob 0's goes
        (lambda: b.bind_lod(0, None), [1, 2]),
        (lambda: b.bind_lod(0, b._lod[0][0], b._lod[0][1]), [1, 2]),
        (lambda: b.bind_cloud_lod(1, b._cloud_lod[1][0], b._cloud_lod[1][1]), [0, 2]),
        (lambda: b.bind_cloud_lod(1, None), [0, 2]),
        (lambda: b.bind_computed_tangents(0, None), [1, 2]),
        (lambda: b.bind_computed_tangents(0, b._tangents[0][1], b._tangents[0][2]), [1, 2]),
        (lambda: b.bind_computed_normals(2, b._computed[0][1], b._computed[0][2]), [0, 1]),
        (lambda: b.bind_computed_normals(2, None), [0, 1]),
        (lambda: b.bind_compact(1, None), [0, 2]),
        (lambda: b.bind_weld(2, None), [0, 1, 2]),                                                          # (a binding it does not name: it stays)
        (lambda: b.bind_adjacency(0, None), [0, 1, 2]),
    ]
    for n, (step, want) in enumerate(steps):
        restore()
        step()
        assert bound() == want, n
    # a later bind of the blob drops it, and so does a reset
    restore()
    b._compact = {}
    b.rebind()
    assert bound() == []
    restore()
    b.reset([golden("c4_unit")])
    b.allocate_outputs(fill=FILL)
    run(b)
    assert not any(k.startswith("compact") for k in b.kernel_times())
    assert L.crthip_batch_bind_compact(b.handle, 0, None) == 0
    b.close()


# ---- 8. single-stream contexts ----

def test_single_stream_context():
    c = make_ctx(True)
    try:
        b = ca.Batch(c, mix_blobs())
        mb, wb, kb = bind_mix(b)
        run(b)
        kb.check(mix_src(b, mb), "single")
        b.close()
    finally:
        c.close()
