"""GPU (-m gpu): crthip_batch_bind_weld through the C ABI - the kernels against the sequential model of the contract (tests/weld.py), raw bytes.
Every blob's arrays live in one device buffer pre-filled with 0xCD, remap at exactly nvert words, the welded index at exactly 3*nface words, with
poisoned gaps between the arrays: nothing but them and the 16-byte records may change.  The model runs on what the oracle decodes of the blob
(the decode's own index is checked against it where it is bound); which path ran is read from Batch.kernel_times()."""
import ctypes as C
import functools

import numpy as np
import pytest

import adjacency as adj
import corto_amd as ca
import weld as wd
from conftest import CLOUD_CASES, MESH_CASES, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = wd.FILL
A = wd.E_ARGUMENT
E_NEEDS_POSITION = -6                                       # CRTHIP_E_NORMAL_NEEDS_POSITION
BLOB = "weld_blob"
THREE = ("weld_insert", "weld_lookup", "weld_index")
ALL_NAMES = MESH_CASES + wd.HANDMADE


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
    return wd.case(name).blob


class Bound:
    """weld bindings of some blobs of a batch: one poisoned device buffer, every remap array at exactly nvert words and every welded index at
    exactly 3*nface words with poisoned gaps between them; the blobs in `records` (default: all) get a device counts record and the blobs in
    `indexed` (default: all) a welded index, the others none; `flags` a blob (default 0)"""

    def __init__(self, b, blobs, records=None, indexed=None, flags=None, fill=FILL, bind=True):
        import torch
        self.b, self.blobs, self.at, off = b, list(blobs), {}, 0
        self.records = set(self.blobs if records is None else records)
        self.indexed = set(self.blobs if indexed is None else indexed)
        self.flags = dict(flags or {})
        for i in self.blobs:
            o = []
            for n in (b.infos[i].nvert * 4, b.infos[i].nface * 12, 16):
                off = (off + 255) & ~255
                o.append((off, n))
                off += n
            self.at[i] = o
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill
        if bind:
            self.bind()

    def binding(self, i):
        o, base = self.at[i], self.buf.data_ptr()
        return ca.WeldBinding(base + o[0][0], base + o[1][0] if i in self.indexed else None, base + o[2][0] if i in self.records else None,
                              self.b.infos[i].nvert, self.b.infos[i].nface * 3, self.flags.get(i, 0), 0)

    def bind(self):
        for i in self.blobs:
            self.b.bind_weld(i, self.binding(i))

    def read(self):
        """after sync: {blob: (remap, welded index or None, counts or None)}; asserts that nothing but the bound arrays and records changed"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, o in self.at.items():
            untouched[o[0][0]:o[0][0] + o[0][1]] = False
            index = counts = None
            if i in self.indexed:
                untouched[o[1][0]:o[1][0] + o[1][1]] = False
                index = host[o[1][0]:o[1][0] + o[1][1]].view(np.uint32).copy()
            if i in self.records:
                untouched[o[2][0]:o[2][0] + 16] = False
                counts = tuple(int(x) for x in host[o[2][0]:o[2][0] + 16].view(np.uint32))
            res[i] = (host[o[0][0]:o[0][0] + o[0][1]].view(np.uint32).copy(), index, counts)
        assert (host[untouched] == self.fill).all(), "bytes outside the bound arrays and the records were written"
        return res


def same(got, name, tag):
    """got: (remap, index or None, counts or None) of a binding; the model of the named case with or without a welded index"""
    exp = wd.model(name, got[1] is not None)
    wd.assert_same((got[0], got[1], exp[2] if got[2] is None else got[2]), exp, (tag, name))


def index_kw(mode):
    return {"u32": dict(index16=False), "u16": dict(index16=True), "unbound": dict(only={"position"})}[mode]


def expect_ran(b, blob, three, index=True):
    ran = set(k for k in b.kernel_times() if k.startswith("weld"))
    want = ({BLOB} if blob else set()) | (set(THREE if index else THREE[:2]) if three else set())
    assert ran == want, (sorted(ran), sorted(want))


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


# ---- 1. the kernels equal the model: the golden meshes and every hand-made case, every index form ----

@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernels_equal_model(ctx, mode):
    b = ca.Batch(ctx, [blob_of(n) for n in ALL_NAMES])
    b.allocate_outputs(fill=FILL, **index_kw(mode))
    n = len(ALL_NAMES)
    wb = Bound(b, range(n), records=range(0, n, 2), indexed=[i for i in range(n) if i % 3 != 1])
    run(b)
    for i, name in enumerate(ALL_NAMES):
        c = wd.case(name)
        assert (b.infos[i].nvert, b.infos[i].nface) == (c.nvert, c.nface), name
        if mode != "unbound":                                                       # (the model's index is the one this decode left)
            assert (b.host_outputs(i)["index"].astype(np.uint32) == c.index).all(), name
    for i, got in wb.read().items():
        same(got, ALL_NAMES[i], mode)
    expect_ran(b, True, True)                                                       # (grid_8193 is the one blob beyond weld_blob)
    b.close()


# ---- 2. the partition boundary: 8 192 vertices are weld_blob's, 8 193 the three kernels'; with and without a record and an index ----

@pytest.mark.parametrize("name,blob", [("grid_8192", True), ("grid_8193", False), ("far_pairs", True), ("coincident", True)])
@pytest.mark.parametrize("record,index", [(True, True), (False, True), (True, False), (False, False)])
def test_paths(ctx, name, blob, record, index):
    b = ca.Batch(ctx, [blob_of(name)])
    b.allocate_outputs(fill=FILL)
    assert wd.in_blob(b.infos[0].nvert) == blob
    wb = Bound(b, [0], records=[0] if record else [], indexed=[0] if index else [])
    run(b)
    same(wb.read()[0], name, (record, index))
    expect_ran(b, blob, not blob, index)                                            # (without an index weld_index does not run)
    b.close()


@functools.lru_cache(maxsize=None)
def heavy():
    """the three kernels on heavy coincidence: the 9 000 vertices of a grid folded onto 9 positions (both coordinates modulo 3), so that a
    slot's word takes a thousand atomic minima from every workgroup; no face collapses, its corners differ modulo 3"""
    import meshlet_bounds as mb
    import meshlet_edges as me
    P, idx = mb.grid(89, 99, 1)
    return me.Case(me.encode_exact(P % 3, idx))


def test_three_kernels_on_heavy_coincidence(ctx):
    c = heavy()
    assert c.nvert == 9000 and not wd.in_blob(c.nvert) and len(np.unique(c.P, axis=0)) == 9
    exp = wd.build(c.P, c.index)
    b = ca.Batch(ctx, [c.blob])
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, [0])
    run(b)
    assert (b.host_outputs(0)["index"] == c.index).all()
    got = wb.read()[0]
    wd.assert_same(got, exp, "heavy")
    wd.check_properties(c.P, c.index, *got, tag="heavy")
    assert exp[2] == (9000, 9, 0, 0)
    expect_ran(b, False, True)
    b.close()


# ---- 3. the position's own output, whatever its form, is that of a batch without the weld ----

FORMS = ["c4_unit", "nrm_estimated_rgb", "torus", "fields32", "fields31", "pos_only", "seam", "grid_8193"]


def allocate(b, form):
    if form == "strided":
        b.allocate_interleaved(fill=FILL)
    else:
        b.allocate_outputs(fill=FILL, quantized={"position"} if form == "quantized" else ())


@pytest.mark.parametrize("form", ["packed", "strided", "quantized"])
def test_position_forms(ctx, form):
    # (the wide fixtures' spans do not fit uint16 grid values: CRTHIP_BIND_QUANTIZED refuses them, with or without a weld)
    names = [n for n in FORMS if form != "quantized" or n not in wd.GOLDEN_WIDE]
    blobs = [blob_of(n) for n in names]
    p = ca.Batch(ctx, blobs)
    allocate(p, form)
    run(p)
    assert not any(k.startswith("weld") for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(names))]
    transforms = [p.quant_transform(i, "position") for i in range(len(names))] if form == "quantized" else None
    p.close()
    b = ca.Batch(ctx, blobs)
    allocate(b, form)
    wb = Bound(b, range(len(names)))
    run(b)
    for i, got in wb.read().items():
        same(got, names[i], form)
        same_outputs(b.host_outputs(i), plain[i], (form, names[i]))
        if transforms:
            assert bytes(b.quant_transform(i, "position")) == bytes(transforms[i]), names[i]
    expect_ran(b, True, True)
    b.close()


# ---- 4. a mixed batch: bound and unbound blobs, a cloud, both paths; every other output as without the binding; decoded twice ----

MIX = ["two_groups", "cloud_diff", "cube24", "nonmanifold_fins", "seam", "grid_8193", "confetti", "far_pairs"]
MIX_BOUND, MIX_RECORDS, MIX_INDEXED = [0, 2, 4, 5, 7], [0, 5, 7], [2, 4, 5]


def mix_blobs():
    return [load_golden(n)["crt"] if n in CLOUD_CASES else blob_of(n) for n in MIX]


def check_mix(b, wb, plain, tag):
    got = wb.read()
    for i in MIX_BOUND:
        same(got[i], MIX[i], (tag, i))
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), plain[i], (tag, i))


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st = run(p)
    assert not any(k.startswith("weld") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    return ref, st


def test_mixed_batch(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, MIX_BOUND, MIX_RECORDS, MIX_INDEXED)
    st = run(b)
    assert (st == mix_plain[1]).all()
    expect_ran(b, True, True)
    check_mix(b, wb, mix_plain[0], "first")
    first = wb.buf.cpu().numpy().copy()
    # decoded twice in a row: the same bytes over the old ones (the table and the record are started again by the schedule), and over fresh poison
    run(b)
    check_mix(b, wb, mix_plain[0], "again")
    assert wb.buf.cpu().numpy().tobytes() == first.tobytes()
    wb2 = Bound(b, MIX_BOUND, MIX_RECORDS, MIX_INDEXED, fill=0x3C)
    run(b)
    check_mix(b, wb2, mix_plain[0], "other buffers")
    # ... re-planned for other blobs, and back
    b.reset([blob_of("torus"), blob_of("coincident")])
    b.allocate_outputs(fill=FILL)
    wo = Bound(b, [1])
    run(b)
    same(wo.read()[1], "coincident", "reset")
    expect_ran(b, True, False)
    b.reset(mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb3 = Bound(b, MIX_BOUND, MIX_RECORDS, MIX_INDEXED)
    run(b)
    check_mix(b, wb3, mix_plain[0], "back")
    b.close()


def test_allocate_outputs_binds_every_mesh(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, weld=True)
    run(b)
    for i, name in enumerate(MIX):
        same_outputs(b.host_outputs(i), mix_plain[0][i], i)
        if name in CLOUD_CASES:
            assert i not in b._weld
            continue
        same(b.weld(i), name, i)
    expect_ran(b, True, True)
    b.rebind()                                                                      # (rebind applies the bindings again)
    run(b)
    same(b.weld(2), "cube24", "rebind")
    b.close()


def test_decode_with_next_parity_1(mix_plain):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["holey_disc", "c4_unit", "coincident", "grid_8193"]
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        w0 = Bound(objs[0], MIX_BOUND, MIX_RECORDS, MIX_INDEXED)
        objs[1].reset([blob_of(n) for n in other])
        objs[1].allocate_outputs(fill=FILL)
        w1 = Bound(objs[1], range(4), [1, 3])
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_plain[1]).all() and (st1 == 0).all()
        check_mix(objs[0], w0, mix_plain[0], "cur")
        got = w1.read()
        for i, n in enumerate(other):
            same(got[i], n, "next")
            assert (objs[1].host_outputs(i)["index"] == wd.case(n).index).all()
    finally:
        for o in objs:
            o.close()
        c.close()


# ---- 5. CRTHIP_WELD_ADJACENCY: the twins of the welded index ----

class Twins:
    """adjacency bindings beside the weld's: a twin array and a record a blob in one poisoned buffer"""

    def __init__(self, b, blobs):
        import torch
        self.b, self.at, off = b, {}, 0
        for i in blobs:
            self.at[i] = (off, off + ((b.infos[i].nface * 12 + 255) & ~255))
            off = self.at[i][1] + 256
        self.buf = torch.full((off + 256,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def bind(self):
        base = self.buf.data_ptr()
        for i, (to, co) in self.at.items():
            self.b.bind_adjacency(i, ca.AdjacencyBinding(base + to, base + co, self.b.infos[i].nface * 3, 0))

    def read(self, i):
        host = self.buf.cpu().numpy()
        to, co = self.at[i]
        return host[to:to + self.b.infos[i].nface * 12].view(np.uint32).copy(), tuple(int(x) for x in host[co:co + 16].view(np.uint32))


FLAGGED = wd.HANDMADE + MESH_CASES


@functools.lru_cache(maxsize=None)
def welded_twins(name):
    """adjacency's model on the model's welded index of a named case, computed once"""
    return adj.build(wd.model(name)[1].reshape(-1, 3), wd.case(name).nvert)


@functools.lru_cache(maxsize=None)
def own_twins(name):
    return adj.build(wd.case(name).index, wd.case(name).nvert)


@pytest.mark.parametrize("weld_first", [True, False])
def test_weld_adjacency(ctx, weld_first):
    b = ca.Batch(ctx, [blob_of(n) for n in FLAGGED])
    b.allocate_outputs(fill=FILL, only={"position"})
    n = len(FLAGGED)
    wb = Bound(b, range(n), flags={i: ca.WELD_ADJACENCY for i in range(n)}, bind=False)
    tw = Twins(b, range(n))
    for binder in ((wb, tw) if weld_first else (tw, wb)):                            # (the order of the two bind calls does not matter)
        binder.bind()
    run(b)
    got = wb.read()
    for i, name in enumerate(FLAGGED):
        c = wd.case(name)
        same(got[i], name, "flagged")
        twin, counts = tw.read(i)
        adj.assert_same((twin, counts), welded_twins(name), ("welded twins", name))   # adjacency's model on the welded index (`same` above: the model's is the kernels')
        adj.check_properties(got[i][1].reshape(-1, 3), c.nvert, twin, counts, tag=name)
        assert counts[3] == 3 * got[i][2][2], name                                   # invalid == 3 * degenerate
        own = own_twins(name)
        if name == "cube24":                                                         # closed once welded; six lone quads before
            assert counts == (36, 0, 0, 0) and (twin[twin] == np.arange(36)).all() and own[1][1] == 24
        if name == "seam":                                                           # only the outer border of the joined grid remains
            nx, ny = wd.SEAM
            assert counts[1:] == (2 * (2 * nx + ny), 0, 0) and own[1][1] == 2 * 2 * (nx + ny)
        if name == "coincident":
            assert counts == (3 * c.nface, 0, 0, 3 * c.nface) and (twin == adj.NO_TWIN).all()
    # removing the weld binding removes the effect: the blob's own index again
    b.bind_weld(0, None)
    run(b)
    adj.assert_same(tw.read(0), own_twins(FLAGGED[0]), "weld removed")
    # ... and a weld without the flag leaves adjacency alone
    b.bind_weld(0, wb.binding(0))
    wb.flags[1] = 0
    b.bind_weld(1, wb.binding(1))
    run(b)
    adj.assert_same(tw.read(0), welded_twins(FLAGGED[0]), "weld back")
    adj.assert_same(tw.read(1), own_twins(FLAGGED[1]), "unflagged")
    assert welded_twins(FLAGGED[0])[1] != own_twins(FLAGGED[0])[1] and welded_twins(FLAGGED[1])[1] != own_twins(FLAGGED[1])[1]
    # ... nor does the flag without an adjacency binding do anything
    b.bind_adjacency(0, None)
    run(b)
    same(wb.read()[0], FLAGGED[0], "no adjacency")
    b.close()


def test_allocate_outputs_weld_adjacency(ctx):
    b = ca.Batch(ctx, [blob_of("cube24"), blob_of("grid_8193"), blob_of("seam")])
    b.allocate_outputs(fill=FILL, adjacency=True, weld="adjacency")
    run(b)
    assert b.adjacency(0)[1] == (36, 0, 0, 0) and b.weld(0)[2] == (24, 8, 0, 0)
    for i, name in enumerate(["cube24", "grid_8193", "seam"]):
        same(b.weld(i), name, "allocate")
        adj.assert_same(b.adjacency(i), adj.build(b.weld(i)[1].reshape(-1, 3), b.infos[i].nvert), name)
    b.close()


# ---- 6. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    import torch
    L = ca.lib()
    b = ca.Batch(ctx, [blob_of("torus"), load_golden("cloud_diff")["crt"], blob_of("two_groups"), blob_of("c4_unit")])
    b.allocate_outputs(fill=FILL, only={"position"})                                  # (neither the index nor every attribute is bound)
    wb = Bound(b, [0, 2])
    good = wb.binding(0)

    def call(i, w):
        return L.crthip_batch_bind_weld(b.handle, i, C.byref(w) if w is not None else None)

    def variant(**kw):
        w = ca.WeldBinding.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    assert L.crthip_batch_bind_weld(None, 0, C.byref(good)) == A
    assert call(4, good) == A and b"no such blob" in L.crthip_last_error()
    assert call(1, good) == A and b"point cloud" in L.crthip_last_error() and b"blob 1" in L.crthip_last_error()
    for kw, word in ((dict(remap=None), b"remap is NULL"), (dict(remap=good.remap + 2), b"remap is NULL or not 4-byte aligned"),
                     (dict(index=good.index + 2), b"index is not 4-byte aligned"), (dict(counts=good.counts + 8), b"counts is not 16-byte aligned"),
                     (dict(remap_capacity=good.remap_capacity - 1), b"remap_capacity"), (dict(index_capacity=good.index_capacity - 1), b"index_capacity"),
                     (dict(flags=2), b"flag"), (dict(flags=0x80000001), b"flag"), (dict(reserved=1), b"reserved"),
                     (dict(flags=ca.WELD_ADJACENCY, index=None), b"needs index")):
        assert call(0, variant(**kw)) == A, kw
        assert b"blob 0" in L.crthip_last_error() and word in L.crthip_last_error(), (kw, L.crthip_last_error())
    # the errors come in the header's order: the point cloud first, then remap, index and counts, the capacities, the flags, reserved, the flag's index
    assert call(1, variant(remap=None, reserved=1)) == A and b"point cloud" in L.crthip_last_error()
    assert call(0, variant(remap=good.remap + 2, index=good.index + 2, remap_capacity=0, flags=2, reserved=1)) == A and b"remap is NULL" in L.crthip_last_error()
    assert call(0, variant(counts=good.counts + 4, remap_capacity=0, flags=2, reserved=1)) == A and b"counts is not" in L.crthip_last_error()
    assert call(0, variant(index_capacity=0, flags=2, reserved=1)) == A and b"index_capacity" in L.crthip_last_error()
    assert call(0, variant(flags=2, reserved=1)) == A and b"flag" in L.crthip_last_error()
    assert call(0, variant(flags=ca.WELD_ADJACENCY, index=None, reserved=1)) == A and b"reserved" in L.crthip_last_error()
    # every blob is held to its OWN sizes
    assert b.infos[2].nvert < good.remap_capacity and call(2, variant(remap_capacity=b.infos[2].nvert - 1)) == A and b"blob 2" in L.crthip_last_error()
    # the position rule of the meshlet bounds: blob 3's position is not bound
    b.bind(3, [ca.AttrBinding() for _ in range(b.infos[3].nattr)])
    roomy = dict(remap_capacity=0xFFFFFFFF, index_capacity=0xFFFFFFFF)
    assert call(3, variant(**roomy)) == E_NEEDS_POSITION and b"blob 3" in L.crthip_last_error() and b"position" in L.crthip_last_error()
    assert call(3, variant(reserved=1, **roomy)) == A                                          # (the arguments come first)
    for kw in (dict(counts=None), dict(index=None), dict(index=None, index_capacity=0), dict(remap_capacity=good.remap_capacity + 5), dict(index_capacity=0xFFFFFFFF),
               dict(flags=ca.WELD_ADJACENCY)):
        assert call(0, variant(**kw)) == 0, kw
    wb.bind()
    run(b)
    got = wb.read()
    same(got[0], "torus", "torus")
    same(got[2], "two_groups", "two_groups")
    # NULL removes it: the other blob's stays, this one's bytes stay as they are
    assert call(0, None) == 0
    wb.buf[wb.at[0][0][0]:wb.at[0][0][0] + 64] = 0x11
    torch.cuda.synchronize()                                                        # (torch's stream; the decode runs on the context's own)
    run(b)
    after = wb.buf.cpu().numpy()
    assert (after[wb.at[0][0][0]:wb.at[0][0][0] + 64] == 0x11).all()
    expect_ran(b, True, False)
    # a later bind of the blob drops it ...
    b._weld = {}
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


# ---- 7. a batch without the binding: no weld kernel, and the outputs the reference decoder's ----

def test_a_batch_without_the_binding(ctx):
    names = MESH_CASES + CLOUD_CASES
    b = ca.Batch(ctx, [load_golden(n)["crt"] for n in names])
    b.allocate_outputs(fill=0, adjacency=True)                                      # (zeros: a cloud's BORDER normals are never written, as in the reference)
    run(b)
    assert not any(k.startswith("weld") for k in b.kernel_times())
    for i, n in enumerate(names):
        g, out = load_golden(n), b.host_outputs(i)
        for k in set(out) - {"nvert", "nface"}:
            assert out[k].dtype == g[k].dtype and out[k].tobytes() == g[k].tobytes(), (n, k)                         # (the fixtures are the reference decoder's own outputs)
        if n in MESH_CASES:
            adj.assert_same(b.adjacency(i), adj.build(np.asarray(g["index"], np.uint32).reshape(-1, 3), b.infos[i].nvert), n)
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """seven decodes on a single-stream context of 256 C4 units (2 112 vertices each: weld_blob) and of the 131 584-face mesh (the three
    kernels), with the binding and without it: the weld kernels' times and the batch's step time"""
    import time
    from corto_amd import synth
    c = make_ctx(True)
    c4 = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32), with_color=False, with_normal=False))
    big = ca.aligned_blob(ca.encode(synth.bumpy_sphere(256, 257), with_normal=False, with_color=False, with_uv=False))
    for what, blobs in (("256 x 2112 vertices", [c4] * 256), ("1 x 131584 faces", [big])):
        for on in (True, False):
            b = ca.Batch(c, blobs)
            b.allocate_outputs(index16=len(blobs) > 1, weld=on)
            rows, steps = {}, []
            for _ in range(7):
                t0 = time.perf_counter()
                run(b)
                steps.append(round(1e6 * (time.perf_counter() - t0), 1))
                for k, v in b.kernel_times().items():
                    if k.startswith("weld") or k == "fill":
                        rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
            print("\nkernel times (us), 7 decodes of %s, weld %s:" % (what, on), rows)
            print("  step (us, decode + sync, profiling on):", steps)
            if on:
                print("  counts of blob 0:", b.weld(0)[2])
            assert any(k.startswith("weld") for k in rows) == on
            b.close()
    c.close()
