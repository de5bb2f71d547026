"""GPU (-m gpu): crthip_batch_bind_bvh through the C ABI - the kernels against the sequential model of the contract (tests/bvh.py), raw bytes.
Every blob's arrays live in one device buffer pre-filled with 0xCD, the nodes at exactly 2*nface - 1 records, the parents at as many words, the
order at exactly nface words, with poisoned gaps between the arrays: nothing but those and the 16-byte records may change.  The model runs on
what the oracle decodes of the blob (the decode's own index is checked against it where it is bound); which path ran is read from
Batch.kernel_times().  Valid blobs hold no absent face: tests/test_bvh_cpu.py covers those."""
import ctypes as C
import functools

import numpy as np
import pytest

import corto_amd as ca
import bvh
import meshlet_edges as me
from conftest import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = 0xCD
A = -8                                                      # CRTHIP_E_ARGUMENT
E_NEEDS_POSITION = -6                                       # CRTHIP_E_NORMAL_NEEDS_POSITION
BLOB = "bvh_blob"
BIG = ("bvh_boxes", "bvh_keys", "bvh_sort_count", "bvh_sort_offsets", "bvh_sort_scatter", "bvh_tree", "bvh_refit")

HANDMADE = {
    "one": lambda: bvh.strip(1, seed=1), "two": lambda: bvh.lattice(1), "lattice": lambda: bvh.lattice(12),
    "f4096": lambda: bvh.lattice(32, m=64),                 # bvh_blob's last face count ...
    "f4097": lambda: bvh.lattice(32, m=64, extra=1),        # ... and the other partition's first: two sort tiles and one pair
    "f4160": lambda: bvh.lattice(40, m=52),                 # about two sort tiles
}
NAMES = ["one", "two", "lattice", "c4_unit", "f4096", "f4097", "f4160"]


@functools.lru_cache(maxsize=None)
def case(name):
    return me.Case(me.encode_exact(*HANDMADE[name]()) if name in HANDMADE else load_golden(name)["crt"])


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's result on a named case, computed once and never changed"""
    c = case(name)
    exp = bvh.build(c.P, c.index)
    bvh.check(c.P, c.index, exp[0], exp[1], exp[2], exp[3])
    return exp


def blob_of(name):
    return case(name).blob


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    c.set_profiling(True)
    yield c
    c.close()


def run(b):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return st


class Bound:
    """BVH bindings of some blobs of a batch: one poisoned device buffer, a blob's nodes at exactly 2*nface - 1 records, its parents, its order
    at exactly nface words and its record, with poisoned gaps between them.  parts: {blob: a string of the optional arrays it binds, of "p"
    (parent), "o" (order), "c" (counts)}"""

    def __init__(self, b, parts, fill=FILL, bind=True):
        import torch
        self.b, self.parts, self.at, off = b, dict(parts), {}, 0
        for i in self.parts:
            nf = b.infos[i].nface
            o = []
            for n in ((2 * nf - 1) * 32, (2 * nf - 1) * 4, nf * 4, 16):
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
        base, o, nf, has = self.buf.data_ptr(), self.at[i], self.b.infos[i].nface, self.parts[i]
        return ca.BvhBinding(base + o[0][0], base + o[1][0] if "p" in has else None, base + o[2][0] if "o" in has else None,
                             base + o[3][0] if "c" in has else None, 2 * nf - 1, nf, 0, 0)

    def bind(self):
        for i in self.parts:
            self.b.bind_bvh(i, self.binding(i))

    def read(self):
        """after sync: {blob: (nodes, parent or None, order or None, counts or None)}; asserts that nothing but the bound arrays changed"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, o in self.at.items():
            got = []
            for k, (what, dt) in enumerate((("n", bvh.NODE), ("p", np.uint32), ("o", np.uint32), ("c", np.uint32))):
                if what == "n" or what in self.parts[i]:
                    untouched[o[k][0]:o[k][0] + o[k][1]] = False
                    got.append(host[o[k][0]:o[k][0] + o[k][1]].view(dt).copy())
                else:
                    got.append(None)
            res[i] = (got[0], got[1], got[2], None if got[3] is None else tuple(int(x) for x in got[3]))
        assert (host[untouched] == self.fill).all(), "bytes outside the nodes, the parents, the order and the records were written"
        return res


def check(wb, names, tag):
    """every bound blob's arrays against the model; names: {blob: case}"""
    got = wb.read()
    for i, (nodes, parent, order, counts) in got.items():
        exp = model(names[i])
        if nodes.tobytes() != exp[0].tobytes():
            bad = int(np.flatnonzero(nodes != exp[0])[0])
            raise AssertionError("%s: node %d differs: got %s expected %s" % ((tag, names[i]), bad, nodes[bad], exp[0][bad]))
        assert parent is None or parent.tobytes() == exp[1].tobytes(), (tag, names[i], "parent")
        assert order is None or order.tobytes() == exp[2].tobytes(), (tag, names[i], "order")
        assert counts is None or counts == exp[3], (tag, names[i], counts, exp[3])
    return got


def index_kw(mode):
    return {"u32": dict(index16=False), "u16": dict(index16=True), "unbound": dict(only={"position"})}[mode]


def expect_ran(b, blob, big):
    ran = set(k for k in b.kernel_times() if k.startswith("bvh"))
    want = ({BLOB} if blob else set()) | (set(BIG) if big else set())
    assert ran == want, (sorted(ran), sorted(want))


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


PARTS = ["poc", "", "p", "o", "c", "poc", "oc"]              # NAMES' optional arrays: each present and absent on both partitions


# ---- 1. the kernels equal the model: 1 and 2 faces, a lattice, both sides of the partition, about two tiles; every index form ----

@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernels_equal_model(ctx, mode):
    b = ca.Batch(ctx, [blob_of(n) for n in NAMES])
    b.allocate_outputs(fill=FILL, **index_kw(mode))
    assert [b.infos[i].nface for i in range(len(NAMES))] == [1, 2, 288, 4096, 4096, 4097, 4160]
    wb = Bound(b, dict(enumerate(PARTS)))
    run(b)
    for i, name in enumerate(NAMES):
        if mode != "unbound":                                                       # (the model's index is the one this decode left)
            assert (b.host_outputs(i)["index"].astype(np.uint32) == case(name).index).all(), name
    got = check(wb, dict(enumerate(NAMES)), mode)
    assert got[0][3] == (1, 1, 0, 0) and got[5][3][:3] == (8193, 4097, 0)
    expect_ran(b, True, True)
    b.close()


@pytest.mark.parametrize("name,blob", [("f4096", True), ("f4097", False)])
@pytest.mark.parametrize("parts", ["poc", ""])
def test_paths(ctx, name, blob, parts):
    b = ca.Batch(ctx, [blob_of(name)])
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, {0: parts})
    run(b)
    check(wb, {0: name}, (name, parts))
    expect_ran(b, blob, not blob)
    b.close()


# ---- 2. the position's own output, whatever its form, is that of a batch without the binding ----

FORMS = ["lattice", "c4_unit", "f4097"]


def allocate(b, form):
    if form == "strided":
        b.allocate_interleaved(fill=FILL)
    else:
        b.allocate_outputs(fill=FILL, quantized={"position"} if form == "quantized" else ())


@pytest.mark.parametrize("form", ["packed", "strided", "quantized"])
def test_position_forms(ctx, form):
    blobs = [blob_of(n) for n in FORMS]
    p = ca.Batch(ctx, blobs)
    allocate(p, form)
    run(p)
    assert not any(k.startswith("bvh") for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(FORMS))]
    transforms = [p.quant_transform(i, "position") for i in range(len(FORMS))] if form == "quantized" else None
    p.close()
    b = ca.Batch(ctx, blobs)
    allocate(b, form)
    wb = Bound(b, {i: "poc" for i in range(len(FORMS))})
    run(b)
    check(wb, dict(enumerate(FORMS)), form)
    for i in range(len(FORMS)):
        same_outputs(b.host_outputs(i), plain[i], (form, FORMS[i]))
        if transforms:
            assert bytes(b.quant_transform(i, "position")) == bytes(transforms[i]), FORMS[i]
    expect_ran(b, True, True)
    b.close()


# ---- 3. a mixed batch: bound and unbound blobs, a cloud, both paths; every other output as without the binding; decoded twice ----

MIX = ["two_groups", "cloud_diff", "c4_unit", "f4097", "lattice", "f4160", "nrm_diff"]
MIX_PARTS = {2: "poc", 3: "pc", 5: "o", 6: "poc"}
MIX_NAMES = dict(enumerate(MIX))


def mix_blobs():
    return [load_golden(n)["crt"] if n == "cloud_diff" else blob_of(n) for n in MIX]


def check_mix(b, wb, plain, tag):
    check(wb, MIX_NAMES, tag)
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), plain[i], (tag, i))


def test_mixed_batch(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st0 = run(p)
    assert not any(k.startswith("bvh") for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    wb = Bound(b, MIX_PARTS)
    st = run(b)
    assert (st == st0).all()
    expect_ran(b, True, True)
    check_mix(b, wb, plain, "first")
    first = wb.buf.cpu().numpy().copy()
    # decoded twice in a row: the same bytes over the old ones (the extent and the arrival counters are started again by the schedule) ...
    run(b)
    check_mix(b, wb, plain, "again")
    assert wb.buf.cpu().numpy().tobytes() == first.tobytes()
    # ... and over fresh poison
    wb2 = Bound(b, MIX_PARTS, fill=0x3C)
    run(b)
    check_mix(b, wb2, plain, "other buffers")
    # NULL removes one blob's binding: the others stay, its bytes stay as they are
    import torch
    b.bind_bvh(3, None)
    o = wb2.at[3][0][0]
    wb2.buf[o:o + 64] = 0x11
    torch.cuda.synchronize()                                                        # (torch's stream; the decode runs on the context's own)
    run(b)
    assert (wb2.buf.cpu().numpy()[o:o + 64] == 0x11).all()
    expect_ran(b, True, True)                                                       # (f4160 is still beyond bvh_blob)
    b.bind_bvh(5, None)
    run(b)
    expect_ran(b, True, False)
    b.close()


def test_allocate_outputs_binds_every_mesh(ctx):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, bvh=True)
    run(b)
    for i, name in enumerate(MIX):
        if name == "cloud_diff":
            assert i not in b._bvh
            continue
        nodes, parent, order, counts = b.bvh(i)
        exp = model(name)
        assert nodes.tobytes() == exp[0].tobytes() and parent.tobytes() == exp[1].tobytes() and order.tobytes() == exp[2].tobytes() and counts == exp[3], name
    expect_ran(b, True, True)
    b.rebind()                                                                      # (rebind applies the bindings again)
    run(b)
    assert b.bvh(3)[0].tobytes() == model("f4097")[0].tobytes()
    b.close()


# ---- 4. bind-time errors, in the header's order, and lifetime ----

def test_errors_and_lifetime(ctx):
    L = ca.lib()
    b = ca.Batch(ctx, [blob_of("lattice"), load_golden("cloud_diff")["crt"], blob_of("two"), blob_of("c4_unit")])
    b.allocate_outputs(fill=FILL, only={"position"})                                  # (neither the index nor every attribute is bound)
    wb = Bound(b, {0: "poc", 2: "poc"}, bind=False)
    good = wb.binding(0)
    err = L.crthip_last_error

    def call(i, v):
        return L.crthip_batch_bind_bvh(b.handle, i, C.byref(v) if v is not None else None)

    def variant(**kw):
        v = ca.BvhBinding.from_buffer_copy(good)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    assert L.crthip_batch_bind_bvh(None, 0, C.byref(good)) == A
    assert call(4, good) == A and b"no such blob" in err()
    assert call(1, good) == A and b"point cloud" in err() and b"blob 1" in err()
    for kw, word in ((dict(nodes=None), b"nodes is NULL"), (dict(nodes=good.nodes + 8), b"nodes is NULL or not 16-byte aligned"),
                     (dict(parent=good.parent + 2), b"not 4-byte aligned"), (dict(order=good.order + 1), b"not 4-byte aligned"),
                     (dict(counts=good.counts + 8), b"counts is not 16-byte aligned"), (dict(node_capacity=good.node_capacity - 1), b"node_capacity"),
                     (dict(order_capacity=good.order_capacity - 1), b"order_capacity"), (dict(flags=1), b"flags or reserved"), (dict(reserved=1), b"flags or reserved")):
        assert call(0, variant(**kw)) == A, kw
        assert b"blob 0" in err() and word in err(), (kw, err())
    # the errors come in the header's order: the point cloud, nodes, the optional arrays' alignment, the two capacities, flags and reserved
    assert call(1, variant(nodes=None)) == A and b"point cloud" in err()
    assert call(0, variant(nodes=None, parent=good.parent + 2, node_capacity=0, order_capacity=0, flags=1)) == A and b"nodes is NULL" in err()
    assert call(0, variant(parent=good.parent + 2, node_capacity=0, order_capacity=0, flags=1)) == A and b"not 4-byte aligned" in err()
    assert call(0, variant(node_capacity=0, order_capacity=0, flags=1)) == A and b"node_capacity" in err()
    assert call(0, variant(order_capacity=0, flags=1)) == A and b"order_capacity" in err()
    # an order capacity counts only with an order; more room is fine
    for v in (variant(order=None, order_capacity=0), variant(parent=None), variant(counts=None), variant(node_capacity=0xFFFFFFFF, order_capacity=0xFFFFFFFF)):
        assert call(0, v) == 0
    # every blob is held to its OWN sizes
    assert call(3, good) == A and b"node_capacity" in err() and b"blob 3" in err()
    # the weld's position rule: blob 3's position is not bound
    b.bind(3, [ca.AttrBinding() for _ in range(b.infos[3].nattr)])
    roomy = variant(node_capacity=0xFFFFFFFF, order_capacity=0xFFFFFFFF)
    assert call(3, roomy) == E_NEEDS_POSITION and b"blob 3" in err() and b"position" in err()
    roomy.reserved = 1
    assert call(3, roomy) == A                                                      # (the arguments come first)
    wb.bind()
    run(b)
    check(wb, {0: "lattice", 2: "two"}, "bound")
    expect_ran(b, True, False)
    # a later bind of the blob drops it ...
    b._bvh = {}
    b.rebind()                                                                      # (crthip_batch_bind_all: every blob bound again)
    run(b)
    expect_ran(b, False, False)
    # ... and so does a reset
    wb.bind()
    b.reset([blob_of("lattice")])
    b.allocate_outputs(fill=FILL)
    run(b)
    expect_ran(b, False, False)
    b.close()
