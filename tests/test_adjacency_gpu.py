"""GPU (-m gpu): crthip_batch_bind_adjacency through the C ABI - the kernels against the sequential model of the contract (tests/adjacency.py), raw
bytes.  Every blob's twin array lives in one device buffer pre-filled with 0xCD, at exactly 3*nface words with poisoned gaps between the
arrays: nothing but the twins and the 16-byte records may change.  The model runs on the index the same decode left; which path ran is read
from Batch.kernel_times()."""
import ctypes as C
import functools

import numpy as np
import pytest

import adjacency as adj
import corto_amd as ca
from conftest import CLOUD_CASES, MESH_CASES, load_golden
from corto_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = adj.FILL
A = adj.E_ARGUMENT
BLOB = "adjacency_blob"
FOUR = ("adjacency_count", "adjacency_offsets", "adjacency_fill", "adjacency_twin")


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


@functools.lru_cache(maxsize=None)
def model(name):
    idx, nvert, _ = adj.golden(name)
    exp = adj.build(idx, nvert)
    adj.check_properties(idx, nvert, *exp, tag=(name, "model"))
    return exp


class Bound:
    """adjacency bindings of some blobs of a batch: one poisoned device buffer, every twin array at exactly 3*nface words with poisoned gaps
    between them; the blobs in `records` (default: all) get a device counts record, the others none"""

    def __init__(self, b, blobs, records=None, fill=FILL):
        import torch
        self.b, self.blobs, self.at, off = b, list(blobs), {}, 0
        self.records = set(self.blobs if records is None else records)
        for i in self.blobs:
            o = []
            for n in (b.infos[i].nface * 12, 16):
                off = (off + 255) & ~255
                o.append((off, n))
                off += n
            self.at[i] = o
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill
        self.bind()

    def binding(self, i):
        o, base = self.at[i], self.buf.data_ptr()
        return ca.AdjacencyBinding(base + o[0][0], base + o[1][0] if i in self.records else None, self.b.infos[i].nface * 3, 0)

    def bind(self):
        for i in self.blobs:
            self.b.bind_adjacency(i, self.binding(i))

    def read(self):
        """after sync: {blob: (twin, counts or None)}; asserts that nothing but the twin arrays and the bound records changed"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, o in self.at.items():
            untouched[o[0][0]:o[0][0] + o[0][1]] = False
            counts = None
            if i in self.records:
                untouched[o[1][0]:o[1][0] + 16] = False
                counts = tuple(int(x) for x in host[o[1][0]:o[1][0] + 16].view(np.uint32))
            res[i] = (host[o[0][0]:o[0][0] + o[0][1]].view(np.uint32).copy(), counts)
        assert (host[untouched] == self.fill).all(), "bytes outside the twin arrays and the records were written"
        return res


def same(got, exp, tag):
    """got: (twin, counts or None) of a binding; exp: the model's"""
    adj.assert_same((got[0], exp[1] if got[1] is None else got[1]), exp, tag)


def index_kw(mode):
    return {"u32": dict(index16=False), "u16": dict(index16=True), "unbound": dict(only={"position"})}[mode]


def expect_ran(b, blob, four):
    ran = set(k for k in b.kernel_times() if k.startswith("adjacency"))
    assert ran == ({BLOB} if blob else set()) | (set(FOUR) if four else set()), sorted(ran)


# ---- 1. the kernels equal the model: the golden meshes, every index form ----

@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernels_equal_model(ctx, mode):
    b = ca.Batch(ctx, [adj.golden(n)[2] for n in MESH_CASES])
    b.allocate_outputs(fill=FILL, **index_kw(mode))
    ab = Bound(b, range(len(MESH_CASES)), records=range(0, len(MESH_CASES), 2))
    run(b)
    if mode != "unbound":                                                           # (the model's index is the one this decode left)
        for i, n in enumerate(MESH_CASES):
            assert (b.host_outputs(i)["index"].astype(np.uint32) == adj.golden(n)[0]).all(), n
    for i, got in ab.read().items():
        same(got, model(MESH_CASES[i]), (mode, MESH_CASES[i]))
    assert all(adj.in_blob(adj.golden(n)[1], len(adj.golden(n)[0])) for n in MESH_CASES)
    expect_ran(b, True, False)
    b.close()


# ---- 2. both paths on bigger meshes: a C4 unit, the two shapes at adjacency_blob's limit, vertex ids beyond 16 bits ----

# bumpy_sphere(64, n) has 64*(n + 1) vertices and 128*n faces: 1 024*n + 272 bytes of lists, within 64 KiB up to n = 63
SHAPES = {"c4_unit": (64, 32), "largest_blob": (64, 63), "smallest_four_kernels": (64, 64), "ids_past_16_bits": (256, 257)}


@functools.lru_cache(maxsize=None)
def big(name):
    return ca.aligned_blob(ca.encode(synth.bumpy_sphere(*SHAPES[name]), with_normal=False, with_color=False, with_uv=False))


@pytest.mark.parametrize("name,nvert,nface,blob", [("c4_unit", 2112, 4096, True), ("largest_blob", 4096, 8064, True),
                                                    ("smallest_four_kernels", 4160, 8192, False), ("ids_past_16_bits", 66048, 131584, False)])
@pytest.mark.parametrize("record", [True, False])
def test_paths_on_bigger_meshes(ctx, name, nvert, nface, blob, record):
    b = ca.Batch(ctx, [big(name)])
    b.allocate_outputs(fill=FILL)
    assert (b.infos[0].nvert, b.infos[0].nface) == (nvert, nface) and adj.in_blob(nvert, nface) == blob
    if name == "largest_blob":
        assert adj.blob_lds(nvert, nface) <= adj.BLOB_LDS_MAX < adj.blob_lds(nvert + 64, nface + 128)
    ab = Bound(b, [0], records=[0] if record else [])
    run(b)
    idx = b.host_outputs(0)["index"]
    got = ab.read()[0]
    if name == "ids_past_16_bits":
        assert idx.max() >= 65536
    exp = adj.build(idx, nvert)
    same(got, exp, name)
    adj.check_properties(idx, nvert, got[0], exp[1], tag=name)
    assert exp[1][2:] == (0, 0) and 0 < exp[1][1] < 3 * nface                        # (an oriented grid with a seam: a border, no duplicate, no invalid face)
    expect_ran(b, blob, not blob)
    b.close()


# ---- 3. a mixed batch: bound and unbound blobs, a cloud, both paths; every other output as without the binding ----

MIX = ["two_groups", "cloud_diff", "torus", "nonmanifold_fins", "icosphere", "confetti"]           # ... and smallest_four_kernels behind them
MIX_BOUND, MIX_RECORDS = [0, 3, 5, 6], [0, 6]


def mix_blobs():
    return [load_golden(n)["crt"] for n in MIX] + [big("smallest_four_kernels")]


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


def mix_model(b, i):
    if i < len(MIX):
        return model(MIX[i])
    return mix_model_big(b.host_outputs(i)["index"].tobytes())


@functools.lru_cache(maxsize=None)
def mix_model_big(index_bytes):
    return adj.build(np.frombuffer(index_bytes, np.uint32).reshape(-1, 3), 4160)


def check_mix(b, ab, plain, tag):
    got = ab.read()
    for i in MIX_BOUND:
        same(got[i], mix_model(b, i), (tag, i))
    for i in range(len(MIX) + 1):
        same_outputs(b.host_outputs(i), plain[i], (tag, i))


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st = run(p)
    assert not any(k.startswith("adjacency") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX) + 1)]
    p.close()
    return ref, st


def test_mixed_batch(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    ab = Bound(b, MIX_BOUND, MIX_RECORDS)
    st = run(b)
    assert (st == mix_plain[1]).all()
    expect_ran(b, True, True)
    check_mix(b, ab, mix_plain[0], "first")
    first = ab.buf.cpu().numpy().copy()
    # decoded twice in a row: the same bytes over the old ones (the ends and the records are zeroed again by the schedule), and over fresh poison
    run(b)
    check_mix(b, ab, mix_plain[0], "again")
    assert ab.buf.cpu().numpy().tobytes() == first.tobytes()
    ab2 = Bound(b, MIX_BOUND, MIX_RECORDS, fill=0x3C)
    run(b)
    check_mix(b, ab2, mix_plain[0], "other buffers")
    # ... re-planned for other blobs, and back
    b.reset([adj.golden("torus")[2], adj.golden("decimated")[2]])
    b.allocate_outputs(fill=FILL)
    ao = Bound(b, [1])
    run(b)
    same(ao.read()[1], model("decimated"), "reset decimated")
    expect_ran(b, True, False)
    b.reset(mix_blobs())
    b.allocate_outputs(fill=FILL)
    ab3 = Bound(b, MIX_BOUND, MIX_RECORDS)
    run(b)
    check_mix(b, ab3, mix_plain[0], "back")
    b.close()


def test_allocate_outputs_binds_every_mesh(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, adjacency=True)
    run(b)
    for i in range(len(MIX) + 1):
        same_outputs(b.host_outputs(i), mix_plain[0][i], i)
        if i < len(MIX) and MIX[i] in CLOUD_CASES:
            assert i not in b._adjacency
            continue
        same(b.adjacency(i), mix_model(b, i), i)
    expect_ran(b, True, True)
    b.close()


def test_decode_with_next_parity_1(mix_plain):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["holey_disc", "c4_unit", "nonmanifold_glued"]
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        a0 = Bound(objs[0], MIX_BOUND, MIX_RECORDS)
        objs[1].reset([adj.golden(n)[2] for n in other] + [big("smallest_four_kernels")])
        objs[1].allocate_outputs(fill=FILL)
        a1 = Bound(objs[1], range(4), [1, 3])
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_plain[1]).all() and (st1 == 0).all()
        check_mix(objs[0], a0, mix_plain[0], "cur")
        got = a1.read()
        for i, n in enumerate(other):
            same(got[i], model(n), ("next", n))
            assert (objs[1].host_outputs(i)["index"] == adj.golden(n)[0]).all()
        same(got[3], mix_model_big(objs[1].host_outputs(3)["index"].tobytes()), "next, four kernels")
    finally:
        for o in objs:
            o.close()
        c.close()


def test_a_resident_batch(ctx, mix_plain):
    import torch
    blobs = mix_blobs()
    offs, total = ca.arena_layout([len(x) for x in blobs])
    host = np.zeros(int(total) + 16, dtype=np.uint8)
    for x, o in zip(blobs, offs):
        host[int(o):int(o) + len(x)] = x
    buf = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    b = ca.Batch.resident(ctx, buf, offs, [len(x) for x in blobs])
    b.allocate_outputs(fill=FILL)
    ab = Bound(b, MIX_BOUND, MIX_RECORDS)
    run(b)
    expect_ran(b, True, True)
    check_mix(b, ab, mix_plain[0], "resident")
    b.close()


# ---- 4. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    import torch
    L = ca.lib()
    b = ca.Batch(ctx, [adj.golden("torus")[2], load_golden("cloud_diff")["crt"], adj.golden("two_groups")[2]])
    b.allocate_outputs(fill=FILL, only={"position"})                                  # (neither the index nor every attribute is bound)
    ab = Bound(b, [0, 2])
    good = ab.binding(0)

    def call(i, a):
        return L.crthip_batch_bind_adjacency(b.handle, i, C.byref(a) if a is not None else None)

    def variant(**kw):
        a = ca.AdjacencyBinding.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.crthip_batch_bind_adjacency(None, 0, C.byref(good)) == A
    assert call(3, good) == A and b"no such blob" in L.crthip_last_error()
    assert call(1, good) == A and b"point cloud" in L.crthip_last_error() and b"blob 1" in L.crthip_last_error()
    for kw, word in ((dict(twin=None), b"aligned"), (dict(twin=good.twin + 2), b"aligned"), (dict(counts=good.counts + 8), b"aligned"), (dict(reserved=1), b"reserved"),
                     (dict(capacity=good.capacity - 1), b"capacity")):
        assert call(0, variant(**kw)) == A, kw
        assert b"blob 0" in L.crthip_last_error() and word in L.crthip_last_error(), (kw, L.crthip_last_error())
    # the errors come in the header's order: the point cloud before the pointers, the pointers before reserved, reserved before the capacity
    assert call(1, variant(twin=good.twin + 2, reserved=1, capacity=0)) == A and b"point cloud" in L.crthip_last_error()
    assert call(0, variant(twin=good.twin + 2, reserved=1, capacity=0)) == A and b"aligned" in L.crthip_last_error()
    assert call(0, variant(reserved=1, capacity=0)) == A and b"reserved" in L.crthip_last_error()
    # every blob is held to its OWN index
    assert 3 * b.infos[2].nface < good.capacity and call(2, variant(capacity=3 * b.infos[2].nface - 1)) == A and b"blob 2" in L.crthip_last_error()
    for kw in (dict(counts=None), dict(capacity=good.capacity + 5), dict(capacity=0xFFFFFFFF)):
        assert call(0, variant(**kw)) == 0, kw
    ab.bind()
    run(b)
    got = ab.read()
    same(got[0], model("torus"), "torus")
    same(got[2], model("two_groups"), "two_groups")
    # NULL removes it: the other blob's stays, this one's bytes stay as they are
    assert call(0, None) == 0
    ab.buf[ab.at[0][0][0]:ab.at[0][0][0] + 64] = 0x11
    torch.cuda.synchronize()                                                        # (torch's stream; the decode runs on the context's own)
    run(b)
    after = ab.buf.cpu().numpy()
    assert (after[ab.at[0][0][0]:ab.at[0][0][0] + 64] == 0x11).all()
    expect_ran(b, True, False)
    # a later bind of the blob drops it ...
    b._adjacency = {}
    b.rebind()                                                                      # (crthip_batch_bind_all: every blob bound again)
    run(b)
    expect_ran(b, False, False)
    # ... and so does a reset
    ab.bind()
    b.reset([adj.golden("torus")[2]])
    b.allocate_outputs(fill=FILL)
    run(b)
    expect_ran(b, False, False)
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """seven decodes on a single-stream context of 256 C4 units (4 096 faces each: adjacency_blob) and of the 131 584-face mesh (the four
    kernels), with the binding and without it: the adjacency kernels' times and the batch's step time"""
    import time
    c = make_ctx(True)
    c4 = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32), with_color=False, with_normal=False))
    for what, blobs in (("256 x 4096 faces", [c4] * 256), ("1 x 131584 faces", [big("ids_past_16_bits")])):
        for on in (True, False):
            b = ca.Batch(c, blobs)
            b.allocate_outputs(index16=len(blobs) > 1, adjacency=on)
            rows, steps = {}, []
            for _ in range(7):
                t0 = time.perf_counter()
                run(b)
                steps.append(round(1e6 * (time.perf_counter() - t0), 1))
                for k, v in b.kernel_times().items():
                    if k.startswith("adjacency") or k == "fill":
                        rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
            print("\nkernel times (us), 7 decodes of %s, adjacency %s:" % (what, on), rows)
            print("  step (us, decode + sync, profiling on):", steps)
            if on:
                print("  counts of blob 0:", b.adjacency(0)[1])
            assert any(k.startswith("adjacency") for k in rows) == on
            b.close()
    c.close()
