"""crthip_batch_bind_compact without a device: the kernels' source on the host (corto_amd.compact_model: csrc/compact.h in both of k_compact.hip's
partitions and its gather, workgroups, threads and so every atomic's order shuffled by a seed) against the sequential model of the contract
(tests/compact.py), byte for byte; the properties every result has whatever the model says; the capacities, with the words behind them keeping
their fill byte; the gathers at every copy unit.  The bind call's errors need a device batch: tests/test_compact_gpu.py."""
import numpy as np
import pytest

import corto_amd as ca
import compact as cp

SEEDS = (0, 7, 12345)


def both_partitions(src, nvert, tag, seeds=SEEDS, faces=None, **caps):
    """the hook in both partitions equals the model; the words behind what is written keep the fill.  Returns the model's result"""
    exp = cp.build(src, nvert, faces=faces, **caps)
    cp.check_properties(src, nvert, exp[0], exp[1], exp[2], exp[3], faces=faces, tag=(tag, "model"))
    nface = len(src) // 3
    for which in (0, 1):
        if which == 0 and not cp.in_blob(nvert, nface):
            with pytest.raises(ca.CortoError):                       # (the decode sends such a set down the other path)
                ca.compact_model(src, nvert, which=0)
            continue
        for seed in seeds:
            newid, order, index, counts = ca.compact_model(src, nvert, faces=faces, which=which, seed=seed, **caps)
            used, F = counts.used, counts.faces
            nord, nidx = min(used, len(order)), min(3 * F, len(index))
            assert (order[nord:] == cp.FILL32).all(), (tag, which, seed, "the order tail was written")
            assert (index[nidx:] == cp.FILL32).all(), (tag, which, seed, "the index tail was written")
            cp.assert_same((newid, order[:nord], index[:nidx], counts), exp, (tag, which, seed))
            cp.check_properties(src, nvert, newid, order[:nord], index[:nidx], counts.as_tuple(), faces=faces, tag=(tag, which, seed))
    return exp


# ---- 1. hook equals model: the mask words' and the blocks' ends; all, none, only the last; unusable ids ----

@pytest.mark.parametrize("name", cp.NAMED)
def test_hook_equals_model(name):
    src, nvert = cp.named(name)
    exp = both_partitions(src, nvert, name)
    kind = name.rsplit("_", 1)[0]
    if kind == "all":
        assert exp[3][1] == nvert and (exp[0] == np.arange(nvert)).all()
    if kind == "none":
        assert exp[3][1:3] == (0, 0) and (exp[0] == cp.NO_VERTEX).all()
    if kind == "last":
        assert exp[3][1] == 1 and exp[0][nvert - 1] == 0 and list(exp[4]) == [nvert - 1]
    if kind == "bad":
        assert (exp[2][::4] == cp.NO_VERTEX).all() and exp[3][1] < nvert + 1


@pytest.mark.parametrize("nvert", [33, 257])
def test_uint16_source(nvert):
    src, _ = cp.named("half_%d" % nvert)
    both_partitions(src.astype(np.uint16), nvert, ("u16", nvert), seeds=(3,))


def test_the_id_0xffffffff_itself():
    src = np.array([0, cp.NO_VERTEX, 2, cp.NO_VERTEX, cp.NO_VERTEX, cp.NO_VERTEX], np.uint32)
    exp = both_partitions(src, 3, "no_vertex")
    assert list(exp[0]) == [0, cp.NO_VERTEX, 1] and list(exp[2]) == [0, cp.NO_VERTEX, 1] + [cp.NO_VERTEX] * 3


@pytest.mark.parametrize("faces", [0, 1, 100, 254])
def test_faces_from_the_record(faces):
    """a LOD level's list: 3*faces of the bound's words are read, the rest is not - it holds ids that would mark other vertices"""
    src = cp.strip(256).copy()
    both_partitions(src, 256, ("faces", faces), faces=faces)
    assert cp.build(src, 256, faces=faces)[3][1] == (faces + 2 if faces else 0)


@pytest.mark.parametrize("name,nvert", [("two_rounds", 65537), ("beyond_blob", 8193), ("blob_edge", 8192)])
def test_partitions_at_their_edges(name, nvert):
    """8 192 | 8 193 vertices: the last set of compact_blob and the first beyond; 65 537 vertices are 257 blocks, two rounds of compact_offsets"""
    rng = np.random.default_rng(5)
    src = rng.integers(0, nvert, size=3 * 3000).astype(np.uint32)
    src[-1] = nvert - 1
    both_partitions(src, nvert, name, seeds=(1,))


# ---- 2. capacities clip: 0, used - 1, used, used + 1 ----

@pytest.mark.parametrize("which_cap", ["vertex", "index"])
@pytest.mark.parametrize("delta", ["zero", -1, 0, 1])
def test_capacities_clip(which_cap, delta):
    src, nvert = cp.named("half_257")
    full = cp.build(src, nvert)
    total = full[3][1] if which_cap == "vertex" else len(src)
    cap = 0 if delta == "zero" else total + delta
    caps = {"vertex_capacity": cap} if which_cap == "vertex" else {"index_capacity": cap}
    exp = both_partitions(src, nvert, (which_cap, delta), **caps)
    assert exp[3][3] == int(cap < total) and exp[3][1] == full[3][1] and exp[3][2] == full[3][2]


# ---- 3. the gathers: every element size, packed and strided on both sides, every copy unit, an interleaved record ----

def aligned_bytes(n, offset, rng=None):
    """n bytes that start `offset` bytes behind a 16-byte boundary, inside a block of their own"""
    block = np.full(n + 32, cp.FILL, np.uint8)
    a = (-block.ctypes.data) % 16 + offset
    view = block[a:a + n]
    if rng is not None:
        view[:] = rng.integers(0, 256, size=n, dtype=np.uint8)
    return view


def run_gather(E, sstride, dstride, soff, doff, which, vcap=None, nvert=300):
    rng = np.random.default_rng(E * 131 + sstride + dstride + soff + doff)
    src, _ = cp.named("half_%d" % nvert)
    exp = cp.build(src, nvert, vertex_capacity=vcap, ngather=1)
    S, D = sstride or E, dstride or E
    vc = nvert if vcap is None else vcap
    source = aligned_bytes(nvert * S, soff, rng)
    dest = aligned_bytes(vc * D, doff)
    _, _, _, counts = ca.compact_model(src, nvert, which=which, seed=E, newid=False, order=which == 1, index=False, vertex_capacity=vcap,
                                       gathers=[(source, E, sstride, dest, dstride)])
    assert counts.as_tuple() == exp[3]
    want = np.full(vc * D, cp.FILL, np.uint8)
    g = cp.gathered(source, exp[4], E, S, vc)
    for j in range(len(g)):
        want[j * D:j * D + E] = g[j]
    assert dest.tobytes() == want.tobytes(), (E, sstride, dstride, soff, doff, which)


@pytest.mark.parametrize("E", [3, 4, 6, 8, 12, 16])
@pytest.mark.parametrize("which", [0, 1])
def test_gather_packed_and_strided(E, which):
    A = 1 if E == 3 else 2 if E == 6 else 4
    for sstride, dstride in ((0, 0), (E + 2 * A, 0), (0, E + A), (E + 3 * A, E + 5 * A), (32, 48) if E == 16 else (E + A, E + A)):
        run_gather(E, sstride, dstride, 0, 0, which)


@pytest.mark.parametrize("soff,doff,E,stride,unit", [(0, 0, 16, 32, 16), (0, 0, 16, 0, 16), (4, 0, 16, 0, 4), (0, 16, 32, 48, 16), (0, 8, 16, 32, 4), (0, 0, 12, 0, 4),
                                                      (2, 0, 8, 0, 2), (0, 6, 12, 14, 2), (1, 0, 4, 0, 1), (0, 0, 3, 0, 1), (0, 3, 16, 16, 1), (0, 0, 6, 0, 2)])
def test_gather_copy_units(soff, doff, E, stride, unit):
    """pointers and strides that select each of the four copy units (csrc/compact.h: compact_unit)"""
    S, D = stride or E, stride or E
    assert max(u for u in (16, 4, 2, 1) if not (soff | doff | E | S | D) % u) == unit
    for which in (0, 1):
        run_gather(E, stride, stride, soff, doff, which)


@pytest.mark.parametrize("delta", ["zero", -1, 0, 1])
def test_gather_clips_at_the_vertex_capacity(delta):
    used = cp.build(cp.named("half_300")[0], 300)[3][1]
    for which in (0, 1):
        run_gather(12, 0, 16, 0, 0, which, vcap=0 if delta == "zero" else used + delta)


@pytest.mark.parametrize("which", [0, 1])
def test_two_gathers_share_one_interleaved_record(which):
    """position (12 bytes at 0) and colour (4 bytes at 12) of a 20-byte record: the four bytes behind them keep the fill"""
    rng = np.random.default_rng(9)
    nvert = 257
    src, _ = cp.named("half_257")
    exp = cp.build(src, nvert, ngather=2)
    pos, col = aligned_bytes(nvert * 12, 0, rng), aligned_bytes(nvert * 4, 0, rng)
    rec = aligned_bytes(nvert * 20, 0)
    ca.compact_model(src, nvert, which=which, seed=2, gathers=[(pos, 12, 0, rec, 20), (col, 4, 0, rec[12:], 20)])
    want = np.full((nvert, 20), cp.FILL, np.uint8)
    n = exp[3][1]
    want[:n, :12] = cp.gathered(pos, exp[4], 12, 12, nvert)
    want[:n, 12:16] = cp.gathered(col, exp[4], 4, 4, nvert)
    assert rec.tobytes() == want.tobytes()


# ---- 4. a cloud set: the level's points are the order; the record and the gathers alone ----

@pytest.mark.parametrize("cells,vcap", [(0, 10), (1, 10), (100, 300), (100, 99), (100, 0), (300, 300)])
def test_cloud_set(cells, vcap):
    rng = np.random.default_rng(cells + vcap)
    nvert = 300
    points = np.full(nvert, cp.FILL32, np.uint32)
    points[:cells] = np.sort(rng.choice(nvert, size=cells, replace=False))
    source = aligned_bytes(nvert * 12, 0, rng)
    dest = aligned_bytes(vcap * 12, 0)
    newid, order, index, counts = ca.compact_model(points, nvert, faces=cells, which=2, seed=1, vertex_capacity=vcap, gathers=[(source, 12, 0, dest, 0)])
    assert newid is None and order is None and index is None
    assert counts.as_tuple() == (nvert, cells, 0, int(cells > vcap))
    want = np.full(vcap * 12, cp.FILL, np.uint8)
    g = cp.gathered(source, points[:cells], 12, 12, vcap)
    want[:g.size] = g.reshape(-1)
    assert dest.tobytes() == want.tobytes()


# ---- 5. what the hook refuses ----

def test_hook_errors():
    src, nvert = cp.named("all_33")
    with pytest.raises(ca.CortoError):
        ca.compact_model(src, nvert, which=3)
    with pytest.raises(ca.CortoError):
        ca.compact_model(src, nvert, faces=len(src) // 3 + 1)
    with pytest.raises(ca.CortoError):
        ca.compact_model(src.astype(np.uint16), nvert, which=2)     # (a cloud's points are uint32)
    with pytest.raises(ca.CortoError) as e:
        ca.compact_model(cp.strip(8194), 8194, which=0)             # (beyond compact_blob)
    assert e.value.code == cp.E_LIMIT
    a = aligned_bytes(64, 0)
    with pytest.raises(ca.CortoError):
        ca.compact_model(src, nvert, gathers=[(a, 8, 4, a, 0)])      # (a stride below the element)
