"""crthip_batch_bind_cloud_lod without a device: the kernels' source on the host (corto_amd.cloud_lod_model: csrc/cloud_lod.h in both of
k_cloud_lod.hip's partitions, workgroups, threads and so every atomic's order shuffled by a seed) against the sequential model of the contract
(tests/cloud_lod.py), byte for byte; the properties every result has whatever the model says; the identities with the mesh levels' remap and the
weld's; the binding's errors in the header's order, through the hook; the declarations.  The bind call itself needs a device batch:
tests/test_cloud_lod_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import cloud_lod as cl
import corto_amd as ca

SEEDS = (0, 7, 12345)
FILL32 = cl.FILL * 0x01010101


def both_partitions(P, shift, K, tag, seeds=SEEDS, weights=True):
    """the hook in both partitions equals the model; the tails behind `cells` words and `chunks` records keep the fill.  Returns the model's result"""
    exp = cl.build(P, shift, K)
    cl.check_properties(P, shift, K, *exp, tag=(tag, "model"))
    nvert = len(P)
    for which in (0, 1):
        if which == 0 and not cl.in_blob(nvert):
            with pytest.raises(ca.CortoError) as e:                    # (the decode sends such a job down the other path)
                ca.cloud_lod_model(P, shift, K, which=0)
            assert e.value.code == cl.E_LIMIT
            continue
        for seed in seeds:
            remap, points, weight, chunks, counts, _ = ca.cloud_lod_model(P, shift, K, which=which, seed=seed, weights=weights)
            cells, nch = counts.cells, counts.chunks
            assert remap.shape == (nvert,) and points.shape == (nvert,) and (points[cells:] == FILL32).all(), (tag, which, seed, "the points' tail was written")
            if weights:
                assert (weight[cells:] == FILL32).all(), (tag, which, seed, "the weights' tail was written")
                weight = weight[:cells]
            if K:
                assert len(chunks) == cl.nchunks(nvert, K) and (chunks[nch:].view(np.uint8) == cl.FILL).all(), (tag, which, seed, "the chunks' tail was written")
                chunks = chunks[:nch]
            cl.assert_same((remap, points[:cells], weight, chunks, counts), exp, (tag, which, seed))
            cl.check_properties(P, shift, K, remap, points[:cells], weight, chunks, counts.as_tuple(), tag=(tag, which, seed))
    return exp


# ---- 1. hook equals model, the properties, the levels ----

@pytest.mark.parametrize("name", cl.NAMED)
def test_hook_equals_model(name):
    c = cl.case(name)
    levels = []
    for shift in cl.SHIFTS[name]:
        exp = both_partitions(c.P, shift, cl.K_of(name), (name, shift))
        assert exp[4] == cl.model(name, shift)[4]
        levels.append((shift, exp[0], exp[1]))
    cl.check_levels(levels, name)


@pytest.mark.parametrize("name,K", [("c31", 32), ("c32", 32), ("c33", 32), ("c64", 32), ("c64", 33), ("c64", 65536), ("lattice_8193", 65536), ("lattice_8193", 8193),
                                     ("onecell_300", 0), ("lattice_8193", 0)])
def test_chunk_sizes_and_no_chunks(name, K):
    """K = 32 at 31, 32, 33 and 64 kept points; an odd K; K = 65536 (one chunk); no chunks at all (chunk_points 0): the record says 0"""
    c = cl.case(name)
    shift = cl.SHIFTS[name][0]
    exp = both_partitions(c.P, shift, K, (name, shift, K), seeds=(3,))
    assert exp[4][2] == {("c31", 32): 1, ("c32", 32): 1, ("c33", 32): 2, ("c64", 32): 2, ("c64", 33): 2}.get((name, K), 1 if K else 0)


@pytest.mark.parametrize("name", ["n257", "onecell_8193"])
def test_without_weights(name):
    c = cl.case(name)
    for shift in cl.SHIFTS[name]:
        both_partitions(c.P, shift, cl.K_of(name), (name, shift, "no weights"), seeds=(5,), weights=False)


def test_named_cases_are_where_the_table_says():
    n = {name: cl.case(name).nvert for name in cl.NAMED}
    assert [n[k] for k in ("n1", "n2", "n255", "n256", "n257", "lattice_8192", "lattice_8193", "plane_257")] == [1, 2, 255, 256, 257, 8192, 8193, 257 * 257]
    assert cl.in_blob(n["lattice_8192"]) and not cl.in_blob(n["lattice_8193"]) and -(-n["plane_257"] // 256) > 256
    for name in ("onecell_300", "onecell_8193"):                       # one cell at the level's shift, weight[0] == nvert; shift 0 dedupes
        exp = cl.model(name, 10)
        assert exp[4][1] == 1 and exp[2].tolist() == [n[name]] and cl.model(name, 0)[4][1] < n[name]
    for name in ("lattice_8192", "n257"):                              # every point in its own cell
        assert cl.model(name, cl.SHIFTS[name][0])[4][1] == n[name]
    P = cl.case("straddle").P.astype(np.int64)                         # -1 and 0 in two cells, -1 and -2^s in one
    s = cl.STRADDLE_SHIFT
    at = {tuple(p): v for v, p in enumerate(P.tolist())}
    r = cl.model("straddle", s)[0]
    assert r[at[(-1, 0, 0)]] != r[at[(0, 0, 0)]] and r[at[(-1, 0, 0)]] == r[at[(-(1 << s), 0, 0)]] and r[at[(0, 0, 0)]] == r[at[((1 << s) - 1, 0, 0)]]
    W = cl.case("wide").P.astype(np.int64)
    assert W.min() < -(1 << 30) and W.max() > (1 << 30) and cl.model("wide", 31)[4][1] <= 8


# ---- 2. the identities: the mesh levels' remap on the same positions, the weld's at shift 0 ----

@pytest.mark.parametrize("name", ["n257", "onecell_300", "straddle", "wide", "lattice_8193", "cloud_border"])
def test_remap_is_lod_models_and_the_welds(name):
    P = cl.case(name).P
    face = np.zeros((1, 3), np.uint32)                                 # one dummy face: crthip_lod_model wants an index
    for shift in sorted(set(cl.SHIFTS[name]) | {0}):
        mine = ca.cloud_lod_model(P, shift, which=1, seed=shift)[0]
        assert mine.tobytes() == ca.lod_model(P, face, shift, which=1, seed=1)[0].tobytes(), (name, shift)
        if shift == 0:
            assert mine.tobytes() == ca.weld_model(P, face, which=1, seed=2)[0].tobytes(), name


# ---- 3. the limit, the declarations, the binding's errors in the header's order ----

def test_partition_0_beyond_8192_is_e_limit():
    P = np.zeros((8193, 3), np.int32)
    with pytest.raises(ca.CortoError) as e:
        ca.cloud_lod_model(P, 0, which=0)
    assert e.value.code == cl.E_LIMIT and "partition 1" in str(e.value)
    ca.cloud_lod_model(P[:8192], 0, which=0)


def test_struct_sizes():
    assert (C.sizeof(ca.CloudLodLevel), C.sizeof(ca.CloudLodBinding), C.sizeof(ca.CloudChunk), C.sizeof(ca.CloudLodCounts)) == (56, 240, 32, 16)
    assert ca.CLOUD_CHUNK_DTYPE.itemsize == 32 and ca.CLOUD_LOD_MAX_LEVELS == 4
    assert ca.CloudLodBinding.chunk_points.offset == 228 and ca.CloudLodLevel.capacity.offset == 40 and ca.CloudChunk.max.offset == 16


def test_binding_errors_in_order_through_the_hook():
    """the hook builds a one-level binding at exactly nvert words and ceil(nvert / K) records and asks cloud_lod_binding_error, the bind call's
    own check: unknown partition and NULL position first, then no points, chunk_points, then the level's pointers, alignments and shift"""
    L = ca.lib()
    n = 40
    P = np.ascontiguousarray(cl.lattice(n), np.int32)
    buf = np.zeros(12 * n + 2 * 32 + 64, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    remap, points, weight, chunks = base, base + 4 * n, base + 8 * n, base + 12 * n + (-(12 * n) % 16)
    pp = P.ctypes.data

    def call(pos=pp, nvert=n, shift=0, K=32, remap=remap, points=points, weight=weight, chunks=chunks, which=0):
        rc = L.crthip_cloud_lod_model(pos, nvert, shift, K, remap, points, weight, chunks, None, None, which, 0)
        return rc, L.crthip_last_error()
    assert call()[0] == 0
    A = cl.E_ARGUMENT
    for kw, word in ((dict(which=2), b"partition"), (dict(pos=None), b"null position"), (dict(nvert=0), b"no points"), (dict(K=31), b"neither 0 nor in 32..65536"),
                     (dict(K=65537), b"neither 0 nor in 32..65536"), (dict(K=0), b"chunk_points is 0 and a level has chunks"), (dict(remap=None), b"remap or points is NULL"),
                     (dict(points=None), b"remap or points is NULL"), (dict(remap=remap + 2), b"not 4-byte aligned"), (dict(points=points + 1), b"not 4-byte aligned"),
                     (dict(weight=weight + 2), b"weight is not 4-byte aligned"), (dict(chunks=chunks + 8), b"chunks or counts is not 16-byte aligned"),
                     (dict(shift=32), b"above 31")):
        rc, msg = call(**kw)
        assert rc == A and word in msg, (kw, rc, msg)
    # the order: the partition before the points, the points before chunk_points, chunk_points before the level, the level's fields in theirs
    for kw, word in ((dict(which=2, nvert=0, K=31), b"partition"), (dict(nvert=0, K=31, remap=None), b"no points"), (dict(K=31, remap=None, shift=32), b"neither 0 nor"),
                     (dict(K=0, remap=None), b"chunk_points is 0"), (dict(remap=None, weight=weight + 2, shift=32), b"remap or points"),
                     (dict(weight=weight + 2, chunks=chunks + 8, shift=32), b"weight is not"), (dict(chunks=chunks + 8, shift=32), b"chunks or counts")):
        rc, msg = call(**kw)
        assert rc == A and word in msg, (kw, rc, msg)
    assert call(K=0, chunks=None)[0] == 0 and call(weight=None)[0] == 0 and call(K=65536)[0] == 0 and call(shift=31)[0] == 0
    assert call(K=40, chunks=None)[0] == 0                             # (chunk_points in range and no level with chunks: fine)
