"""CPU: the cases of tests/table_edges.py - every one is on the edge it is named for, measured on the oracle's integers, and the kernels' source
on the host (corto_amd.weld_model, corto_amd.lod_model, corto_amd.adjacency_model, both partitions each) equals the sequential models
(tests/weld.py, tests/lod.py, tests/adjacency.py) on it byte for byte.  A change to the encoder, to the hash or to a builder that takes a case
off its edge fails here, not silently on the GPU.  No kernel runs."""
import numpy as np
import pytest

import adjacency as adj
import corto_amd as ca
import lod as ld
import table_edges as te
import weld as wd

SEEDS = (0, 1, 7)                             # tests/test_weld_cpu.py's first three
FILL32 = ld.FILL * 0x01010101


def weld_hooks(case, exp, tag, with_index=True):
    """crthip_weld_model in both partitions against the model; partition 0 refuses a blob beyond weld_blob's LDS"""
    for which in (0, 1):
        if which == 0 and not wd.in_blob(case.nvert):
            with pytest.raises(ca.CortoError):
                ca.weld_model(case.P, case.index, which=0)
            continue
        for seed in SEEDS:
            got = ca.weld_model(case.P, case.index, which=which, seed=seed, with_index=with_index)
            wd.assert_same(got[:3], exp, (tag, which, seed))
            if seed == SEEDS[0]:
                wd.check_properties(case.P, case.index, got[0], got[1], got[2].as_tuple(), tag=(tag, which, seed))


def lod_hooks(case, shift, exp, tag):
    """crthip_lod_model in both partitions against the model, the index tail behind 3*faces words untouched"""
    for which in (0, 1):
        if which == 0 and not ld.in_blob(case.nvert, case.nface):
            with pytest.raises(ca.CortoError):
                ca.lod_model(case.P, case.index, shift, which=0)
            continue
        for seed in SEEDS:
            remap, lindex, counts, _ = ca.lod_model(case.P, case.index, shift, which=which, seed=seed)
            written = 3 * counts.faces
            assert (lindex[written:] == FILL32).all(), (tag, shift, which, seed, "the index tail was written")
            ld.assert_same((remap, lindex[:written], counts), exp, (tag, shift, which, seed))
            if seed == SEEDS[0]:
                ld.check_properties(case.P, case.index, shift, remap, lindex[:written], counts.as_tuple(), tag=(tag, shift, which, seed))


def lod_levels(fn, args, shifts, tag):
    c = fn(*args)
    levels = []
    for shift in shifts:
        exp = te.lod_model(fn, shift, *args)
        lod_hooks(c, shift, exp, tag)
        levels.append((shift, exp[0], exp[2]))
    ld.check_levels(levels, tag)
    return [l[2] for l in levels]


def adj_hooks(case, exp, tag):
    for which in (0, 1):
        if which == 0 and not adj.in_blob(case.nvert, case.nface):
            with pytest.raises(ca.CortoError):
                ca.adjacency_model(case.index, case.nvert, which=0)
            continue
        for seed in SEEDS:
            got = ca.adjacency_model(case.index, case.nvert, which=which, seed=seed)
            adj.assert_same(got, exp, (tag, which, seed))
            if seed == SEEDS[0]:
                adj.check_properties(case.index, case.nvert, got[0], got[1].as_tuple(), tag=(tag, which, seed))


# ---- the hash's port ----

def test_the_port_of_the_hash():
    """murmur3's finaliser at its published points, and the two's-complement words of negative coordinates; what ties the port to the
    library is test_pile_lds and test_pile_cells: the walks of keys that the port says share a home slot"""
    assert [int(x) for x in te.weld_fmix([0, 1, 0xFFFFFFFF])] == [0, 0x514E28B7, 0x81F16F39]
    assert te.words([-1, -2 ** 31, 5]).tolist() == [0xFFFFFFFF, 0x80000000, 5]
    h = int(te.weld_hash([[0, 0, 0]])[0])
    f = lambda x: int(te.weld_fmix([x])[0])                          # noqa: E731
    assert h == f(f(f(0x9E3779B9))) and te.home([[0, 0, 0]], 64)[0] == h & 63
    assert te.occupied([63, 63, 63, 5], 64) == {63, 0, 1, 5} and te.total_walk([63, 63, 63, 5], 64) == te.total_walk([5, 63, 63, 63], 64) == 7


# ---- A. pile-ups ----

def test_pile_lds():
    c = te.pile_lds()
    n = te.PILE_LDS
    assert (c.nvert, c.nface, wd.slots(c.nvert)) == (n, n - 2, 256) == (96, 94, 256) and wd.in_blob(c.nvert)
    assert wd.multiplicities(c.P) == [1] * n and c.P.min() < 0 < c.P.max()
    homes = te.home(c.P, 256)
    assert (homes == 255).all()
    assert te.occupied(homes.tolist(), 256) == {255} | set(range(n - 1))           # the chain runs past the last slot: 255, 0, 1, ..., 94
    exp = te.weld_model(te.pile_lds)
    assert exp[2] == (96, 96, 0, 0)
    for which in (0, 1):
        for seed in SEEDS:
            # n distinct keys of one home slot: walks of 1, 2, ..., n slots in whatever order they come
            assert ca.weld_model(c.P, c.index, which=which, seed=seed)[3] == (n * (n + 1) // 2, n) == (4656, 96)
    weld_hooks(c, exp, "pile_lds")
    assert lod_levels(te.pile_lds, (), (0,), "pile_lds") == [(96, 94, 0, 0)]          # at shift 0 the positions' pile is the cells'
    for which in (0, 1):
        assert ca.lod_model(c.P, c.index, 0, which=which, seed=3)[3][:2] == (4656, 96)


def test_pile_mem():
    c = te.pile_mem()
    assert (c.nvert, c.nface) == (8493, 11218) and wd.slots(c.nvert) == 32768 and not wd.in_blob(c.nvert)
    assert wd.multiplicities(c.P) == [1] * c.nvert
    assert int((te.home(c.P, 32768) == 32767).sum()) == te.PILE_MEM == 300           # more than a workgroup's 256 vertices on one chain
    exp = te.weld_model(te.pile_mem)
    assert exp[2] == (8493, 8493, 0, 0)
    for seed in SEEDS:
        # the longest walk depends on the order the vertices come in, the total does not
        total, longest = ca.weld_model(c.P, c.index, which=1, seed=seed)[3]
        assert 256 <= te.PILE_MEM <= longest and total == te.total_walk(te.home(c.P, 32768).tolist(), 32768) == 69393
    weld_hooks(c, exp, "pile_mem")
    weld_hooks(c, te.weld_model(te.pile_mem, False), "pile_mem, no index", with_index=False)
    assert lod_levels(te.pile_mem, (), (0,), "pile_mem") == [(8493, 11218, 0, 0)]
    # the face table in memory (T = 32 768): distinct keys that start on one slot come by themselves among 11 218 faces - five of them when
    # this was written; a chain that wraps does not (slot 32 767 stays empty).  The hook's face walks visit the slots the port foretells
    keys = te.face_keys(te.lod_model(te.pile_mem, 0)[1])
    Tf = wd.slots(c.nface)
    assert len(keys) == c.nface and Tf == 32768 and te.pile_figures(keys, Tf)[0] >= 3
    for seed in SEEDS:
        stats = ca.lod_model(c.P, c.index, 0, which=1, seed=seed)[3]
        assert stats[1] >= te.PILE_MEM and stats[2] == te.total_walk(te.home(keys, Tf).tolist(), Tf)


def test_pile_cells():
    c = te.pile_cells()
    n = te.PILE_CELLS
    assert (c.nvert, c.nface) == (2 * n, 2 * n - 2) == (96, 94) and ld.in_blob(c.nvert, c.nface) and wd.slots(c.nvert) == 256
    cells = te.distinct_cells(c, te.PILE_SHIFT)
    assert len(cells) == n and (te.home(cells, 256) == 255).all() and cells.min() < 0
    assert sorted(np.unique(c.P.astype(np.int64) >> te.PILE_SHIFT, axis=0, return_counts=True)[1].tolist()) == [2] * n
    counts = lod_levels(te.pile_cells, (), (0, te.PILE_SHIFT), "pile_cells")
    assert counts == [(96, 94, 0, 0), (48, 48, 0, 46)]
    for which in (0, 1):
        for seed in SEEDS:
            # a cell's second vertex walks to the slot its first one took: twice the walks of n distinct keys of one home slot
            assert ca.lod_model(c.P, c.index, te.PILE_SHIFT, which=which, seed=seed)[3][:2] == (n * (n + 1), n) == (2352, 48)
    weld_hooks(c, te.weld_model(te.pile_cells), "pile_cells")


def test_pile_cells_mem():
    c = te.pile_cells_mem()
    T = wd.slots(c.nvert)
    assert (c.nvert, c.nface, T) == (8793, 11518, 32768) and not ld.in_blob(c.nvert, c.nface)
    cells = te.distinct_cells(c, te.PILE_SHIFT)
    on_chain = cells[te.home(cells, T) == T - 1]
    assert len(on_chain) == te.PILE_MEM >= 256
    P = c.P.astype(np.int64) >> te.PILE_SHIFT
    assert all(int((P == cell).all(axis=1).sum()) == 2 for cell in on_chain[::37])    # two vertices a cell (a sample: the counts below say all)
    counts = lod_levels(te.pile_cells_mem, (), (0, te.PILE_SHIFT), "pile_cells_mem")
    assert counts[0][0] == c.nvert and counts[1][0] == len(cells) == te.PILE_MEM + 512                # (the grid beside it lies in 512 cells)
    assert counts[1][1:] == (te.PILE_MEM, 10920, te.PILE_MEM - 2)
    for seed in SEEDS:
        vtotal, vlongest = ca.lod_model(c.P, c.index, te.PILE_SHIFT, which=1, seed=seed)[3][:2]
        assert vlongest >= te.PILE_MEM and vtotal >= te.PILE_MEM * (te.PILE_MEM + 1)
    weld_hooks(c, te.weld_model(te.pile_cells_mem), "pile_cells_mem")


def test_pile_faces():
    """the face table of one wave: recomputed from what the encoder left, so a change of its numbering that takes the figure away fails here"""
    c = te.pile_faces()
    assert (c.nvert, c.nface) == (24, 32) and wd.slots(c.nface) == 64 and ld.in_blob(c.nvert, c.nface)
    exp = te.lod_model(te.pile_faces, 0)
    assert exp[2] == (24, 32, 0, 0)
    keys = te.face_keys(exp[1])
    assert len(np.unique(keys, axis=0)) == 32
    most, _, taken, homes = te.pile_figures(keys, 64)
    assert most >= 3                                                                  # distinct keys that start on one slot
    assert {63, 0} <= taken and 0 not in homes                                        # a chain that wraps: nobody starts on slot 0
    # the port's "rotated triple under weld_hash" is the library's face key: 32 distinct keys walk these slots in all in whatever order
    foretold = te.total_walk(te.home(keys, 64).tolist(), 64)
    assert foretold > 32
    for which in (0, 1):
        for seed in SEEDS:
            assert ca.lod_model(c.P, c.index, 0, which=which, seed=seed)[3][2] == foretold, (which, seed)
    lod_levels(te.pile_faces, (), (0,), "pile_faces")
    weld_hooks(c, te.weld_model(te.pile_faces), "pile_faces")


# ---- B. beyond one round of lod_offsets, ids beyond 16 bits ----

@pytest.mark.parametrize("name", sorted(te.BIG_STRIPS))
def test_big_strips(name):
    c = te.big_strip(name)
    nface = te.BIG_STRIPS[name]
    assert (c.nvert, c.nface) == (te.BIG_NVERT[name], nface) and not ld.in_blob(c.nvert, c.nface)
    assert c.P.min() == 0                                                             # no negative coordinate: one cell at shift 31
    blocks = -(-nface // 256)
    assert blocks == {"strip_65536": 256, "strip_65537": 257}[name]                   # one round of lod_offsets_job, and two
    assert c.index.max() >= 65536 and 3 * nface > 65536
    counts = lod_levels(te.big_strip, (name,), te.BIG_SHIFTS, name)
    assert counts[0] == (c.nvert, nface, 0, 0)                                        # 256 kept faces in every full block
    assert counts[1] == (c.nvert - nface // 2, (nface + 1) // 2, nface // 2, 0)
    assert counts[1] == {"strip_65536": (65537, 32768, 32768, 0), "strip_65537": (65539, 32769, 32768, 0)}[name]
    assert counts[2] == (1, 0, nface, 0)                                              # 256 degenerate faces in every full block, no index word
    remap4 = te.lod_model(te.big_strip, ld.STRIP_SHIFT, name)[0]
    moved = np.flatnonzero(remap4 != np.arange(c.nvert))
    assert len(moved) and max(int(moved.max()), int(remap4[moved].max())) >= 65536    # remap words beyond 16 bits
    assert te.lod_model(te.big_strip, ld.STRIP_SHIFT, name)[1].max() >= 65536


def test_doubled_strip():
    c = te.doubled_strip()
    assert c.nvert == 65540 and c.nvert >= 65537 and c.nface == 2 * te.DOUBLED and wd.slots(c.nvert) == 262144 and not wd.in_blob(c.nvert)
    assert wd.multiplicities(c.P) == [2] * (c.nvert // 2)
    exp = te.weld_model(te.doubled_strip)
    assert exp[2] == (c.nvert, c.nvert // 2, 0, 0)
    assert (exp[0][65536:] < 65536).all()                                             # ids at or above 65 536 go to ids below
    assert (exp[1] != c.index.reshape(-1)).any()
    weld_hooks(c, exp, "doubled_strip")


# ---- C. adjacency at its limits ----

ADJ_FIGURES = {"adj_lds_exact": (4172, 8138, 65536), "adj_lds_over": (4173, 8139, 65552), "adj_scan_4352": (4351, 8317, 67312), "adj_scan_4353": (4352, 8318, 67344)}


@pytest.mark.parametrize("name", sorted(te.ADJ_K))
def test_sphere_and_strip(name):
    c = te.sphere_and_strip(te.ADJ_K[name])
    assert (c.nvert, c.nface, adj.blob_lds(c.nvert, c.nface)) == ADJ_FIGURES[name]
    assert adj.in_blob(c.nvert, c.nface) == (name == "adj_lds_exact")
    if name == "adj_lds_exact":
        assert adj.blob_lds(c.nvert, c.nface) == adj.BLOB_LDS_MAX
    if name.startswith("adj_scan"):
        assert c.nvert + 1 == int(name[-4:]) and 4352 == 17 * 256
    exp = te.adj_model(te.sphere_and_strip, te.ADJ_K[name])
    assert exp[1][2:] == (0, 0) and 0 < exp[1][1] < 3 * c.nface
    adj_hooks(c, exp, name)


def test_the_library_draws_the_lds_limit_where_the_model_does():
    """adjacency_blob's partition takes the blob of exactly 64 KiB and refuses the one of a vertex and a face more"""
    c = te.sphere_and_strip(te.ADJ_K["adj_lds_exact"])
    ca.adjacency_model(c.index, c.nvert, which=0)
    c = te.sphere_and_strip(te.ADJ_K["adj_lds_over"])
    with pytest.raises(ca.CortoError):
        ca.adjacency_model(c.index, c.nvert, which=0)


@pytest.mark.parametrize("name", sorted(te.ADJ_STRIPS))
def test_strips_at_a_round_of_the_scan(name):
    c = te.adj_strip(te.ADJ_STRIPS[name])
    assert (c.nvert, c.nface) == (te.ADJ_STRIPS[name], te.ADJ_STRIPS[name] - 2) and adj.in_blob(c.nvert, c.nface)
    adj_hooks(c, te.adj_model(te.adj_strip, te.ADJ_STRIPS[name]), name)


@pytest.mark.parametrize("name", sorted(te.FANS))
def test_fans(name):
    c = te.fan_case(te.FANS[name])
    assert c.nface == te.VALENCE and c.nvert == te.VALENCE + (1 if te.FANS[name] else 2) and adj.in_blob(c.nvert, c.nface)
    v = te.valences(c)
    assert v.max() == te.VALENCE and int((v == te.VALENCE).sum()) == 1
    exp = te.adj_model(te.fan_case, te.FANS[name])
    assert exp[1] == (900, 300 if te.FANS[name] else 302, 0, 0)
    adj_hooks(c, exp, name)


def test_fan_in_four_kernels():
    c = te.fan_in_four_kernels()
    assert (c.nvert, c.nface) == (4526, 8492) and not adj.in_blob(c.nvert, c.nface)
    v = te.valences(c)
    assert v.max() == te.VALENCE > 256 and int((v == te.VALENCE).sum()) == 1       # more half-edges than a workgroup's 256 start at one vertex
    adj_hooks(c, te.adj_model(te.fan_in_four_kernels), "fan_in_four_kernels")


def test_the_case_lists():
    assert [cid for cid, *_ in te.PILES] == ["pile_lds", "pile_mem", "pile_cells", "pile_cells_mem", "pile_faces"]
    for cid, fn, args, _ in te.PILES:
        c = fn(*args)
        beyond = cid in te.PILES_BEYOND_BLOB
        assert wd.in_blob(c.nvert) == ld.in_blob(c.nvert, c.nface) == (not beyond), cid
    blob = [cid for cid, _, b in te.adjacency_cases() if b]
    assert len(te.adjacency_cases()) == 10 and "adj_lds_exact" in blob and len(blob) == 6
    for cid, c, b in te.adjacency_cases():
        assert adj.in_blob(c.nvert, c.nface) == b, cid
