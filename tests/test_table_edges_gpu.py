"""GPU (-m gpu): the weld, level-of-detail and adjacency kernels at the edges of tests/table_edges.py (tests/test_table_edges_cpu.py shows that
every case is on the edge it is named for) - raw bytes against the sequential models (tests/weld.py, tests/lod.py, tests/adjacency.py) on the
oracle's integers, and the properties that do not rest on the models.  Every array lives in a device buffer pre-filled with 0xCD at exactly
its bound (the Bound classes of the three features' GPU tests): nothing outside the arrays' written words and the records may change.  One
batch a group of cases."""
import functools

import numpy as np
import pytest

import adjacency as adj
import corto_amd as ca
import lod as ld
import table_edges as te
import weld as wd
from test_adjacency_gpu import Bound as AdjBound, expect_ran as adj_ran
from test_lod_gpu import Bound as LodBound, expect_ran as lod_ran
from test_weld_gpu import Bound as WeldBound, expect_ran as weld_ran, make_ctx, run, same_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = wd.FILL


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def decoded_index_is_the_oracles(b, i, case, tag):
    """the models run on Case.index: the index this decode left is that one, and every id in it is a vertex"""
    got = b.host_outputs(i)["index"].astype(np.uint32).reshape(-1, 3)
    assert (b.infos[i].nvert, b.infos[i].nface) == (case.nvert, case.nface), tag
    assert (got == case.index).all() and got.max() < case.nvert, tag


# ---- A. pile-ups: distinct keys on one probe chain that wraps, in LDS and in memory; the weld on every blob and the levels on every blob ----

PILE_IDS = [cid for cid, *_ in te.PILES]
WELD_RECORDS = {"pile_lds", "pile_cells", "pile_faces"}                              # every other blob (the three kernels with a record: B)
LOD_RECORDS = {"pile_mem", "pile_cells"}                                             # lod_blob and the six kernels, each with a record and without
WELD_INDEXED = {"pile_lds", "pile_mem", "pile_faces"}                                # both paths with a welded index and without one


def decode_piles(ctx, order, tag):
    """one batch of the cases of A in `order`; {case: (the weld's remap and index or None, [a level's remap and index])} after every check"""
    piles = [te.PILES[k] for k in order]
    at = {cid: i for i, (cid, *_) in enumerate(piles)}
    b = ca.Batch(ctx, [fn(*args).blob for _, fn, args, _ in piles])
    b.allocate_outputs(fill=FILL)
    wb = WeldBound(b, range(len(piles)), records=[at[c] for c in WELD_RECORDS], indexed=[at[c] for c in WELD_INDEXED])
    lb = LodBound(b, {i: shifts for i, (_, _, _, shifts) in enumerate(piles)}, records=[at[c] for c in LOD_RECORDS])
    run(b)
    welds = wb.read()
    levels = lb.read(lambda i, k: te.lod_model(piles[i][1], piles[i][3][k], *piles[i][2])[2][1])
    out = {}
    for i, (cid, fn, args, shifts) in enumerate(piles):
        c = fn(*args)
        decoded_index_is_the_oracles(b, i, c, (tag, cid))
        assert wd.in_blob(c.nvert) == ld.in_blob(c.nvert, c.nface) == (cid not in te.PILES_BEYOND_BLOB), cid
        remap, windex, counts = welds[i]
        assert (windex is not None) == (cid in WELD_INDEXED) and (counts is not None) == (cid in WELD_RECORDS)
        exp = te.weld_model(fn, windex is not None)
        counts = exp[2] if counts is None else counts
        wd.assert_same((remap, windex, counts), exp, (tag, cid, "weld"))
        wd.check_properties(c.P, c.index, remap, windex, counts, tag=(tag, cid, "weld"))
        seen = []
        for shift, (lremap, lindex, lcounts) in zip(shifts, levels[i]):
            assert (lcounts is not None) == (cid in LOD_RECORDS)
            exp = te.lod_model(fn, shift, *args)
            lcounts = exp[2] if lcounts is None else lcounts
            ld.assert_same((lremap, lindex, lcounts), exp, (tag, cid, "lod", shift))
            ld.check_properties(c.P, c.index, shift, lremap, lindex, lcounts, tag=(tag, cid, "lod", shift))
            seen.append((shift, lremap, lcounts))
        ld.check_levels(seen, (tag, cid))
        out[cid] = (welds[i][:2], [l[:2] for l in levels[i]])
    # One batch a group: what ran is known for the batch, not for a blob.  Both paths of both features ran; that pile_lds, pile_cells and
    # pile_faces took the one-workgroup kernels and pile_mem and pile_cells_mem the others rests on in_blob above, which the features' own
    # tests pin on the device with one blob a batch at 8 192 | 8 193 (test_weld_gpu.py, test_lod_gpu.py: test_paths)
    weld_ran(b, True, True)
    lod_ran(b, True, True)
    b.close()
    return out


def same_arrays(a, b, tag):
    assert (a is None) == (b is None), tag
    assert a is None or a.tobytes() == b.tobytes(), tag


def test_pile_ups(ctx):
    first = decode_piles(ctx, range(len(te.PILES)), "first")
    fresh = make_ctx()
    try:
        again = decode_piles(fresh, range(len(te.PILES) - 1, -1, -1), "fresh context, the other order")
    finally:
        fresh.close()
    for cid in PILE_IDS:                                                             # (both equal the models' bytes; said once more without them)
        for x, y in zip(first[cid][0], again[cid][0]):
            same_arrays(x, y, (cid, "weld"))
        assert len(first[cid][1]) == len(again[cid][1])
        for (r0, i0), (r1, i1) in zip(first[cid][1], again[cid][1]):
            same_arrays(r0, r1, (cid, "lod remap"))
            same_arrays(i0, i1, (cid, "lod index"))


# ---- B. 256 and 257 blocks of faces: one round of lod_offsets and two; ids, remap words and block numbers beyond 16 bits ----

def test_beyond_one_round_of_offsets(ctx):
    names = sorted(te.BIG_STRIPS)
    cases = [te.big_strip(n) for n in names] + [te.doubled_strip()]
    blobs = [c.blob for c in cases]
    p = ca.Batch(ctx, blobs)
    p.allocate_outputs(fill=FILL)
    run(p)
    assert not any(k.startswith(("lod", "weld")) for k in p.kernel_times())
    plain = [p.host_outputs(i) for i in range(len(cases))]
    p.close()
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=FILL)
    # a device record on every level of both strips: the counts below are the kernels' own, never the model's (the six kernels with their
    # record in scratch: pile_cells_mem above)
    lb = LodBound(b, {0: te.BIG_SHIFTS, 1: te.BIG_SHIFTS})
    wb = WeldBound(b, [2])
    run(b)
    for i, c in enumerate(cases):
        decoded_index_is_the_oracles(b, i, c, i)
        same_outputs(b.host_outputs(i), plain[i], i)

    def no_model_here(i, k):
        raise AssertionError("blob %d, level %d has no record" % (i, k))
    levels = lb.read(no_model_here)                                                  # (reads 3*faces words by the device's `faces`)
    host = lb.buf.cpu().numpy()
    for i, name in enumerate(names):
        nface = te.BIG_STRIPS[name]
        assert -(-nface // 256) == 256 + i
        seen = []
        for k, shift in enumerate(te.BIG_SHIFTS):
            remap, lindex, counts = levels[i][k]
            assert counts is not None
            ld.assert_same((remap, lindex, counts), te.lod_model(te.big_strip, shift, name), (name, shift))
            seen.append((shift, remap, counts))
        ld.check_levels(seen, name)
        # the device's records: `faces` is lod_offsets' running base after one round and after two, `degenerate` at shift 31 what lod_keep's
        # workgroups added up from 256 a full block
        assert [l[2] for l in seen] == [(cases[i].nvert, nface, 0, 0), (cases[i].nvert - nface // 2, (nface + 1) // 2, nface // 2, 0), (1, 0, nface, 0)]
        assert seen[2][2][1] == 0 and len(levels[i][2][1]) == 0
        off, size = lb.at[i][2][1]                                                   # one cell: no word of the level's index is written
        assert size == 12 * nface and (host[off:off + size] == FILL).all(), name
    got = wb.read()[2]
    exp = te.weld_model(te.doubled_strip)
    wd.assert_same(got, exp, "doubled_strip")
    assert got[2] == (65540, 32770, 0, 0) and (got[0][65536:] < 65536).all()
    lod_ran(b, False, True)
    weld_ran(b, False, True)
    b.close()


# ---- C. adjacency: the LDS limit to the byte, the scan's rounds, a valence above a workgroup's half-edges ----

@functools.lru_cache(maxsize=None)
def adj_expected(case):
    """the model on a case's decoded index, computed once"""
    return adj.build(case.index, case.nvert)


def check_adjacency(b, ab, cases, tag):
    got = ab.read()
    for i, (cid, c, _) in enumerate(cases):
        decoded_index_is_the_oracles(b, i, c, (tag, cid))
        exp = adj_expected(c)
        twin, counts = got[i]
        counts = exp[1] if counts is None else counts
        adj.assert_same((twin, counts), exp, (tag, cid))
        adj.check_properties(c.index, c.nvert, twin, counts, tag=(tag, cid))


def test_adjacency_limits(ctx):
    cases = te.adjacency_cases()
    assert {True, False} == {blob for _, _, blob in cases}
    b = ca.Batch(ctx, [c.blob for _, c, _ in cases])
    b.allocate_outputs(fill=FILL)
    for i, (cid, c, blob) in enumerate(cases):
        assert adj.in_blob(b.infos[i].nvert, b.infos[i].nface) == blob, cid
    ab = AdjBound(b, range(len(cases)), records=range(0, len(cases), 2))
    run(b)
    check_adjacency(b, ab, cases, "limits")
    adj_ran(b, True, True)                                                           # (for the batch; a blob's own path: the one-blob batches below)
    b.close()


@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("name", ["adj_lds_exact", "adj_lds_over"])
def test_the_lds_limit_alone_in_its_batch(ctx, name, record):
    """the launch's LDS request is exactly this blob's: 65 536 bytes, and for a vertex and a face more none at all"""
    c = te.sphere_and_strip(te.ADJ_K[name])
    blob = name == "adj_lds_exact"
    assert adj.in_blob(c.nvert, c.nface) == blob and (adj.blob_lds(c.nvert, c.nface) == adj.BLOB_LDS_MAX) == blob
    b = ca.Batch(ctx, [c.blob])
    b.allocate_outputs(fill=FILL)
    ab = AdjBound(b, [0], records=[0] if record else [])
    run(b)
    check_adjacency(b, ab, [(name, c, blob)], (name, record))
    adj_ran(b, blob, not blob)
    b.close()
