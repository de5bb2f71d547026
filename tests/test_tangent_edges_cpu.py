"""CPU: the cases of tests/tangent_edges.py - every one is on the side it is named for (its k range, its wraps, kB - kT, its face or vertex
count relative to the kernels' blocks, its size class by the library's own headers), holds no more than tangent_edges.FALLBACK_CAP fallback
vertices, and the kernels' source on the host (corto_amd.tangent_model, in the partition the case takes on the device) equals the numpy model
on it byte for byte.  The floors are below the measured figures (profiles/computed_tangents.md has the table): a change to corto_amd.synth
or the size-class meshes that flattens a case fails here, not silently on the GPU.  No kernel runs."""
import tempfile

import numpy as np
import pytest

import corto_amd as ca
import computed_tangents as ct
import size_classes as sc
import tangent_edges as te
import value_ranges as vr

FMTS = [ca.FMT_FLOAT, ca.FMT_INT16]


def hook_equals_model(e, tag, nfmts=FMTS, seed=1):
    """the hook in the case's own partition, every output format x normal format, against the model"""
    which = 0 if te.one_workgroup(e.nvert) else 1
    for nfmt in nfmts:
        for fmt in FMTS:
            got = ca.tangent_model(e.P, e.t, e.index, e.normal(nfmt), fmt=fmt, which=which, seed=seed)
            ct.assert_bytes(got, e.model(fmt, nfmt)[0], (tag, fmt, nfmt, which))


def capped(e, tag):
    for nfmt in FMTS:
        fb = int(e.model(ca.FMT_FLOAT, nfmt)[1].sum())
        assert fb <= te.FALLBACK_CAP, (tag, nfmt, fb)


def redone(e):
    """K-DELTA's int16 records cannot hold the blob's positions or uvs (tests/value_ranges.py: host_rule)"""
    return any(vr.host_rule(e.tr["_raw_" + nm], e.tr["_delta_" + nm])[0] for nm in ("position", "uv"))


# ---- 1. value edges ----

@pytest.mark.parametrize("nvert", [2304, 2305, 3073])
def test_full_width(nvert):
    """measured: k 36..39 / 37..39 / 37..39; wrapped vertices 715 / 792 / 979; kT < kB at 558 / 518 / 728 vertices, kT > kB at 524 / 539 / 687,
    kB - kT up to 5 / 5 / 4; 1 fallback vertex; det < 0 on half the faces"""
    e = te.full_width(nvert)
    f = te.Figures(e)
    assert e.nvert == nvert and te.one_workgroup(nvert) == (nvert == 2304)
    assert np.abs(e.P).max() >= 2 ** 30 and np.abs(e.t).max() >= 2 ** 29
    assert f.k.min() >= 30 and f.k.max() <= 40
    assert te.exact_sums_differ(e.P, e.t, e.index) > 0
    assert (f.kB - f.kT).max() >= 4 and (f.kT - f.kB).max() >= 1
    assert (f.kT < f.kB).sum() > 100 and (f.kT > f.kB).sum() > 100
    assert 0.4 * e.nface < (f.det < 0).sum() < 0.6 * e.nface
    if nvert == 2305:                                                           # the figures of the batch-wide case, as measured
        assert (int(f.k.min()), int(f.k.max())) == (37, 39) and int((f.kT < f.kB).sum()) == 518 and int((f.kT > f.kB).sum()) == 539
        assert int((f.kB - f.kT).max()) == 5 and int(f.fallback.sum()) == 1
    capped(e, nvert)
    assert redone(e)
    hook_equals_model(e, ("full width", nvert))


@pytest.mark.parametrize("nvert", [2304, 2305])
def test_deep_grid(nvert):
    """measured: k 0..10 in one blob, kB - kT up to 10, kT - kB up to 2, 2 fallback vertices, nothing wraps (the widest sum has 34 bits)"""
    e = te.deep(nvert)
    f = te.Figures(e)
    assert e.nvert == nvert and te.one_workgroup(nvert) == (nvert == 2304)
    assert f.k.min() == 0 and f.k.max() >= 8 and len(np.unique(f.k)) >= 8       # a shift that varies from vertex to vertex
    assert (f.kB - f.kT).max() >= 4 and (f.kT - f.kB).max() >= 1
    assert te.exact_sums_differ(e.P, e.t, e.index) == 0
    capped(e, nvert)
    assert redone(e)
    hook_equals_model(e, ("deep", nvert))


@pytest.mark.parametrize("nvert", [2304, 2305])
def test_extreme_ends(nvert):
    """uvs at +-(2^31 - 1) exactly, positions past +-2^30 (what a float32 input and the value coder's 32-bit fields leave): differences of 33
    bits, products past 2^63.  Measured: k 28..39 / 20..39, the widest |sum| has 63 bits, 2 289 / 2 293 vertices wrap, kB - kT and kT - kB up to 21"""
    e = te.extreme_ends(nvert)
    f = te.Figures(e)
    assert e.nvert == nvert
    assert e.t.max() == te.TOP and e.t.min() == -te.TOP and np.abs(e.P).max() >= 2 ** 30
    d = e.t.astype(np.int64)[e.index.astype(np.int64)]
    assert np.abs(d[:, 1] - d[:, 0]).max() >= 2 ** 32 - 8192                    # a difference that needs tan_wide's 33rd bit
    assert f.widest >= 63 and f.k.max() >= 39
    assert te.exact_sums_differ(e.P, e.t, e.index) > e.nvert // 2
    assert (f.kB - f.kT).max() >= 4 and (f.kT - f.kB).max() >= 4
    capped(e, nvert)
    assert redone(e)
    hook_equals_model(e, ("extreme ends", nvert))


@pytest.mark.parametrize("nvert", [2304, 2305])
def test_extreme_rescale(nvert):
    """the far end of tan_rescale.  Measured: d = k - kT is 32 or more at the three crafted vertices (kB - kT up to 33 / 34) with a T that
    tan_blob_keep_T does not leave at zero - a shift by d taken modulo 32, as the hardware's 32-bit shifts take it, would give T back
    unshifted there (tried once: the hook built without the branch leaves other bytes at exactly these three vertices of the 2 304-vertex blob,
    and nowhere else in this module; the batch-wide kernels do not rescale); d is 1..23 on a kept T at 726 / 714 vertices; kT - kB up to
    23 / 24; 3 fallback vertices, the crafted ones"""
    e = te.extreme_rescale(nvert)
    f = te.Figures(e)
    assert e.nvert == nvert
    assert int((f.d >= 31).sum()) >= 1                                          # the branch of tan_rescale
    far = (f.d >= 32) & f.T_kept
    assert int(far.sum()) == te.RESCALE_CENTRES                                 # ... on values that a masked shift would not clear
    assert f.fallback[far].all()                                                # (T shifts to nothing: the contract's fallback)
    assert int(((f.d >= 1) & (f.d <= 23) & f.T_kept).sum()) > 100               # the shift proper
    assert f.widest >= 63 and e.t.max() == te.TOP and e.t.min() == -te.TOP
    capped(e, nvert)
    assert redone(e)
    hook_equals_model(e, ("extreme rescale", nvert))


# ---- 2. the affine sheet through a blob ----

@pytest.mark.parametrize("n", te.SHEETS)
def test_affine_sheet_blob(n):
    """k is 13..15; the model deviates from the exact answer (A[:, 0] made orthogonal to the decoded normal, float64) by 3.2e-8 with FLOAT
    normals and 5.0e-8 with INT16 ones, at both sizes and with u negated - under the bound of 1e-6 that tests/test_computed_tangents_cpu.py
    carries for the hook (a few float32 roundings of a unit vector, 2^-24 each)"""
    for negate in (False, True):
        e = te.sheet(n, negate)
        f = te.Figures(e)
        assert e.nvert == n * n and te.one_workgroup(e.nvert) == (n == 8)
        assert f.k.min() >= 13 and f.k.max() <= 15 and not f.fallback.any()
        for nfmt in FMTS:
            dev = te.sheet_deviation(e.model(ca.FMT_FLOAT, nfmt)[0], e.normal(nfmt), negate)
            print("sheet %d negate %s normals %d: k %d..%d, model deviates by %.3g" % (n, negate, nfmt, f.k.min(), f.k.max(), dev))
            assert dev <= te.SHEET_BOUND, dev
        hook_equals_model(e, ("sheet", n, negate))
    plain, mirrored = te.sheet(n, False), te.sheet(n, True)
    assert (plain.index == mirrored.index).all() and (plain.P == mirrored.P).all()
    assert (mirrored.model(ca.FMT_FLOAT)[0] == -plain.model(ca.FMT_FLOAT)[0]).all()       # exactly: the sums mirror


# ---- 3. block, round and slot edges ----

@pytest.mark.parametrize("cid", te.EDGE_IDS)
def test_edge_case_is_where_it_is_named(cid):
    e = te.edge_case(cid)                                                       # (asserts nvert and nface)
    c = te.constants()
    wide = cid in [x[0] for x in te.WIDE_EDGES]
    assert te.one_workgroup(e.nvert) == (not wide)
    kind, _, n = cid.partition("_")
    n = int(n.split("_")[0]) if kind != "tetrahedron" else 0
    if kind == "faces":
        assert n == e.nface and abs(e.nface - 6 * c["TAN_BLOCK"]) <= 1
    elif kind == "vertices":
        assert n == e.nvert and abs(e.nvert - 3 * c["TAN_BLOCK"]) <= 1
    elif kind == "round":
        assert n == e.nface and min(abs(e.nface - c["TAN_ROUND_FACES"]), abs(e.nface - 2 * c["TAN_ROUND_FACES"])) <= 1
    elif kind == "slots":
        assert n == e.nvert and abs(e.nvert - c["TAN_THREADS"]) <= 1
    else:
        assert (e.nvert, e.nface) == (4, 4)
    if cid.endswith("deep"):
        f = te.Figures(e)
        assert f.k.min() == 0 and f.k.max() >= 8
    capped(e, cid)
    hook_equals_model(e, cid, nfmts=[ca.FMT_FLOAT])


def test_the_edges_come_in_threes():
    c = te.constants()
    nf = sorted(te.edge_case(x[0]).nface for x in te.WIDE_EDGES if x[0].startswith("faces"))
    assert nf == [6 * c["TAN_BLOCK"] - 1, 6 * c["TAN_BLOCK"], 6 * c["TAN_BLOCK"] + 1]          # the last: a block of a single face
    nv = sorted(te.edge_case(x[0]).nvert for x in te.WIDE_EDGES if x[0].startswith("vertices") and not x[0].endswith("deep"))
    assert nv == [3 * c["TAN_BLOCK"] - 1, 3 * c["TAN_BLOCK"], 3 * c["TAN_BLOCK"] + 1]
    r = c["TAN_ROUND_FACES"]
    assert sorted(te.edge_case(x[0]).nface for x in te.BLOB_EDGES if x[0].startswith("round")) == [r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1]
    assert sorted(te.edge_case(x[0]).nvert for x in te.BLOB_EDGES if x[0].startswith("slots")) == [c["TAN_THREADS"] - 1, c["TAN_THREADS"], c["TAN_THREADS"] + 1]


def test_one_batch_holds_every_wide_edge():
    batch = te.one_batch()
    ids = [cid for cid, _ in batch]
    assert [i for i in ids if i in [x[0] for x in te.WIDE_EDGES]] == [x[0] for x in te.WIDE_EDGES]
    assert ids.count(None) == 2 and sum(1 for i in ids if i and te.one_workgroup(te.edge_case(i).nvert)) == 2
    assert ids[0] is not None and not te.one_workgroup(te.edge_case(ids[0]).nvert)
    for cid, blob in batch:
        info = ca.probe(blob)
        if cid is None:
            assert info.nface == 0 or "uv" not in [a["name"] for a in info.attrs()]


# ---- 4. the blobs beside the other pipelines ----

def test_sizes_by_the_probe():
    """the unfused-normals blob is past normal_fused and batch-wide; the record blob is past both one-workgroup limits; the big ones are where
    they are named: beyond K-DELTA's LDS records for three components, at the last uint16 index, past it"""
    with tempfile.TemporaryDirectory(prefix="tangent_edges") as d:
        p = sc.Probe(d)
        try:
            n = te.unfused_nvert()
            assert not p.fused(n, 2 * n - 4)["fused"] and p.fused(n - 1, 2 * n - 6)["fused"] and not te.one_workgroup(n)
            for nvert, _ in te.BIG:
                assert not p.delta_in_lds(nvert, 3) and not p.delta_in_lds(nvert, 3, wide=True) and not p.fused(nvert, 2 * nvert - 4)["fused"]
        finally:
            p.close()
    assert te.record_nvert() > te.blob_max() and te.record_nvert() > te.qo.blob_max()
    assert [n for n, _ in te.BIG] == [32768, 65535, 65537] and [u for _, u in te.BIG] == [True, True, False]


@pytest.mark.parametrize("nvert", [n for n, _ in te.BIG])
def test_big_blobs(nvert):
    """measured: 2 - 4 fallback vertices; encode, oracle and model well under a second each"""
    e = te.sized(nvert)
    assert e.nvert == nvert and e.nface == 2 * nvert - 4 and int(e.index.max()) == nvert - 1
    capped(e, nvert)
    hook_equals_model(e, ("big", nvert), nfmts=[ca.FMT_INT16])


def test_companion_blobs():
    """the blobs that sit beside the named ones in a batch: the cap and the hook on them too (a blob without stored normals gets the direction
    of its decoded position as one - any normal serves the comparison)"""
    for e, stored in te.companions():
        if stored:
            capped(e, e.nvert)
            hook_equals_model(e, ("companion", e.nvert), nfmts=[ca.FMT_FLOAT])
        else:
            pos = e.tr["position"].astype(np.float64)
            nrm = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(np.float32)
            exp, fb, _ = e.model(ca.FMT_INT16, normal=nrm)
            assert int(fb.sum()) <= te.FALLBACK_CAP, (e.nvert, int(fb.sum()))
            got = ca.tangent_model(e.P, e.t, e.index, nrm, fmt=ca.FMT_INT16, which=0 if te.one_workgroup(e.nvert) else 1, seed=2)
            ct.assert_bytes(got, exp, ("companion", e.nvert, "computed"))
