"""CPU: the cases of tests/meshlet_edges.py - every one reaches the figures it is named for, measured on the oracle's integers by the models
(tests/meshlets.py, tests/meshlet_bounds.py), and the kernels' source on the host (corto_amd.meshlet_model in both partitions,
corto_amd.meshlet_bounds_model) equals the models on it byte for byte.  A change to corto_amd.synth, to the size-class meshes or to the encoder
that takes a case off its edge fails here, not silently on the GPU.  No kernel runs."""
import numpy as np
import pytest

import corto_amd as ca
import meshlet_bounds as mb
import meshlet_edges as me
import meshlets as ml

SEEDS = (0, 3)


def hooks_equal_models(case, params, tag):
    """both hooks on the oracle's integers at `params` against the models, and the properties that do not rest on the models"""
    build = case.build(params)
    ml.check_properties(case.index, case.groups, params, *build, tag=(tag, params, "model"))
    for which in (0, 1):
        got = ca.meshlet_model(case.index, case.groups, *params, which=which, seed=SEEDS[which])
        ml.assert_same(got, build, (tag, params, which))
    exp = case.bounds(params)
    mb.check_properties(case.P, *build[:3], exp, tag=(tag, params, "model"))
    for seed in SEEDS:
        mb.assert_same(ca.meshlet_bounds_model(case.P, case.index, *build, seed=seed), exp, (tag, params, seed))


def records(case, params):
    return [(f, f["record"]) for f in me.figures(case, params)]


def axis_of(r):
    return [int(x) for x in r["cone_axis"]]


def test_every_case_on_the_hooks():
    for cid, case, triples in me.all_cases():
        for params in triples:
            hooks_equal_models(case, params, cid)


# ---- 1. empty and cancelling cones ----

def test_coincident():
    c = me.coincident()
    fs = records(c, me.P_SMALL)
    assert len(fs) >= 2 and (c.P == 12345).all()
    for f, r in fs:
        assert r["box_min"].tolist() == r["box_max"].tolist() == r["center"].tolist() == [12345] * 3
        assert r["radius"] == 0 and f["cone"] == 0 and axis_of(r) == [0, 0, 0] and r["cone_cutoff"] == 127


def test_collinear():
    c = me.collinear()
    assert (c.P[:, 1:] == 0).all() and len(set(c.P[:, 0].tolist())) == c.nvert and (c.P[:, 0] % 7 == 0).all()
    fs = records(c, me.P_SMALL)
    assert len(fs) >= 2
    for f, r in fs:
        assert r["radius"] > 0 and f["cone"] == 0 and axis_of(r) == [0, 0, 0] and r["cone_cutoff"] == 127


@pytest.mark.parametrize("n", [200, 255])
def test_closed_one_meshlet(n):
    """the exact normals of a closed surface sum to zero: cone faces, and len > 0 is false"""
    c = me.closed_one_meshlet(n)
    fs = records(c, me.P_ONE)
    assert len(fs) == 1
    f, r = fs[0]
    assert (f["nv"], f["nt"]) == (n, 2 * n - 4) and f["cone"] == 2 * n - 4, (f["nv"], f["nt"], f["cone"])
    assert f["S"] == [0, 0, 0] and f["S_exact"] == [0, 0, 0]
    assert r["radius"] > 0 and axis_of(r) == [0, 0, 0] and r["cone_cutoff"] == 127


def test_flat_grids():
    seen = set()
    for axis, sign in me.FLAT:
        c = me.flat_grid(axis, sign)
        fs = records(c, me.P_SMALL)
        want = [0, 0, 0]
        want["xyz".index(axis)] = 127 * sign
        assert len(fs) >= 2
        for f, r in fs:
            assert f["cone"] == f["nt"] and axis_of(r) == want and r["cone_cutoff"] == 2, (axis, sign, axis_of(r), r["cone_cutoff"])
            assert r["box_min"]["xyz".index(axis)] == r["box_max"]["xyz".index(axis)] == 0
        seen.add(tuple(want))
    assert len(seen) == 6                                                           # both signs of every axis


# ---- 2. the shift edge and the cutoff's clamp ----

def test_shift_edge():
    """|N| = 2^24 - 1 (shift 0, the last without), 2^24 and 2^24 + 1 (shift 1, the second loses its low bit) as the largest |component| of some
    meshlet's S, in each component and with each sign; and the count of meshlets is the bound's"""
    c = me.shift_edge()
    fs = records(c, me.P_FACE)
    seen = set()
    for f, r in fs:
        assert (f["nv"], f["nt"], f["cone"]) == (3, 1, 1) and f["S"] == f["S_exact"] and r["cone_cutoff"] == 2
        big = max(range(3), key=lambda k: abs(f["S"][k]))
        assert abs(f["S"][big]) in me.SHIFT_MAGNITUDES
        if sum(1 for x in f["S"] if x) == 1:
            seen.add((abs(f["S"][big]), big, f["S"][big] > 0))
            assert axis_of(r) == [127 * ((x > 0) - (x < 0)) for x in f["S"]]
    assert seen == {(mag, k, s) for mag in me.SHIFT_MAGNITUDES for k in range(3) for s in (False, True)}
    assert len(fs) == 18 + len(me.SHIFT_TILTS)
    assert [max(0, mag.bit_length() - 24) for mag in me.SHIFT_MAGNITUDES] == [0, 1, 1]
    assert c.build(me.P_FACE)[3][0] == c.nface == ca.meshlet_bound(c.nface, c.groups, *me.P_FACE).meshlets


def test_a_missed_shift_edge_changes_the_bytes():
    """an axis-aligned normal hides the shift; the tilted faces do not: the model with every shift one too large, or one too small, writes
    other records for the faces named for that error, at each of the three magnitudes where the error can happen"""
    c = me.shift_edge()
    exp, fs = c.bounds(me.P_FACE), me.figures(c, me.P_FACE)
    covered = set()
    for dk in (1, -1):
        got = me.bounds_with_shift(c, me.P_FACE, dk)
        changed = {k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()}
        for legs, y, dks in me.SHIFT_TILTS:
            a, b = me.SHIFT_LEGS[legs]
            at = [k for k, f in enumerate(fs) if sorted(abs(x) for x in f["S"]) == sorted([b, y, a * b])]
            assert len(at) == 1, (legs, y, at)
            if dk in dks:
                assert at[0] in changed, (legs, y, dk)
                covered.add((a * b, dk))
    assert covered == {(me.SHIFT_MAGNITUDES[0], 1)} | {(mag, dk) for mag in me.SHIFT_MAGNITUDES[1:] for dk in (1, -1)}
    assert me.bounds_with_shift(c, me.P_FACE, 0).tobytes() == exp.tobytes()


def test_cutoff_clamp():
    """int(sqrtf(1 - m*m)*127) + 2 at 126, the last value the clamp leaves alone, and at 127 and beyond it with m > 0.1, by the model"""
    c = me.cutoff_clamp()
    fs = records(c, me.P_FOLD)
    assert len(fs) == len(me.FOLDS) and all((f["nv"], f["nt"], f["cone"]) == (4, 2, 2) for f, _ in fs)
    raw = sorted(f["raw_cutoff"] for f, _ in fs)
    assert raw == sorted(me.FOLD_RAW), raw
    assert 126 in raw and 127 in raw and max(raw) > 127
    for f, r in fs:
        assert f["m"] > np.float32(0.1) and r["cone_cutoff"] == min(127, f["raw_cutoff"])


# ---- 3. lane-stride rounds ----

def test_rounds():
    c = me.rounds()
    hv, hf = me.classes_hit(c, me.ROUND_PARAMS)
    assert hv == set(range(len(me.VERTEX_CLASSES))), hv
    assert hf == set(range(len(me.FACE_CLASSES))), hf
    counts = {int(n) for params in me.ROUND_PARAMS for n in c.build(params)[0][:, 2]}
    assert {65, 128, 129, 192, 193, 254} <= counts                                  # a round of one lane, full rounds, a round less one lane
    assert all(f["cone"] > 0 for params in me.ROUND_PARAMS for f in me.figures(c, params))


def test_full_meshlet():
    a, b = me.full_meshlet(250), me.full_meshlet(252)
    assert a.build(me.P_ONE)[0][:, 2:].tolist() == [[250, 512]]
    m = b.build(me.P_ONE)[0][:, 2:].tolist()
    assert len(m) == 2 and m[0] == [252, 512] and m[1][1] == b.nface - 512
    for c in (a, b):
        f = me.figures(c, me.P_ONE)[0]
        assert f["cone"] == 512 and any(f["S"])


# ---- 4. wide values ----

@pytest.mark.parametrize("stored", [True, False])
def test_wide(stored):
    c = me.wide(stored)
    assert c.redone() and int(np.abs(c.P.astype(np.int64)).max()) == 1074789632
    assert ("normal" in c.tr) == stored
    for n, params in enumerate(me.WIDE_PARAMS):
        fs = me.figures(c, params)
        if n == 0:
            assert max(f["nv"] for f in fs) == 255 and any(f["nv"] > 64 and f["nt"] > 448 for f in fs)
        else:
            assert len(fs) == 8
        hit = [f for f in fs if f["nv"] > (64 if n == 0 else 0) and f["span"] >= 2 ** 31 and 2 ** 60 <= f["r2"] < 2 ** 63 and f["S"] != f["S_exact"]]
        assert hit, params                                                          # one meshlet with all of it: S wrapped modulo 2^64
        assert max(abs(x) for f in hit for x in f["S"]).bit_length() >= 62


# ---- 5. the grid ----

def test_grid_counts():
    got = [me.grid_case(i).build(me.grid_params(i))[3][0] for i in range(len(me.GRID_COUNTS))]
    assert got == me.GRID_COUNTS == [1, 2, 3, 4, 5, 1]
    assert sum(1 for n in got if n % mb_waves()) == 5                                # five blobs end on a partial workgroup of K-MLB
    for i in range(len(me.GRID_COUNTS)):
        hooks_equal_models(me.grid_case(i), me.grid_params(i), ("grid", i))


def mb_waves():
    """MB_WAVES of csrc/meshlet_bounds.h: meshlets a workgroup of K-MLB"""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "corto_amd", "csrc", "meshlet_bounds.h")).read()
    return int(re.search(r"constexpr uint32_t MB_WAVES = (\d+);", src).group(1))


# ---- 6. 4 | 5 segments ----

def test_segments():
    c = me.segment_case()
    assert c.groups in ((), (c.nface,))
    got = []
    for params, nsegs in me.segment_params():
        assert c.build(params)[3][3] == nsegs == ca.meshlet_bound(c.nface, c.groups, *params).segments
        got.append(nsegs)
        hooks_equal_models(c, params, "segments")
    assert got == [1, 2, 4, 5]
    (_, _, q), (_, _, q1) = me.segment_params()[2][0], me.segment_params()[3][0]
    assert q1 == q - 1 and 4 * q >= c.nface > 4 * q1
