"""GPU (-m gpu): k_meshlet_blob, k_meshlet_segments / k_meshlet_place and k_meshlet_bounds at the edges of tests/meshlet_edges.py
(tests/test_meshlet_edges_cpu.py shows that every case reaches the figures it is named for) - raw bytes against the sequential models
(tests/meshlets.py, tests/meshlet_bounds.py) on the oracle's integers, the properties that do not rest on the models, every other output
against a batch without the bindings.  The meshlet arrays and the records live in device buffers pre-filled with 0xCD, each array at exactly
its bound: nothing past the counts may change."""
import pytest

import corto_amd as ca
import meshlet_bounds as mb
import meshlet_edges as me
import meshlets as ml
from test_meshlet_bounds_gpu import BoundB
from test_meshlets_gpu import Bound, expect_ran, index_kw, make_ctx, run, same_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = mb.FILL
KERNEL = "meshlet_bounds"


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def plain_outputs(ctx, blobs, **kw):
    """the outputs of a batch of these blobs without a meshlet binding"""
    p = ca.Batch(ctx, blobs)
    p.allocate_outputs(fill=FILL, **kw)
    run(p)
    assert not any(k.startswith("meshlet") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(blobs))]
    p.close()
    return ref


def check(b, bb, cases, params, ref, tag):
    """a decoded batch whose blob i is cases[i] bound at params[i]: meshlets and, where bb has them, records against the models; the
    properties; the other outputs against `ref`"""
    meshlets = bb.read()
    bounds = bb.read_bounds() if isinstance(bb, BoundB) else {}
    for i, case in enumerate(cases):
        build = case.build(params[i])
        ml.assert_same(meshlets[i], build, (tag, i, params[i], "meshlets"))
        got = meshlets[i]
        ml.check_properties(case.index, case.groups, params[i], *got[:3], got[3].as_tuple(), tag=(tag, i, params[i]))
        if i in bounds:
            mb.check_properties(case.P, *got[:3], bounds[i], tag=(tag, i, params[i]))
            mb.assert_same(bounds[i], case.bounds(params[i]), (tag, i, params[i], "bounds"))
        same_outputs(b.host_outputs(i), ref[i], (tag, i, "the batch without bindings"))
    return meshlets, bounds


def decode_bound(ctx, cases, params, tag, device_counts=True, mode="u32", **kw):
    """one batch of `cases`, blob i bound at params[i] with bounds, decoded twice (the same bytes over the old ones), checked"""
    kw = dict(index_kw(mode), **kw)
    blobs = [c.blob for c in cases]
    ref = plain_outputs(ctx, blobs, **kw)
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=FILL, **kw)
    bb = BoundB(b, dict(enumerate(params)), device_counts=device_counts)
    for again in range(2):
        run(b)
        assert KERNEL in b.kernel_times()
        res = check(b, bb, cases, params, ref, (tag, mode, again))
    return b, bb, res


# ---- 1, 2, 3. the cones' edges, the shift edge, the clamp, 512 faces: one batch, every blob at the triple of its own ----

def cones():
    return [(cid, case, triples[0]) for cid, case, triples in me.all_cases() if len(triples) == 1]


@pytest.mark.parametrize("mode,device_counts", [("u32", True), ("u16", False)])
def test_cone_edges(ctx, mode, device_counts):
    CONES = cones()
    ids = [cid for cid, _, _ in CONES]
    assert {"coincident", "collinear", "closed_200", "closed_255", "flat_z+", "flat_x-", "flat_y-", "shift_edge", "cutoff_clamp", "full_512", "past_512"} <= set(ids)
    b, bb, (meshlets, bounds) = decode_bound(ctx, [c for _, c, _ in CONES], [p for _, _, p in CONES], "cones", device_counts, mode)
    at = ids.index("shift_edge")                                                     # the count at its capacity: every record written, the poison behind intact
    assert meshlets[at][3].meshlets == bb.bat[at][1] == bb.at[at][0].meshlets == me.shift_edge().nface
    b.close()


def test_lane_stride_rounds(ctx):
    """one blob six times in a batch, each at a triple of ROUND_PARAMS: every short last round of the vertex and the face loops"""
    c = me.rounds()
    b, _, _ = decode_bound(ctx, [c] * len(me.ROUND_PARAMS), me.ROUND_PARAMS, "rounds")
    b.close()


# ---- 4. wide values in big meshlets, on a fresh context and on one that has learned the wide layout ----

@pytest.fixture(scope="module")
def wide_ref(ctx):
    return {how: plain_outputs(ctx, [me.wide(how == "float").blob], **kw) for how, kw in WIDE_KW.items()}


WIDE_KW = {"float": {}, "computed_normals": dict(computed_normals=True, only={"position", "index", "normal"})}


@pytest.mark.parametrize("how", sorted(WIDE_KW))
@pytest.mark.parametrize("single", [False, True], ids=["two_streams", "single_stream"])
def test_wide_values(wide_ref, single, how):
    """the blob alone on a fresh context, where K-DELTA's int16 records overflow and the position is redone in the kernel with K-MLB behind it,
    then again on that context, which has learned the wide layout: the model's bytes both times"""
    case = me.wide(how == "float")
    for params in me.WIDE_PARAMS:
        c = make_ctx(single)
        try:
            b = ca.Batch(c, [case.blob])
            b.allocate_outputs(fill=FILL, **WIDE_KW[how])
            bb = BoundB(b, {0: params})
            for again in (False, True):
                run(b)
                st = b.stats()
                assert (st.delta_redone > 0, st.delta_wide) == ((True, 0) if not again else (False, 1)), (params, again, st.delta_redone, st.delta_wide)
                ran = set(b.kernel_times())
                assert KERNEL in ran and ("normal_blob_computed" in ran or how == "float"), sorted(ran)
                check(b, bb, [case], [params], wide_ref[how], ("wide", how, single, params, again))
            b.close()
        finally:
            c.close()


# ---- 5. the grid: partial last workgroups behind one another ----

@pytest.mark.parametrize("device_counts", [True, False], ids=["device_counts", "counts_in_scratch"])
def test_partial_workgroups(ctx, device_counts):
    """blobs of 1, 2, 3, 4, 5 and 1 meshlets in this order, all with bounds: five end on a partial workgroup with another job's blocks behind"""
    n = len(me.GRID_COUNTS)
    cases, params = [me.grid_case(i) for i in range(n)], [me.grid_params(i) for i in range(n)]
    b, _, (meshlets, bounds) = decode_bound(ctx, cases, params, "grid", device_counts)
    assert [meshlets[i][3].meshlets for i in range(n)] == [len(bounds[i]) for i in range(n)] == me.GRID_COUNTS
    b.close()


# ---- 6. the builder: 1, 2, 4 and 5 segments ----

@pytest.mark.parametrize("bounds", [False, True], ids=["meshlets", "with_bounds"])
@pytest.mark.parametrize("mode", ["u32", "u16"])
def test_four_and_five_segments(ctx, mode, bounds):
    """each blob alone in its batch: meshlet_blob alone up to MESHLET_BLOB_SEGS (4) segments, meshlet_segments and meshlet_place alone from 5;
    with bounds K-MLB reads what each path left"""
    case = me.segment_case()
    ref = plain_outputs(ctx, [case.blob], **index_kw(mode))
    for params, nsegs in me.segment_params():
        b = ca.Batch(ctx, [case.blob])
        b.allocate_outputs(fill=FILL, **index_kw(mode))
        bb = BoundB(b, {0: params}) if bounds else Bound(b, {0: params})
        run(b)
        expect_ran(b, nsegs <= 4, nsegs > 4)
        assert (KERNEL in b.kernel_times()) == bounds
        meshlets, _ = check(b, bb, [case], [params], ref, ("segments", mode, params))
        assert meshlets[0][3].segments == nsegs
        b.close()
