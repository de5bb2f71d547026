"""The decoder's size-class limits by the planner's own predicates (tests/cpp/size_class_probe.cpp on the library's headers), and every mesh of
tests/test_size_classes_gpu.py on the side of its limit it is named for - sized from ca.probe(blob), the decoded counts the planner sees.
No GPU: the probe is host code and the encoder runs on the CPU."""
import functools

import pytest

import corto_amd as ca
import size_classes as sc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    p = sc.Probe(tmp_path_factory.mktemp("size_class_probe"))
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def counts(kind, *args):
    """decoded (nvert, nface) of a case's blob"""
    blob = {"delta": lambda N, u8, nv: sc.delta_blob(N, u8, nv)[0], "group": lambda nv, comps: sc.group_blob(nv, list(comps))[0],
            "normal": sc.normal_blob, "nface": sc.nface_blob, "format": sc.format_blob,
            "closed": lambda nv: ca.encode(sc.closed_mesh(nv), normal_prediction=ca.ESTIMATED, with_color=False, with_uv=False)}[kind](*args)
    info = ca.probe(blob)
    return info.nvert, info.nface


def test_probe_reproduces_the_limits(probe):
    """the last size inside every class, from the headers: the table the GPU module's sizes were picked from"""
    assert probe.const("DELTA16_LDS_MAX") == 128 * 1024 and probe.const("NORMAL_LDS_MAX") == 150 * 1024
    assert probe.const("NORMAL_FN_LDS_MAX") == 100 * 1024 and probe.const("DELTA16_NVERT_MAX") == 32767
    got = {tag: probe.delta_last(N, u8, wide) for tag, N, u8, wide, _ in sc.DELTA_LIMITS}
    assert got == {tag: last for tag, _, _, _, last in sc.DELTA_LIMITS}
    assert int(probe.ask("fused_last_closed")[0]) == sc.FUSED_LAST == 10822
    assert int(probe.ask("fn_last_closed", probe.const("NORMAL_FN_LDS_MAX"))[0]) == sc.FN_LAST == 2681
    # (meshes with HOLES faces fewer: BORDER's limit)
    last = max(nv for nv in range(sc.FUSED_LAST - 50, sc.FUSED_LAST + 50) if probe.fused(nv, 2 * nv - 4 - sc.HOLES)["fused"])
    assert last == sc.BORDER_LAST
    # position + uv at ~9K vertices: each alone in LDS, not the two in one workgroup
    assert probe.groups(9000, [(3, False), (2, False)]) == ([], [[0], [1]])
    assert probe.groups(8000, [(3, False), (2, False)]) == ([], [[0, 1]])


@pytest.mark.parametrize("case", sc.delta_cases(), ids=[c[0] for c in sc.delta_cases()])
def test_delta_record_cases_are_on_their_side(probe, case):
    cid, tag, N, u8, wide, nvert, inside = case
    nv, _ = counts("delta", N, u8, nvert)
    assert nv == nvert, (cid, nv)
    assert probe.delta_in_lds(nv, N, u8, wide) == inside, "%s: %d vertices %s K-DELTA's LDS records" % (cid, nv, "left" if inside else "entered")
    # (both attributes of a generic case: one workgroup each or the tiles, never a mixed decode)
    n = 1 if u8 else 2
    tiles, groups = probe.groups(nv, [(N, u8)] * n, wide)
    assert (tiles == list(range(n))) == (not inside) and (len(sum(groups, [])) == n) == inside, (cid, tiles, groups)


@pytest.mark.parametrize("case", sc.GROUP_CASES, ids=[c[0] for c in sc.GROUP_CASES])
def test_delta_group_cases_split_as_named(probe, case):
    cid, nvert, comps, want = case
    nv, _ = counts("group", nvert, tuple(comps))
    assert nv == nvert
    assert probe.groups(nv, [(N, False) for N in comps]) == (want[0], want[1]), cid
    if cid == "host_shared":            # (N=4 has N=3's 8-byte records but hosts no `a`: in its place, two groups)
        assert probe.groups(nv, [(4, False), (1, False)]) == ([], [[0], [1]])


@pytest.mark.parametrize("case", sc.normal_cases(), ids=[c[0] for c in sc.normal_cases()])
def test_normal_cases_are_on_their_side(probe, case):
    cid, pred, nvert, fused, _, _ = case
    nv, nf = counts("normal", pred, nvert)
    assert nv == nvert, (cid, nv)
    assert nf == 2 * nv - 4 - (0 if pred == ca.ESTIMATED else sc.HOLES), (cid, nf)
    f = probe.fused(nv, nf)
    assert f["fused"] == fused, "%s: %d vertices / %d faces crossed normal_fused (%s)" % (cid, nv, nf, f)
    assert f["nvert_ok"] and f["nface_ok"], (cid, f)          # (the LDS bound decides here)


def test_unfused_batch_and_format_cases_are_on_their_side(probe):
    sides = [probe.fused(*counts("closed", nv))["fused"] for nv in sc.UNFUSED_BATCH]
    assert sides == [False, True, False, False], sides
    for cid, nvert, N, normals in sc.FORMAT_CASES:
        nv, nf = counts("format", nvert, N, normals)
        assert nv == nvert and (nv * N) % 4 in (1, 2, 3) and nv * N > 10 * 1024, cid
        assert not probe.delta_in_lds(nv, N), cid                                 # k_delta_tiles
        if normals:
            assert not probe.fused(nv, nf)["fused"], cid                         # normal_faces ... normal_vertex


@pytest.mark.parametrize("case", sc.FN_CASES, ids=[c[0] for c in sc.FN_CASES])
def test_face_normal_layout_cases(probe, case):
    """k_normal_blob keeps a blob's face normals in LDS when they fit the launch's request, else in scratch: no label shows which, so
    the probe (the planner's request, plan_jobs.cpp, and the kernel's test, k_normal.hip) pins each case"""
    cid, single, nverts, want = case
    fn_max = 0 if single else probe.const("NORMAL_FN_LDS_MAX")
    blobs = [counts("closed", nv) for nv in nverts]
    assert [b[0] for b in blobs] == nverts
    lds_bytes, layout = probe.fn_layout(fn_max, blobs)
    assert layout == want, (cid, lds_bytes, layout)


def test_nface_bound_is_reachable_with_duplicated_faces(probe):
    """3*nface <= 65535 binds before the LDS limit only when nface > ~2.05*nvert: never for a closed (or open) manifold mesh, whose
    nface < 2*nvert; duplicated faces reach it at 8 000 vertices with the LDS request still inside NORMAL_LDS_MAX"""
    for nv in range(100, 32768, 97):                          # manifold meshes: the LDS bound (or none) decides
        f = probe.fused(nv, 2 * nv - 4)
        assert f["nface_ok"] or not f["lds_ok"], (nv, f)
    inside, outside = counts("nface", sc.NFACE_MAX), counts("nface", sc.NFACE_MAX + 1)
    assert inside == (sc.NFACE_BASE, sc.NFACE_MAX) and outside == (sc.NFACE_BASE, sc.NFACE_MAX + 1)
    fi, fo = probe.fused(*inside), probe.fused(*outside)
    assert fi["fused"] and not fo["fused"] and not fo["nface_ok"] and fo["lds_ok"] and fo["nvert_ok"], (fi, fo)


def test_unreachable_conditions(probe):
    """conditions another bound always takes first - written down so that a change of the headers that makes them reachable is seen:
    nvert <= 32767 in normal_fused (32 768 vertices need more than NORMAL_LDS_MAX whatever nface: the boundary words alone are 128 KB),
    DELTA16_NVERT_MAX in delta_lds_need (the LDS limit comes first for every record), and k_normal_blob's third face-normal layout -
    recomputing them per vertex - which the planner never leaves a blob to: face normals that do not fit NORMAL_FN_LDS_MAX (0 on a
    single-stream context) always get a scratch array, and those that fit raise the launch's request to their size"""
    for nf in (0, 1, 1000, 21845):
        assert not probe.fused(32768, nf)["lds_ok"]
    for _, N, u8, wide, last in sc.DELTA_LIMITS:
        assert last < 32767
    fn_max = probe.const("NORMAL_FN_LDS_MAX")
    sizes = [(nv, 2 * nv - 4) for nv in (4, 100, 1000, 2000, 2681, 2682, 4000, 8000, 10822, 10823)]
    for m in (0, fn_max):
        for a in sizes:
            for b in sizes:
                assert "recompute" not in probe.fn_layout(m, [a, b])[1], (m, a, b)
