"""Every case of tests/value_ranges.py on the side it is named for, before a GPU sees it - from the oracle's integers (its _raw_* / _delta_* traces),
the reference's value coders restated in tests/cstream_model.py and the host model of K-DELTA in tests/test_delta16_model_cpu.py.  No GPU: the
encoder and the oracle run on the CPU."""
import functools

import numpy as np
import pytest

import corto_amd as ca
import value_ranges as vr
from oracle import oracle as oc
from test_delta16_model_cpu import kernel_model

PAIRS = vr.delta_edge_cases()


@functools.lru_cache(maxsize=None)
def traced(case):
    return oc.decode(case.blob(), trace=True)


def sides(case):
    """(redone by the host rule, by the kernel model, the loop that finishes, raw outside, result outside) of one case's blob"""
    o = traced(case)
    P = o["_prediction"]
    redone = model = raw_out = res_out = 0
    loops = set()
    for name, strategy, rel in case.attrs:
        raw, val = o["_raw_" + name], o["_delta_" + name]
        assert np.array_equal(val, vr.s32(case.base + rel)), (case.id, name)        # the oracle decodes the crafted integers
        r, bad_raw, bad_res = vr.host_rule(raw, val)
        got, _, ovf, loop = kernel_model(raw, P, bool(strategy & ca.PARALLEL), False)
        assert np.array_equal(got, val.astype(np.int64)), (case.id, name)
        assert int(ovf) == r, "%s %s: the host rule says %d, the kernel model %d" % (case.id, name, r, ovf)
        redone |= r; model |= int(ovf); raw_out |= bad_raw; res_out |= bad_res
        if r:
            loops.add(loop or "window")
        # the same flag from either loop alone (what $CORTO_DELTA_ROUNDS=1 runs)
        assert int(kernel_model(raw, P, bool(strategy & ca.PARALLEL), False, "rounds")[2]) == r, (case.id, name)
    return redone, loops, raw_out, res_out


@pytest.mark.parametrize("pair", PAIRS, ids=[p[0].id[:-3] for p in PAIRS])
def test_delta_edge_cases_are_on_their_side(pair):
    inside, outside = pair
    assert (inside.redone, outside.redone) == (0, 1)
    for case in pair:
        n = ca.probe(case.blob()).nvert
        assert 150 <= n <= 1500
        redone, loops, raw_out, res_out = sides(case)
        assert redone == case.redone, "%s: named %d, the rule says %d (raw %s, result %s)" % (case.id, case.redone, redone, raw_out, res_out)
        if case.redone:
            if case.why == "raw":                                # a raw delta alone: every result fits
                assert raw_out and not res_out, (case.id, raw_out, res_out)
            else:
                assert case.why == "result" and res_out, (case.id, case.why, raw_out, res_out)
    # the loop the overflowing attribute finishes in is the one the pair names
    o = traced(outside)
    for name, strategy, rel in outside.attrs:
        if vr.host_rule(o["_raw_" + name], o["_delta_" + name])[0]:
            loop = kernel_model(o["_raw_" + name], o["_prediction"], bool(strategy & ca.PARALLEL), False)[3] or "window"
            assert loop == outside.loop, (outside.id, name, loop)
    # the pair differs in the edge value alone
    for (n0, s0, r0), (n1, s1, r1) in zip(inside.attrs, outside.attrs):
        assert (n0, s0) == (n1, s1) and (r0 != r1).sum() <= 1, inside.id


def test_delta_edge_cases_cover_the_table():
    """every kind of edge at every place on both meshes; both loops; every N, both strategies, first and last component; raw-only and result
    overflows; a 32767 -> 32768 slip in the host rule is seen by a named case (checked here, on the CPU)"""
    seen = {tuple(p[0].id.split("_")[3:-1]) for p in PAIRS if p[0].id.startswith("N")}
    for kind in vr.KINDS:
        for where in vr.WHERES:
            for key in ("window", "rounds"):
                assert tuple(kind.split("_")) + (where, key) in seen, (kind, where, key)
    assert {p[1].loop for p in PAIRS} == {"window", "rounds"} and {p[1].why for p in PAIRS} == {"raw", "result"}
    # a rule with 32768 in place of 32767 (or -32769 for -32768) calls these outside cases inside
    lax = 0
    for inside, outside in PAIRS:
        o = traced(outside)
        for name, strategy, rel in outside.attrs:
            raw, val = o["_raw_" + name].astype(np.int64), o["_delta_" + name].astype(np.int64)
            relv = vr.s32(val - val[0])
            if vr.host_rule(raw, val)[0] and raw[1:].max() <= vr.HI + 1 and relv.max() <= vr.HI + 1 and raw[1:].min() >= vr.LO - 1 and relv.min() >= vr.LO - 1:
                lax += 1
    assert lax >= len(PAIRS) - 2, lax                          # (all but the two far_delta pairs sit exactly one step outside)


def test_the_16_bit_disc_of_the_parity_test_is_outside():
    """tests/test_gpu_parity.py::test_delta_values_beyond_int16_are_redone_and_the_context_learns decodes six meshes at 14 .. 20 position bits and
    asserts delta_redone: by the host rule the 17- and 20-bit ones and the 16-bit holey disc (a result, no raw delta) are redone - three blobs"""
    from corto_amd import synth
    far = synth.bumpy_sphere(40, 20, seed=5)
    far.position = far.position + np.float32(900.0)
    meshes = [(synth.bumpy_sphere(48, 24, seed=1), 14), (synth.bumpy_sphere(24, 12, seed=2), 17), (far, 14), (synth.torus(24, 12, seed=3), 20),
              (synth.bumpy_sphere_flipped(32, 16, seed=4), 15), (synth.holey_disc(20, seed=6), 16)]
    sides = []
    for k, (m, bits) in enumerate(meshes):
        blob = ca.encode(m, position_bits=bits, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER if k % 2 else ca.DIFF)
        o = oc.decode(blob, trace=True, color_components=4)
        rules = {a["name"]: vr.host_rule(o["_raw_" + a["name"]], o["_delta_" + a["name"]]) for a in oc.parse_header(blob)["attrs"]
                 if a["codec"] == 1 or (a["codec"] == 2 and k % 2 == 0)}                # (colours are bytes; estimated normals are not delta-coded)
        sides.append(max(r[0] for r in rules.values()))
        if bits == 16:
            assert rules["position"] == (1, False, True)
    assert sides == [0, 1, 0, 1, 0, 1]


HANDON = vr.handon_cases()


@pytest.mark.parametrize("case", HANDON, ids=[c.id for c in HANDON])
def test_handon_cases_have_the_named_widths(case):
    blob = case.blob()
    n = ca.probe(blob).nvert
    widths = vr.stream_widths(blob, case.names)
    strategies = {a["name"]: a["strategy"] for a in oc.parse_header(blob)["attrs"]}
    for name in case.names:
        if case.id.startswith("widen"):
            assert max(widths[name]) <= (16 if strategies[name] & ca.CORRELATED else 15), (case.id, widths)
            assert (n * len(case.attrs[0][2][0])) % 64 != 0
        else:
            assert widths[name] == case.widths[name], (case.id, name, widths[name])
    assert vr.expected_streams(widths, strategies) == case.streams, (case.id, widths)
    o = oc.decode(blob, trace=True)
    redone = 0
    for name in case.names:
        redone |= vr.host_rule(o["_raw_" + name], o["_delta_" + name])[0]
    assert redone == case.redone, case.id
    if case.id.endswith("_w16") and "corr" in case.id or case.id == "position_w16":            # both extremes of the width are there
        raw = o["_raw_" + case.names[0]]
        assert raw[1:].min() == vr.LO and raw[1:].max() == vr.HI, case.id


def test_handon_thresholds_are_pinned_from_both_sides():
    """16 -> 17 in widths_fit's CORRELATED bound would hand the width-17 streams on; 15 -> 16 in the per-component one the width-16 streams: each
    has named cases whose int16_streams would change (by the case table)"""
    by = {c.id: c for c in HANDON}
    assert by["corr_window_w16"].streams == 1 and by["corr_window_w17_pos"].streams == 0 and by["corr_window_w17_neg"].streams == 0
    assert by["position_w16"].streams == 1 and by["position_w17"].streams == 0
    for N in (1, 2, 3, 4):
        assert by["comp_N%d_w15" % N].streams == N and by["comp_N%d_w16_neg" % N].streams == 0 and by["comp_N%d_w16_neg" % N].redone == 0


NORMALS = vr.normal_cases()


def finite(a):
    return bool(np.isfinite(a).all())


@pytest.mark.parametrize("case", NORMALS, ids=[c[0] for c in NORMALS])
def test_normal_cases_are_in_contract(case):
    cid, blob, pred, bits, fused = case
    f = oc.decode(blob)
    assert finite(f["normal"]) and finite(f["position"]), cid


def narrowed(blob, pred):
    """vertices whose octahedral coordinate the int16 output narrows to another value (normal_attribute.cpp:293: Point2s): for DIFF the decoded
    coordinates themselves; for the estimated predictions the int16 normal against the f32 normal pushed through the same last step"""
    if pred == ca.DIFF:
        d = oc.decode(blob, trace=True)["_delta_normal"].astype(np.int64)
        return int(((d < vr.LO) | (d > vr.HI)).any(axis=1).sum())
    f = oc.decode(blob)["normal"]
    i = oc.decode(blob, normal_format=oc.FMT_INT16)["normal"]
    want = np.trunc(f * np.float32(32767)).astype(np.int64)
    return int((np.abs(want - i.astype(np.int64)) > 2).any(axis=1).sum())      # (a narrowed coordinate changes sign: nothing subtle)


def test_int16_narrowing_occurs_at_16_bits():
    """at normal_bits = 16 (unit 32768) a coordinate of +32768 - an axis normal - narrows to -32768: every prediction has a case where the int16
    output differs from the un-narrowed one, and none has below 16 bits"""
    for pred, pname in vr.PREDS:
        n16 = [narrowed(b, pred) for cid, b, p, bits, fused in NORMALS if p == pred and bits == 16 and fused]
        assert max(n16) > 0, (pname, n16)
        low = [narrowed(b, pred) for cid, b, p, bits, fused in NORMALS if p == pred and bits == 15 and fused]
        assert max(low) == 0, (pname, low)


@pytest.mark.parametrize("pred", [ca.ESTIMATED, ca.BORDER], ids=["est", "border"])
def test_correction_pair_is_16_and_17_bits(pred):
    b16, b17 = vr.correction_pair(pred)
    assert vr.correction_width(b16) == 16 and vr.correction_width(b17) == 17
    assert finite(oc.decode(b16)["normal"]) and finite(oc.decode(b17)["normal"])


def test_noisy_normals_cross_the_hand_on_threshold():
    """what separates 15 bits from 16: with noise the correction streams of ESTIMATED / BORDER normals reach width 16 at 15 bits and 17 at 16"""
    w = {bits: max(vr.correction_width(b) for cid, b, p, bts, fused in NORMALS if p != ca.DIFF and bts == bits and fused) for bits in (8, 15, 16)}
    assert w[8] <= 10 and w[15] == 16 and w[16] == 17, w


COLOURS = vr.colour_cases()


@pytest.mark.parametrize("case", COLOURS, ids=[c[0] for c in COLOURS])
def test_colour_cases_wrap(case):
    cid, blob, cc, path = case
    info = ca.probe(blob)
    a = [x for x in info.attrs() if x["name"] == "color"][0]
    assert a["components"] == cc and a["strategy"] == 0         # (the encoder's colours are first-neighbour: value_ranges.colour_cases)
    assert vr.colour_wraps(blob, cc) > 0, cid
    if path == "delta_tiles":
        assert info.nvert == vr.TILES_NVERT
    elif path == "cloud":
        assert info.nface == 0


POSITIONS = vr.position_cases()


@pytest.mark.parametrize("case", POSITIONS, ids=[c[0] for c in POSITIONS])
def test_position_cases_are_in_contract(case):
    cid, blob, pred = case
    o = oc.decode(blob)
    assert finite(o["normal"]) and finite(o["position"]), cid
    assert finite(oc.decode(blob, normal_format=oc.FMT_INT16)["position"])


def test_every_position_family_keeps_every_bit_count():
    ids = {c[0] for c in POSITIONS}
    for m in vr.POSITION_MESHES:
        for bits in (22, 24, 28):
            assert {"%s_b%d_est" % (m, bits), "%s_b%d_border" % (m, bits)} <= ids
        for bits in (1, 2, 3):
            assert "%s_b%d_diff" % (m, bits) in ids
