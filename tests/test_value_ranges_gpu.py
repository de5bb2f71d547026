"""GPU (-m gpu): the decoder on both sides of every value-range limit (tests/value_ranges.py; tests/test_value_ranges_cpu.py checks that each case
is on the side it is named for), bit for bit against the oracle, with the counter each pair is named for - crthip_batch_stats.delta_redone,
.int16_streams, the context's kernel labels - on the named side, on two-stream and single-stream contexts; and the encoders' entry points on
the normal, colour and position corners against the host encoder.  Well-formed blobs of the project's own encoder throughout."""
import functools

import numpy as np
import pytest

import corto_amd as ca
import value_ranges as vr
from oracle import oracle as oc
from test_size_classes_gpu import assert_same, device_buffer, normal_path

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

SINGLE = pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])


def make_ctx(single, profiling=False):
    c = ca.Context(0)
    if single:
        c.set_single_stream(True)
    if profiling:
        c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctxs():
    cs = {False: make_ctx(False, True), True: make_ctx(True, True)}
    yield cs
    for c in cs.values():
        c.close()


class Scope:
    """the contexts and batches a test makes, closed behind it whether it passes or not (batches first)"""

    def __init__(self):
        self.ctxs, self.batches = [], []

    def ctx(self, single):
        self.ctxs.append(make_ctx(single))
        return self.ctxs[-1]

    def batch(self, ctx, blobs):
        self.batches.append(ca.Batch(ctx, blobs))
        return self.batches[-1]

    def close(self):
        for x in self.batches + self.ctxs:
            x.close()


@pytest.fixture
def scope():
    s = Scope()
    yield s
    s.close()


def run(scope, ctx, blobs, **kw):
    """one decode through ca.Batch.allocate_outputs"""
    kw.setdefault("fill", 0)
    b = scope.batch(ctx, blobs)
    b.allocate_outputs(**kw)
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return b


# ------------------------------------------------------------------------------------------------------------------------------------
# K-DELTA's int16 check

PAIRS = vr.delta_edge_cases()


@functools.lru_cache(maxsize=None)
def expected(case, fmt):
    """{name: the bytes of the attribute's output} by the oracle"""
    blob = case.blob()
    nv = ca.probe(blob).nvert
    if fmt == ca.FMT_FLOAT:
        o = oc.decode(blob, bind=set(case.names))
        return {nm: o[nm].tobytes() for nm in case.names}
    N = {a["name"]: a["N"] for a in oc.parse_header(blob)["attrs"]}
    return {nm: oc.decode_attr_format(blob, nm, fmt)[:nv * N[nm] * 4].tobytes() for nm in case.names}


def bound_batch(scope, ctx, case, fmt):
    """a batch of the case's blob with its named attributes bound packed in `fmt` (the others unbound) and a u32 index"""
    b = scope.batch(ctx, [case.blob()])
    info = b.infos[0]
    bufs, binds = {}, []
    for a in info.attrs():
        bd = ca.AttrBinding()
        if a["name"] in case.names:
            bufs[a["name"]] = device_buffer(info.nvert * a["components"] * 4)
            bd.buffer, bd.format = bufs[a["name"]].data_ptr(), fmt
        binds.append(bd)
    idx = device_buffer(info.nface * 12)
    b.bind(0, binds, idx.data_ptr(), ca.FMT_UINT32)
    return b, bufs, idx


def decode_and_check(b, bufs, case, fmt, tag):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), (tag, st)
    want = expected(case, fmt)
    for nm, t in bufs.items():
        got = t.cpu().numpy().tobytes()
        if got != want[nm]:
            g, w = np.frombuffer(got, np.int32), np.frombuffer(want[nm], np.int32)
            bad = np.flatnonzero(g != w)
            raise AssertionError("%s %s: %d of %d words differ, first at %d: got %d expected %d" % (tag, nm, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]]))
    return b.stats()


@SINGLE
@pytest.mark.parametrize("pair", PAIRS, ids=[p[0].id[:-3] for p in PAIRS])
def test_delta_edge_pairs(scope, pair, single):
    """last inside / first outside K-DELTA's int16 check, each on a fresh context, as INT32 and as FLOAT: delta_redone is the CPU module's number,
    the bytes the oracle's; the outside case again on its context: planned wide, nothing redone, the same bytes"""
    for case in pair:
        for fmt in (ca.FMT_INT32, ca.FMT_FLOAT):
            ctx = scope.ctx(single)
            tag = "%s fmt %d single %s" % (case.id, fmt, single)
            b, bufs, idx = bound_batch(scope, ctx, case, fmt)
            st = decode_and_check(b, bufs, case, fmt, tag)
            assert st.delta_redone == case.redone and st.delta_wide == 0, (tag, st.delta_redone, st.delta_wide)
            if case.redone:
                st = decode_and_check(b, bufs, case, fmt, tag + " again")
                assert st.delta_redone == 0 and st.delta_wide == 1, (tag, "again", st.delta_redone, st.delta_wide)
            b.close(); ctx.close()


@SINGLE
@pytest.mark.parametrize("env", [{"CORTO_DELTA_ROUNDS": "1"}, {"CORTO_DELTA_WIDE": "1"}, {"CORTO_DELTA_ROUNDS": "1", "CORTO_DELTA_WIDE": "1"}],
                         ids=lambda e: "+".join(sorted(e)))
def test_delta_edge_pairs_under_context_settings(scope, monkeypatch, env, single):
    """both sides of every pair with the round loop from vertex 1 (its own check sees the edge) and with 32-bit records (nothing can overflow): one
    context a setting, the inside cases in one batch (nothing redone, the context stays narrow), then the outside cases (every blob redone)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = scope.ctx(single)                                   # (the switches are read when a context is made)
    wide = "CORTO_DELTA_WIDE" in env
    for side in (0, 1):
        cases = [p[side] for p in PAIRS]
        names = {nm for c in cases for nm in c.names}
        b = run(scope, ctx, [c.blob() for c in cases], only=names | {"index"})
        st = b.stats()
        assert st.delta_wide == int(wide) and st.delta_redone == (0 if wide else sum(c.redone for c in cases)), (env, side, st.delta_wide, st.delta_redone)
        for i, c in enumerate(cases):
            got = b.host_outputs(i)
            want = expected(c, ca.FMT_FLOAT)
            for nm in c.names:
                assert got[nm].tobytes() == want[nm], (env, c.id, nm)
        b.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# K-BIT's hand-on

HANDON = vr.handon_cases()


@SINGLE
@pytest.mark.parametrize("case", HANDON, ids=[c.id for c in HANDON])
def test_handon_cases(scope, case, single):
    """int16_streams and delta_redone as the case table names them, on a fresh context; the oracle's bytes"""
    ctx = scope.ctx(single)
    b, bufs, idx = bound_batch(scope, ctx, case, ca.FMT_FLOAT)
    st = decode_and_check(b, bufs, case, ca.FMT_FLOAT, case.id)
    assert st.int16_streams == case.streams and st.delta_redone == case.redone and st.delta_wide == 0, (case.id, st.int16_streams, st.delta_redone)
    b.close(); ctx.close()


@SINGLE
def test_handon_cases_with_32_bit_values(scope, monkeypatch, single):
    """the same blobs with $CORTO_VALUES_I32=1: nothing handed on as halfwords, the same bytes (one context, the cases that are not redone in one
    batch, then the others)"""
    monkeypatch.setenv("CORTO_VALUES_I32", "1")
    ctx = scope.ctx(single)
    for redone in (0, 1):
        cases = [c for c in HANDON if c.redone == redone]
        b = run(scope, ctx, [c.blob() for c in cases], only={nm for c in cases for nm in c.names} | {"index"})
        st = b.stats()
        assert st.int16_streams == 0 and st.delta_redone == redone * len(cases), (redone, st.int16_streams, st.delta_redone)
        for i, c in enumerate(cases):
            got = b.host_outputs(i)
            want = expected(c, ca.FMT_FLOAT)
            for nm in c.names:
                assert got[nm].tobytes() == want[nm], (c.id, nm)
        b.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# normals, colours, positions: batched by family

NORMAL_KEYS = ["position", "normal", "index"]
FORMATS = [(ca.FMT_FLOAT, False, "f32"), (ca.FMT_INT16, True, "i16")]


def check_batch(scope, ctx, items, keys, fused=None, **kw):
    """items [(id, blob)] in one batch against the oracle; fused: the normal path the batch must take (None: not asserted).  Returns the kernels
    that ran (a profiling context)"""
    b = run(scope, ctx, [x[1] for x in items], **kw)
    okw = {k: v for k, v in kw.items() if k in ("normal_format", "index16", "color_components")}
    for i, (cid, blob) in enumerate(items):
        ref = oc.decode(blob, **okw)
        assert_same(b.host_outputs(i), ref, [k for k in keys if k in ref], cid)
    ran = set(b.kernel_times())
    if fused is not None:
        normal_path(ran, fused, items[0][0])
    b.close()
    return ran


@SINGLE
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[2] for f in FORMATS])
@pytest.mark.parametrize("pred", vr.PREDS, ids=[p[1] for p in vr.PREDS])
def test_normal_bits_1_to_16(scope, ctxs, pred, fmt, single):
    """normal_bits 1, 2, 3, 8, 15, 16 with noisy normals on a closed mesh, an open one and a cloud, f32 and int16 output: the fused kernel, and at
    15 / 16 bits the unfused chain on meshes past its limit"""
    cases = [c for c in vr.normal_cases() if c[2] == pred[0]]
    kw = dict(normal_format=fmt[0], index16=fmt[1])
    meshes = [(c[0], c[1]) for c in cases if c[4] and ca.probe(c[1]).nface]
    clouds = [(c[0], c[1]) for c in cases if c[4] and not ca.probe(c[1]).nface]
    check_batch(scope, ctxs[single], meshes, NORMAL_KEYS, fused=None if pred[0] == ca.DIFF else True, **kw)
    if clouds:                                                # (none under ESTIMATED)
        check_batch(scope, ctxs[single], clouds, NORMAL_KEYS, **kw)
    unfused = [(c[0], c[1]) for c in cases if not c[4]]
    if unfused:
        check_batch(scope, ctxs[single], unfused, NORMAL_KEYS, fused=False, **kw)


@SINGLE
@pytest.mark.parametrize("pred", [ca.ESTIMATED, ca.BORDER], ids=["est", "border"])
def test_correction_stream_at_16_and_17_bits(scope, pred, single):
    """k_normal_blob takes the corrections as halfwords (diffs_i16) when their widest field is 16 bits and as words when it is 17: one normal turned
    a step further, one int16 stream fewer, nothing else changes; the oracle's bytes as f32 and int16 on both sides"""
    streams = []
    for blob in vr.correction_pair(pred):
        for fmt, i16, fname in FORMATS:
            ctx = scope.ctx(single)
            b = run(scope, ctx, [blob], normal_format=fmt, index16=i16)
            assert_same(b.host_outputs(0), oc.decode(blob, normal_format=fmt, index16=i16), NORMAL_KEYS, fname)
            streams.append(b.stats().int16_streams)
            assert b.stats().delta_redone == 0
    assert streams[0] == streams[1] and streams[2] == streams[3] and streams[0] - streams[2] == 1, streams


@SINGLE
def test_colour_quantisation(scope, ctxs, single):
    """every color_bits tuple, 3 and 4 stored components out as 4, random bytes (the u8 sums wrap): K-DELTA's LDS records, k_delta_tiles at 13 105
    vertices, clouds (k_cloud_* then k_dequant); packed and in an interleaved vertex record (stride 16)"""
    cases = vr.colour_cases()
    for path in ("delta_lds16", "delta_tiles", "cloud"):
        items = [(c[0], c[1]) for c in cases if c[3] == path]
        ran = check_batch(scope, ctxs[single], items, ["color", "index"], only={"color", "index"}, color_components=4)
        if path == "cloud":
            assert {"cloud_sums", "cloud_apply", "dequantize"} <= ran and not ({"delta_lds16", "delta_tiles"} & ran), sorted(ran)
        else:
            assert path in ran and not ({"delta_lds16", "delta_tiles"} - {path}) & ran, (path, sorted(ran))
        b = scope.batch(ctxs[single], [x[1] for x in items])
        metas = b.allocate_interleaved(fill=0)
        assert all(m[1] == 16 for m in metas)                 # position f32x3 | colour u8x4
        b.decode()
        assert (b.sync() == 0).all()
        for i, (cid, blob) in enumerate(items):
            ref = oc.decode(blob, color_components=4, index16=True)
            assert_same(b.host_outputs(i), ref, ["position", "color"] + (["index"] if "index" in ref else []), cid + " interleaved")
        b.close()


@SINGLE
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[2] for f in FORMATS])
def test_position_bits_beyond_20_and_below_4(scope, ctxs, fmt, single):
    """22, 24 and 28 bits under ESTIMATED / BORDER normals (sphere, Delaunay disc with holes, cone with a high-valence apex), 1 .. 3 bits under DIFF"""
    cases = vr.position_cases()
    for pred, pname in vr.PREDS:
        items = [(c[0], c[1]) for c in cases if c[2] == pred]
        check_batch(scope, ctxs[single], items, ["position", "normal", "color", "uv", "index"], fused=None if pred == ca.DIFF else True,
                    normal_format=fmt[0], index16=fmt[1], color_components=4)


# ------------------------------------------------------------------------------------------------------------------------------------
# the encoders at the corners

def test_encoders_at_the_corners(scope):
    """the normal, colour and position cases through encode(ctx=), encode_batch, encode_batch_resident and encode_batch_to_device: the host
    encoder's bytes from each"""
    items = vr.encoder_corners()
    ms, ks = [m for _, m, _ in items], [k for _, _, k in items]
    want = [ca.encode(m, **k).tobytes() for m, k in zip(ms, ks)]
    ctx = scope.ctx(False)

    def same(tag, blobs):
        assert len(blobs) == len(want), tag
        for (cid, _, _), g, w in zip(items, blobs, want):
            assert len(g) == len(w) and bytes(g) == w, (tag, cid, len(g), len(w))
    same("encode_batch", [b.tobytes() for b in ca.encode_batch(ms, ctx, kw=ks)])
    dm = [ca.mesh_to_device(m) for m in ms]
    same("encode_batch_resident", [b.tobytes() for b in ca.encode_batch_resident(dm, ctx, kw=ks)])
    out, offs, lens = ca.encode_batch_to_device(dm, ctx, kw=ks, resident=True)
    arena = out.cpu().numpy()
    same("encode_batch_to_device", [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)])
    same("encode(ctx=)", [ca.encode(m, ctx=ctx, **k).tobytes() for m, k in zip(ms, ks)])
