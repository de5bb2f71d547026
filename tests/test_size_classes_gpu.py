"""GPU (-m gpu): the decoder on both sides of every size-class limit (tests/size_classes.py; tests/test_size_classes_cpu.py checks that each
case is on the side it is named for), bit for bit against the oracle, each case on the path it is meant to take (the context's kernel
labels), on a two-stream context (the tiles beside the automaton) and a single-stream one (behind it)."""
import functools

import numpy as np
import pytest

import corto_amd as ca
import size_classes as sc
from oracle import oracle as oc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = 0xCD


def make_ctx(single):
    c = ca.Context(0)
    if single:
        c.set_single_stream(True)
    c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctxs():
    cs = {False: make_ctx(False), True: make_ctx(True)}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    p = sc.Probe(tmp_path_factory.mktemp("size_class_probe"))
    yield p
    p.close()


def assert_same(got, exp, keys, tag):
    for k in keys:
        a, e = got[k], exp[k]
        assert a.dtype == e.dtype and a.shape == e.shape, (tag, k, a.dtype, e.dtype, a.shape, e.shape)
        if a.tobytes() != e.tobytes():
            bad = np.argwhere(a.reshape(len(a), -1) != e.reshape(len(e), -1))
            raise AssertionError("%s %s: %d mismatching entries, first %s got %s expected %s" % (
                tag, k, len(bad), bad[0], a.reshape(len(a), -1)[bad[0][0]], e.reshape(len(e), -1)[bad[0][0]]))


def decode(ctx, blobs, **kw):
    """one decode through ca.Batch: the batch and the kernels that ran"""
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=0, **kw)
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return b, set(b.kernel_times())


@functools.lru_cache(maxsize=None)
def delta_blob(N, u8, nvert):
    blob, names = sc.delta_blob(N, u8, nvert)
    return blob, names, oc.decode(blob, bind=set(names), color_components=N if u8 else 4)


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("case", sc.delta_cases(), ids=[c[0] for c in sc.delta_cases()])
def test_delta_records_at_their_limits(ctxs, monkeypatch, case, single):
    """last inside / first outside K-DELTA's LDS records (int16, colour bytes, 32-bit): k_delta_lds16 on one side, k_delta_tiles on the
    other; two generic attributes of N components (parallelogram, first neighbour) or a colour, the positions unbound"""
    cid, tag, N, u8, wide, nvert, inside = case
    blob, names, ref = delta_blob(N, u8, nvert)
    if wide:
        monkeypatch.setenv("CORTO_DELTA_WIDE", "1")
        ctx = make_ctx(single)
    else:
        ctx = ctxs[single]
    b, ran = decode(ctx, [blob], only=set(names) | {"index"}, color_components=N if u8 else None)
    assert_same(b.host_outputs(0), ref, names + ["index"], cid)
    assert ("delta_lds16" in ran) == inside and ("delta_tiles" in ran) == (not inside), (cid, sorted(ran))
    b.close()
    if wide:
        ctx.close()


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("case", sc.GROUP_CASES, ids=[c[0] for c in sc.GROUP_CASES])
def test_delta_groups(ctxs, case, single):
    """attributes of one blob split over k_delta_lds16 workgroups (with and without the hosted `a`), beside k_delta_tiles jobs and
    five-component slices (tests/test_size_classes_cpu.py pins the split)"""
    cid, nvert, comps, (tiles, groups) = case
    blob, names = sc.group_blob(nvert, comps)
    ref = oc.decode(blob, bind=set(names))
    b, ran = decode(ctxs[single], [blob], only=set(names) | {"index"})
    assert_same(b.host_outputs(0), ref, names + ["index"], cid)
    assert ("delta_tiles" in ran) == bool(tiles) and ("delta_lds16" in ran) == bool(groups), (cid, sorted(ran))
    b.close()


NORMAL_KEYS = ["position", "normal", "index"]


def normal_path(ran, fused, tag):
    if fused:
        assert "normal_blob" in ran and "normal_faces" not in ran and "normal_vertex" not in ran, (tag, sorted(ran))
    else:
        assert "normal_faces" in ran and "normal_vertex" in ran and "normal_blob" not in ran, (tag, sorted(ran))


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("case", sc.normal_cases(), ids=[c[0] for c in sc.normal_cases()])
def test_normals_at_the_fused_limit(ctxs, case, single):
    """each side of normal_fused, ESTIMATED (closed meshes) and BORDER (open ones), f32 / int16 normals, u32 / u16 indices"""
    cid, pred, nvert, fused, fmt, i16 = case
    blob = sc.normal_blob(pred, nvert)
    ref = oc.decode(blob, normal_format=fmt, index16=i16)
    b, ran = decode(ctxs[single], [blob], normal_format=fmt, index16=i16)
    assert_same(b.host_outputs(0), ref, NORMAL_KEYS, cid)
    normal_path(ran, fused, cid)
    b.close()


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
def test_normals_at_the_nface_bound(ctxs, single):
    """3*nface <= 65535: 8 000 vertices and duplicated faces, nface on the bound (k_normal_blob) and one past it (the chain)"""
    for nface, fused in ((sc.NFACE_MAX, True), (sc.NFACE_MAX + 1, False)):
        blob = sc.nface_blob(nface)
        b, ran = decode(ctxs[single], [blob])
        assert_same(b.host_outputs(0), oc.decode(blob), NORMAL_KEYS, "nface %d" % nface)
        normal_path(ran, fused, nface)
        b.close()


def closed_est(nvert, seed=0):
    return ca.encode(sc.closed_mesh(nvert, seed=seed), normal_prediction=ca.ESTIMATED, with_color=False, with_uv=False)


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
def test_unfused_normal_blobs_in_one_batch(ctxs, single):
    """three unfused ESTIMATED blobs in one batch (their vertices and faces at vbase / fbase in the chain's arrays) and a fused one"""
    blobs = [closed_est(nv, seed=k) for k, nv in enumerate(sc.UNFUSED_BATCH)]
    b, ran = decode(ctxs[single], blobs)
    for i, x in enumerate(blobs):
        assert_same(b.host_outputs(i), oc.decode(x), NORMAL_KEYS, "blob %d" % i)
    assert {"normal_blob", "normal_faces", "normal_vertex"} <= ran, sorted(ran)
    b.close()


@pytest.mark.parametrize("case", sc.FN_CASES, ids=[c[0] for c in sc.FN_CASES])
def test_face_normal_layouts(ctxs, probe, case):
    """k_normal_blob's face normals in LDS, in scratch, and in LDS because a bigger partner raised the launch's request - the same
    meshes, bit for bit (the probe names the layout: no label shows it)"""
    cid, single, nverts, want = case
    blobs = [closed_est(nv, seed=k) for k, nv in enumerate(nverts)]
    fn_max = 0 if single else probe.const("NORMAL_FN_LDS_MAX")
    assert probe.fn_layout(fn_max, [(ca.probe(x).nvert, ca.probe(x).nface) for x in blobs])[1] == want, cid
    b, ran = decode(ctxs[single], blobs)
    for i, x in enumerate(blobs):
        assert_same(b.host_outputs(i), oc.decode(x), NORMAL_KEYS, "%s blob %d" % (cid, i))
    normal_path(ran, True, cid)
    b.close()


def device_buffer(nbytes):
    import torch
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("case", sc.FORMAT_CASES, ids=[c[0] for c in sc.FORMAT_CASES])
def test_output_formats_on_the_large_classes(ctxs, case, single):
    """generic outputs as INT32 ... UINT8 and DOUBLE (GenericAttr::dequantize in place over the int32 array) and a strided float binding,
    on attributes in k_delta_tiles and on positions the unfused normal chain reads: the oracle's buffer, nvert*N*8 bytes prefilled,
    byte for byte - the partly written last dword of the 8- and 16-bit formats and the fill behind the format's span included"""
    cid, nvert, N, normals = case
    blob = sc.format_blob(nvert, N, normals)
    info = ca.probe(blob)
    attrs = info.attrs()
    ref = oc.decode(blob)
    ctx = ctxs[single]
    for fmt in sc.FORMATS + ["strided"]:
        b = ca.Batch(ctx, [blob])
        bufs, binds = {}, []
        for a in attrs:
            n = nvert * a["components"]
            bd = ca.AttrBinding()
            if a["codec"] == ca.CODEC_NORMAL:
                bufs[a["name"]] = device_buffer(nvert * 12)
                bd.format = ca.FMT_FLOAT
            elif fmt == "strided":
                stride = 4 * a["components"] + 8
                bufs[a["name"]] = device_buffer(nvert * stride)
                bd.format, bd.stride = ca.FMT_FLOAT, stride
            else:
                bufs[a["name"]] = device_buffer(n * 8)
                bd.format = fmt
            bd.buffer = bufs[a["name"]].data_ptr()
            binds.append(bd)
        idx = device_buffer(info.nface * 12)
        b.bind(0, binds, idx.data_ptr(), ca.FMT_UINT32)
        b.decode()
        st = b.sync()
        assert (st == 0).all(), st
        ran = set(b.kernel_times())
        tag = "%s fmt %s" % (cid, fmt)
        assert "delta_tiles" in ran and "dequantize" in ran, (tag, sorted(ran))
        if normals:
            normal_path(ran, False, tag)
            assert bufs["normal"].cpu().numpy().view(np.float32).reshape(-1, 3).tobytes() == ref["normal"].tobytes(), tag
        assert idx.cpu().numpy().view(np.uint32).reshape(-1, 3).tobytes() == ref["index"].tobytes(), tag
        for a in attrs:
            if a["codec"] == ca.CODEC_NORMAL:
                continue
            got = bufs[a["name"]].cpu().numpy()
            if fmt == "strided":
                w = 4 * a["components"]
                rec = got.reshape(nvert, w + 8)
                assert rec[:, :w].tobytes() == ref[a["name"]].tobytes(), (tag, a["name"])
                assert (rec[:, w:] == FILL).all(), (tag, a["name"])
            else:
                want = oc.decode_attr_format(blob, a["name"], fmt, fill=FILL)
                span = len(want) if fmt == ca.FMT_DOUBLE else len(want) // 2
                assert (want[span:] == FILL).all() and (got[span:] == FILL).all(), (tag, a["name"])
                if got.tobytes() != want.tobytes():
                    bad = np.flatnonzero(got != want)
                    raise AssertionError("%s %s: %d bytes differ, first at %d of %d" % (tag, a["name"], len(bad), bad[0], len(want)))
        b.close()
