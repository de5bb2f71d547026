"""GPU (-m gpu): k_tangent_blob, k_tangent_faces and k_tangent_vertex at the edges of tests/tangent_edges.py (tests/test_tangent_edges_cpu.py
shows that every case is on the side it is named for) - raw bytes against the numpy model of the contract (tests/computed_tangents.py) on the
oracle's integers, every other output against the oracle, the kernels each case is named for in kernel_times().  Outputs are pre-filled with
0xA5: every byte between a batch's outputs must still hold it."""
import numpy as np
import pytest

import corto_amd as ca
import computed_tangents as ct
import tangent_edges as te
from oracle import oracle as oc
from test_computed_tangents_gpu import FILL, Q, binding, device_bytes, expect_tangent, make_ctx, run, same_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

F32, I16 = ca.FMT_FLOAT, ca.FMT_INT16
FORMATS = [(F32, F32), (F32, I16), (I16, F32), (I16, I16)]                      # (tangents, normals)
BLOB, WIDE = {"tangent_blob"}, {"tangent_faces", "tangent_vertex"}


@pytest.fixture(scope="module")
def ctxs():
    cs = {False: make_ctx(False), True: make_ctx(True)}
    yield cs
    for c in cs.values():
        c.close()


_ORACLE = {}


def oracle_of(e, nfmt, i16):
    """the oracle's outputs of the blob of inputs `e` (tangent_edges caches them: one object a case), computed once a format"""
    key = (id(e), nfmt, i16)
    if key not in _ORACLE:
        _ORACLE[key] = oc.decode(e.blob, normal_format=nfmt, index16=i16)
    return _ORACLE[key]


def ran(b, want, never=frozenset()):
    names = set(b.kernel_times())
    assert set(want) <= names and not (set(never) & names), (sorted(want), sorted(never), sorted(names))


def classes(es):
    """(kernels that must run, kernels that must not) for a batch of these inputs"""
    small, wide = any(te.one_workgroup(e.nvert) for e in es), any(not te.one_workgroup(e.nvert) for e in es)
    return (BLOB if small else set()) | (WIDE if wide else set()), (set() if small else BLOB) | (set() if wide else WIDE)


def gaps_untouched(b):
    """every byte of the batch's one output buffer that belongs to no output still holds the fill"""
    buf = b._keep[0]
    raw = buf.cpu().numpy()
    free = np.ones(len(raw), bool)
    for o in b.outputs:
        for t, _ in o.values():
            at = t.data_ptr() - buf.data_ptr()
            free[at:at + t.numel() * t.element_size()] = False
    assert (raw[free] == FILL).all(), int((raw[free] != FILL).sum())


def check(b, i, e, fmt, nfmt, i16, tag, stored=True):
    """blob i of a decoded batch: the oracle's outputs, the model's tangents (stored normals: the oracle's; else the ones the batch wrote)"""
    got = b.host_outputs(i)
    assert got["tangent"].shape == (e.nvert, 4), tag
    if stored:
        same_outputs(got, oracle_of(e, nfmt, i16), (tag, "oracle"))
        ct.assert_bytes(got["tangent"], e.model(fmt, nfmt)[0], (tag, "model"))
    else:
        same_outputs(got, oracle_of(e, nfmt, i16), (tag, "oracle"), skip=("tangent", "normal"))
        ct.assert_bytes(got["tangent"], expect_tangent(e, got, fmt), (tag, "model on the batch's normals"))
    return got


# ---- 1. value edges ----

@pytest.mark.parametrize("cid", te.VALUE_IDS)
def test_value_edges(cid):
    """each blob alone on a fresh context, where K-DELTA's int16 records overflow and the attribute is redone in the kernel, then again on that
    context, which has learned the wide layout: the model's bytes both times, in every pair of tangent and normal formats"""
    e = te.value_case(cid)
    want, never = classes([e])
    for n, (fmt, nfmt) in enumerate(FORMATS):
        ctx = make_ctx(n % 2 == 1)
        try:
            b = ca.Batch(ctx, [e.blob])
            b.allocate_outputs(fill=FILL, normal_format=nfmt, index16=n >= 2, computed_tangents=True, tangent_format=fmt)
            for again in (False, True):
                run(b)
                st = b.stats()
                assert (st.delta_redone > 0, st.delta_wide) == ((True, 0) if not again else (False, 1)), (cid, fmt, nfmt, again, st.delta_redone, st.delta_wide)
                ran(b, want, never)
                check(b, 0, e, fmt, nfmt, n >= 2, (cid, fmt, nfmt, "again" if again else "fresh"))
                gaps_untouched(b)
            b.close()
        finally:
            ctx.close()


# ---- 2. the affine sheet: an answer that does not rest on the model ----

@pytest.mark.parametrize("n", te.SHEETS)
def test_affine_sheet(ctxs, n):
    """the CPU twin measured the model 3.2e-8 (FLOAT normals) and 5.0e-8 (INT16 normals) from the exact answer at k = 13..15"""
    es = [te.sheet(n, False), te.sheet(n, True)]
    want, never = classes(es)
    for nfmt in (F32, I16):
        b = ca.Batch(ctxs[nfmt == I16], [e.blob for e in es])
        b.allocate_outputs(fill=FILL, normal_format=nfmt, computed_tangents=True, tangent_format=F32)
        run(b)
        ran(b, want, never)
        for i, e in enumerate(es):
            got = check(b, i, e, F32, nfmt, False, ("sheet", n, nfmt, i))
            dev = te.sheet_deviation(got["tangent"], got["normal"], negate_u=bool(i))
            print("sheet %d normals %d negate %d: deviates by %.3g" % (n, nfmt, i, dev))
            assert dev <= te.SHEET_BOUND, (n, nfmt, i, dev)
        b.close()


# ---- 3. block, round and slot edges ----

def decode_cases(ctx, cases, fmt, nfmt, i16, tag):
    """[(id or None, blob)] in one batch; the named ones checked; returns the batch (open)"""
    b = ca.Batch(ctx, [blob for _, blob in cases])
    outs = b.allocate_outputs(fill=FILL, normal_format=nfmt, index16=i16, computed_tangents=True, tangent_format=fmt)
    run(b)
    for i, (cid, blob) in enumerate(cases):
        if cid is None:
            assert "tangent" not in outs[i]
            same_outputs(b.host_outputs(i), oc.decode(blob, normal_format=nfmt, index16=i16), (tag, "bystander", i))
        else:
            check(b, i, te.edge_case(cid), fmt, nfmt, i16, (tag, cid, fmt))
    gaps_untouched(b)
    return b


FMT2 = pytest.mark.parametrize("fmt", [F32, I16], ids=["f32", "i16"])


@FMT2
def test_blob_edges(ctxs, fmt):
    """k_tangent_blob alone: one and two face rounds +-1, a lane's first slot +-1, a tetrahedron"""
    b = decode_cases(ctxs[fmt == I16], [(c[0], te.edge_case(c[0]).blob) for c in te.BLOB_EDGES], fmt, I16 if fmt == F32 else F32, fmt == F32, "blob edges")
    ran(b, BLOB, WIDE)
    b.close()


@FMT2
def test_wide_edges(ctxs, fmt):
    """k_tangent_faces and k_tangent_vertex alone, each blob a batch of its own (fblock0 = vblock0 = 0): six blocks of faces -1, full, +1 (a last
    block of one face), three blocks of vertices +-1"""
    for c in te.WIDE_EDGES:
        b = decode_cases(ctxs[fmt == F32], [(c[0], te.edge_case(c[0]).blob)], fmt, fmt, fmt == I16, "wide edge alone")
        ran(b, WIDE, BLOB)
        b.close()


@FMT2
def test_one_batch(ctxs, fmt):
    """every batch-wide edge in one batch - block maps and accumulators at non-zero offsets - with two one-workgroup blobs, a cloud and a mesh
    without uv between them"""
    b = decode_cases(ctxs[fmt == I16], te.one_batch(), fmt, I16 if fmt == F32 else F32, fmt == I16, "one batch")
    ran(b, BLOB | WIDE)
    b.close()


# ---- 4. beside what the batch-wide path shares scratch or buffers with ----

@FMT2
def test_beside_unfused_computed_normals(ctxs, fmt):
    """the unfused normal pipeline's counters and the tangents' sums lie in the same zeroed region: a blob past normal_fused with computed normals and
    tangents, a batch-wide blob with stored normals, a one-workgroup blob"""
    es = [te.sized(te.unfused_nvert(), "computed"), te.sized(3000), te.sized(1500)]
    nfmt, i16 = (I16, True) if fmt == F32 else (F32, False)
    kw = dict(fill=FILL, normal_format=nfmt, index16=i16, computed_normals=True)
    plain = ca.Batch(ctxs[fmt == I16], [e.blob for e in es])
    plain.allocate_outputs(**kw)
    run(plain)
    assert not any(k.startswith("tangent") for k in plain.kernel_times())
    b = ca.Batch(ctxs[fmt == I16], [e.blob for e in es])
    b.allocate_outputs(computed_tangents=True, tangent_format=fmt, **kw)
    for again in range(2):
        run(b)
        ran(b, {"normal_faces", "normal_vertex", "tangent_faces", "tangent_vertex", "tangent_blob"})
        for i, e in enumerate(es):
            got = check(b, i, e, fmt, nfmt, i16, ("unfused", i, fmt, again), stored=i > 0)
            same_outputs(got, plain.host_outputs(i), ("unfused", i, fmt, again, "the batch without tangents"))
            ct.assert_bytes(got["tangent"], expect_tangent(e, got, fmt), ("unfused", i, fmt, again))
        gaps_untouched(b)
    plain.close(); b.close()


def test_quantized_interleaved_record(ctxs):
    """the 28-byte record of test_interleaved_record (uint16 position x 3 | pad | int16 normal x 3 | pad | int16 tangent x 4 | uint16 uv x 2) on a
    blob past TANGENT_BLOB_MAX and past the quantised outputs' one-workgroup limit: the tangent kernels read integers that live in scratch"""
    e = te.sized(te.record_nvert())
    nv, nf = e.nvert, e.nface
    packed = ca.Batch(ctxs[False], [e.blob])
    packed.allocate_outputs(fill=FILL, normal_format=I16, index16=True, quantized=("position", "uv"), computed_tangents=True, tangent_format=I16)
    run(packed)
    ran(packed, WIDE | {"quant_range", "quant_store"}, BLOB | {"quant_out_blob"})
    ref = packed.host_outputs(0)
    ct.assert_bytes(ref["tangent"], e.model(I16, I16)[0], "packed")
    o = oracle_of(e, I16, True)
    ct.assert_bytes(ref["normal"], o["normal"], "packed normal")
    ct.assert_bytes(ref["index"], o["index"], "packed index")
    tail = 64
    for single in (False, True):
        b = ca.Batch(ctxs[single], [e.blob])
        names = [a["name"] for a in b.infos[0].attrs()]
        assert sorted(names) == ["normal", "position", "uv"]
        vb, ib = device_bytes(nv * 28 + tail), device_bytes(nf * 6 + tail)
        at = {"position": (0, ca.FMT_UINT16, Q), "normal": (8, I16, 0), "uv": (24, ca.FMT_UINT16, Q)}
        b.bind(0, [binding(vb.data_ptr() + at[n][0], at[n][1], 28, at[n][2]) for n in names], ib.data_ptr(), ca.FMT_UINT16)
        b.bind_computed_tangents(0, vb.data_ptr() + 16, I16, 28)
        run(b)
        ran(b, WIDE, BLOB)
        raw = vb.cpu().numpy()
        rec = raw[:nv * 28].reshape(nv, 28)
        field = lambda o, w, dt: np.ascontiguousarray(rec[:, o:o + w]).view(dt)
        ct.assert_bytes(field(16, 8, np.int16), ref["tangent"], ("record tangent", single))
        ct.assert_bytes(field(0, 6, np.uint16), ref["position"].view(np.uint16), ("record position", single))
        ct.assert_bytes(field(8, 6, np.int16), ref["normal"], ("record normal", single))
        ct.assert_bytes(field(24, 4, np.uint16), ref["uv"].view(np.uint16), ("record uv", single))
        assert (rec[:, 6:8] == FILL).all() and (rec[:, 14:16] == FILL).all()
        assert (raw[nv * 28:] == FILL).all()                                    # nothing behind the last vertex
        iraw = ib.cpu().numpy()
        ct.assert_bytes(iraw[:nf * 6].view(np.uint16).reshape(nf, 3), ref["index"], ("record index", single))
        assert (iraw[nf * 6:] == FILL).all()
        b.close()
    packed.close()


def test_integers_in_scratch(ctxs):
    """a DOUBLE position and a strided FLOAT uv: neither buffer can hold the integers, K-DELTA leaves them in scratch and the tangent kernels read
    them there - batch-wide and one workgroup in one batch"""
    es = [te.sized(te.record_nvert()), te.edge_case("round_1025")]
    b = ca.Batch(ctxs[True], [e.blob for e in es])
    keep = []
    for i, e in enumerate(es):
        nv, nf = e.nvert, e.nface
        names = [a["name"] for a in b.infos[i].attrs()]
        bufs = {"position": device_bytes(nv * 24 + 16), "uv": device_bytes(nv * 16 + 16), "normal": device_bytes(nv * 12 + 16), "tangent": device_bytes(nv * 16 + 16),
                "index": device_bytes(nf * 12 + 16)}
        how = {"position": (ca.FMT_DOUBLE, 0), "uv": (F32, 16), "normal": (F32, 0)}
        b.bind(i, [binding(bufs[n].data_ptr(), how[n][0], how[n][1]) for n in names], bufs["index"].data_ptr(), ca.FMT_UINT32)
        b.bind_computed_tangents(i, bufs["tangent"].data_ptr(), F32, 0)
        keep.append(bufs)
    run(b)
    ran(b, BLOB | WIDE)
    for i, e in enumerate(es):
        nv, nf = e.nvert, e.nface
        raw = {k: t.cpu().numpy() for k, t in keep[i].items()}
        o = oracle_of(e, F32, False)
        ct.assert_bytes(raw["tangent"][:nv * 16].view(np.float32).reshape(nv, 4), e.model(F32, F32)[0], ("scratch tangent", i))
        assert raw["position"][:nv * 24].tobytes() == oc.decode_attr_format(e.blob, "position", ca.FMT_DOUBLE)[:nv * 24].tobytes(), ("scratch position", i)
        assert raw["uv"].tobytes() == ct.strided(o["uv"], 16, offset=0).tobytes() + bytes([FILL]) * (len(raw["uv"]) - (nv - 1) * 16 - 8), ("scratch uv", i)
        ct.assert_bytes(raw["normal"][:nv * 12].view(np.float32).reshape(nv, 3), o["normal"], ("scratch normal", i))
        ct.assert_bytes(raw["index"][:nf * 12].view(np.uint32).reshape(nf, 3), o["index"], ("scratch index", i))
        for k, used in (("tangent", nv * 16), ("position", nv * 24), ("normal", nv * 12), ("index", nf * 12)):
            assert (raw[k][used:] == FILL).all(), (k, i)
    b.close()


@pytest.mark.parametrize("nvert,u16", te.BIG, ids=["%d_%s" % (n, "u16" if u else "u32") for n, u in te.BIG])
def test_big_blobs(ctxs, nvert, u16):
    """beyond K-DELTA's LDS records (k_delta_tiles leaves the positions), the last uint16 index, a uint32-only one"""
    e = te.sized(nvert)
    fmt, nfmt = (I16, I16) if u16 else (F32, F32)
    b = ca.Batch(ctxs[u16], [e.blob])
    b.allocate_outputs(fill=FILL, normal_format=nfmt, index16=u16, computed_tangents=True, tangent_format=fmt)
    run(b)
    ran(b, WIDE | {"delta_tiles"}, BLOB)
    check(b, 0, e, fmt, nfmt, u16, ("big", nvert))
    gaps_untouched(b)
    b.close()


def test_repeat_and_replan():
    """one batch object: three decodes in a row, a reset to another blob list (other sizes, other scratch offsets), a reset back - the accumulators
    are zeroed for every decode, wherever the plan puts them"""
    first = [te.full_width(2305), te.sized(3000), te.edge_case("round_1025")]
    second = [te.edge_case("slots_257"), te.deep(2305), te.edge_case("faces_6145"), te.full_width(3073)]
    ctx = make_ctx(True)
    b = ca.Batch(ctx, [e.blob for e in first])
    try:
        for es, fmt, nfmt, i16, times in ((first, F32, I16, True, 3), (second, I16, F32, False, 2), (first, F32, I16, True, 1)):
            if es is not first or times == 1:
                b.reset([e.blob for e in es])
            b.allocate_outputs(fill=FILL, normal_format=nfmt, index16=i16, computed_tangents=True, tangent_format=fmt)
            for n in range(times):
                run(b)
                ran(b, BLOB | WIDE)
                for i, e in enumerate(es):
                    check(b, i, e, fmt, nfmt, i16, ("repeat", len(es), n, i))
                gaps_untouched(b)
    finally:
        b.close()
        ctx.close()


def test_decode_with_next_equals_plain():
    """tests/test_computed_tangents_gpu.py's pipelined lane with a batch-wide blob in both groups: full-width values in one, computed normals (the
    unfused pipeline) in the other"""
    groups = [([te.full_width(2305), te.edge_case("slots_257"), te.sized(3000)], False),
              ([te.sized(te.unfused_nvert(), "computed"), te.sized(1500, "computed"), te.sized(2400, "computed")], True)]
    ctx = make_ctx(True)
    objs = [ca.Batch(ctx, []), ca.Batch(ctx, [])]
    objs[1].set_parity(1)
    try:
        refs = []
        for es, computed in groups:
            kw = dict(fill=FILL, normal_format=I16, index16=True, computed_normals=computed, computed_tangents=True, tangent_format=I16)
            p = ca.Batch(ctx, [e.blob for e in es])
            p.allocate_outputs(**kw)
            run(p)
            run(p)                                                              # (the context has learned the first group's wide layout)
            ran(p, BLOB | WIDE)
            refs.append([p.host_outputs(i) for i in range(len(es))])
            p.close()
        for k, (es, computed) in enumerate(groups):
            objs[k].reset([e.blob for e in es])
            objs[k].allocate_outputs(fill=FILL, normal_format=I16, index16=True, computed_normals=computed, computed_tangents=True, tangent_format=I16)
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == 0).all() and (st1 == 0).all()
        for k, (es, computed) in enumerate(groups):
            for i, e in enumerate(es):
                got = check(objs[k], i, e, I16, I16, True, ("pair", k, i), stored=not computed)
                same_outputs(got, refs[k][i], ("pair", k, i, "plain"), skip=())
    finally:
        for o in objs:
            o.close()
        ctx.close()
