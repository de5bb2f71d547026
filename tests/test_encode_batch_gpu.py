"""crthip_encode_batch on the device: every blob byte-identical to the host encoder's (crthip_encode) and, for the golden
cases, to the reference's own bytes."""
import os
import sys

import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

E_ARGUMENT, E_LIMIT = -8, -11


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.close()


def _cases():
    sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def test_golden_cases_in_one_batch(ctx):
    cs = _cases()
    blobs = ca.encode_batch([m for _, m, _ in cs], ctx, kw=[k for _, _, k in cs])
    for (name, _, _), b in zip(cs, blobs):
        assert b.tobytes() == load_golden(name)["crt"].tobytes(), name


def _corpus():
    S = synth
    items = []
    for p in (ca.DIFF, ca.ESTIMATED, ca.BORDER):
        for e in (0, 1):
            items.append((S.bumpy_sphere(24 + 4 * p, 12, seed=10 * p + e, color_components=3 + e), dict(normal_prediction=p, entropy=e)))
            items.append((S.shuffled(S.delaunay_disc(300, seed=p + 3 * e, holes=3), seed=p), dict(normal_prediction=p, entropy=e)))
            items.append((S.cone_fan(40, 2, seed=p + e), dict(normal_prediction=p, entropy=e, position_bits=12)))
            items.append((S.decimated(S.icosphere(2, seed=p + e), keep=0.5, seed=p), dict(normal_prediction=p, entropy=e)))
            items.append((S.confetti(60, seed=p + e), dict(normal_prediction=p, entropy=e)))
            items.append((S.bumpy_sphere_flipped(16, 8, seed=p + e), dict(normal_prediction=p, entropy=e)))
            items.append((S.non_manifold(S.delaunay_disc(200, seed=5 + p, holes=2), seed=p + e, fins=4, dups=3, reversed_dups=3, bowties=2, glue=2),
                          dict(normal_prediction=p, entropy=e)))
            items.append((S.point_cloud(30, 20, seed=p + e), dict(normal_prediction=p, entropy=e)))
            items.append((S.torus(20, 10, seed=p + e), dict(normal_prediction=p, entropy=e, with_uv=False)))
            items.append((S.full_width_values(S.bumpy_sphere(9, 7, seed=p + e), seed=p), dict(normal_prediction=ca.DIFF, entropy=e, position_bits=0, position_q=1.0, uv_bits=0)))
    for s in range(90):
        m = S.bumpy_sphere(10 + s % 30, 6 + s % 5, seed=100 + s, color_components=3 + s % 2)
        if s % 3 == 0:
            m.radius = (0.5 + np.arange(m.nvert, dtype=np.float32) % 7).reshape(-1, 1)
        if s % 4 == 0:
            m.groups = [m.nface // 3, m.nface]
            m.group_props = [{"material": "m%d" % s}, {}]
        items.append((m, dict(normal_prediction=s % 3, entropy=s % 2, exif={"k": str(s)} if s % 5 == 0 else None)))
    # unreferenced vertices, all faces degenerate, an empty cloud
    m = S.bumpy_sphere(16, 8, seed=7)
    extra = np.random.default_rng(1).random((20, 3), dtype=np.float32)
    m.position = np.ascontiguousarray(np.vstack([m.position, extra]))
    for a in ("normal", "uv", "radius"):
        v = getattr(m, a)
        if v is not None:
            setattr(m, a, np.ascontiguousarray(np.vstack([v, np.repeat(v[:1], 20, axis=0)])))
    if m.color is not None:
        m.color = np.ascontiguousarray(np.vstack([m.color, np.repeat(m.color[:1], 20, axis=0)]))
    items.append((m, dict(normal_prediction=ca.ESTIMATED)))
    d = S.bumpy_sphere(8, 4, seed=8)
    d.index = np.ascontiguousarray(np.repeat(d.index[:, :1], 3, axis=1))
    items.append((d, dict(normal_prediction=ca.BORDER)))
    e = S.point_cloud(4, 4, seed=9)
    e.position = e.position[:0].copy()
    for a in ("normal", "color", "uv", "radius"):
        if getattr(e, a) is not None:
            setattr(e, a, getattr(e, a)[:0].copy())
    items.append((e, dict(normal_prediction=ca.DIFF)))
    return items


def test_mixed_corpus_matches_single_encodes(ctx):
    items = _corpus()
    assert len(items) >= 150
    blobs, st = ca.encode_batch([m for m, _ in items], ctx, kw=[k for _, k in items], with_stats=True)
    from oracle import refcodec as rc
    for i, ((m, k), b) in enumerate(zip(items, blobs)):
        assert b.tobytes() == ca.encode(m, **k).tobytes(), i
        if rc.available() and i % 7 == 0 and m.nvert:
            assert b.tobytes() == rc.encode(m, **k).tobytes(), i
    assert st["value_streams"] > len(items)
    for name in ("enc_quantize_batch", "enc_est_normal", "enc_delta", "enc_zkeys", "enc_zsort", "enc_pack", "enc_tun_parse"):
        assert name in st["kernel_times"], name


def test_point_clouds_device_and_host_sorted(ctx):
    big = synth.point_cloud(1500, 1400, seed=11)                    # 2.1 M points: the radix sort over many workgroups
    assert big.nvert >= 2_000_000
    blobs, st = ca.encode_batch([big], ctx, kw=dict(normal_prediction=ca.DIFF, position_bits=20), with_stats=True)
    assert st["clouds_device_sorted"] == 1 and st["clouds_host_sorted"] == 0
    assert blobs[0].tobytes() == ca.encode(big, normal_prediction=ca.DIFF, position_bits=20).tobytes()
    # duplicated quantised points
    dup = synth.point_cloud(40, 20, seed=12)
    dup.position[1::5] = dup.position[0::5][:len(dup.position[1::5])]
    blobs, st = ca.encode_batch([dup], ctx, kw=dict(normal_prediction=ca.BORDER), with_stats=True)
    assert st["clouds_host_sorted"] == 1 and blobs[0].tobytes() == ca.encode(dup, normal_prediction=ca.BORDER).tobytes()
    # coordinates beyond 21 bits: points that differ only above bit 21 share a key
    wide = synth.point_cloud(40, 20, seed=13)
    kw = dict(normal_prediction=ca.DIFF, position_bits=0, position_q=1.0)
    wide.position = np.ascontiguousarray((wide.position * np.float32(2 ** 24)).astype(np.float32))
    wide.position[3] = wide.position[2] + np.float32(2 ** 22)
    blobs, st = ca.encode_batch([wide], ctx, kw=kw, with_stats=True)
    assert st["clouds_host_sorted"] == 1 and blobs[0].tobytes() == ca.encode(wide, **kw).tobytes()


def test_per_mesh_errors_leave_the_neighbours_alone(ctx):
    a, b, c = synth.bumpy_sphere(16, 8, seed=1), synth.bumpy_sphere(16, 8, seed=2), synth.bumpy_sphere(16, 8, seed=3)
    b.index = b.index.copy(); b.index[5, 1] = b.nvert + 3
    huge = synth.Mesh(position=np.zeros(((1 << 23) + 1, 3), dtype=np.float32))   # a cloud: its position logs are one Tunstall stream
    meshes = [a, b, c, huge]
    blobs, status = ca.encode_batch(meshes, ctx, kw=dict(normal_prediction=ca.BORDER), raise_on_error=False)
    assert status[1] == E_ARGUMENT and len(blobs[1]) == 0
    assert status[0] == 0 and status[2] == 0
    assert blobs[0].tobytes() == ca.encode(a, normal_prediction=ca.BORDER).tobytes()
    assert blobs[2].tobytes() == ca.encode(c, normal_prediction=ca.BORDER).tobytes()
    assert status[3] == E_LIMIT and len(blobs[3]) == 0
    with pytest.raises(ca.CortoError):
        ca.encode_batch(meshes, ctx, kw=dict(normal_prediction=ca.BORDER))


def test_size_query_and_repeat_give_the_same_bytes(ctx):
    import ctypes as C
    ms = [synth.bumpy_sphere(20, 10, seed=s) for s in range(6)] + [synth.point_cloud(20, 10, seed=1)]
    descs = (ca.MeshDesc * len(ms))()
    keep = []
    for i, m in enumerate(ms):
        descs[i], kp = ca._mesh_desc(m)
        keep.append(kp)
    offs0 = np.zeros(len(ms) + 1, dtype=np.uint64)
    total = ca.lib().crthip_encode_batch(ctx.handle, len(ms), descs, 0, None, 0, offs0.ctypes.data_as(C.c_void_p), None, None, None, None, None)
    assert total > 0 and offs0[-1] == total
    runs = []
    for _ in range(2):
        out = np.zeros(total, dtype=np.uint8)
        offs = np.zeros(len(ms) + 1, dtype=np.uint64)
        r = ca.lib().crthip_encode_batch(ctx.handle, len(ms), descs, 3, out.ctypes.data_as(C.c_void_p), total, offs.ctypes.data_as(C.c_void_p),
                                         None, None, None, None, None)
        assert r == total and (offs == offs0).all()
        runs.append(out)
    assert runs[0].tobytes() == runs[1].tobytes()
    for i, m in enumerate(ms):
        assert runs[0][int(offs0[i]):int(offs0[i + 1])].tobytes() == ca.encode(m).tobytes(), i


def test_round_trip_through_the_batch_decoder(ctx):
    from oracle import oracle as oc
    ms = [synth.bumpy_sphere(24, 12, seed=s) for s in range(4)]
    blobs = [ca.aligned_blob(b) for b in ca.encode_batch(ms, ctx, kw=dict(normal_prediction=ca.BORDER))]
    bt = ca.Batch(ctx, blobs)
    bt.allocate_outputs()
    bt.decode()
    assert (bt.sync() == 0).all()
    for i, b in enumerate(blobs):
        got, ref = bt.host_outputs(i), oc.decode(b)
        for k in ("position", "normal", "color", "uv", "index"):
            assert got[k].tobytes() == ref[k].tobytes(), (i, k)
    bt.close()


def test_clers_stream_over_the_tunstall_limit_is_found_after_the_topology_pass(ctx):
    """2.2 M separate triangles: 6.6 M vertices (under the 2^23 checked up front) but 4 CLERS symbols a triangle (a VERTEX and three
    BOUNDARY), 8.8 M > 2^23 - known only once the topology pass has run.  That mesh alone gets CRTHIP_E_LIMIT."""
    nt = 2_200_000
    pos = np.random.default_rng(3).random((3 * nt, 3), dtype=np.float32)
    big = synth.Mesh(position=pos, index=np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3))
    small = synth.bumpy_sphere(16, 8, seed=4)
    kw = dict(with_normal=False, with_color=False, with_uv=False)
    blobs, status = ca.encode_batch([small, big], ctx, kw=kw, raise_on_error=False, host_threads=4)
    assert status[1] == E_LIMIT and len(blobs[1]) == 0
    assert status[0] == 0 and blobs[0].tobytes() == ca.encode(small, **kw).tobytes()


def test_cli_several_files_match_single_runs(ctx, tmp_path):
    """corto_hip a.ply b.ply c.ply: one crthip_encode_batch, each file to <stem>.crt - the same bytes as three single-file runs
    (the host encoder); -o and -P are refused with several files"""
    import subprocess
    from cli_common import our_cli, run, write_ply
    meshes = [synth.bumpy_sphere(24, 12, seed=31), synth.torus(20, 10, seed=32), synth.point_cloud(30, 20, seed=33)]
    single, multi = tmp_path / "single", tmp_path / "multi"
    single.mkdir(); multi.mkdir()
    names = ["a.ply", "b.ply", "c.ply"]
    for d in (single, multi):
        for nm, m in zip(names, meshes):
            write_ply(str(d / nm), m)
    opts = ["-v", "13", "-N", "estimated"]
    for nm in names:
        run(our_cli(), [nm] + opts, str(single))
    run(our_cli(), names + opts, str(multi))
    for nm in names:
        crt = nm.replace(".ply", ".crt")
        assert (multi / crt).read_bytes() == (single / crt).read_bytes(), nm
    for bad in (["-o", "x.crt"], ["-P", "x.ply"]):
        r = subprocess.run([our_cli()] + bad + names, cwd=str(multi), capture_output=True, timeout=120)
        assert r.returncode != 0
