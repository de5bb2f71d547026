"""GPU (-m gpu): crthip_encode_batch_to_device - the blobs of a batch spliced on the GPU and left in device memory.  The arena copied back
holds, at the reported offsets, the host encoder's bytes (crthip_encode_attrs) and, for the golden cases, the reference's own; zeros lie
between the blobs; nothing is written outside the arena; the result goes into a resident decode as it is.

What is NOT handed over here, on purpose: a pageable-memory device_out, and a cap that leaves device_out's allocation.  Were the pointer
check ever missing, such a test would turn into a device fault on a machine others share.  The extent rule (resident_array_ok in
encode_batch.cpp) is covered by review; a misaligned and a pinned-host device_out, which cannot fault, are tested.

One context; every input seeded.  Run as one pytest invocation under a time limit of its own."""
import sys

import numpy as np
import pytest
import torch

import corto_amd as ca
from corto_amd import synth
from conftest import GOLDEN, aligned, load_golden
from test_encode_batch_gpu import _corpus
from test_encode_device_out_cpu import _tiny_items
from test_encode_resident_gpu import _Unaligned, _dev, _host_encode

pytestmark = pytest.mark.gpu

E_ARGUMENT = -8
E_LIMIT = -11
MODES = ("host", "device", "split")
SPLICE_JOB_BYTES = 24                                               # sizeof(SpliceJob), csrc/device_plan.h


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.set_encode_topology("host")
    c.close()


def _cases():
    sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def _to_device(ctx, items, resident, **kw):
    if resident:
        ms, ks = _dev(items)
    else:
        ms, ks = [m for m, _ in items], [k for _, k in items]
    return ca.encode_batch_to_device(ms, ctx, kw=ks, resident=resident, **kw)


def _check_arena(out, offs, lens, expect, total, tag):
    """the arena copied back: every blob at its offset, zeros up to the next blob, offsets = arena_layout(lens)"""
    host = out.cpu().numpy()
    want_offs, want_total = ca.arena_layout(lens)
    assert offs.tolist() == want_offs.tolist() and total == want_total, tag
    for i, e in enumerate(expect):
        o, n = int(offs[i]), int(lens[i])
        assert n == len(e), (tag, i)
        assert host[o:o + n].tobytes() == e, (tag, i)
        assert not host[o + n:(o + n + 15) & ~15].any(), (tag, i, "padding")
    return host


def test_golden_cases_resident_and_host_inputs(ctx):
    cs = _cases()
    items = [(m, k) for _, m, k in cs]
    expect = [load_golden(name)["crt"].tobytes() for name, _, _ in cs]
    for resident in (True, False):
        for mode in MODES:
            ctx.set_encode_topology(mode)
            out, offs, lens, st = _to_device(ctx, items, resident, with_stats=True)
            _check_arena(out, offs, lens, expect, st["total"], (resident, mode))
            assert st["kernel_times"]["enc_splice"]["launches"] == 1, (resident, mode)
            assert st["splice"]["arena_bytes"] == st["total"] == st["splice"]["literal_bytes"] + st["splice"]["device_bytes"]
    ctx.set_encode_topology("host")


def test_mixed_corpus_in_every_topology_mode(ctx):
    items = _corpus()
    rng = np.random.default_rng(2)
    for i in range(0, len(items), 13):                              # generic attributes on some of them
        m, k = items[i]
        if m.nvert:
            items[i] = (m, dict(k, attributes=[("weight", rng.standard_normal((m.nvert, 3)).astype(np.float32), 0.01, ca.CORRELATED),
                                               ("label", rng.integers(-300, 300, (m.nvert, 1)).astype(np.int16), 1.0, 0)]))
    assert len(items) >= 150
    expect = [_host_encode(m, k).tobytes() for m, k in items]
    for mode in MODES:
        ctx.set_encode_topology(mode)
        out, offs, lens, st = _to_device(ctx, items, True, with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], mode)
        assert st["clouds_host_sorted"] >= 0 and st["kernel_times"]["enc_splice"]["launches"] == 1
    ctx.set_encode_topology("device")
    out, offs, lens, st = _to_device(ctx, items, False, with_stats=True)
    _check_arena(out, offs, lens, expect, st["total"], "host inputs")
    ctx.set_encode_topology("host")


def test_tiny_shapes_three_ways(ctx, monkeypatch):
    """One batch of the shapes where a block's header, payload and address can disagree (_tiny_items: TUNSTALL and NONE items side by
    side in one chunk, so both kinds of block header meet in one plan and one gather) through crthip_encode_batch, through
    crthip_encode_batch_to_device and, item by item, through the host encoder: the same bytes, in every topology mode; then to the
    device once more in several chunks.  The host encoder takes the 0-vertex cloud, so it is in."""
    items = _tiny_items()
    ms, ks = [m for m, _ in items], [k for _, k in items]
    expect = [ca.encode(m, **k).tobytes() for m, k in items]
    for mode in MODES:
        ctx.set_encode_topology(mode)
        blobs, bs = ca.encode_batch(ms, ctx, kw=ks, with_stats=True)
        assert [b.tobytes() for b in blobs] == expect, mode
        out, offs, lens, st = ca.encode_batch_to_device(ms, ctx, kw=ks, with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], ("tiny", mode))
        assert st["splice"]["launches"] == 1 and st["value_streams"] == bs["value_streams"], mode
    ctx.set_encode_topology("host")
    # In several chunks: a chunk's image is its job region (64 KiB) and a few 256-byte regions per attribute of every item.  The first
    # budget, in steps of 8 KiB, that holds every item alone (a smaller one refuses the call before any device work: E_LIMIT) cannot hold
    # the ten together: the other nine take far more than one step.
    st = None
    for budget in range(72 << 10, 160 << 10, 8 << 10):
        monkeypatch.setenv("CORTO_ENCODE_IMAGE_BUDGET", str(budget))
        small = ca.Context(0)
        monkeypatch.delenv("CORTO_ENCODE_IMAGE_BUDGET")
        try:
            out, offs, lens, st = ca.encode_batch_to_device(ms, small, kw=ks, with_stats=True)
        except ca.CortoError as e:
            assert e.code == E_LIMIT, e
            continue
        finally:
            small.close()
        break
    assert st is not None and 2 <= st["splice"]["launches"] <= len(items), (budget, st and st["splice"])
    _check_arena(out, offs, lens, expect, st["total"], ("tiny, chunks", budget))


def test_tied_clouds(ctx):
    dup = synth.point_cloud(40, 20, seed=12)
    dup.position[1::5] = dup.position[0::5][:len(dup.position[1::5])]
    items = [(dup, dict(normal_prediction=ca.BORDER)), (synth.point_cloud(30, 20, seed=3), dict(normal_prediction=ca.DIFF, entropy=0))]
    out, offs, lens, st = _to_device(ctx, items, True, with_stats=True)
    assert st["clouds_host_sorted"] == 1
    _check_arena(out, offs, lens, [ca.encode(m, **k).tobytes() for m, k in items], st["total"], "tied")


def test_poison_nothing_outside_the_arena(ctx):
    items = [(m, k) for _, m, k in _cases()[:10]]
    ms, ks = _dev(items)
    bound = ca.encode_batch_bound(ms, kw=ks)
    out = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out, offs, lens, st = ca.encode_batch_to_device(ms, ctx, kw=ks, out=out, with_stats=True)
    total = st["total"]
    assert 0 < total <= bound
    host = _check_arena(out, offs, lens, [ca.encode(m, **k).tobytes() for m, k in items], total, "poison")
    assert (host[total:] == 0xA5).all()
    # one byte short: nothing at all is written, and the total is still returned
    out2 = torch.full((bound + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ca.CortoError) as err:
        ca.encode_batch_to_device(ms, ctx, kw=ks, out=out2, cap=total - 1)
    assert str(total) in str(err.value)
    torch.cuda.synchronize()
    assert bool((out2 == 0xA5).all())
    # sizing only: device_out NULL
    import ctypes as C
    n, descs, lists, with_attrs, keep, _ = ca._batch_descs(ms, ks, ca._device_ptr_getter("test"))
    o = np.zeros(n, dtype=np.uint64); ln = np.zeros(n, dtype=np.uint32)
    r = ca.lib().crthip_encode_batch_to_device(ctx.handle, n, descs, None, 0, 1, None, 0, ca._np_ptr(o), ca._np_ptr(ln), None, None, None, None, None)
    assert r == total and ln.tolist() == lens.tolist() and o.tolist() == offs.tolist()


def test_per_mesh_errors_leave_the_neighbours_alone(ctx):
    a, b, c = synth.bumpy_sphere(16, 8, seed=1), synth.bumpy_sphere(16, 8, seed=2), synth.bumpy_sphere(16, 8, seed=3)
    b.index = b.index.copy(); b.index[5, 1] = b.nvert + 3
    kw = dict(normal_prediction=ca.BORDER)
    ea, ec = ca.encode(a, **kw).tobytes(), ca.encode(c, **kw).tobytes()
    for mode in MODES:
        ctx.set_encode_topology(mode)
        for resident in (True, False):
            out, offs, lens, status = _to_device(ctx, [(a, kw), (b, kw), (c, kw)], resident, raise_on_error=False)
            assert status.tolist() == [0, E_ARGUMENT, 0], (mode, resident)
            assert lens[1] == 0
            _check_arena(out, offs, lens, [ea, b"", ec], int(ca.arena_layout(lens)[1]), (mode, resident))
    ctx.set_encode_topology("host")
    # an input array off its element alignment
    ms, ks = _dev([(a, kw), (c, kw)])
    raw = torch.zeros(a.position.nbytes + 16, dtype=torch.uint8, device="cuda:0")
    raw[2:2 + a.position.nbytes] = torch.from_numpy(a.position.view(np.uint8).reshape(-1)).to("cuda:0")
    ms[0].position = _Unaligned(raw, 2, a.position.shape)
    out, offs, lens, status = ca.encode_batch_to_device(ms, ctx, kw=ks, resident=True, raise_on_error=False)
    assert status.tolist() == [E_ARGUMENT, 0] and lens[0] == 0
    _check_arena(out, offs, lens, [b"", ec], int(ca.arena_layout(lens)[1]), "misaligned input")
    with pytest.raises(ca.CortoError):
        ca.encode_batch_to_device(ms, ctx, kw=ks, resident=True)


def test_a_bad_device_out_is_an_argument_error(ctx):
    items = [(synth.bumpy_sphere(16, 8, seed=1), {})]
    ms, ks = _dev(items)
    good = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda:0")
    off = good[8:]                                                  # 8 mod 16, inside the same allocation
    assert off.data_ptr() % 16 == 8
    with pytest.raises(ca.CortoError) as err:
        ca.encode_batch_to_device(ms, ctx, kw=ks, out=off, cap=1 << 19)
    assert err.value.code == E_ARGUMENT and "device_out" in str(err.value)
    pinned = torch.zeros(1 << 20, dtype=torch.uint8).pin_memory()
    with pytest.raises(ca.CortoError) as err:
        ca.encode_batch_to_device(ms, ctx, kw=ks, out=pinned)
    assert err.value.code == E_ARGUMENT and "device_out" in str(err.value)
    torch.cuda.synchronize()
    assert bool((good == 0xA5).all()) and not pinned.any()


def test_closed_loop_encode_to_device_then_resident_decode(ctx):
    from oracle import oracle as oc
    items = [(synth.bumpy_sphere(64, 32, seed=s), dict(normal_prediction=ca.BORDER)) for s in range(16)]      # C4 units
    items += [(m, k) for name, m, k in _cases() if name in ("nrm_diff", "two_groups", "torus", "icosphere", "cloud_diff")]
    ctx.set_encode_topology("device")
    out, offs, lens = _to_device(ctx, items, True)
    ctx.set_encode_topology("host")
    batch = ca.Batch.resident(ctx, out, offs, lens)
    assert batch.walk_stats().device_walked == len(items)
    batch.allocate_outputs(fill=0)
    batch.decode()
    assert (batch.sync() == 0).all()
    # against the decode of the HOST-encoded blobs
    blobs = [ca.encode(m, **k) for m, k in items]
    ref = ca.Batch(ctx, [aligned(b) for b in blobs])
    ref.allocate_outputs(fill=0)
    ref.decode()
    assert (ref.sync() == 0).all()
    for i, ((m, k), b) in enumerate(zip(items, blobs)):
        got, want = batch.host_outputs(i), ref.host_outputs(i)
        assert set(got) == set(want)
        for key in want:
            assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), (i, key)
        if i % 5 == 0:
            o = oc.decode(aligned(b), color_components=4 if m.color is None else m.color.shape[1])
            for key in ("position", "index"):
                if key in o:
                    assert got[key].tobytes() == o[key].tobytes(), (i, key)
    batch.close(); ref.close()


def test_what_crosses_the_link(ctx):
    """Derived, not measured.  Every device-sourced byte of the splice is one the host-output path copies back at least once (bit words
    exactly; raw logs, symbols and codewords padded), and the host-output path copies nothing back that the new one adds: so
    bytes_from_device(to_device) <= bytes_from_device(resident) - device_bytes.  Under device topology nothing else goes up either:
    bytes_to_device(to_device) <= bytes_to_device(resident) + literal_bytes + the job table (24 bytes a piece, 4 a tile start)."""
    items = [(synth.bumpy_sphere(64, 32, seed=s), dict(normal_prediction=s % 3, entropy=s % 2)) for s in range(24)]
    items += [(synth.point_cloud(60, 40, seed=s), dict(normal_prediction=ca.DIFF)) for s in range(4)]
    ms, ks = _dev(items)
    for mode in MODES:
        ctx.set_encode_topology(mode)
        _, rs = ca.encode_batch_resident(ms, ctx, kw=ks, with_stats=True)
        _, _, _, ds = ca.encode_batch_to_device(ms, ctx, kw=ks, with_stats=True)
        sp = ds["splice"]
        print("%s: bytes_from_device resident %d, to_device %d, device_bytes %d; bytes_to_device resident %d, to_device %d, literal %d, pieces %d, jobs %d, enc_splice %.1f us"
              % (mode, rs["bytes_from_device"], ds["bytes_from_device"], sp["device_bytes"], rs["bytes_to_device"], ds["bytes_to_device"],
                 sp["literal_bytes"], sp["pieces"], sp["jobs"], sp["splice_kernel_us"]))
        assert ds["bytes_from_device"] <= rs["bytes_from_device"] - sp["device_bytes"], mode
        assert sp["device_bytes"] > 0 and sp["jobs"] >= sp["pieces"] > len(items)
        if mode == "device":
            # the job table: 24 bytes a piece and 4 a tile start, pieces + 1 of them; the literal buffer is packed: literal_bytes on the link
            table = sp["pieces"] * SPLICE_JOB_BYTES + (sp["pieces"] + 1) * 4
            assert ds["bytes_to_device"] <= rs["bytes_to_device"] + sp["literal_bytes"] + table, mode
        assert ds["kernel_times"]["enc_splice"]["launches"] == 1 and "enc_splice" not in rs["kernel_times"]
    ctx.set_encode_topology("host")


def test_a_batch_in_several_chunks_continues_the_arena(ctx, monkeypatch):
    """A batch beyond one device image is encoded chunk by chunk, each chunk spliced where the last one ended.  $CORTO_ENCODE_IMAGE_BUDGET
    (a context's test hook, read when it is made) makes a batch of small meshes take that path: a context of its own, here alone."""
    items = _corpus()
    expect = [_host_encode(m, k).tobytes() for m, k in items]
    monkeypatch.setenv("CORTO_ENCODE_IMAGE_BUDGET", str(1 << 20))              # 1 MiB: every item of the corpus fits it alone, the corpus does not
    small = ca.Context(0)
    monkeypatch.delenv("CORTO_ENCODE_IMAGE_BUDGET")
    try:
        ms, ks = _dev(items)
        bound = ca.encode_batch_bound(ms, kw=ks)
        for mode in ("host", "device"):
            small.set_encode_topology(mode)
            out = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            out, offs, lens, st = ca.encode_batch_to_device(ms, small, kw=ks, out=out, with_stats=True)
            chunks = st["splice"]["launches"]
            assert 1 < chunks <= len(items) and st["kernel_times"]["enc_splice"]["launches"] == chunks, mode
            total = st["total"]
            host = _check_arena(out, offs, lens, expect, total, ("chunks", mode))
            assert (host[total:] == 0xA5).all()
            assert st["splice"]["literal_bytes"] + st["splice"]["device_bytes"] == total
            # an arena below the bound: the batch is sized first, then written - exactly as large as needed ...
            out2 = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            _, offs2, lens2, st2 = ca.encode_batch_to_device(ms, small, kw=ks, out=out2, cap=total, with_stats=True)
            assert st2["total"] == total and offs2.tolist() == offs.tolist() and lens2.tolist() == lens.tolist()
            assert torch.equal(out2[:total], out[:total]) and bool((out2[total:] == 0xA5).all())
            # ... and one byte short: nothing at all is written, by any chunk
            out3 = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            with pytest.raises(ca.CortoError) as err:
                ca.encode_batch_to_device(ms, small, kw=ks, out=out3, cap=total - 1)
            assert str(total) in str(err.value)
            torch.cuda.synchronize()
            assert bool((out3 == 0xA5).all()), mode
        # the host-output encoders take the same chunks and give the same blobs
        blobs = ca.encode_batch_resident(ms, small, kw=ks)
        assert [b.tobytes() for b in blobs] == expect
    finally:
        small.close()
