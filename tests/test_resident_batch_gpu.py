"""GPU (-m gpu): batches whose .crt bytes live only in device memory (crthip_batch_create_resident / _reset_resident, Batch.resident).
Against a batch created from host copies of the same blobs: the same blob infos, exif, groups and properties, the same statuses and
byte-identical outputs; no blob payload comes back to the host; malformed blobs fail with the host walk's code; blobs too big for a
walk record are walked on the host and still decode identically; one object reset across subsets, orders and host resets."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import corto_amd as ca
import resident_corpus as rc
from conftest import ALL_CASES, aligned, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1():
    c = ca.Context(0)
    c.set_single_stream(True)
    yield c
    c.close()


def c4_blobs():
    z = np.load(os.path.join(rc.GOLDEN, "c4_blobs16.npz"))
    return [np.ascontiguousarray(z["crt_%02d" % i], dtype=np.uint8) for i in range(16)]


def fixtures():
    return [np.ascontiguousarray(load_golden(n)["crt"], dtype=np.uint8) for n in ALL_CASES]


def place(blobs, seed, gaps=True):
    """the blobs in ONE device buffer, in a shuffled order with gaps between them: (buffer, offsets, lens) in the blobs' order"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(blobs))
    offs = np.zeros(len(blobs), dtype=np.uint64)
    pos = 16 * int(rng.integers(0, 8)) if gaps else 0
    for i in order:
        offs[i] = pos
        pos += (len(blobs[i]) + 15) // 16 * 16 + (16 * int(rng.integers(0, 12)) if gaps else 0)
    host = np.zeros(pos + 64, dtype=np.uint8)
    for b, o in zip(blobs, offs):
        host[int(o):int(o) + len(b)] = b
    buf = torch.from_numpy(host).to("cuda:0")
    return buf, offs, np.array([len(b) for b in blobs], dtype=np.uint32)


def outputs(b, interleaved):
    if interleaved:
        b.allocate_interleaved(fill=0)
    else:
        b.allocate_outputs(fill=0)
    b.decode()
    st = b.sync(raise_on_error=False)
    return st, b._keep[0].cpu().numpy()


def probe_group_props(blob, g):
    n = ca.lib().crthip_probe_group_props(blob.ctypes.data, len(blob), g, None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    ca.lib().crthip_probe_group_props(blob.ctypes.data, len(blob), g, buf, n)
    parts = buf.raw[:n].split(b"\0")[:-1]
    return {parts[k].decode(): parts[k + 1].decode() for k in range(0, len(parts), 2)}


def assert_same_batches(host, res, blobs, interleaved):
    assert len(host) == len(res) == len(blobs)
    for i, blob in enumerate(blobs):
        assert bytes(host.infos[i]) == bytes(res.infos[i]), i                    # crthip_batch_info, field by field
        hb = aligned(blob)
        assert res.exif(i) == ca.probe_exif(hb) == host.exif(i), i
        groups = ca.probe_groups(hb)
        assert res.groups(i) == groups == host.groups(i), i
        for g in range(len(groups)):
            assert res.group_props(i, g) == probe_group_props(hb, g), (i, g)
    st_h, out_h = outputs(host, interleaved)
    st_r, out_r = outputs(res, interleaved)
    assert st_h.tolist() == st_r.tolist()
    assert out_h.tobytes() == out_r.tobytes()
    return st_r


@pytest.mark.parametrize("single_stream", [False, True], ids=["two_streams", "one_stream"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["default", "interleaved"])
def test_resident_parity(ctx, ctx1, single_stream, interleaved):
    c = ctx1 if single_stream else ctx
    by = dict(rc.golden_blobs())
    blobs = fixtures() + c4_blobs() + [rc.crafted(by["c4_unit"]), rc.crafted(by["group_props"])]
    buf, offs, lens = place(blobs, seed=3 + int(single_stream))
    host = ca.Batch(c, [aligned(b) for b in blobs])
    res = ca.Batch.resident(c, buf, offs, lens)
    ws = res.walk_stats()
    assert (ws.device_walked, ws.host_walked) == (len(blobs), 0)
    hs = host.walk_stats()
    assert (hs.device_walked, hs.host_walked, hs.bytes_to_host) == (0, len(blobs), 0)
    st = assert_same_batches(host, res, blobs, interleaved)
    assert (st == 0).all(), st
    host.close(); res.close()


def test_no_payload_comes_back(ctx):
    blobs = c4_blobs() * 16
    buf, offs, lens = place(blobs, seed=5)
    res = ca.Batch.resident(ctx, buf, offs, lens)
    ws = res.walk_stats()
    assert ws.device_walked == 256 and ws.host_walked == 0
    assert ws.bytes_to_host <= 1024 * 256 and ws.bytes_to_host * 10 < int(lens.sum())     # a C4 blob is ~14.6 KB
    assert ws.walk_kernel_us > 0
    host = ca.Batch(ctx, [aligned(b) for b in blobs])
    st_h, out_h = outputs(host, False)
    st_r, out_r = outputs(res, False)
    assert (st_r == 0).all() and (st_h == 0).all()
    assert out_h.tobytes() == out_r.tobytes()
    host.close(); res.close()


def _code(fn):
    try:
        b = fn()
    except ca.CortoError as e:
        return e.code, str(e)
    b.close()
    return 0, ""


def test_malformed_blobs_fail_like_the_host_walk(ctx):
    """every truncation of a small blob and byte edits over a C4 blob's header and first framing words: a resident create gives the
    code a host create gives"""
    small = np.ascontiguousarray(load_golden("fields31")["crt"], dtype=np.uint8)
    c4 = np.ascontiguousarray(load_golden("c4_unit")["crt"], dtype=np.uint8)
    bad = [small[:k] for k in range(len(small) + 1)]
    for p in range(0, 480):
        for v in (c4[p] ^ 0xFF, 0, c4[p] ^ 0x80):
            e = c4.copy()
            e[p] = v
            bad.append(e)
    buf, offs, lens = place(bad, seed=9, gaps=False)
    codes = {}
    for i, b in enumerate(bad):
        want, _ = _code(lambda: ca.Batch(ctx, [aligned(b)]))
        got, _ = _code(lambda: ca.Batch.resident(ctx, buf, offs[i:i + 1], lens[i:i + 1]))
        assert got == want, (i, got, want)
        codes[want] = codes.get(want, 0) + 1
    assert {0, -2, -3}.issubset(codes), codes
    # one bad blob in the middle of a batch: the same code, the same blob named
    good = c4_blobs()[:9]
    mixed = good[:4] + [good[4][:3000]] + good[5:]
    buf2, offs2, lens2 = place(mixed, seed=10)
    want = _code(lambda: ca.Batch(ctx, [aligned(b) for b in mixed]))
    got = _code(lambda: ca.Batch.resident(ctx, buf2, offs2, lens2))
    assert got[0] == want[0] == -3 and "(blob 4)" in got[1] and "(blob 4)" in want[1]


@pytest.mark.parametrize("which", ["big_exif", "many_streams"])
def test_blob_too_big_for_a_record_is_walked_on_the_host(ctx, which):
    blob = {"big_exif": rc.big_exif_blob, "many_streams": rc.many_streams_blob}[which]()
    c4 = c4_blobs()
    blobs = [c4[0], blob, c4[1]]
    buf, offs, lens = place(blobs, seed=12)
    res = ca.Batch.resident(ctx, buf, offs, lens)
    ws = res.walk_stats()
    assert (ws.device_walked, ws.host_walked) == (2, 1)
    assert ws.bytes_to_host == 3 * 1024 + len(blob)
    host = ca.Batch(ctx, [aligned(b) for b in blobs])
    st = assert_same_batches(host, res, blobs, False)
    assert (st == 0).all(), st
    host.close(); res.close()


def test_one_object_across_subsets_orders_and_host_resets(ctx):
    by = dict(rc.golden_blobs())
    pool = fixtures() + c4_blobs() + [v for k, v in by.items() if k.startswith("nonlattice_blobs8:")]
    pool = (pool + c4_blobs())[:64]
    cache, offs, lens = place(pool, seed=21)                  # a 64-blob cache tensor
    rng = np.random.default_rng(22)
    b = None
    for rnd in range(6):
        pick = rng.choice(64, size=int(rng.integers(6, 24)), replace=rnd % 3 == 2)
        blobs = [pool[i] for i in pick]
        host = ca.Batch(ctx, [aligned(x) for x in blobs])
        if rnd == 3:
            b.reset([aligned(x) for x in blobs])              # a host reset between resident ones
            assert b.walk_stats().host_walked == len(blobs)
        elif b is None:
            b = ca.Batch.resident(ctx, cache, offs[pick], lens[pick])
        else:
            b.reset_resident(cache, offs[pick], lens[pick])
            assert b.walk_stats().device_walked == len(blobs)
        assert_same_batches(host, b, blobs, rnd % 2 == 1)
        host.close()
    b.close()


def test_argument_errors(ctx):
    c4 = c4_blobs()[:2]
    buf, offs, lens = place(c4, seed=30)
    with pytest.raises(ca.CortoError) as e:
        ca.Batch.resident(ctx, buf, offs + np.uint64(4), lens)
    assert e.value.code == -8
    h = C.c_void_p()
    assert ca.lib().crthip_batch_create_resident(ctx.handle, 2, None, offs.ctypes.data, lens.ctypes.data, C.byref(h)) == -8
    # a failed reset leaves the object empty-handed; the next reset works
    b = ca.Batch.resident(ctx, buf, offs, lens)
    with pytest.raises(ca.CortoError) as e:
        b.reset_resident(buf, offs + np.uint64(8), lens)
    assert e.value.code == -8 and ca.lib().crthip_batch_size(b.handle) == 0
    b.reset_resident(buf, offs, lens)
    assert len(b) == 2 and b.walk_stats().device_walked == 2
    b.close()
