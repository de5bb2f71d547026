"""GPU (-m gpu): every row of tests/enc_size_classes.py - the inputs on either side of the encoders' tile and size-class limits - through every
entry point that reaches its kernel: ca.encode(ctx=), encode_batch, encode_batch_resident, encode_batch_to_device (read back),
tunstall_encode_blocks, encode_values.  Both sides of a limit go in one call where the limit is per item.  The expected bytes are the host
encoder's (a separate code path, pinned to the reference by tests/test_encode_size_classes_cpu.py) and the reference's own through the fixture
tests/golden/enc_boundaries.npz - and the reference itself where oracle/_ref travelled.  Beside the bytes each test asserts the path taken,
from the statistics the calls return (kernel launches, clouds_device_sorted, host-made tables, the topology counters): a row that silently
moved to the other path fails.

What has no counter: whether build_image staged an input array or sent it from the caller's array (DIRECT_BYTES) - the CPU module pins the
side, the bytes are checked here on both sides in one call and alone; and whether k_enc_tun_parse kept a trie in LDS - the CPU module pins which
rows are of which kind, host-made tables are counted here.

Out of scope: the corner sort's 32-bit pass needs 16.7 M estimated-normal vertices in one chunk and is left unreached (the 24-bit pass is the
65 536-vertex batch); the Tunstall coder's 2^23 stream limit is pinned by test_per_mesh_errors_leave_the_neighbours_alone.

Every input seeded.  Run as one pytest invocation under a time limit of its own."""
import numpy as np
import pytest

import corto_amd as ca
import cstream_model as cm
import enc_size_classes as ec
from oracle import refcodec as rc

pytestmark = pytest.mark.gpu

E_LIMIT = -11
TOPO_KERNELS = ("enc_topo_compact", "enc_topo_pair", "enc_topo_walk")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    p = ec.Probe(tmp_path_factory.mktemp("enc_size_probe"))
    yield p
    p.close()


def _context(mode):
    c = ca.Context(0)
    c.set_encode_topology(mode)
    return c


@pytest.fixture(scope="module")
def host():
    c = _context("host")
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    c = _context("device")
    yield c
    c.close()


@pytest.fixture(scope="module")
def split():
    c = _context("split")
    yield c
    c.close()


def _items(rows):
    """[(id, mesh, keywords)] of table rows"""
    return [(r[0],) + ec.build(r) for r in rows]


def _batch_items(batch):
    bid, items, _ = batch
    return [("%s.%d" % (bid, k),) + b(**kw) for k, (b, kw) in enumerate(items)]


def _expected(items):
    """the host encoder's bytes of every item, held to the reference's (the fixture; the reference itself where it travelled)"""
    want = []
    for cid, m, kw in items:
        e = ca.encode(m, **kw).tobytes()
        if cid not in ec.NO_REFERENCE:
            assert ec.reference_matches(cid, e), "%s: the host encoder's bytes are not the reference's" % cid
            if rc.available():
                assert rc.encode(m, **kw).tobytes() == e, cid
        want.append(e)
    return want


def _same(tag, items, blobs, want):
    assert len(blobs) == len(want), tag
    for (cid, _, _), b, w in zip(items, blobs, want):
        assert len(b) == len(w) and bytes(b) == w, (tag, cid, len(b), len(w))


def _every_entry_point(ctx, items, want, tag, single=True):
    """the items as one batch through encode_batch, encode_batch_resident and encode_batch_to_device (host arrays and device arrays), and one by
    one through crthip_encode_gpu; returns the statistics of the three batch calls that took device arrays or host arrays: (host arrays,
    resident, to_device)"""
    ms, ks = [m for _, m, _ in items], [k for _, _, k in items]
    blobs, st = ca.encode_batch(ms, ctx, kw=ks, with_stats=True)
    _same((tag, "encode_batch"), items, [b.tobytes() for b in blobs], want)
    dm = [ca.mesh_to_device(m) for m in ms]
    blobs, st_r = ca.encode_batch_resident(dm, ctx, kw=ks, with_stats=True)
    _same((tag, "encode_batch_resident"), items, [b.tobytes() for b in blobs], want)
    stats = [st, st_r]
    for resident, arrays in ((True, dm), (False, ms)):
        out, offs, lens, st_d = ca.encode_batch_to_device(arrays, ctx, kw=ks, resident=resident, with_stats=True)
        arena = out.cpu().numpy()
        want_offs, want_total = ca.arena_layout(lens)
        assert offs.tolist() == want_offs.tolist() and st_d["total"] == want_total, tag
        _same((tag, "encode_batch_to_device", resident), items, [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], want)
        for o, n in zip(offs, lens):
            assert not arena[int(o) + int(n):(int(o) + int(n) + 15) & ~15].any(), (tag, "padding")
        stats.append(st_d)
    if single:
        for (cid, m, kw), w in zip(items, want):
            assert ca.encode(m, ctx=ctx, **kw).tobytes() == w, (tag, "encode(ctx=)", cid)
    return stats


def _launches(st, name):
    return st["kernel_times"][name]["launches"] if name in st["kernel_times"] else 0


def _topology_counters(st, mode, items, tag):
    """the topology mode's counters: device mode walks every mesh on the GPU, split mode those whose state fits LDS, host mode none"""
    meshes = [m for _, m, _ in items if m.nface]
    fits = sum(ca.encode_topology_fits_lds(m) for m in meshes)
    want = {"host": (0, 0), "device": (len(meshes), fits), "split": (fits, fits)}[mode]
    assert (st["topology_device"], st["topology_lds"]) == want, (tag, mode, st["topology_device"], st["topology_lds"], want)
    for name in TOPO_KERNELS:
        assert (_launches(st, name) > 0) == (want[0] > 0), (tag, mode, name)


# ------------------------------------------------------------------------------------------------------------------------------------
# meshes

def test_block_rows_in_one_batch(host, dev, split):
    """255 / 256 / 257 and 1023 / 1024 / 1025 vertices under DIFF, ESTIMATED and BORDER in one batch: the last thread of a job's last 256-block,
    the first of the next (k_enc_quantize_batch, k_enc_corners, k_enc_est_normal, k_enc_input_check through enc_job_of), and k_enc_delta's
    DENC_BLOCK; every job's blocks start behind a neighbour's"""
    items = _items(ec.BLOCK_CASES)
    want = _expected(items)
    for mode, ctx in (("host", host), ("device", dev), ("split", split)):
        stats = _every_entry_point(ctx, items, want, ("blocks", mode), single=mode == "host")
        for st in stats:
            _topology_counters(st, mode, items, "blocks")
            assert _launches(st, "enc_quantize_batch") == 1 and _launches(st, "enc_delta") == 1, mode
            assert st["clouds_device_sorted"] == 0 and st["clouds_host_sorted"] == 0
        for st in stats[1:3]:                                                     # device arrays: the input pass ran
            assert _launches(st, "enc_input_check") >= 1, mode


def test_border_compaction_rows(host, dev):
    """open meshes whose 255 / 256 / 257 / 511 / 512 / 513 boundary vertices are spread over the encode order: k_enc_delta's BORDER compaction
    carries its running count over steps of 256 vertices, and the count passes 256 and 512 inside a step"""
    items = _items(ec.BORDER_CASES)
    want = _expected(items)
    for mode, ctx in (("host", host), ("device", dev)):
        for st in _every_entry_point(ctx, items, want, ("border", mode), single=mode == "host"):
            _topology_counters(st, mode, items, "border")
            assert _launches(st, "enc_delta") == 1


@pytest.mark.parametrize("batch", ec.CORNER_BATCHES + ec.VBASE_BATCHES, ids=[b[0] for b in ec.CORNER_BATCHES + ec.VBASE_BATCHES])
def test_estimate_batches(host, dev, probe, batch):
    """the corner sort of a batch's estimated normals: corner totals on either side of one and two RS_TILE (4 095 / 4 098, 8 190 / 8 193), and
    vertex totals on either side of 2^8 and 2^16 - one, two and three radix passes, seen in the launch count: a histogram, a scan and a
    scatter a pass, beside k_enc_corners and k_enc_est_normal"""
    bid, _, side = batch
    items = _batch_items(batch)
    want = _expected(items)
    verts = sum(m.nvert for _, m, _ in items)
    bits = probe.num("rs_bits", verts)
    if bid.startswith("vbase"):
        assert bits == side, (bid, verts, bits)
    for mode, ctx in (("host", host), ("device", dev)):
        for st in _every_entry_point(ctx, items, want, (bid, mode), single=False):
            assert _launches(st, "enc_est_normal") == 2 + 3 * (bits // 8), (bid, mode, _launches(st, "enc_est_normal"), bits)
            _topology_counters(st, mode, items, bid)


def test_jobs_of_no_items(host, dev, split, monkeypatch):
    """a cloud of no vertices first, an item of vertices and no faces in the middle, a mesh whose faces are all degenerate last, among ordinary
    neighbours: blocks of the jobs behind an empty one are found (enc_job_of), nothing is launched for nothing.  Then the same batch cut into
    several device images ($CORTO_ENCODE_IMAGE_BUDGET, read when a context is made), so that chunk cuts fall beside the empty items"""
    items = [("zero.%s" % n,) + b(**kw) for n, b, kw in ec.ZERO_BATCH]
    assert [m.nvert == 0 for _, m, _ in items] == [True] + [False] * 6 and items[3][1].nface == 0 and items[3][1].nvert > 0
    want = _expected(items)
    for mode, ctx in (("host", host), ("device", dev), ("split", split)):
        for st in _every_entry_point(ctx, items, want, ("zero", mode), single=mode == "host"):
            _topology_counters(st, mode, items, "zero")
            assert st["clouds_device_sorted"] == 2 and st["clouds_host_sorted"] == 0, mode       # the 257-point cloud and the faceless item; not the empty one
    # per topology mode (the device pass's scratch makes an item's image larger), the smallest power-of-two budget that holds every item
    # alone: under twice the largest single image, so the four items of about that size cannot share one chunk
    ms, ks = [m for _, m, _ in items], [k for _, _, k in items]

    def chunked(small, mode):
        """every batch entry point on a context with a budget; the chunk counts that encode_batch_to_device reports"""
        counts = []
        small.set_encode_topology(mode)
        dm = [ca.mesh_to_device(m) for m in ms]
        for resident, arrays in ((False, ms), (True, dm)):
            out, offs, lens, st = ca.encode_batch_to_device(arrays, small, kw=ks, resident=resident, with_stats=True)
            arena = out.cpu().numpy()
            _same(("zero", "chunks to_device", mode, resident), items, [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], want)
            counts.append(st["splice"]["launches"])
        _same(("zero", "chunks", mode), items, [b.tobytes() for b in ca.encode_batch(ms, small, kw=ks)], want)
        _same(("zero", "chunks resident", mode), items, [b.tobytes() for b in ca.encode_batch_resident(dm, small, kw=ks)], want)
        return counts

    for mode in ("host", "device", "split"):
        counts = None
        for shift in range(13, 24):
            monkeypatch.setenv("CORTO_ENCODE_IMAGE_BUDGET", str(1 << shift))
            small = ca.Context(0)
            monkeypatch.delenv("CORTO_ENCODE_IMAGE_BUDGET")
            try:
                counts = chunked(small, mode)
            except ca.CortoError as e:
                assert e.code == E_LIMIT, e                                       # an item alone is beyond this budget: the next one
                continue
            finally:
                small.close()
            print("%s: image budget 2^%d: chunks %s" % (mode, shift, counts))
            break
        assert counts is not None and all(2 <= c <= len(items) for c in counts), (mode, counts)


def test_fits_lds_pairs_in_device_and_split_mode(host, dev, split, probe):
    """the last closed mesh whose walk state fits LDS and the next one; the pair at 3*nface = 65 535 / 65 538 (both outside: the state's
    bytes decide long before the face bound); a small mesh beside 65 534 and 65 535 vertices (the vertex bound) - in one batch, so one
    k_enc_topo_walk launch of each kind.  Device mode walks all six on the GPU, split mode the two that fit"""
    items = _items(ec.FITS_CASES)
    for (cid, m, _), row in zip(items, ec.FITS_CASES):
        assert probe.fits(m.nvert, m.nface) == row[3] == ca.encode_topology_fits_lds(m), cid
    want = _expected(items)
    nfit = sum(row[3] for row in ec.FITS_CASES)
    assert 0 < nfit < len(items)
    for mode, ctx in (("device", dev), ("split", split), ("host", host)):
        for st in _every_entry_point(ctx, items, want, ("fits", mode), single=False):
            _topology_counters(st, mode, items, "fits")
            if mode == "device":
                assert (st["topology_device"], st["topology_lds"]) == (len(items), nfit) and _launches(st, "enc_topo_walk") == 2     # the LDS walk and the global one
            if mode == "split":
                assert (st["topology_device"], st["topology_lds"]) == (nfit, nfit) and _launches(st, "enc_topo_walk") == 1


def test_direct_bytes_rows(host, dev):
    """a position array, a 4-byte colour and an index array 4 / 12 bytes below DIRECT_BYTES and at it: staged into the chunk's one upload, or sent
    from the caller's array - both in one call (the staged inputs lie in front of the direct ones), and each alone.  The index goes up only
    for the device topology pass; device arrays are read in place (the same rows, for the kernels' sake)"""
    items = _items(ec.DIRECT_CASES)
    want = _expected(items)
    for mode, ctx in (("host", host), ("device", dev)):
        for st in _every_entry_point(ctx, items, want, ("direct", mode), single=mode == "host"):
            _topology_counters(st, mode, items, "direct")
        for (cid, m, kw), w in zip(items, want):
            blobs, st = ca.encode_batch([m], ctx, kw=kw, with_stats=True)
            assert blobs[0].tobytes() == w, (cid, mode)
            raw = m.position.nbytes + (m.color.nbytes if kw.get("with_color", True) and m.color is not None else 0) + (m.index.nbytes if mode == "device" else 0)
            assert st["bytes_to_device"] >= raw, (cid, mode)


# ------------------------------------------------------------------------------------------------------------------------------------
# clouds

def test_cloud_rows_keep_the_device_sort(host, dev):
    """1, 2, 3 points and RS_TILE, 2*RS_TILE -1 / +0 / +1 points with distinct quantised positions, in one batch: every cloud's order is the
    device radix sort's (64 key bits: eight passes of a histogram, a scan and a scatter, then the flag kernel; one point is not sorted)"""
    items = _items(ec.CLOUD_CASES)
    want = _expected(items)
    sorted_clouds = sum(1 for _, m, _ in items if m.nvert >= 2)
    for mode, ctx in (("host", host), ("device", dev)):
        for st in _every_entry_point(ctx, items, want, ("clouds", mode), single=mode == "host"):
            assert st["clouds_device_sorted"] == len(items) and st["clouds_host_sorted"] == 0, mode
            assert _launches(st, "enc_zsort") == 25 * sorted_clouds + (len(items) - sorted_clouds), _launches(st, "enc_zsort")
            assert _launches(st, "enc_zkeys") == 2 * len(items)
            _topology_counters(st, mode, items, "clouds")


# ------------------------------------------------------------------------------------------------------------------------------------
# the Tunstall coder

def _reference_block(row, got):
    assert ec.reference_matches(row[0], got.tobytes()), "%s: not the reference's block (%d bytes)" % (row[0], len(got))
    if rc.available():
        assert rc.tunstall_compress_block(ec.build(row)).tobytes() == got.tobytes(), row[0]


def test_tunstall_rows_in_one_call(host, probe):
    """streams of 63 .. 129 symbols (one window, two, three), ENC_STAGE + ENC_STAGE_PAD, 2*ENC_STAGE, ENC_HIST_CHUNK and 2*ENC_HIST_CHUNK -1 / +0 / +1,
    each as six uneven symbols (trie from the device, parsed from LDS), two symbols at 0.4 % (words of up to 255 symbols: the look-ahead; a trie
    beyond ENC_TRIE_LDS_MAX, made by the host and walked in global memory) and one symbol with a single other one 1, 2, 3 positions before the
    end (a stream that ends inside a word, beside each edge) - and the two alphabets on either side of ENC_TRIE_LDS_MAX.  One launch holds all"""
    rows = ec.TUN_CASES + ec.TRIE_CASES
    streams = [ec.build(r) for r in rows]
    host_made = 0
    for r, s in zip(rows, streams):
        nsym, lengths = ec.stream_lengths(s)
        host_made += not probe.trie(nsym, lengths)[2]
    assert 0 < host_made < len(rows)
    blocks, times = ca.tunstall_encode_blocks(host, streams, with_times=True)
    for r, b in zip(rows, blocks):
        _reference_block(r, b)
    for name in ("enc_hist", "enc_tables", "enc_trie", "enc_tun_parse"):
        assert name in times, name
    assert times["enc_trie"]["launches"] == host_made, (times["enc_trie"]["launches"], host_made)      # (= streams the host made tables for)
    # either side of ENC_TRIE_LDS_MAX alone in one call: one trie from the device (in LDS), one from the host (in global memory)
    blocks, times = ca.tunstall_encode_blocks(host, [ec.build(r) for r in ec.TRIE_CASES], with_times=True)
    assert times["enc_trie"]["launches"] == 1
    for r, b in zip(ec.TRIE_CASES, blocks):
        _reference_block(r, b)
    # and every row alone: its window, stage and chunk edges without a neighbour's launch geometry
    for r, s in zip(rows, streams):
        if len(s) <= 8193:
            _reference_block(r, ca.tunstall_encode_blocks(host, [s])[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# value arrays

def test_value_rows_in_one_call(host, probe):
    """crthip_encode_values: 255 .. 513 elements as ARRAY and VALUES (the last item of a 256-item tile, the first of the next; the partial word
    carried from tile to tile); VALUES whose log arrays start 1, 2, 3 bytes off a dword, one of them ENC_HIST_CHUNK + 1 long; ARRAY of 16
    components 32 bits wide behind a 16-bit carry - the fullest tile k_enc_pack can be given; a tile that ends on a word and one that ends one
    bit past it.  Words against the restatement of the reference's coders, blocks against the reference's (the fixture)"""
    rows = ec.VALUE_CASES
    streams = [ec.build(r) for r in rows]
    got, times = ca.encode_values(host, streams, with_times=True)
    assert times["enc_pack"]["launches"] == 1 and "enc_tun_parse" in times
    host_made = 0
    for r, (kind, a), g in zip(rows, streams, got):
        assert ec.reference_matches(r[0], g.tobytes()), "%s: not the reference's stream (%d bytes)" % (r[0], len(g))
        words, logs = cm.model_array(a) if kind == ca.ENC_ARRAY else cm.model_values(a.astype(np.int32))
        nw = int(np.frombuffer(g[:4].tobytes(), dtype="<u4")[0])
        assert nw == len(words) and g[4:4 + 4 * nw].tobytes() == words.astype("<u4").tobytes(), r[0]
        if rc.available():
            assert g.tobytes() == cm.expected_stream(words, [rc.tunstall_compress_block(lg) for lg in logs]), r[0]
        for lg in logs:
            if len(np.unique(lg)) >= 2:
                host_made += not probe.trie(*ec.stream_lengths(lg))[2]
    assert times["enc_trie"]["launches"] == host_made
    # without the entropy coder: the widths come back as they are
    raw = ca.encode_values(host, streams, entropy=0)
    for r, (kind, a), g in zip(rows, streams, raw):
        words, logs = cm.model_array(a) if kind == ca.ENC_ARRAY else cm.model_values(a.astype(np.int32))
        assert g.tobytes() == cm.expected_stream(words, [np.array([len(x)], dtype="<u4").tobytes() + x.tobytes() for x in logs]), r[0]
