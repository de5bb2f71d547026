"""The encoders' tile and size-class limits by the library's own headers (tests/cpp/enc_size_probe.cpp), and every row of
tests/enc_size_classes.py on the side of its limit it is named for - by the probe's answer for the row's real counts.  For every mesh and cloud
row the host models of the device code (the topology pass, the input pass, the splice) equal the host encoder, and the host encoder equals the
reference: through the fixture tests/golden/enc_boundaries.npz everywhere, and against the reference itself where oracle/_ref exists.
No GPU: the probe is host code and every encoder here runs on the CPU.  tests/test_encode_size_classes_gpu.py runs the same rows on the device.

Out of scope: the corner sort's 32-bit pass (16.7 M estimated-normal vertices in one chunk) is left unreached - the 24-bit pass is the
65 536-vertex batch; the Tunstall coder's 2^23 stream limit is pinned by test_per_mesh_errors_leave_the_neighbours_alone."""
import functools
import os
import re

import numpy as np
import pytest

import corto_amd as ca
import cstream_model as cm
import enc_size_classes as ec
from oracle import oracle as oc
from oracle import refcodec as rc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    p = ec.Probe(tmp_path_factory.mktemp("enc_size_probe"))
    yield p
    p.close()


@functools.lru_cache(maxsize=64)
def _built(cid):
    row = {r[0]: r for r in ec.mesh_rows()}[cid]
    return ec.build(row)


def _ids(rows):
    return [r[0] for r in rows]


# ------------------------------------------------------------------------------------------------------------------------------------
# the limits

def test_probe_reproduces_the_limits(probe):
    """the values the tables were sized from"""
    want = dict(ENC_PACK_MAX_N=16, ENC_STAGE=4096, ENC_STAGE_PAD=576, ENC_HIST_CHUNK=1 << 18, ENC_TRIE_LDS_MAX=24 * 1024, RS_TILE=4096, RS_THREADS=256,
                DENC_BLOCK=1024, ETOPO_LDS_MAX=156 * 1024, ESP_TILE=4096, DIRECT_BYTES=1 << 20, ENC_PACK_TILE_WORDS=256 * 16 + 4, ENC_PARSE_WINDOW=64,
                ENC_DELTA_SCAN=256, ENC_JOB_BLOCK=256)
    assert {k: probe.num("const", k) for k in want} == want
    assert probe.num("fits_last_closed") == ec.FITS_LAST == 2283
    assert [probe.num("rs_blocks", n) for n in (0, 1, 4096, 4097, 8192, 8193)] == [1, 1, 1, 2, 2, 3]
    assert [probe.num("rs_bits", v) for v in (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [8, 8, 16, 16, 24, 24, 32]
    assert probe.num("parse_lds", 0) == 768 + 4096 + 576 and probe.num("parse_lds", 24 * 1024) == 768 + 4096 + 576 + 48 * 1024
    assert [probe.num("esp_tiles", m, b) for m, b in ((0, 4096), (0, 4097), (5, 4091), (5, 4092))] == [1, 2, 1, 2]
    assert probe.parse(4096 + 576) == (False, True) and probe.parse(4096 + 576 + 1) == (False, False)
    # the fullest tile k_enc_pack can be given - 256 elements of ENC_PACK_MAX_N components, 32 bits each, behind a carry of 31 bits - ends
    # inside the word after the tile's, which the buffer has (and one more, for the field that straddles it)
    top = (31 + 256 * probe.num("const", "ENC_PACK_MAX_N") * 32) // 32
    assert top + 1 < probe.num("const", "ENC_PACK_TILE_WORDS")


RESTATED = {                                              # what enc_size_probe.cpp restates, and the source line it restates
    "encode_batch.cpp": [r"constexpr uint64_t DIRECT_BYTES = 1u << 20;", r"uint32_t rs_blocks(uint32_t n) { return std::max(1u, (n + RS_TILE - 1)/RS_TILE); }",
                         r"while(bits < 32 && (vbase >> bits)) bits += 8;", r"fb += (J.nface + 255)/256; vb += (J.nvert + 255)/256;",
                         r"blocks += J.kind == DENC_NRM_BORDER ? 1u : (J.count + DENC_BLOCK - 1)/DENC_BLOCK;", r"if(b < DIRECT_BYTES) memcpy("],
    "k_encode.hip": [r"constexpr uint32_t ENC_PACK_TILE_WORDS = 256*ENC_PACK_MAX_N;", r"__shared__ uint32_t buf[ENC_PACK_TILE_WORDS + 4];",
                     r"if(base + 64 + ENC_STAGE_PAD > s1 && s1 < size) {", r"s0 = base; s1 = min(size, s0 + ENC_STAGE + ENC_STAGE_PAD);",
                     r"bound += l > 2 ? (l - 1)/2 : 0u;", r"E.level_bound = 1 + bound;", r"if(S.ntrie <= trie_lds_entries) enc_parse_body<true>(S, as_lds(lds_));",
                     r"for(uint32_t base = 0; base < nitems; base += 256) {"],
    "k_encode_batch.hip": [r"for(uint32_t base = 0; base < J.count; base += 256) {", r"const uint32_t first = (blockIdx.x - block_start[j])*DENC_BLOCK;"],
    "encode_gpu.cpp": [r"for(uint32_t b = 0; b < sizes[i]; b += ENC_HIST_CHUNK) chunks.push_back(", r"const uint64_t entries = (uint64_t)hd[1]*tabs[i].nsym*tabs[i].nsym;",
                       r"if(entries <= ENC_TRIE_LDS_MAX) { dev_ids.push_back(i);"],
}


@pytest.mark.parametrize("name", sorted(RESTATED))
def test_what_the_probe_restates_is_still_what_the_sources_say(name):
    """rules that live inside a .cpp or .hip file cannot be called from the probe: it restates them, and this holds the restatement to the text"""
    text = re.sub(r"\s+", " ", open(os.path.join(ec.ROOT, "corto_amd", "csrc", name)).read())
    for line in RESTATED[name]:
        assert re.sub(r"\s+", " ", line) in text, "%s no longer has `%s`: tests/cpp/enc_size_probe.cpp restates it" % (name, line)


# ------------------------------------------------------------------------------------------------------------------------------------
# every row on its side

@pytest.mark.parametrize("row", ec.BLOCK_CASES, ids=_ids(ec.BLOCK_CASES))
def test_block_rows_are_on_their_side(probe, row):
    m, kw = ec.build(row)
    info = ca.probe(ca.aligned_blob(ca.encode(m, **kw)))
    assert (info.nvert, m.nvert) == (row[2]["nvert"], row[2]["nvert"]), row[0]
    got = (probe.num("job_blocks", info.nvert), probe.num("delta_blocks", info.nvert))
    assert got == row[3], "%s: %d vertices are %s job blocks / k_enc_delta workgroups, the row is named for %s" % (row[0], info.nvert, got, row[3])


def test_block_rows_hold_the_last_and_the_first_of_each_block(probe):
    jb, db = probe.num("const", "ENC_JOB_BLOCK"), probe.num("const", "DENC_BLOCK")
    sizes = sorted(ec.BLOCK_SIDES)
    assert sizes == [jb - 1, jb, jb + 1, db - 1, db, db + 1]


@pytest.mark.parametrize("row", ec.BORDER_CASES, ids=_ids(ec.BORDER_CASES))
def test_border_rows_are_on_their_side(probe, row):
    m, kw = ec.build(row)
    scan = probe.num("const", "ENC_DELTA_SCAN")
    nb = ec.boundary_vertices(m)
    assert nb == row[3]
    assert m.nvert > 2 * scan and nb in (scan - 1, scan, scan + 1, 2 * scan - 1, 2 * scan, 2 * scan + 1), (row[0], nb, scan)
    # the boundary vertices are spread over the encode order: the compaction's running count passes `scan` well inside the mesh, not in its first step
    t = ca.encode_topology_model(m, 0, **kw)
    order = t["quads"][:, 0]
    onb = np.zeros(m.nvert, bool)
    idx = m.index.astype(np.int64)
    x = np.zeros(m.nvert, dtype=np.int64)
    for k in range(3):
        np.bitwise_xor.at(x, idx[:, k], idx[:, (k + 1) % 3]); np.bitwise_xor.at(x, idx[:, k], idx[:, (k + 2) % 3])
    onb[x != 0] = True
    w = np.cumsum(onb[order])
    steps_with_boundary = len({int(i) // scan for i in np.nonzero(onb[order])[0]})
    assert steps_with_boundary >= 4 and w[scan - 1] < scan - 1, (row[0], steps_with_boundary, int(w[scan - 1]))


@pytest.mark.parametrize("batch", ec.CORNER_BATCHES + ec.VBASE_BATCHES, ids=_ids(ec.CORNER_BATCHES + ec.VBASE_BATCHES))
def test_estimate_batches_are_on_their_side(probe, batch):
    bid, items, side = batch
    built = [b(**kw) for b, kw in items]
    assert all(k["normal_prediction"] in (ca.ESTIMATED, ca.BORDER) for _, k in built)
    infos = [ca.probe(ca.aligned_blob(ca.encode(m, **k))) for m, k in built]
    corners, verts = sum(3 * i.nface for i in infos), sum(m.nvert for m, _ in built)
    if bid.startswith("corners"):
        assert corners == int(bid.split("_")[1]), (bid, corners)
        assert probe.num("rs_blocks", corners) == side, "%s: %d corners are %d radix workgroups" % (bid, corners, probe.num("rs_blocks", corners))
    else:
        assert verts == int(bid.split("_")[1]), (bid, verts)
        assert probe.num("rs_bits", verts) == side, "%s: %d vertices sort over %d key bits" % (bid, verts, probe.num("rs_bits", verts))


def test_corner_batches_hold_the_last_and_the_first_of_each_tile(probe):
    tile = probe.num("const", "RS_TILE")
    want = [tile - tile % 3 - (0 if tile % 3 else 3), tile + 3 - tile % 3, 2 * tile - (2 * tile) % 3 - (0 if (2 * tile) % 3 else 3), 2 * tile + 3 - (2 * tile) % 3]
    assert [int(b[0].split("_")[1]) for b in ec.CORNER_BATCHES] == want          # 4095, 4098, 8190, 8193: corners come in threes


@pytest.mark.parametrize("row", ec.FITS_CASES, ids=_ids(ec.FITS_CASES))
def test_fits_lds_rows_are_on_their_side(probe, row):
    m, kw = ec.build(row)
    assert probe.fits(m.nvert, m.nface) == row[3], "%s: %d vertices / %d faces crossed enc_topo_fits_lds" % (row[0], m.nvert, m.nface)
    assert ca.encode_topology_fits_lds(m) == row[3], row[0]                       # the exported rule says the same
    if "faces" in row[0]:
        assert 3 * m.nface == int(row[0].split("_")[2])
        assert not probe.fits(4, m.nface)                                         # whatever the vertex count: the state's bytes decide first
    if "nvert" in row[0]:
        assert m.nvert == int(row[0].split("_")[2]) and probe.fits(65534, m.nface) and not probe.fits(65535, m.nface)


def test_the_face_bound_of_fits_lds_is_shadowed(probe):
    """3*nface <= 65535 never decides: the largest face count whose 16-bit state fits ETOPO_LDS_MAX is far below it.  Written down so that a
    change of the headers that makes the bound reachable is seen"""
    last = max(nf for nf in range(1, 22000) if probe.fits(3, nf))
    assert 3 * last < 65535 // 4, last


@pytest.mark.parametrize("row", ec.DIRECT_CASES, ids=_ids(ec.DIRECT_CASES))
def test_direct_rows_are_on_their_side(probe, row):
    m, kw = ec.build(row)
    array, nbytes, direct = row[3]
    real = {"position": m.position, "color": m.color, "index": m.index}[array].nbytes
    assert real == nbytes, (row[0], real)
    assert (probe.ask("direct", real)[0] == "1") == direct, "%s: %d bytes crossed DIRECT_BYTES" % (row[0], real)
    edge = probe.num("const", "DIRECT_BYTES")
    assert edge - 12 < nbytes < edge + 12


@pytest.mark.parametrize("row", ec.CLOUD_CASES, ids=_ids(ec.CLOUD_CASES))
def test_cloud_rows_are_on_their_side(probe, row):
    m, kw = ec.build(row)
    assert m.nvert == row[2]["n"] and m.nface == 0
    assert probe.num("rs_blocks", m.nvert) == row[3], (row[0], probe.num("rs_blocks", m.nvert))
    # distinct quantised points: the blob's own positions, decoded by the oracle, have no two equal rows
    pos = oc.decode(ca.aligned_blob(ca.encode(m, **kw)))["position"]
    assert len(np.unique(pos.view(np.uint32).reshape(-1, 3), axis=0)) == m.nvert, row[0]


def test_cloud_rows_hold_the_last_and_the_first_of_each_tile(probe):
    tile = probe.num("const", "RS_TILE")
    assert sorted(ec.CLOUD_SIDES) == [1, 2, 3, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1]


@pytest.mark.parametrize("n", sorted(ec.TUN_SIDES))
def test_tunstall_rows_are_on_their_side(probe, n):
    got = probe.parse(n) + (probe.num("hist_chunks", n),)
    assert got == ec.TUN_SIDES[n], "%d symbols: (one window, staged once, histogram workgroups) = %s, the rows are named for %s" % (n, got, ec.TUN_SIDES[n])


def test_tunstall_rows_hold_the_last_and_the_first_of_each_edge(probe):
    w, st, pad, ch = (probe.num("const", k) for k in ("ENC_PARSE_WINDOW", "ENC_STAGE", "ENC_STAGE_PAD", "ENC_HIST_CHUNK"))
    want = {e + d for e in (w, 2 * w, st + pad, 2 * st, ch, 2 * ch) for d in (-1, 0, 1)}
    assert set(ec.TUN_SIDES) == want
    for row in ec.TUN_CASES:
        s = ec.build(row)
        assert len(s) == row[2]["n"] and s.dtype == np.uint8
        nsym = len(np.unique(s))
        assert (3 <= nsym <= 6 and (nsym == 6 or len(s) < 200)) if row[2]["kind"] == "six" else nsym == 2, row[0]     # (the short ones miss a rare symbol)
        if row[2]["kind"].startswith("tail"):
            assert list(np.nonzero(s != s[0])[0]) == [len(s) - int(row[2]["kind"][4:])], row[0]


def _lengths(block):
    nsym, probs = ec.block_tables(block)
    return nsym, oc.tunstall_tables(probs)[1]


@pytest.mark.parametrize("row", ec.TRIE_CASES, ids=_ids(ec.TRIE_CASES))
def test_trie_rows_are_on_their_side(probe, row):
    s = ec.build(row)
    nsym = len(np.unique(s))
    assert nsym == row[2]["nsym"]
    # the probabilities the coder sees: count*255/size for every symbol, all equal here - any order gives the same dictionary lengths
    probs = np.stack([np.arange(nsym), np.full(nsym, (len(s) // nsym) * 255 // len(s))], 1).astype(np.uint8)
    lengths = oc.tunstall_tables(probs)[1]
    bound, entries, device = probe.trie(nsym, lengths)
    assert bound == 1 and entries == nsym * nsym, (row[0], bound, entries)
    assert device == row[3], "%s: a trie bound of %d entries crossed ENC_TRIE_LDS_MAX" % (row[0], entries)
    if rc.available():
        blk = rc.tunstall_compress_block(s)
        n2, l2 = _lengths(blk)
        assert n2 == nsym and probe.trie(n2, l2) == (bound, entries, device)      # the reference's own table says the same


def test_trie_rows_are_the_last_and_the_first(probe):
    cap = probe.num("const", "ENC_TRIE_LDS_MAX")
    a, b = ec.TRIE_CASES[0][2]["nsym"], ec.TRIE_CASES[1][2]["nsym"]
    assert b == a + 1 and a * a <= cap < b * b
    assert probe.ask("trie_in_lds", a * a, a * a)[0] == "1" and probe.ask("trie_in_lds", b * b, a * a)[0] == "0"


def test_tunstall_rows_hold_both_kinds_of_trie_at_every_length(probe):
    """at every length the six-symbol stream's trie is built on the device and parsed from LDS, and the two-symbol streams' - dictionaries whose
    words reach 255 symbols, the look-ahead ENC_STAGE_PAD is sized for - outgrow ENC_TRIE_LDS_MAX: made by the host, walked in global memory.
    One call of all rows is a launch that holds both kinds"""
    cap = probe.num("const", "ENC_TRIE_LDS_MAX")
    longest = 0
    for row in ec.TUN_CASES:
        nsym, lengths = ec.stream_lengths(ec.build(row))
        bound, entries, device = probe.trie(nsym, lengths)
        if row[2]["kind"] != "two":                                # (some of the short two-symbol streams' dictionaries are small enough for the device)
            assert device == (row[2]["kind"] == "six"), (row[0], bound, entries)
        elif row[2]["n"] > 129:
            assert not device, (row[0], bound, entries)
        assert device or probe.ask("trie_in_lds", entries, cap)[0] == "0"
        if row[2]["kind"] == "two" and row[2]["n"] > 4096:
            longest = max(longest, int(lengths.max()))
    assert longest == 255, longest


@pytest.mark.parametrize("row", ec.VALUE_CASES, ids=_ids(ec.VALUE_CASES))
def test_value_rows_are_on_their_side(probe, row):
    kind, a = ec.build(row)
    nitems = a.shape[0] if kind == ca.ENC_ARRAY else a.size
    assert probe.num("job_blocks", nitems) == row[3], (row[0], nitems)
    assert a.shape[1] <= probe.num("const", "ENC_PACK_MAX_N")
    words, logs = cm.model_array(a) if kind == ca.ENC_ARRAY else cm.model_values(a.astype(np.int32))
    if kind == ca.ENC_ARRAY:
        first = int(logs[0][:256].astype(np.int64).sum()) * a.shape[1]              # bits of the first tile
        if row[0] == "values_full_tiles":
            assert a.shape[1] == probe.num("const", "ENC_PACK_MAX_N") and first % 32 == 16
            assert (logs[0][1:] == 32).all() and a.shape[0] > 2 * 256 + 1          # a carry into two whole tiles of 32-bit fields and a partial one
        if row[0] == "values_word_edge_0":
            assert first % 32 == 0
        if row[0] == "values_word_edge_1":
            assert first % 32 == 1
    if row[0].endswith("_heads"):                                                    # the log arrays' heads: 0..3 bytes off a dword
        assert {(c * a.shape[0]) % 4 for c in range(a.shape[1])} == {0, 1, 2, 3}, row[0]
    if rc.available():
        data = cm.expected_stream(words, [rc.tunstall_compress_block(lg) for lg in logs])
        assert ec.reference_matches(row[0], data), row[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# the host models of the device code, the host encoder, the reference

T_ARRAYS = ("faces", "group_end", "quads", "clers", "split_words")
T_COUNTS = ("nvert", "nface", "max_front", "split_bits")


def _input_bits(r):
    return (r["index_out_of_range"], r["recipe"], r["mn"].view(np.uint32).tolist(), r["mx"].view(np.uint32).tolist(),
            int(np.array([r["sum"]], dtype=np.float64).view(np.uint64)[0]), int(np.array([r["step"]], dtype=np.float32).view(np.uint32)[0]))


@pytest.mark.parametrize("cid", _ids(ec.mesh_rows()))
def test_models_equal_the_host_encoder_and_the_reference(cid):
    """the source the device runs, compiled for the host in the kernels' partition, against the host encoder: the topology pass array by array,
    the input pass bit for bit, the splice byte for byte at two misalignments of the arena; and the host encoder against the reference"""
    m, kw = _built(cid)
    host = ca.encode(m, **kw)
    if m.nface:
        a, b = ca.encode_topology_model(m, 0, **kw), ca.encode_topology_model(m, 1, **kw)
        for k in T_ARRAYS:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (cid, k)
        for k in T_COUNTS:
            assert a[k] == b[k], (cid, k, a[k], b[k])
        info = ca.probe(ca.aligned_blob(host))
        assert (a["nvert"], a["nface"]) == (info.nvert, info.nface), cid
    if m.nvert:
        assert _input_bits(ca.encode_input_model(m, 0, **kw)) == _input_bits(ca.encode_input_model(m, 1, **kw)), cid
    for mis in (0, 5):
        blob, pad = ca.encode_splice_model(m, dst_misalign=mis, **kw)
        assert blob.tobytes() == host.tobytes(), (cid, mis)
        assert len(pad) == (-len(blob)) % 16 and not pad.any(), (cid, mis)
    if cid in ec.NO_REFERENCE:
        return                                                                    # (the reference faults on these inputs: enc_size_classes.NO_REFERENCE)
    assert ec.reference_matches(cid, host.tobytes()), "%s: the host encoder's bytes are not the reference's (fixture)" % cid
    if rc.available():
        assert rc.encode(m, **kw).tobytes() == host.tobytes(), cid


def test_tunstall_fixture_is_the_reference(have_ref):
    """the fixture's blocks are what the reference writes today (where it is here); the device module compares with the fixture"""
    if not have_ref:
        return
    for row in ec.TUN_CASES + ec.TRIE_CASES:
        assert ec.reference_matches(row[0], rc.tunstall_compress_block(ec.build(row)).tobytes()), row[0]
