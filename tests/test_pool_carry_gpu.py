"""crthip_batch_decode_with_next and the pool's pipelined lanes: a lane decodes a stream of batches two at a time - the mesh stage of one
with the entropy stage of the next, the next's K-TAB inside k_front's grid and its K-STREAM inside k_delta_lds16's when both batches allow
it.  Everything here is raw-byte equality with the oracle (tolerance 0), with the carry on and with $CORTO_CARRY=0, on items that DIFFER in
size and content - with one item a mix-up of a lane's two batch objects would be invisible."""
import numpy as np
import pytest

import corto_amd as ca
from conftest import aligned
from corto_amd import synth
from oracle import oracle as oc

KEYS = ("position", "normal", "color", "uv", "radius", "index")
DTS = {"position": (np.float32, 3), "normal": (np.float32, 3), "color": (np.uint8, 4), "uv": (np.float32, 2), "index": (np.uint32, 3)}


def enc(mesh, **kw):
    kw.setdefault("normal_prediction", ca.BORDER)
    return ca.aligned_blob(ca.encode(mesh, **kw))


def c4_item(n, seed0):
    return [enc(synth.bumpy_sphere(64, 32, seed=seed0 + i), position_bits=14, uv_bits=12, normal_bits=10) for i in range(n)]


def flipped_item(n, seed0):
    return [enc(synth.bumpy_sphere_flipped(64, 32, seed=seed0 + i), position_bits=14, uv_bits=12, normal_bits=10) for i in range(n)]


def small_item(n, seed0):
    return [enc(synth.bumpy_sphere(40, 20, seed=seed0 + i), position_bits=13, uv_bits=11, normal_bits=9) for i in range(n)]


_refs = {}


def ref_of(blob):
    k = blob.tobytes()
    if k not in _refs:
        _refs[k] = oc.decode(blob)
    return _refs[k]


def assert_blob(got, ref, tag):
    for k in KEYS:
        if k not in ref:
            continue
        assert k in got, (tag, k)
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (tag, k)
        assert got[k].tobytes() == ref[k].tobytes(), (tag, k)


# ---- the pool ----------------------------------------------------------------------------------------------------------------

def pool_round(pool, items, steps, tag):
    """one run; every lane's every blob against the oracle of the item the lane says it holds; returns {(item, blob, key): bytes}"""
    rep, stamps = pool.run(items, steps=steps, warmup=0)
    assert rep.steps == steps and rep.failed_blobs == 0 and rep.first_error == 0 and len(stamps) == steps, (tag, rep.failed_blobs, rep.first_error)
    assert rep.poisoned_lanes == pool.lanes, (tag, rep.poisoned_lanes)
    assert (np.diff(stamps) >= 0).all() and stamps[-1] > 0, tag
    seen = {}
    for lane in range(pool.lanes):
        it, slot = pool.lane_item(lane)
        assert 0 <= it < len(items) and slot == 0, (tag, lane, it)
        for i, blob in enumerate(items[it]):
            ref = ref_of(blob)
            for k, (dt, w) in DTS.items():
                got = pool.lane_read(lane, i, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                if got.tobytes() != ref[k].tobytes():            # (whose bytes, then?  another item's blob at this place of the block is a mixed-up lane)
                    n = min(64, got.nbytes)
                    other = [(j, m) for j, item in enumerate(items) for m, b2 in enumerate(item)
                             if k in ref_of(b2) and ref_of(b2)[k].tobytes()[:n] == got.tobytes()[:n]]
                    raise AssertionError((tag, lane, it, i, k, "first bytes are those of (item, blob)", other, got.tobytes()[:16].hex()))
                seen[(it, i, k)] = got.tobytes()
        assert (pool.lane_read(lane, 0, "#tail", np.uint8, 256) == 0xA5).all(), (tag, lane)
    return seen


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_pool_lanes_pipelined_over_distinct_items(monkeypatch):
    """three items that differ in size and content (C4 units, flipped-diagonal units, a smaller grid: 64, 72 and 80 blobs -
    a batch shares dictionaries, and so can be carried, from 64 blobs on), so that the two
    batches alive on a lane are never the same blobs; step counts 1, 2, lanes - 1, lanes + 1 and 5 x lanes (prologue, epilogue, lanes that draw
    no ticket); afterwards every lane's every blob against the oracle and the block's tail still poisoned.  The same with the switch off,
    and the two bit-identical."""
    items = [c4_item(64, 100), flipped_item(72, 200), small_item(80, 300)]
    seen = {}
    for carry in ("1", "0"):
        monkeypatch.setenv("CORTO_CARRY", carry)
        pool = ca.Pool([0], threads=2, depth=2)              # four contexts on four hardware queues' worth of streams: single-stream lanes
        try:
            lanes = pool.lanes
            assert lanes == 4
            for steps in (1, 2, lanes - 1, lanes + 1, 5 * lanes):
                got = pool_round(pool, items, steps, "carry=%s steps=%d" % (carry, steps))
                for key, val in got.items():
                    assert seen.setdefault(key, val) == val, (carry, steps, key)
        finally:
            pool.close()
    assert {k[0] for k in seen} == {0, 1, 2}                 # every item was some lane's last batch in some run


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_pool_lanes_with_items_that_cannot_carry(monkeypatch):
    """a 34K-vertex mesh, a point cloud, a blob with long Tunstall streams and a batch of fewer than 64 streams, interleaved with items
    that can carry: their entropy stage runs as launches of its own (or with their mesh stage); the bytes are the oracle's"""
    items = [c4_item(64, 400),
             [enc(synth.bumpy_sphere(264, 130, seed=3))],
             flipped_item(64, 500),
             [enc(synth.point_cloud(90, 45, seed=2), normal_prediction=ca.DIFF)] * 3,
             [enc(synth.bumpy_sphere(512, 250, seed=1))],
             c4_item(5, 600)]
    for carry in ("1", "0"):
        monkeypatch.setenv("CORTO_CARRY", carry)
        pool = ca.Pool([0], threads=2, depth=2)
        try:
            rep, _ = pool.run(items, steps=36, warmup=0)
            assert rep.failed_blobs == 0 and rep.first_error == 0
            for lane in range(pool.lanes):
                it, _slot = pool.lane_item(lane)
                for i, blob in enumerate(items[it]):
                    ref = ref_of(blob)
                    for k, (dt, w) in DTS.items():
                        if k not in ref:
                            continue
                        got = pool.lane_read(lane, i, k, dt, (ref["nface"] if k == "index" else ref["nvert"]) * w)
                        assert got.tobytes() == ref[k].tobytes(), (carry, lane, it, i, k)
                assert (pool.lane_read(lane, 0, "#tail", np.uint8, 256) == 0xA5).all(), (carry, lane)
        finally:
            pool.close()


# ---- the entry point itself --------------------------------------------------------------------------------------------------------

def run_lane(ctx, seq):
    """seq: a list of lists of blobs, decoded as one lane's stream of batches on two batch objects; per batch (status, outputs, kernel names
    of the call that ran its mesh stage)"""
    objs = [ca.Batch(ctx, []), ca.Batch(ctx, [])]
    objs[1].set_parity(1)
    res, prev = [], None
    try:
        def collect(b):
            st = b.sync(raise_on_error=False)
            res.append((st.copy(), [b.host_outputs(i) for i in range(len(b))], set(b.kernel_times())))
        for k, blobs in enumerate(seq):
            o = objs[k & 1]
            o.reset(blobs)
            o.allocate_outputs(fill=0)
            if prev is None:
                o.decode_entropy()
            else:
                prev.decode_with_next(o)
                collect(prev)
            prev = o
        prev.decode_with_next(None)
        collect(prev)
    finally:
        for o in objs:
            o.close()
    return res


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("carry", ["1", "0"])
def test_decode_with_next_on_one_context(monkeypatch, carry):
    """a lane's stream of batches through crthip_batch_decode_with_next: items that carry, items that cannot, back to back.  With the carry
    on, a batch whose entropy stage rode in the grids of the batch before it has no K-TAB / K-STREAM launch of its own."""
    monkeypatch.setenv("CORTO_CARRY", carry)
    seq = [c4_item(64, 700), flipped_item(66, 1710), small_item(70, 2720), c4_item(64, 3730),
           [enc(synth.bumpy_sphere(264, 130, seed=4))], c4_item(64, 4740),
           [enc(synth.point_cloud(90, 45, seed=5), normal_prediction=ca.DIFF)], flipped_item(64, 5750),
           [enc(synth.bumpy_sphere(512, 250, seed=2))], c4_item(4, 6760), c4_item(64, 7770), c4_item(64, 8780)]
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        c.set_profiling(True)
        res = run_lane(c, seq)
    finally:
        c.close()
    assert len(res) == len(seq)
    for k, (st, outs, names) in enumerate(res):
        assert (st == 0).all(), (k, st)
        for i, blob in enumerate(seq[k]):
            assert_blob(outs[i], ref_of(blob), (carry, k, i))
    # A batch's entropy stage is enqueued by the call before its mesh stage only when that call carries it (or is the lane's first); otherwise it
    # runs in front of its own mesh stage, as in crthip_batch_decode.  So the K-TAB / K-STREAM launches of a call are its OWN batch's:
    tun = [bool({"tunstall_tables", "tunstall_stream"} & r[2]) for r in res]
    for k in (0, 1, 10, 11):
        assert "front" in res[k][2] and "delta_lds16" in res[k][2], (k, res[k][2])
    assert not tun[0]                                        # the first batch's stage ran alone, in the call before
    # batch 1 (flipped units) was carried by batch 0's grids, batch 11 by batch 10's - or, with the switch off, nothing was
    assert tun[1] == tun[11] == (carry == "0"), (carry, tun)
    # ... a batch behind one whose grids cannot carry (a 34K-vertex mesh, a cloud) runs its own, and so does one that cannot be carried (four
    # blobs: fewer than 64 streams) - whose grids, however, carry the batch behind it
    assert tun[5] and tun[7] and tun[9], (carry, tun)
    assert tun[10] == (carry == "0"), (carry, tun)


def corrupt_item(rng):
    """the fuzz tests' recipe on C4 blobs (byte flips, a burst, a garbage tail, a zeroed window), intact ones in between; only what the host
    walk accepts"""
    blobs, intact = [], []
    for i in range(100):
        b = enc(synth.bumpy_sphere(64, 32, seed=9000 + i), position_bits=14, uv_bits=12, normal_bits=10).copy()
        body = oc.parse_header(b)["body_offset"]
        mode = i % 5
        if mode == 0:
            for p in rng.integers(body, len(b), 6):
                b[p] ^= rng.integers(1, 256)
        elif mode == 1:
            p = int(rng.integers(body, max(body + 1, len(b) - 64))); b[p:p + 48] ^= 0xA5
        elif mode == 2:
            p = int(rng.integers(body, len(b))); b[p:] = rng.integers(0, 256, len(b) - p, dtype=np.uint8)
        elif mode == 3:
            p = int(rng.integers(body, max(body + 1, len(b) - 200))); b[p:p + 160] = 0
        blobs.append(aligned(b)); intact.append(mode == 4)
    return blobs, intact


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("carry", ["1", "0"])
def test_corrupt_batch_as_next_and_as_cur(monkeypatch, carry):
    """a batch with corrupted blobs between two intact batches - it is `next` of one call and `cur` of the following one: its per-blob
    statuses are those of crthip_batch_decode on a plain context, its intact blobs and both neighbouring batches the oracle's bytes.
    The decoder reports such blobs by status; nothing here is meant to fault."""
    monkeypatch.setenv("CORTO_CARRY", carry)
    blobs, intact = corrupt_item(np.random.default_rng(11))
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        keep = []
        for i, b in enumerate(blobs):
            try:
                ca.Batch(c, [b]).close(); keep.append(i)
            except ca.CortoError:
                assert not intact[i]
        assert len(keep) >= 64                              # (enough blobs to share dictionaries: the batch can be carried)
        bad = [blobs[i] for i in keep]
        plain = ca.Batch(c, bad)
        plain.allocate_outputs(fill=0)
        plain.decode()
        st_plain = plain.sync(raise_on_error=False).copy()
        plain.close()
        assert set(np.unique(st_plain)) <= {0, -5}
        good_a, good_b = c4_item(64, 9500), flipped_item(64, 9700)
        res = run_lane(c, [good_a, bad, good_b])
    finally:
        c.close()
    assert (res[1][0] == st_plain).all(), (res[1][0], st_plain)
    for j, i in enumerate(keep):
        if intact[i]:
            assert res[1][0][j] == 0
            assert_blob(res[1][1][j], ref_of(blobs[i]), (carry, "intact among corrupt", j))
    for k, item in ((0, good_a), (2, good_b)):
        assert (res[k][0] == 0).all(), (k, res[k][0])
        for i, blob in enumerate(item):
            assert_blob(res[k][1][i], ref_of(blob), (carry, "neighbour", k, i))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_decode_with_next_argument_errors():
    c = ca.Context(0)
    try:
        c.set_single_stream(True)
        a, b = ca.Batch(c, c4_item(2, 990)), ca.Batch(c, c4_item(2, 992))
        a.allocate_outputs(fill=0); b.allocate_outputs(fill=0)
        with pytest.raises(ca.CortoError):
            a.decode_with_next(b)                            # `a` was never `next`
        a.decode_entropy()
        with pytest.raises(ca.CortoError):
            a.decode_with_next(b)                            # the same parity
        a.decode()                                           # a planned batch finishes through crthip_batch_decode too
        assert (a.sync() == 0).all()
        for i, blob in enumerate(a.blobs):
            assert_blob(a.host_outputs(i), ref_of(blob), ("decode after decode_entropy", i))
        a.close(); b.close()
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_two_parities_keep_their_own_blocks():
    """a context's two sets of per-call blocks, told apart by everything that differs between them: batch P0 (parity 0, three blobs) and P1
    (parity 1, five blobs - so the status words' offsets differ - one of which fails alone with CRTHIP_E_FORMAT on a quantised position of
    span 65536, which also puts quant records behind P1's status words), then P0 again with two other blobs.  P1 is synced after the
    context has moved on.  Every sync returns its own batch's statuses, every output written is the oracle's, P1's transforms are those
    of a lone decode, and the prediction triples are read from the set of the batch decoded last and refused for the others."""
    import quantized_outputs as qo
    from conftest import load_golden
    FILL, BAD = 0xA5, 2
    sphere = lambda seed: enc(synth.bumpy_sphere(24, 12, seed=seed))
    p0 = [sphere(31), sphere(32), sphere(33)]
    p1 = [sphere(41), sphere(42), qo.traced("edge_65536")[0], sphere(43), sphere(44)]
    p0b = [ca.aligned_blob(load_golden("c4_unit")["crt"]), sphere(51)]
    qo.assert_edge("edge_65536")
    traces = {}

    def trace(blob):
        return traces.setdefault(blob.tobytes(), oc.decode(blob, trace=True))

    def prediction(b, i, blob):
        want = trace(blob)["_prediction"]
        got = b.debug_read(i, "prediction", want.size * 4).view(np.uint32).reshape(-1, 3)
        assert np.array_equal(got[1:], want[1:]), i

    def refused(b):
        with pytest.raises(ca.CortoError) as ei:
            b.debug_read(0, "prediction", 12)
        assert ei.value.code == qo.E_ARGUMENT

    def plain(b, blobs, tag):
        for i, blob in enumerate(blobs):
            assert_blob(b.host_outputs(i), ref_of(blob), (tag, i))

    c = ca.Context(0)
    A, B = ca.Batch(c, []), ca.Batch(c, [])
    try:
        c.set_single_stream(True)
        B.set_parity(1)
        A.reset(p0); A.allocate_outputs(fill=FILL)
        B.reset(p1); B.allocate_outputs(fill=FILL, quantized=("position",))
        A.decode_entropy()
        A.decode_with_next(B)
        prediction(A, 2, p0[2]); refused(B)
        assert list(A.sync(raise_on_error=False)) == [0, 0, 0]
        plain(A, p0, "P0")
        A.reset(p0b); A.allocate_outputs(fill=FILL)
        B.decode_with_next(A)
        prediction(B, 4, p1[4]); refused(A)                  # (parity 1's scratch block)
        A.decode_with_next(None)
        prediction(A, 1, p0b[1]); refused(B)
        st1 = B.sync(raise_on_error=False)                   # harvested when the context moved on to P0'
        assert list(st1) == [0, 0, qo.E_FORMAT, 0, 0], st1
        assert list(A.sync(raise_on_error=False)) == [0, 0]
        plain(A, p0b, "P0'")
        recs = {}
        for i, blob in enumerate(p1):
            got, ref, e = B.host_outputs(i), ref_of(blob), qo.Expected(blob, trace(blob), "position")
            t = B.quant_transform(i, "position")
            e.check_record(t, ("P1", i))
            recs[i] = bytes(t)
            assert e.written == (i != BAD)
            if e.written:
                assert got["position"].dtype == np.uint16 and got["position"].tobytes() == e.out.tobytes(), i
            else:
                assert (got["position"].view(np.uint8) == FILL).all()      # the refused attribute: nothing written
            for k in ("normal", "color", "uv", "grid", "index"):
                if k in ref:
                    assert got[k].tobytes() == ref[k].tobytes(), ("P1", i, k)
        lone = ca.Batch(c, p1)
        lone.allocate_outputs(fill=FILL, quantized=("position",))
        lone.decode()
        assert list(lone.sync(raise_on_error=False)) == list(st1)
        for i in range(len(p1)):
            if i != BAD:
                assert bytes(lone.quant_transform(i, "position")) == recs[i], i
        lone.close()
    finally:
        A.close(); B.close(); c.close()
