"""crthip_batch_bind_compact's contract as a sequential model, written from include/corto_hip.h (a boolean array, a running count and loops - no
mask words, no scans, no blocks), the properties every result has whatever the model says, and the named inputs.  Not a test module:
tests/test_compact_cpu.py and tests/test_compact_gpu.py import it."""
import numpy as np

E_ARGUMENT = -8
E_FORMAT = -7
E_LIMIT = -11
FILL = 0xCD
FILL32 = FILL * 0x01010101
NO_VERTEX = 0xFFFFFFFF
BLOB_MAX = 8192                                # compact_blob's limit as csrc/compact.h states it: nvert and the bound nface


def in_blob(nvert, nface):
    return nvert <= BLOB_MAX and nface <= BLOB_MAX


def build(src, nvert, faces=None, vertex_capacity=None, index_capacity=None, has_order=True, has_index=True, ngather=0):
    """One mesh set.  src: the id list (3*nface words, of which 3*faces are read).  Returns (newid (nvert,), order cut to the capacity, index cut
    to the capacity, counts (vertices, used, faces, clipped), the full order)."""
    src = [int(x) for x in np.asarray(src).reshape(-1)]                        # (python integers: the loops below are the model)
    F = len(src) // 3 if faces is None else faces
    vcap = nvert if vertex_capacity is None else vertex_capacity
    icap = len(src) if index_capacity is None else index_capacity
    used = [False] * nvert
    for k in range(3 * F):
        if src[k] < nvert:
            used[src[k]] = True
    newid = np.full(nvert, NO_VERTEX, np.uint32)
    order = []
    count = 0
    for v in range(nvert):
        if used[v]:
            newid[v] = count
            order.append(v)
            count += 1
    index = [NO_VERTEX] * (3 * F)
    ids = newid.tolist()
    for k in range(3 * F):
        if src[k] < nvert:
            index[k] = ids[src[k]]
    index = np.array(index, np.uint32).reshape(-1)
    clipped = int(((has_order or ngather) and count > vcap) or (has_index and 3 * F > icap))
    order = np.array(order, np.uint32)
    return newid, order[:vcap], index[:icap], (nvert, count, F, clipped), order


def gathered(source, order, E, stride, vertex_capacity):
    """what a gather leaves: the E bytes of every vertex of order[:vertex_capacity] of a source given as bytes with a byte stride, back to back"""
    raw = np.asarray(source).view(np.uint8).reshape(-1)
    out = np.zeros((min(len(order), vertex_capacity), E), np.uint8)
    for j, v in enumerate(order[:vertex_capacity]):
        out[j] = raw[int(v) * stride:int(v) * stride + E]
    return out


def check_properties(src, nvert, newid, order, index, counts, faces=None, tag=""):
    """The model-free properties.  order and index are the written parts; counts the record as a tuple"""
    src = np.asarray(src).reshape(-1).astype(np.uint64)
    F = len(src) // 3 if faces is None else faces
    vertices, used, cfaces, clipped = counts
    assert vertices == nvert and cfaces == F and clipped in (0, 1), (tag, counts)
    assert used <= min(nvert, 3 * F), (tag, counts)
    assert len(order) <= used and len(index) <= 3 * F, tag
    assert (np.diff(order.astype(np.int64)) > 0).all(), (tag, "order is not strictly ascending")
    if newid is not None:
        assert newid.shape == (nvert,), tag
        assert (newid[order] == np.arange(len(order))).all(), (tag, "newid[order[j]] != j")
        assert int((newid != NO_VERTEX).sum()) == used, (tag, "the used count is not the number of new ids")
    ok = src[:len(index)] < nvert
    assert (index[ok] < used).all(), (tag, "an index word is not below used")
    assert (index[~ok] == NO_VERTEX).all(), (tag, "an unusable id did not become CRTHIP_NO_VERTEX")
    if newid is not None:
        assert (index[ok] == newid[src[:len(index)][ok].astype(np.int64)]).all(), tag


def assert_same(got, exp, tag):
    """(newid, order, index, counts) against build()'s first four, byte for byte"""
    for name, g, e in zip(("newid", "order", "index"), got[:3], exp[:3]):
        if g is None:
            continue
        assert g.dtype == np.uint32 and g.tobytes() == e.tobytes(), (tag, name, g[:8], e[:8])
    c = got[3]
    assert (c.as_tuple() if hasattr(c, "as_tuple") else tuple(c)) == tuple(exp[3]), (tag, "counts", c, exp[3])


# ---- the named inputs --------------------------------------------------------------------------------------------------------------------------

def strip(nvert):
    """a triangle strip over nvert >= 3 vertices: every vertex used, nvert - 2 faces"""
    f = np.arange(nvert - 2, dtype=np.uint32)
    return np.stack([f, f + 1, f + 2], 1).reshape(-1)


def every_other(nvert, rng):
    """random faces over the even vertices only: about half the vertices used, in no order"""
    even = np.arange(0, nvert, 2, dtype=np.uint32)
    return rng.choice(even, size=3 * max(1, nvert // 3)).astype(np.uint32)


def only_last(nvert):
    return np.full(3, nvert - 1, np.uint32)


def with_bad_ids(nvert, rng):
    """a few usable ids among ids >= nvert, nvert itself and 0xFFFFFFFF"""
    src = rng.integers(0, max(nvert, 1), size=3 * 40).astype(np.uint32)
    src[::4] = nvert
    src[1::7] = NO_VERTEX
    src[2::9] = nvert + 12345
    return src


MASK_EDGES = (1, 31, 32, 33, 63, 64, 65)       # a mask word's ends
BLOCK_EDGES = (255, 256, 257)                  # a block of 256 vertices' ends


def named(name, seed=1):
    """-> (src uint32, nvert)"""
    rng = np.random.default_rng(seed)
    kind, n = name.rsplit("_", 1)
    n = int(n)
    if kind == "all":
        return (strip(n) if n >= 3 else np.arange(3, dtype=np.uint32) % n), n
    if kind == "none":
        return np.zeros(0, np.uint32), n
    if kind == "last":
        return only_last(n), n
    if kind == "half":
        return every_other(n, rng), n
    if kind == "bad":
        return with_bad_ids(n, rng), n
    raise KeyError(name)


NAMED = ["%s_%d" % (k, n) for n in MASK_EDGES + BLOCK_EDGES for k in ("all", "none", "last", "half", "bad")]
