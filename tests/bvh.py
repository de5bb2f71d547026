"""A sequential model of crthip_batch_bind_bvh, written from the contract in include/corto_hip.h alone: numpy boxes, Python's sorted on
(key, f), and the recursive split definition.  With it the properties any valid output has, whatever built it, a box query on grid units,
and the hand-made inputs the tests share.  No test here: tests/test_bvh_cpu.py and tests/test_bvh_gpu.py use it."""
import numpy as np

LEAF = 0xFFFFFFFF
NO_NODE = 0xFFFFFFFF
ABSENT_KEY = 0x80000000
I32_MAX, I32_MIN = 2**31 - 1, -2**31
NODE = np.dtype([("min", np.int32, 3), ("left", np.uint32), ("max", np.int32, 3), ("right", np.uint32)])


def face_boxes(position, index):
    """present (F,) bool, bmin and bmax (F, 3) int64: the empty box for an absent face"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    present = (idx < len(pos)).all(axis=1)
    safe = np.where(present[:, None], idx, 0)
    corners = pos[safe] if len(pos) else np.zeros((len(idx), 3, 3), np.int64)
    bmin = np.where(present[:, None], corners.min(axis=1), I32_MAX)
    bmax = np.where(present[:, None], corners.max(axis=1), I32_MIN)
    return present, bmin, bmax


def face_keys(present, bmin, bmax):
    """key (F,) as Python ints"""
    F = len(present)
    m = (bmin + bmax) >> 1                                           # int64, arithmetic shift
    keys = [ABSENT_KEY] * F
    if not present.any():
        return keys
    L = m[present].min(axis=0)
    H = m[present].max(axis=0)
    E = int(max(((int(H[c]) & 0xFFFFFFFF) - (int(L[c]) & 0xFFFFFFFF)) & 0xFFFFFFFF for c in range(3)))
    k = max(0, E.bit_length() - 10)
    for f in range(F):
        if not present[f]:
            continue
        cell = [((((int(m[f][c]) & 0xFFFFFFFF) - (int(L[c]) & 0xFFFFFFFF)) & 0xFFFFFFFF) >> k) for c in range(3)]
        assert all(x < 1024 for x in cell)
        key = 0
        for i in range(10):
            key |= ((cell[0] >> i) & 1) << (3 * i + 2) | ((cell[1] >> i) & 1) << (3 * i + 1) | ((cell[2] >> i) & 1) << (3 * i)
        keys[f] = key
    return keys


def clz64(x):
    return 64 - int(x).bit_length()


def build(position, index):
    """(nodes NODE (2F - 1,), parent uint32 (2F - 1,), order uint32 (F,), (nodes, faces, absent, height), keys)"""
    present, bmin, bmax = face_boxes(position, index)
    F = len(present)
    keys = face_keys(present, bmin, bmax)
    order = sorted(range(F), key=lambda f: (keys[f], f))
    code = [(keys[order[j]] << 32) | j for j in range(F)]
    nodes = np.zeros(2 * F - 1, NODE)
    parent = np.full(2 * F - 1, 0xDEADBEEF, np.uint32)
    height = {}

    def leaf(j):
        n = F - 1 + j
        f = order[j]
        nodes[n] = (tuple(bmin[f]), f, tuple(bmax[f]), LEAF)
        height[n] = 0
        return n

    def visit(a, b, n):
        """the internal node n over [a, b], a < b"""
        P = clz64(code[a] ^ code[b])
        # the LARGEST m in [a, b - 1] with clz64(c_a ^ c_m) > P: the codes ascend, so that prefix length does not grow with m - a bisection
        lo, hi = a, b - 1                                            # (m = a qualifies: clz64(0) = 64 > P)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if clz64(code[a] ^ code[mid]) > P:
                lo = mid
            else:
                hi = mid - 1
        m = lo
        left = leaf(a) if a == m else visit(a, m, m)
        right = leaf(b) if m + 1 == b else visit(m + 1, b, m + 1)
        parent[left] = n
        parent[right] = n
        nodes[n] = (tuple(np.minimum(nodes[left]["min"], nodes[right]["min"])), left, tuple(np.maximum(nodes[left]["max"], nodes[right]["max"])), right)
        height[n] = 1 + max(height[left], height[right])
        return n

    root = leaf(0) if F == 1 else visit(0, F - 1, 0)
    assert root == 0
    parent[0] = NO_NODE
    return nodes, parent, np.array(order, np.uint32), (2 * F - 1, F, int((~present).sum()), height[0]), keys


def check(position, index, nodes, parent=None, order=None, counts=None):
    """the properties of any valid output, with no model of the tree: every face in exactly one leaf, every internal id in 0..F - 2 once,
    parent agreeing with the children, every internal box the union of its children's, leaves' boxes the faces', height <= 64 and the longest
    path, order a permutation sorted by (key, f) that the leaves follow"""
    present, bmin, bmax = face_boxes(position, index)
    F = len(present)
    keys = face_keys(present, bmin, bmax)
    assert len(nodes) == 2 * F - 1
    seen_faces, seen_internal = [], []
    depth = {0: 0}
    stack = [0]
    longest = 0
    while stack:
        n = stack.pop()
        nd = nodes[n]
        longest = max(longest, depth[n])
        if nd["right"] == LEAF:
            assert n >= F - 1, "a leaf's id is F - 1 + j"
            f = int(nd["left"])
            seen_faces.append(f)
            assert tuple(nd["min"]) == tuple(bmin[f]) and tuple(nd["max"]) == tuple(bmax[f])
            if order is not None:
                assert order[n - (F - 1)] == f
            continue
        assert n < F - 1
        seen_internal.append(n)
        l, r = int(nd["left"]), int(nd["right"])
        assert tuple(nd["min"]) == tuple(np.minimum(nodes[l]["min"], nodes[r]["min"]))
        assert tuple(nd["max"]) == tuple(np.maximum(nodes[l]["max"], nodes[r]["max"]))
        for c in (l, r):
            assert c not in depth, "a node is reached once"
            depth[c] = depth[n] + 1
            if parent is not None:
                assert parent[c] == n
            stack.append(c)
    assert sorted(seen_faces) == list(range(F))
    assert sorted(seen_internal) == list(range(F - 1))
    assert longest <= 64
    if parent is not None:
        assert parent[0] == NO_NODE
    if order is not None:
        assert sorted(int(f) for f in order) == list(range(F))
        ranked = [(keys[int(f)], int(f)) for f in order]
        assert ranked == sorted(ranked)
    if counts is not None:
        assert tuple(counts) == (2 * F - 1, F, int((~present).sum()), longest)
    return longest


def box_query(nodes, qmin, qmax, height):
    """the leaves' faces whose box overlaps [qmin, qmax] (grid units, inclusive), and the nodes visited; a stack of height + 1 entries"""
    stack = [0]
    hits, visited = [], 0
    while stack:
        assert len(stack) <= height + 1
        nd = nodes[stack.pop()]
        visited += 1
        # (an empty box has min > max in every component: the test fails on it, whatever the query)
        if not all(nd["min"][c] <= qmax[c] and nd["max"][c] >= qmin[c] for c in range(3)):
            continue
        if nd["right"] == LEAF:
            hits.append(int(nd["left"]))
        else:
            stack.append(int(nd["right"]))
            stack.append(int(nd["left"]))
    return hits, visited


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------

def lattice(n, step=7, seed=0, m=None, extra=0):
    """an n x m (default n x n) grid of quads as 2*n*m triangles over (n + 1)(m + 1) vertices, z a small noise, and `extra` lone triangles
    beside it: (position int32, index uint32)"""
    m = n if m is None else m
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing="ij")
    pos = np.stack([x.ravel() * step - 1000, y.ravel() * step - 500, rng.integers(-9, 10, (n + 1) * (m + 1))], axis=1).astype(np.int32)
    v = lambda i, j: i * (m + 1) + j   # noqa: E731
    idx = []
    for i in range(n):
        for j in range(m):
            idx += [(v(i, j), v(i + 1, j), v(i, j + 1)), (v(i + 1, j), v(i + 1, j + 1), v(i, j + 1))]
    for e in range(extra):
        k = len(pos)
        pos = np.concatenate([pos, np.array([[-1100 - 9 * e, -600, 40], [-1104 - 9 * e, -600, 40], [-1100 - 9 * e, -596, 44]], np.int32)])
        idx.append((k, k + 1, k + 2))
    return pos, np.array(idx, np.uint32)


def strip(nface, seed=0, spread=2000):
    """nface triangles over nface + 2 random vertices, face f = (f, f + 1, f + 2): any face count"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(-spread, spread, (nface + 2, 3)).astype(np.int32)
    f = np.arange(nface, dtype=np.uint32)
    return pos, np.stack([f, f + 1, f + 2], axis=1)


def disc(npoints, seed=0, scale=30000):
    """a Delaunay disc as bench.py's realistic leg makes them (corto_amd.synth.delaunay_disc, no holes), its positions rounded to a grid"""
    from corto_amd import synth
    m = synth.delaunay_disc(npoints, seed, holes=0)
    return np.round(np.asarray(m.position, np.float64) * scale).astype(np.int32), np.asarray(m.index, np.uint32).reshape(-1, 3)
