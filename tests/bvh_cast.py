"""A sequential model of crthip_bvh_cast, written from the contract in include/corto_hip.h alone: a brute force over ALL faces in Python's
arbitrary-precision integers - no tree, nothing of csrc/bvh_cast.h - with the face test, the range rule and the (t, f) minimum; and the
segment generators the tests share.  No test here: tests/test_bvh_cast_cpu.py and tests/test_bvh_cast_gpu.py use it."""
import numpy as np

ANY, FRONT = 1, 2
NO_FACE = 0xFFFFFFFF
MISS, HIT, RANGE, TREE = 0, 1, 2, 3
R = 1 << 19
SEGMENT = np.dtype([("p", np.int32, 3), ("user0", np.uint32), ("q", np.int32, 3), ("user1", np.uint32)])
HITREC = np.dtype([("status", np.uint32), ("face", np.uint32), ("side", np.uint32), ("reserved", np.uint32), ("num", np.uint64), ("den", np.uint64)])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def face_test(P, Q, a, b, c, front=False, widest=None):
    """None, or (K, D) of a hit; widest: a one-element list that keeps the largest magnitude any intermediate reached"""
    d, A, B, C = sub(Q, P), sub(a, P), sub(b, P), sub(c, P)
    n = cross(sub(B, A), sub(C, A))
    D, K = dot(d, n), dot(A, n)
    U, V, W = dot(d, cross(B, C)), dot(d, cross(C, A)), dot(d, cross(A, B))
    assert U + V + W == D
    if widest is not None:
        widest[0] = max([widest[0]] + [abs(x) for x in (D, K, U, V, W)] + [abs(x) for x in n])
    if D == 0:
        return None
    if not ((U >= 0 and V >= 0 and W >= 0) or (U <= 0 and V <= 0 and W <= 0)):
        return None
    if not (K == 0 or (K < 0) == (D < 0)) or abs(K) > abs(D):
        return None
    if front and D >= 0:
        return None
    return K, D


def cast(position_u16, index, segments, base=(0, 0, 0), flags=0, written=True, nvert=None, widest=None):
    """The hit records (HITREC) of `segments` (SEGMENT) against every face: position_u16 (nvert, 3) the buffer's halfwords, so that
    p[v] = base + position_u16[v]"""
    pos = [tuple(int(x) + int(base[c]) for c, x in enumerate(row)) for row in np.asarray(position_u16).reshape(-1, 3)]
    nv = len(pos) if nvert is None else nvert
    faces = [tuple(int(x) for x in f) for f in np.asarray(index).reshape(-1, 3)]
    out = np.zeros(len(segments), HITREC)
    for i, s in enumerate(segments):
        P, Q = tuple(int(x) for x in s["p"]), tuple(int(x) for x in s["q"])
        if not written or not all(-R <= E[c] - int(base[c]) < R for E in (P, Q) for c in range(3)):
            out[i] = (RANGE, NO_FACE, 0, 0, 0, 0)
            continue
        best = None                                                  # (|K|, |D|, f, side)
        for f, (ia, ib, ic) in enumerate(faces):
            if ia >= nv or ib >= nv or ic >= nv:
                continue
            h = face_test(P, Q, pos[ia], pos[ib], pos[ic], bool(flags & FRONT), widest)
            if h is None:
                continue
            K, D = abs(h[0]), abs(h[1])
            if best is None or K * best[1] < best[0] * D:             # strictly nearer; equal t keeps the lower id, met first
                best = (K, D, f, int(h[1] < 0))
        if best is None:
            out[i] = (MISS, NO_FACE, 0, 0, 0, 0)
        elif flags & ANY:
            out[i] = (HIT, NO_FACE, 0, 0, 0, 0)
        else:
            out[i] = (HIT, best[2], best[3], 0, best[0], best[1])
    return out


def cast_fast(position_u16, index, segments, base=(0, 0, 0), flags=0, written=True, nvert=None):
    """cast()'s records for big inputs: still every face and no tree, but the face test runs in numpy int64 over all faces of a segment at
    once - exact, because in range every quantity stays below 2^63 (the contract's bounds) - and only the (t, f) minimum over the faces
    that are hit runs on Python integers.  tests/test_bvh_cast_cpu.py holds it equal to cast()"""
    base = np.asarray([int(b) for b in base], np.int64)
    pos = np.asarray(position_u16).reshape(-1, 3).astype(np.int64) + base
    nv = len(pos) if nvert is None else nvert
    idx = np.asarray(index).reshape(-1, 3).astype(np.int64)
    present = (idx < nv).all(axis=1)
    safe = np.where(present[:, None], idx, 0)
    a, b, c = (pos[safe[:, k]] if len(pos) else np.zeros((len(idx), 3), np.int64) for k in range(3))
    crs = lambda u, v: np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)   # noqa: E731
    n = crs(b - a, c - a)
    out = np.zeros(len(segments), HITREC)
    for i, s in enumerate(segments):
        P, Q = s["p"].astype(np.int64), s["q"].astype(np.int64)
        if not written or not ((P - base >= -R) & (P - base < R) & (Q - base >= -R) & (Q - base < R)).all():
            out[i] = (RANGE, NO_FACE, 0, 0, 0, 0)
            continue
        d, A, B, C = Q - P, a - P, b - P, c - P
        D, K = n @ d, (A * n).sum(axis=1)
        U, V, W = crs(B, C) @ d, crs(C, A) @ d, crs(A, B) @ d
        hit = present & (D != 0) & (((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0)))
        hit &= ((K == 0) | ((K < 0) == (D < 0))) & (np.abs(K) <= np.abs(D))
        if flags & FRONT:
            hit &= D < 0
        best = None
        for f in np.flatnonzero(hit):
            k, dd = abs(int(K[f])), abs(int(D[f]))
            if best is None or k * best[1] < best[0] * dd:
                best = (k, dd, int(f), int(D[f] < 0))
        if best is None:
            out[i] = (MISS, NO_FACE, 0, 0, 0, 0)
        elif flags & ANY:
            out[i] = (HIT, NO_FACE, 0, 0, 0, 0)
        else:
            out[i] = (HIT, best[2], best[3], 0, best[0], best[1])
    return out


def segments(p, q):
    p = np.asarray(p, np.int64).reshape(-1, 3)
    q = np.asarray(q, np.int64).reshape(-1, 3)
    s = np.zeros(len(p), SEGMENT)
    s["p"], s["q"] = p, q
    s["user0"] = np.arange(len(p), dtype=np.uint32) * 2654435761 & 0xFFFFFFFF   # (never read: any bits)
    s["user1"] = ~s["user0"]
    return s


def quantize(position):
    """integer positions (nvert, 3) -> (base (3,), uint16 (nvert, 3)) as CRTHIP_BIND_QUANTIZED stores them: base the minimum a component"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    base = pos.min(axis=0) if len(pos) else np.zeros(3, np.int64)
    rel = pos - base
    assert rel.max(initial=0) <= 65535
    return base, rel.astype(np.uint16)


# ---- segment generators (all in absolute grid units) -----------------------------------------------------------------------------------------

def vertex_shots(position, ids, reach=50, both=True):
    """through vertex v along z, from above (and from below): the vertex is the segment's midpoint"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    p, q = [], []
    for v in ids:
        x, y, z = (int(t) for t in pos[v])
        p.append((x, y, z + reach)); q.append((x, y, z - reach))
        if both:
            p.append((x, y, z - reach)); q.append((x, y, z + reach))
    return segments(p, q)


def edge_midpoint_shots(position, index, faces, reach=60, both=True):
    """through the midpoint of every edge of the named faces: from `reach` above one end of the edge to `reach` below the other, so that
    P + Q = a + b and the segment crosses the edge exactly at its midpoint (t = 1/2), whether or not that is an integer point"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    p, q = [], []
    for f in faces:
        c = [int(x) for x in np.asarray(index).reshape(-1, 3)[f]]
        for k in range(3):
            a, b = pos[c[k]], pos[c[(k + 1) % 3]]
            P = (int(a[0]), int(a[1]), int(a[2]) + reach)
            Q = (int(b[0]), int(b[1]), int(b[2]) - reach)
            p.append(P); q.append(Q)
            if both:
                p.append(Q); q.append(P)
    return segments(p, q)


def random_segments(position, n, seed=0, margin=40, base=None):
    """n segments between random points of the positions' box grown by `margin`, clipped to the range of `base` (default: the minimum)"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0) - margin, pos.max(axis=0) + margin
    b = pos.min(axis=0) if base is None else np.asarray(base, np.int64)
    lo, hi = np.maximum(lo, b - R), np.minimum(hi, b + R - 1)
    return segments(rng.integers(lo, hi + 1, (n, 3)), rng.integers(lo, hi + 1, (n, 3)))


def camera_grid(position, w, h, margin=5):
    """w*h parallel segments along -z over the positions' xy box, from above the box to below it: coherent"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    xs = np.linspace(lo[0], hi[0], w).round().astype(np.int64)
    ys = np.linspace(lo[1], hi[1], h).round().astype(np.int64)
    x, y = np.meshgrid(xs, ys, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.full(w * h, hi[2] + margin)], axis=1)
    q = np.stack([x.ravel(), y.ravel(), np.full(w * h, lo[2] - margin)], axis=1)
    return segments(p, q)
