"""The decoder's VALUE-range limits (what the kernels decide from the values of a blob, not from its size) and the blobs that sit on either
side of each: shared by tests/test_value_ranges_cpu.py (every case is on the side it is named for, by the oracle's integers and the host model
of K-DELTA) and tests/test_value_ranges_gpu.py (every case against the oracle, the counter it is named for on the named side).

* K-DELTA's int16 records (k_delta.hip): every raw delta d[i], i >= 1, and every result v[i] - v[0] mod 2^32 must lie in [-32768, 32767], else the
  blob's attribute is redone on 32-bit values (crthip_batch_stats.delta_redone, counted a BLOB).  delta_edge_cases()
* K-BIT's int16 hand-on (plan_jobs.cpp: widths_fit): a CORRELATED attribute whose widest field is <= 16 bits, a per-component one whose widest
  is <= 15 (crthip_batch_stats.int16_streams, counted a stream).  handon_cases()
* normal_bits 1 .. 16, colour quantisation other than the default, position_bits beyond 20 and below 4.  normal_cases(), colour_cases(),
  position_cases()

How an edge is crafted: an int32 generic attribute at q = 1 goes through the encoder and the decoder's integer stages unchanged, and the
decoded vertex order depends on the faces alone - a probe attribute id = arange(nvert) reads it off the oracle (topology()).  A case states the
values it wants in DECODED order, relative to vertex 0; blob() scatters them to the input order and adds the base."""
import functools

import numpy as np

import corto_amd as ca
import size_classes as sc
from corto_amd import synth
from cstream_model import model_array, model_values
from oracle import oracle as oc

BASE = 1000000                       # vertex 0 of every crafted attribute: absolute values are never int16
WRAP_BASE = (1 << 31) - 100          # ... or just below INT32_MAX: relative values from +100 on wrap to just above INT32_MIN
LO, HI = -32768, 32767

MESHES = {"window": lambda: synth.bumpy_sphere(24, 12, seed=1),                    # 312 vertices, the window loop finishes
          "rounds": lambda: synth.bumpy_sphere_flipped(48, 24, seed=2),            # 1 200, handed to the round loop (parallelogram attributes)
          "small": lambda: synth.bumpy_sphere_flipped(17, 9, seed=3)}              # 170


def s32(x):
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


@functools.lru_cache(maxsize=None)
def topology(key):
    """(mesh, order, P): order[j] = the input vertex that decodes as vertex j, P the oracle's prediction triples (a, b, c) in decoded order"""
    m = MESHES[key]()
    ids = np.arange(m.nvert, dtype=np.int32).reshape(-1, 1)
    o = oc.decode(ca.encode(m, with_normal=False, with_color=False, with_uv=False, attributes=[("id", ids, 1.0, 0)]), trace=True)
    order = o["_delta_id"][:, 0].astype(np.int64)
    assert sorted(order.tolist()) == list(range(m.nvert))
    P = o["_prediction"].astype(np.int64)
    assert (P[1:, 0] < np.arange(1, m.nvert)).all()           # one component: every vertex but the first is predicted
    return m, order, P


def predicted(rel, P, para):
    """the prediction of every decoded vertex from `rel` (nvert, N), as the encoder forms it (encoder.cpp: first neighbour, or a + b - c)"""
    i = np.arange(len(P))
    a, b, c = P[:, 0], P[:, 1], P[:, 2]
    pred = np.zeros_like(rel)
    has = a < i
    pred[has] = rel[a[has]]
    if para:
        use = has & (b < i) & (c < i) & (a != b)
        pred[use] += rel[b[use]] - rel[c[use]]
    return pred


def host_rule(raw, values):
    """the documented rule on the oracle's integers (_raw_* and _delta_* of one attribute): any raw delta d[i], i >= 1, or any
    (v[i] - v[0]) mod 2^32 outside [-32768, 32767] -> (redone, a raw delta is outside, a result is outside)"""
    raw, values = np.asarray(raw, dtype=np.int64), np.asarray(values, dtype=np.int64)
    rel = s32(values - values[0])
    bad_raw = bool(((raw[1:] < LO) | (raw[1:] > HI)).any())
    bad_res = bool(((rel < LO) | (rel > HI)).any())
    return int(bad_raw or bad_res), bad_raw, bad_res


def filler(n, N, seed=0):
    """small smooth values for the components (and attributes) that carry no edge"""
    j = np.arange(n)[:, None]
    r = (j * 3 + (np.arange(N)[None, :] + seed) * 7) % 11 - 5
    r[0] = 0
    return r.astype(np.int64)


class Case:
    """one blob: attrs = [(name, strategy, rel (nvert, N) in decoded order)], what it is named for"""

    def __init__(self, cid, mesh, attrs, redone=0, loop=None, why=None, base=BASE, streams=None, widths=None, positions=None):
        self.id, self.mesh, self.attrs, self.redone, self.loop, self.why, self.base = cid, mesh, attrs, redone, loop, why, base
        self.streams, self.widths, self.positions = streams, widths, positions
        self._blob = None

    @property
    def names(self):
        return [a[0] for a in self.attrs] + (["position"] if self.positions is not None else [])

    def blob(self):
        if self._blob is None:
            self._blob = _blob(self)
        return self._blob


def _blob(case):
    m, order, _ = topology(case.mesh)
    attrs = []
    for name, strategy, rel in case.attrs:
        v = np.zeros(rel.shape, dtype=np.int64)
        v[order] = s32(case.base + rel)
        # INT32 input divides in float (vertex_attribute.h:79-104): exact below 2^24; the wrap base goes in as DOUBLE, exact everywhere
        attrs.append((name, v.astype(np.float64) if case.base == WRAP_BASE else v.astype(np.int32), 1.0, strategy))
    kw = {}
    if case.positions is not None:                            # integer positions at q = 1 (CORRELATED | PARALLEL, the encoder's choice)
        pos = np.zeros(case.positions.shape, dtype=np.float32)
        pos[order] = (case.base + case.positions).astype(np.float32)
        m = synth.Mesh(pos, m.index, m.normal, m.color, m.uv)
        kw = dict(position_bits=0, position_q=1.0)
    return ca.encode(m, with_normal=False, with_color=False, with_uv=False, attributes=attrs, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. K-DELTA's int16 check

def ramp(n, sign, step=1024):
    """0 at vertex 0, up (down) 1 024 a decoded vertex to a plateau 7 short of the edge: the raw deltas stay small, the sums grow.  (step = 32 757:
    the plateau from vertex 1 on, for an edge at vertex 1 - the vertices predicted from it then lie next to it)"""
    j = np.arange(n)
    return sign * (np.minimum(j * step, 32757) + j % 4)


def _where(n, P, where, parent_not_0=False):
    e = {"v1": 1, "mid": n // 2, "last": n - 1}[where]
    while parent_not_0 and P[e, 0] == 0:
        e += 1
    return e


def _edge_rel(key, N, comp, para, kind, where, outside):
    """relative values (nvert, N) of one edge attribute, the edge in component `comp`: last inside (outside = 0) or first outside (1)"""
    m, order, P = topology(key)
    n = m.nvert
    rel = filler(n, N)
    x = np.zeros(n, dtype=np.int64)
    if kind == "pos_result":                                  # (a) a result at +32767 | +32768
        x = ramp(n, 1, 32757 if where == "v1" else 1024)
        x[_where(n, P, where)] = HI + outside
    elif kind == "neg_result":                                # (b) a result at -32768 | -32769
        x = ramp(n, -1, 32757 if where == "v1" else 1024)
        x[_where(n, P, where)] = LO - outside
    elif kind == "neg_spike":                                 # (c) a lone spike: the vertex predicted from it has a raw delta of +32767 | +32768
        e = _where(n, P, where)
        x[e] = (LO - outside) if where == "last" else (LO + 1 - outside)      # (nothing is predicted from the last vertex: there the result decides)
    elif kind == "pos_delta":                                 # (c) a low parent and a raw delta of +32767 | +32768 on top of its prediction
        e = _where(n, P, where, parent_not_0=True)
        x[P[e, 0]] = -26000
        rel[:, comp] = x
        x[e] = predicted(rel, P, para)[e, comp] + HI + outside
    rel[:, comp] = x
    return rel


KINDS = ["pos_result", "neg_result", "neg_spike", "pos_delta"]
WHERES = ["v1", "mid", "last"]


def delta_edge_pairs():
    """[(inside Case, outside Case)]: N = 1 .. 4, parallelogram and first neighbour, the edge in the first and in the last component - each with
    the four kinds of edge; the place of the edge (decoded vertex 1, a middle vertex, the last) and the mesh (the window loop finishes / the round
    loop does) rotate so that every (kind, place, mesh) occurs.  The named side (`redone`), its reason (`why`) and the loop are what
    tests/test_value_ranges_cpu.py checks against the oracle's integers and the host model.  First-neighbour attributes stay in the window on every
    connected family of corto_amd.synth (the round loop takes them only under $CORTO_DELTA_ROUNDS=1, which the GPU module sets for every pair)."""
    out, idx = [], 0
    for N in (1, 2, 3, 4):
        for comp in sorted({0, N - 1}):
            for strategy in (ca.PARALLEL, 0):
                for kind in KINDS:
                    where, key = WHERES[idx % 3], ("window", "rounds")[(idx // 12) % 2]
                    idx += 1
                    para = bool(strategy & ca.PARALLEL)
                    loop = "rounds" if key == "rounds" and para else "window"
                    tag = "N%d_c%d_%s_%s_%s_%s" % (N, comp, "par" if para else "fn", kind, where, key)
                    # an edge at vertex 1 is its own raw delta; a lone spike and a raw delta leave every result inside
                    why = "raw" if kind in ("neg_spike", "pos_delta") and not (kind == "neg_spike" and where == "last") else "result"
                    pair = []
                    for outside in (0, 1):
                        rel = _edge_rel(key, N, comp, para, kind, where, outside)
                        pair.append(Case(tag + ("_out" if outside else "_in"), key, (("g", strategy, rel),), redone=outside, loop=loop,
                                         why=why if outside else None))
                    out.append(tuple(pair))
    # (c) as the issue words it: a predicted value near -30 000 under a value near +10 000 - far outside, the results inside.  Its partner: +2 000
    for key, strategy in (("window", ca.PARALLEL), ("rounds", 0)):
        m, order, P = topology(key)
        pair = []
        for outside in (0, 1):
            rel = filler(m.nvert, 2)
            e = _where(m.nvert, P, "mid", parent_not_0=True)
            rel[:, 1] = 0
            rel[P[e, 0], 1] = -30000
            rel[e, 1] = 10000 if outside else 2000
            pair.append(Case("far_delta_%s_%s" % (key, "out" if outside else "in"), key, (("g", strategy, rel),), redone=outside,
                             loop="window" if not strategy or key == "window" else "rounds", why="raw" if outside else None))
        out.append(tuple(pair))
    # (f) absolute values that wrap mod 2^32 while the relative ones fit: vertex 0 at INT32_MAX - 99, the ramp goes up through the wrap.  (A base just
    # above INT32_MIN does not come back from the reference's own coder - profiles/EXPERIMENTS.md - so the wrap is pinned from this end only)
    for key, strategy, sign in (("window", ca.PARALLEL, 1), ("rounds", ca.PARALLEL, 1), ("window", 0, 1)):
        m, order, P = topology(key)
        pair = []
        for outside in (0, 1):
            rel = filler(m.nvert, 2, seed=3)
            x = ramp(m.nvert, sign)
            x[m.nvert // 2] = HI + outside
            rel[:, 0] = x
            pair.append(Case("wrap_%s_%s_%s" % ("par" if strategy else "fn", key, "out" if outside else "in"), key, (("g", strategy, rel),), redone=outside,
                             loop="rounds" if key == "rounds" and strategy else "window", why="result" if outside else None, base=WRAP_BASE))
        out.append(tuple(pair))
    # several attributes in one blob, only one of them past the edge (the others come out right, none redone for it)
    for tag, key, spec in (("group_a", "window", [(2, ca.PARALLEL, None), (3, 0, "pos_result"), (1, ca.PARALLEL, None)]),
                           ("group_b", "rounds", [(4, ca.PARALLEL, "neg_result"), (2, 0, None), (3, ca.PARALLEL, None), (1, 0, None)])):
        m, order, P = topology(key)
        pair = []
        for outside in (0, 1):
            attrs = []
            for k, (N, strategy, kind) in enumerate(spec):
                if kind is None:
                    rel = filler(m.nvert, N, seed=k) + ramp(m.nvert, 1 if k % 2 else -1)[:, None] // (k + 2)
                else:
                    rel = _edge_rel(key, N, N - 1, bool(strategy & 1), kind, "last" if k else "mid", outside)
                attrs.append(("g%d" % k, strategy, rel))
            pair.append(Case("%s_%s" % (tag, "out" if outside else "in"), key, tuple(attrs), redone=outside,
                             loop="rounds" if key == "rounds" else "window", why="result" if outside else None))
        out.append(tuple(pair))
    return out


@functools.lru_cache(maxsize=None)
def delta_edge_cases():
    return delta_edge_pairs()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. K-BIT's int16 hand-on

def _raw_edge(key, N, strategy, comp, lo_delta, hi_delta, results_fit=True):
    """values whose raw deltas reach exactly lo_delta (at the last decoded vertex) and hi_delta (at a middle one: a parent at -10 000 when the delta
    itself is beyond +32767, so that every result stays inside), small elsewhere"""
    m, order, P = topology(key)
    n = m.nvert
    para = bool(strategy & ca.PARALLEL)
    rel = filler(n, N)
    x = np.zeros(n, dtype=np.int64)
    e = _where(n, P, "mid", parent_not_0=True)
    if hi_delta is not None:
        x[P[e, 0]] = -10000
        rel[:, comp] = x
        x[e] = predicted(rel, P, para)[e, comp] + hi_delta
    if lo_delta is not None:
        rel[:, comp] = x
        x[n - 1] = predicted(rel, P, para)[n - 1, comp] + lo_delta
    rel[:, comp] = x
    return rel


def _plateau(key, N):
    """small raw deltas, results far outside int16 (a ramp to +-40 000 in every component): handed on as halfwords AND redone"""
    n = topology(key)[0].nvert
    j = np.arange(n)
    return filler(n, N) + np.stack([(1 if c % 2 == 0 else -1) * np.minimum(j * 500, 40000) for c in range(N)], 1)


@functools.lru_cache(maxsize=None)
def handon_cases():
    """[Case]: `widths` = the widest field of every stream in blob order {name: [w, ...]} (one stream for a CORRELATED attribute, N otherwise),
    `streams` = crthip_batch_stats.int16_streams, `redone` = delta_redone.  A CORRELATED stream of width 17 holds a raw delta outside int16 by
    definition, so its blob is redone as well: that pair differs in both counters, the per-component pairs at -32768 differ in int16_streams alone."""
    C, PAR = ca.CORRELATED, ca.PARALLEL
    out = []
    mk = functools.partial(Case, base=0)                      # (vertex 0 at 0: its own field, the absolute value, must not be the widest)
    for key in ("window", "small"):
        for strategy in (C, C | PAR):
            t = "corr%s_%s" % ("_par" if strategy & PAR else "", key)
            out.append(mk(t + "_w16", key, (("g", strategy, _raw_edge(key, 3, strategy, 0, LO, HI)),), streams=1, redone=0, widths={"g": [16]}))
            out.append(mk(t + "_w17_pos", key, (("g", strategy, _raw_edge(key, 3, strategy, 2, LO, HI + 1)),), streams=0, redone=1, widths={"g": [17]}))
            out.append(mk(t + "_w17_neg", key, (("g", strategy, -_raw_edge(key, 3, strategy, 1, None, HI + 2)),), streams=0, redone=1, widths={"g": [17]}))
    # the positions themselves (CORRELATED | PARALLEL at position_bits = 0, q = 1), bound; no other attribute
    out.append(mk("position_w16", "window", (), streams=1, redone=0, widths={"position": [16]}, positions=_raw_edge("window", 3, C | PAR, 1, LO, HI)))
    out.append(mk("position_w17", "window", (), streams=0, redone=1, widths={"position": [17]}, positions=_raw_edge("window", 3, C | PAR, 1, LO, HI + 1)))
    # one width a component: |v| <= 32767 is 15 bits, -32768 is 16 (and fits int16: not handed on, not redone), +32768 is 16 and redone
    for N in (1, 2, 3, 4):
        strategy = PAR if N % 2 else 0
        comp = N - 1
        w = lambda edge: {"g": [edge if c == comp else 4 for c in range(N)]}
        t = "comp_N%d" % N
        out.append(mk(t + "_w15", "window", (("g", strategy, _raw_edge("window", N, strategy, comp, LO + 1, HI)),), streams=N, redone=0, widths=w(15)))
        out.append(mk(t + "_w16_neg", "window", (("g", strategy, _raw_edge("window", N, strategy, comp, LO, HI)),), streams=0, redone=0, widths=w(16)))
        out.append(mk(t + "_w16_pos", "window", (("g", strategy, _raw_edge("window", N, strategy, comp, LO + 1, HI + 1)),), streams=0, redone=1, widths=w(16)))
    # handed on and redone: halfwords widened in place (k_delta.hip), nvert*N no multiple of 64
    for key in ("window", "small"):
        for N in (1, 2, 3, 4):
            strategy = (PAR, 0)[N % 2]
            out.append(mk("widen_N%d_%s" % (N, key), key, (("g", strategy, _plateau(key, N)),), streams=N, redone=1, widths={"g": [10] * N}))
        out.append(mk("widen_corr_%s" % key, key, (("g", C | PAR, _plateau(key, 3)),), streams=1, redone=1, widths={"g": [10]}))
    # neighbours in one blob: one handed on, the other not
    out.append(mk("mixed_comp", "window", (("h", PAR, _raw_edge("window", 2, PAR, 0, LO + 1, HI)), ("w", PAR, _raw_edge("window", 2, PAR, 1, LO, HI))),
                    streams=2, redone=0, widths={"h": [15, 4], "w": [4, 16]}))
    out.append(mk("mixed_corr", "window", (("h", C, _raw_edge("window", 3, C, 0, LO, HI)), ("w", C, _raw_edge("window", 3, C, 2, LO, HI + 1))),
                    streams=1, redone=1, widths={"h": [16], "w": [17]}))
    return out


def stream_widths(blob, names):
    """{name: [widest field of each stream]} by the reference's value coders on the oracle's raw deltas"""
    o = oc.decode(blob, trace=True)
    strategy = {a["name"]: a["strategy"] for a in oc.parse_header(blob)["attrs"]}
    out = {}
    for nm in names:
        raw = o["_raw_" + nm]
        logs = model_array(raw)[1] if strategy[nm] & ca.CORRELATED else model_values(raw)[1]
        out[nm] = [int(lg.max()) for lg in logs]
    return out


def expected_streams(widths, strategies):
    """plan_jobs.cpp's rule: a CORRELATED attribute is handed on when its stream's widest field is <= 16, another when all of its are <= 15"""
    n = 0
    for nm, w in widths.items():
        if strategies[nm] & ca.CORRELATED:
            n += int(w[0] <= 16)
        else:
            n += len(w) if max(w) <= 15 else 0
    return n


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. normals

NORMAL_BITS = (1, 2, 3, 8, 15, 16)
NOISE = (0.0, 0.6, 3.0)
PREDS = ((ca.DIFF, "diff"), (ca.ESTIMATED, "est"), (ca.BORDER, "border"))
AXES = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, -1], [0, -1, 0], [0, 0, 1]], dtype=np.float32)


def noisy(mesh, amp, seed=0, axes=True):
    """`mesh` with Gaussian noise of amplitude `amp` added to its normals before they are normalised again, and six vertices whose normals are the
    axes (at 16 bits their octahedral coordinate is +32768: what the int16 output narrows)"""
    rng = np.random.default_rng(1000 + seed)
    nrm = mesh.normal.astype(np.float64) + amp * rng.standard_normal(mesh.normal.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(np.float32)
    if axes:
        at = (np.arange(6) * (mesh.nvert // 7) + 3) % mesh.nvert
        nrm[at] = AXES
    return synth.Mesh(mesh.position, mesh.index, nrm, mesh.color, mesh.uv)


NORMAL_MESHES = {"closed": lambda: synth.closed_sphere(20, 12, seed=5), "open": lambda: synth.holey_disc(14, seed=3),
                 "cloud": lambda: synth.point_cloud(19, 11, seed=6)}


@functools.lru_cache(maxsize=None)
def normal_specs():
    """[(id, mesh, encode keywords, prediction, normal_bits, fused)]: every bit count x prediction x mesh (clouds: DIFF and BORDER) at one noise amplitude each
    (all three at 15 and 16 bits, where large corrections are what matters); for 15 and 16 bits also meshes past size_classes.FUSED_LAST (the
    unfused chain).  Each is decoded to f32 and to int16 normals"""
    out, k = [], 0
    for bits in NORMAL_BITS:
        for pred, pname in PREDS:
            for mname, make in NORMAL_MESHES.items():
                if mname == "cloud" and pred == ca.ESTIMATED:
                    continue
                amps = NOISE if bits >= 15 else (NOISE[k % 3],)
                k += 1
                for amp in amps:
                    kw = dict(normal_bits=bits, normal_prediction=pred, with_color=False, with_uv=False)
                    out.append(("%s_%s_b%d_n%g" % (mname, pname, bits, amp), noisy(make(), amp, seed=bits), kw, pred, bits, True))
    for bits, pred, pname in ((15, ca.ESTIMATED, "est"), (16, ca.ESTIMATED, "est"), (16, ca.BORDER, "border")):
        nvert = (sc.FUSED_LAST if pred == ca.ESTIMATED else sc.BORDER_LAST) + 1
        kw = dict(normal_bits=bits, normal_prediction=pred, with_color=False, with_uv=False)
        out.append(("unfused_%s_b%d" % (pname, bits), noisy(sc.normal_mesh(pred, nvert), 0.6, seed=bits), kw, pred, bits, False))
    return out


@functools.lru_cache(maxsize=None)
def normal_cases():
    """[(id, blob, prediction, normal_bits, fused)] of normal_specs()"""
    return [(cid, ca.encode(m, **kw), pred, bits, fused) for cid, m, kw, pred, bits, fused in normal_specs()]


def correction_width(blob):
    """widest field of a normal attribute's correction stream (encodeArray: one width a vertex), over the corrections the blob holds"""
    o = oc.decode(blob, trace=True)
    d = o["_raw_normal"][:o["_trace"]["normal_ndiffs"]]
    return int(model_array(d)[1][0].max()) if len(d) else 0      # (a cloud with BORDER normals holds none)


@functools.lru_cache(maxsize=None)
def correction_pair(pred):
    """ESTIMATED / BORDER at normal_bits = 16 without noise on the open mesh (a disc: every normal in the upper half, where the octahedral map has no
    fold and small angles are small corrections), one vertex's normal turned away from its estimate until the correction stream's widest field is
    exactly 16, and one step on, 17: (blob16, blob17)"""
    base = NORMAL_MESHES["open"]()
    m0 = noisy(base, 0.0, axes=False)
    # a boundary vertex (on an edge that one face only has): corrected under both predictions
    e = np.sort(np.concatenate([base.index[:, [0, 1]], base.index[:, [1, 2]], base.index[:, [2, 0]]]).astype(np.int64), axis=1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    v = int(u[cnt == 1][len(u[cnt == 1]) // 2][0])
    n0 = m0.normal[v].astype(np.float64)
    t = np.cross(n0, [0.3, -0.5, 0.8]); t /= np.linalg.norm(t)

    def blob(angle):
        nrm = m0.normal.copy()
        nrm[v] = (np.cos(angle) * n0 + np.sin(angle) * t).astype(np.float32)
        return ca.encode(synth.Mesh(m0.position, m0.index, nrm, m0.color, m0.uv), normal_bits=16, normal_prediction=pred, with_color=False, with_uv=False)
    assert correction_width(blob(0.0)) <= 16
    lo, hi = 0.0, None
    for a in np.linspace(0.05, 3.0, 60):                      # the first angle past 16 bits, then bisect to the step where the width changes
        if correction_width(blob(a)) > 16:
            hi = a
            break
        lo = a
    assert hi is not None
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if correction_width(blob(mid)) > 16:
            hi = mid
        else:
            lo = mid
    return blob(lo), blob(hi)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. colours

COLOR_BITS = [(b, b, b, b) for b in range(1, 9)] + [(8, 1, 8, 1), (1, 8, 1, 8), (3, 5, 2, 7), (6, 7, 6, 5)]
TILES_NVERT = 13105                  # one past size_classes.DELTA_LIMITS' u8 records: k_delta_tiles


def random_colours(mesh, components, seed):
    rng = np.random.default_rng(2000 + seed)
    col = rng.integers(0, 256, (mesh.nvert, components), dtype=np.uint8)
    col[5] = (0, 255, 0, 255)[:components]                    # r and b below g at every quantisation: cr + y and cb + y wrap (a one-bit green rarely does)
    col[9] = (255, 0, 255, 0)[:components]
    return synth.Mesh(mesh.position, mesh.index, mesh.normal, col, mesh.uv)


@functools.lru_cache(maxsize=None)
def colour_specs():
    """[(id, mesh, encode keywords, stored components, path)], every one decoded to 4 components: uniformly random bytes, every color_bits tuple with 3 and 4 stored
    components on the LDS records and on a cloud, alternating on the 13 105-vertex mesh.
    The encoder gives colours strategy 0 (encoder.cpp, as upstream: GenericAttr<uchar>::deltaEncode): first neighbour only, K-DELTA's packed
    two-register records (LdsVal<6>).  It never writes a parallelogram colour, so the four-component records with parallelogram prediction are left
    to the hand-made blobs of tests/test_gpu_parity.py."""
    out = []
    for k, cb in enumerate(COLOR_BITS):
        tag = "".join(str(b) for b in cb)
        for cc in (3, 4):
            m = random_colours(synth.bumpy_sphere(21, 13, seed=k), cc, k)
            out.append(("lds_%s_c%d" % (tag, cc), m, dict(color_bits=cb, with_normal=False, with_uv=False), cc, "delta_lds16"))
            m = random_colours(synth.point_cloud(17, 9, seed=k), cc, 50 + k)
            out.append(("cloud_%s_c%d" % (tag, cc), m, dict(color_bits=cb, with_normal=False, with_uv=False), cc, "cloud"))
        cc = 3 + k % 2
        m = random_colours(sc.closed_mesh(TILES_NVERT, color_components=cc), cc, 100 + k)
        out.append(("tiles_%s_c%d" % (tag, cc), m, dict(color_bits=cb, with_normal=False, with_uv=False), cc, "delta_tiles"))
    return out


@functools.lru_cache(maxsize=None)
def colour_cases():
    """[(id, blob, stored components, path)] of colour_specs()"""
    return [(cid, ca.encode(m, **kw), cc, path) for cid, m, kw, cc, path in colour_specs()]


def colour_wraps(blob, cc):
    """vertices where a channel's u8 sum wraps on the way out (point.h:214: r = cr + y, b = cb + y mod 256)"""
    c = oc.decode(blob, trace=True, color_components=4)["_delta_color"].astype(np.int64)
    return int(((c[:, 2] + c[:, 0] > 255) | (c[:, 1] + c[:, 0] > 255)).sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. position bits

POSITION_MESHES = {"sphere": lambda: synth.closed_sphere(22, 13, seed=7), "delaunay": lambda: synth.delaunay_disc(420, seed=5, holes=4),
                   "cone": lambda: synth.cone_fan(90, 4, seed=9)}


@functools.lru_cache(maxsize=None)
def position_specs():
    """[(id, mesh, encode keywords, prediction)]: 22, 24 and 28 bits with ESTIMATED and BORDER normals (float cross products of integers that no longer fit a float's
    mantissa, summed in face order), 1, 2 and 3 bits with DIFF normals (most faces collapse: out of contract for estimated normals)"""
    out = []
    for mname, make in POSITION_MESHES.items():
        for bits in (22, 24, 28):
            for pred, pname in PREDS[1:]:
                out.append(("%s_b%d_%s" % (mname, bits, pname), make(), dict(position_bits=bits, normal_prediction=pred), pred))
        for bits in (1, 2, 3):
            out.append(("%s_b%d_diff" % (mname, bits), make(), dict(position_bits=bits, normal_prediction=ca.DIFF), ca.DIFF))
    return out


@functools.lru_cache(maxsize=None)
def position_cases():
    """[(id, blob, prediction)] of position_specs()"""
    return [(cid, ca.encode(m, **kw), pred) for cid, m, kw, pred in position_specs()]


def encoder_corners():
    """[(id, mesh, encode keywords)]: the normal, colour and position cases, for the encoders' entry points"""
    return [s[:3] for s in normal_specs()] + [s[:3] for s in colour_specs()] + [s[:3] for s in position_specs()]
