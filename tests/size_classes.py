"""The decoder's size classes (which K-DELTA and K-NRM kernel, which LDS layout) and the meshes that sit on either side of each limit:
shared by tests/test_size_classes_cpu.py (every case is on its intended side, by the planner's own predicates) and
tests/test_size_classes_gpu.py (every case against the oracle, on the path it is meant to take).

The predicates come from tests/cpp/size_class_probe.cpp, which includes the library's headers: nothing here restates a formula, so a
changed limit moves the probe's answers and the CPU module names the cases that crossed sides."""
import os
import subprocess

import numpy as np

import corto_amd as ca
from corto_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Probe:
    """tests/cpp/size_class_probe.cpp (or another probe of tests/cpp: `source`), built into `workdir` and kept running: one query a line"""

    def __init__(self, workdir, source="size_class_probe"):
        exe = os.path.join(str(workdir), source)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(ROOT, "corto_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", source + ".cpp"), "-o", exe])
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, *q):
        self.p.stdin.write(" ".join(str(x) for x in q) + "\n")
        self.p.stdin.flush()
        r = self.p.stdout.readline().split()
        assert r and r[0] != "?", q
        return r

    def const(self, name):
        return int(self.ask("const", name)[0])

    def delta_in_lds(self, nvert, N, u8=False, wide=False):
        return self.ask("delta", nvert, N, int(u8), int(wide))[1] == "1"

    def delta_last(self, N, u8=False, wide=False):
        return int(self.ask("delta_last", N, int(u8), int(wide))[0])

    def groups(self, nvert, comps, wide=False):
        """the K-DELTA jobs of one blob's attributes [(N, u8), ...] in order: (tile job indices, [lds16 workgroup job indices, ...])"""
        r = " ".join(self.ask("groups", int(wide), nvert, *["%d:%d" % (n, int(u8)) for n, u8 in comps])).split("|")
        return [int(x) for x in r[0].split()[1:]], [[int(x) for x in g.split()[1:]] for g in r[1:]]

    def fused(self, nvert, nface):
        r = self.ask("fused", nvert, nface)
        return dict(fused=r[0] == "1", nvert_ok=r[1] == "1", nface_ok=r[2] == "1", lds_ok=r[3] == "1", lds=int(r[4]), lds_fn=int(r[5]))

    def fn_layout(self, fn_max, blobs):
        """one k_normal_blob launch of blobs [(nvert, nface), ...]: its LDS request and each blob's face-normal layout"""
        r = self.ask("fn", fn_max, *[x for b in blobs for x in b])
        return int(r[0]), r[1:]

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=30)


# ------------------------------------------------------------------------------------------------------------------------------------
# meshes of an exact vertex count

def closed_mesh(nvert, seed=0, color_components=4):
    """a closed genus-0 mesh of exactly `nvert` vertices (nface = 2*nvert - 4): a closed UV sphere just below the count, then as many
    faces split at their centroid (one vertex and two faces each) as vertices are missing, spread over the sphere"""
    nu = max(8, int(np.sqrt(2 * nvert)))
    rows = (nvert - 2) // nu
    m = synth.closed_sphere(nu, rows + 1, seed=seed, color_components=color_components)
    extra = nvert - m.nvert
    assert 0 <= extra < nu, (nvert, m.nvert)
    if extra == 0:
        return m
    idx = m.index.astype(np.int64)
    pick = (np.arange(extra) * (len(idx) // extra) + seed % 7) % len(idx)
    tri = idx[pick]
    c = m.position[tri].mean(axis=1)
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * 1.003
    new = m.nvert + np.arange(extra)
    keep = np.ones(len(idx), bool)
    keep[pick] = False
    a, b, d = tri[:, 0], tri[:, 1], tri[:, 2]
    faces = np.concatenate([idx[keep], np.stack([a, b, new], 1), np.stack([b, d, new], 1), np.stack([d, a, new], 1)])
    nrm = np.concatenate([m.normal, (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(m.normal.dtype)])
    uv = np.concatenate([m.uv, m.uv[tri].mean(axis=1).astype(m.uv.dtype)])
    col = np.concatenate([m.color, m.color[tri[:, 0]]])
    out = synth.Mesh(np.concatenate([m.position, c.astype(m.position.dtype)]), faces.astype(m.index.dtype), nrm, col, uv)
    assert out.nvert == nvert and out.nface == 2 * nvert - 4
    return out


def open_mesh(nvert, holes, seed=0):
    """closed_mesh(nvert) with `holes` faces removed, spread out (nface = 2*nvert - 4 - holes): a boundary for BORDER normals"""
    m = closed_mesh(nvert, seed=seed)
    drop = np.zeros(m.nface, bool)
    drop[(np.arange(holes) * (m.nface // holes) + 3) % m.nface] = True
    return synth.Mesh(m.position, m.index[~drop], m.normal, m.color, m.uv)


def generic_values(mesh, N, seed=0):
    """N smooth float components a vertex (positions through a few sines): int16-sized deltas at q = 1/1024"""
    p = mesh.position.astype(np.float64)
    k = 1.0 + 0.37 * np.arange(N) + 0.11 * seed
    return np.stack([np.sin(k[c] * p[:, c % 3] + 0.5 * p[:, (c + 1) % 3]) * 0.75 for c in range(N)], 1).astype(np.float32)


Q = 1.0 / 1024


def bare(mesh, attributes, **kw):
    """blob of `mesh` with only positions + the generic `attributes` [(name, N, strategy), ...]"""
    attrs = [(name, generic_values(mesh, N, seed=k), Q, strategy) for k, (name, N, strategy) in enumerate(attributes)]
    return ca.encode(mesh, with_normal=False, with_color=False, with_uv=False, attributes=attrs, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases.  Sizes are the headers' limits (the probe's `delta_last` etc.) on the day these were written; the CPU module checks, for the
# blob each case encodes, that it is still on the side it is named for.

# K-DELTA records: (tag, N, u8, wide, last nvert inside).  Generic attributes a parallelogram and a first-neighbour one of N components,
# or a colour of N bytes
DELTA_LIMITS = [("i16_N1", 1, False, False, 16380), ("i16_N2", 2, False, False, 13104), ("i16_N3", 3, False, False, 10920),
                ("i16_N4", 4, False, False, 9360), ("u8_N3", 3, True, False, 13104), ("u8_N4", 4, True, False, 13104),
                ("wide_N1", 1, False, True, 13104), ("wide_N2", 2, False, True, 9360), ("wide_N3", 3, False, True, 6552),
                ("wide_N4", 4, False, True, 5956)]


def delta_cases():
    """[(id, tag, N, u8, wide, nvert, inside)]: last inside and first outside of every record limit"""
    out = []
    for tag, N, u8, wide, last in DELTA_LIMITS:
        for nvert, inside in ((last, True), (last + 1, False)):
            out.append(("%s_%d" % (tag, nvert), tag, N, u8, wide, nvert, inside))
    return out


def delta_blob(N, u8, nvert, seed=0):
    """the blob of one K-DELTA record case; bind `names` only (positions stay unbound: no job of their own)"""
    if u8:
        m = closed_mesh(nvert, seed=seed, color_components=N)
        return ca.encode(m, with_normal=False, with_uv=False), ["color"]
    m = closed_mesh(nvert, seed=seed)
    return bare(m, [("g_par", N, ca.PARALLEL), ("g_fn", N, 0)]), ["g_par", "g_fn"]


# K-DELTA groups: (id, nvert, [generic N, ...] in blob order, what the planner must make of them (tile jobs, lds16 groups) - job indices)
GROUP_CASES = [
    ("split_2_2_2", 9000, [2, 2, 2], ([], [[0, 1], [2]])),                  # each fits, two fit together, the third does not
    ("host_after", 9000, [2, 2, 3], ([], [[0, 1], [2]])),                   # the N=3 attribute (the graph's `a`) in a group of its own,
    ("host_first", 9000, [3, 2, 2], ([], [[0], [1, 2]])),                   # ... ahead of the ones that would have used its halfwords
    ("host_shared", 9000, [3, 1], ([], [[0, 1]])),                          # fits only because the N=1 one uses the N=3 one's halfwords
    ("tiles_and_lds", 10000, [4, 1, 2], ([0], [[1, 2]])),                   # N=4 beyond its records, the others in LDS: both kernels
    ("slices", 4000, [5, 1, 3, 4], ([0, 1], [[2, 3, 4]])),                  # five components: two slices of k_delta_tiles<true>
]


def group_blob(nvert, comps, seed=0):
    m = closed_mesh(nvert, seed=seed)
    names = ["g%d" % k for k in range(len(comps))]
    return bare(m, [(n, N, ca.PARALLEL if k % 2 == 0 else 0) for k, (n, N) in enumerate(zip(names, comps))]), names


# normals: k_normal_blob against the normal_faces ... normal_vertex chain.  FUSED_LAST: the largest closed mesh normal_fused takes;
# BORDER meshes get HOLES faces removed (a boundary): six faces fewer move their limit to BORDER_LAST
FUSED_LAST, HOLES, BORDER_LAST = 10822, 6, 10825


def normal_cases():
    """[(id, prediction, nvert, fused, normal_format, index16)]: each side of normal_fused, ESTIMATED on closed meshes and BORDER on open
    ones, f32 and int16 normals, u32 and u16 indices"""
    out = []
    for pred, pname in ((ca.ESTIMATED, "est"), (ca.BORDER, "border")):
        last = FUSED_LAST if pred == ca.ESTIMATED else BORDER_LAST
        for nvert, fused in ((last, True), (last + 1, False)):
            for fmt, i16 in ((ca.FMT_FLOAT, False), (ca.FMT_INT16, True)) if pred == ca.ESTIMATED else ((ca.FMT_FLOAT, True), (ca.FMT_INT16, False)):
                out.append(("%s_%d_%s_%s" % (pname, nvert, "f32" if fmt == ca.FMT_FLOAT else "i16", "u16" if i16 else "u32"), pred, nvert, fused, fmt, i16))
    return out


def normal_mesh(pred, nvert, seed=0):
    return closed_mesh(nvert, seed=seed) if pred == ca.ESTIMATED else open_mesh(nvert, HOLES, seed=seed)


def normal_blob(pred, nvert, seed=0):
    return ca.encode(normal_mesh(pred, nvert, seed=seed), normal_prediction=pred, with_color=False, with_uv=False)


# 3*nface <= 65535 (k_normal_blob counts a vertex's incident faces in 16 bits): a closed mesh never reaches it before the LDS limit,
# duplicated faces do (the encoder keeps them on the same vertices) - NFACE_BASE vertices with nface just at / just past the bound
NFACE_BASE, NFACE_MAX = 8000, 65535 // 3


def nface_blob(nface, seed=0):
    m = closed_mesh(NFACE_BASE, seed=seed)
    dups = nface - m.nface
    m = synth.non_manifold(m, seed=seed, fins=0, dups=dups, reversed_dups=0, bowties=0, glue=0)
    assert m.nface == nface, (m.nface, nface)
    return ca.encode(m, normal_prediction=ca.ESTIMATED, with_color=False, with_uv=False)


# face normals of k_normal_blob: (id, single-stream context, [nvert of each closed ESTIMATED blob in the batch], layout of each).
# FN_LAST: the largest closed mesh whose face normals fit NORMAL_FN_LDS_MAX
FN_LAST = 2681
FN_CASES = [
    ("lds_two_stream", False, [FN_LAST], ["lds"]),
    ("scratch_single_stream", True, [FN_LAST], ["scratch"]),
    ("scratch_two_stream_past_100k", False, [FN_LAST + 1], ["scratch"]),
    ("lds_by_partner_single_stream", True, [2000, 9000], ["lds", "scratch"]),
    ("lds_by_partner_two_stream", False, [FN_LAST + 1, 9000], ["lds", "scratch"]),
]

# unfused ESTIMATED blobs in one batch (vbase / fbase), a fused one between them
UNFUSED_BATCH = [FUSED_LAST + 1, FUSED_LAST - 500, 12001, 11003]

# output formats on the large classes: (id, nvert, generic N, normals): nvert*N spans many 1 024-element dequantize blocks and
# nvert*N % 4 is 1, 2 or 3
FORMAT_CASES = [
    ("tiles_N1", 20001, 1, False),      # 20 001 % 4 = 1, beyond N=1's records
    ("tiles_N2", 14001, 2, False),      # 28 002 % 4 = 2
    ("tiles_N3", 11001, 3, False),      # 33 003 % 4 = 3
    ("unfused_normals_N3", 11001, 3, True),
]
FORMATS = [ca.FMT_INT32, ca.FMT_UINT32, ca.FMT_INT16, ca.FMT_UINT16, ca.FMT_INT8, ca.FMT_UINT8, ca.FMT_DOUBLE]


def format_blob(nvert, N, normals, seed=0):
    """a blob with a generic N-component attribute `g` (first neighbour) and positions; with estimated normals (which read the integer
    positions) when `normals`"""
    m = closed_mesh(nvert, seed=seed)
    attrs = [("g", generic_values(m, N, seed=seed), Q, 0)]
    return ca.encode(m, normal_prediction=ca.ESTIMATED, with_normal=normals, with_color=False, with_uv=False, attributes=attrs)
