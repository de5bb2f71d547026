"""Quantised vertex outputs (CRTHIP_BIND_QUANTIZED): the cases and the expected values, shared by tests/test_quantized_outputs_cpu.py (the
kernels' source on the host, corto_amd.quant_out_model) and tests/test_quantized_outputs_gpu.py (the kernels).

Ground truth is the oracle's trace: `_delta_<name>` are an attribute's delta-decoded integers d, so
    out = (d - d.min(0)) as uint16,  base = d.min(0),  span = d.max(0) - d.min(0) (in 64 bits),  q from the header,
and ((base + out) as int32 as float32) * float32(q) must be the oracle's FLOAT array byte for byte.  Tolerance 0 everywhere.
QOUT_BLOB_MAX comes from tests/cpp/quant_out_probe.cpp, which includes the library's header: nothing here holds a copy."""
import functools

import numpy as np

import corto_amd as ca
import size_classes as sc
from corto_amd import synth
from oracle import oracle as oc

FILL = 0xA5
E_FORMAT, E_ARGUMENT, E_LIMIT = -7, -8, -11
SPAN_MAX = 65535

CONSTANTS = ("QOUT_BLOB_MAX", "QOUT_BLOCK", "QOUT_THREADS", "QOUT_SPAN_MAX", "RECORD_BYTES", "JOB_BYTES")


@functools.lru_cache(maxsize=None)
def _constants():
    """the probe built, asked and closed: once a session"""
    import tempfile
    with tempfile.TemporaryDirectory(prefix="quant_out_probe") as d:
        p = sc.Probe(d, source="quant_out_probe")
        try:
            return {n: p.const(n) for n in CONSTANTS}
        finally:
            p.close()


def constant(name):
    """a constant of csrc/kernels.h / quant_out.h by name"""
    return _constants()[name]


def blob_max():
    return constant("QOUT_BLOB_MAX")


class Expected:
    """what a quantised binding of attribute `name` of `blob` must leave, from the oracle's trace `tr` (shared: never modified)"""

    def __init__(self, blob, tr, name):
        a = [x for x in oc.parse_header(blob)["attrs"] if x["name"] == name][0]
        d = tr["_delta_" + name].astype(np.int64)
        self.name, self.N, self.q, self.nvert = name, a["N"], np.float32(a["q"]), d.shape[0]
        self.d = d
        self.base = d.min(0) if len(d) else np.zeros(self.N, np.int64)
        self.span = d.max(0) - self.base if len(d) else np.zeros(self.N, np.int64)
        self.written = int((self.span <= SPAN_MAX).all())
        self.out = (d - self.base).astype(np.uint16)
        self.float = tr[name]
        if self.written:                                      # the record's contract, on the expectation itself
            back = ((self.base + self.out).astype(np.int32).astype(np.float32) * self.q).astype(np.float32)
            assert back.tobytes() == np.ascontiguousarray(self.float, np.float32).tobytes(), name

    def check_record(self, t, tag=""):
        N = self.N
        assert t.components == N and t.written == self.written and np.float32(t.q).tobytes() == self.q.tobytes() and t.reserved == 0, (tag, t.as_dict())
        assert list(t.base[:N]) == [int(x) for x in self.base] and list(t.span[:N]) == [int(x) for x in self.span], (tag, t.as_dict(), self.base, self.span)
        assert list(t.base[N:]) == [0] * (4 - N) and list(t.span[N:]) == [0] * (4 - N), (tag, t.as_dict())

    def record_bytes(self):
        """the 48 bytes of the record"""
        t = ca.QuantTransform()
        for c in range(self.N):
            t.base[c], t.span[c] = int(self.base[c]), int(self.span[c])
        t.q, t.components, t.written = float(self.q), self.N, self.written
        return bytes(t)


@functools.lru_cache(maxsize=None)
def traced(key):
    """(blob, oracle trace) of a case by name"""
    blob = ca.aligned_blob(BLOBS[key]())
    return blob, oc.decode(blob, trace=True)


def expected(key, name):
    blob, tr = traced(key)
    return Expected(blob, tr, name)


# ------------------------------------------------------------------------------------------------------------------------------------
# the model's inputs: integers of every vertex count and N = 1..4, through the encoder and the oracle

MODEL_NVERT = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def grid_values(nvert, N, seed=0):
    """(nvert, N) int32: smooth, signed, a negative minimum, spans well inside 16 bits; component 1 of N >= 3 is constant (span 0)"""
    j = np.arange(nvert, dtype=np.float64)
    v = np.stack([np.rint(9000.0 * np.sin(0.013 * (c + 1) * j + seed + c)) - 1000 * c for c in range(N)], 1)
    if N >= 3:
        v[:, 1] = -77
    return v.astype(np.int32)


def exact_cloud(nvert, seed=0):
    """a point cloud of exactly nvert vertices with the attributes g1..g4 (N = 1..4 int32 components)"""
    j = np.arange(nvert, dtype=np.float64)
    pos = np.stack([np.cos(0.01 * j + seed), np.sin(0.017 * j), 0.001 * j], 1).astype(np.float32)
    m = synth.Mesh(pos)
    attrs = [("g%d" % N, grid_values(nvert, N, seed), 1.0, ca.PARALLEL if N % 2 else 0) for N in (1, 2, 3, 4)]
    return m, attrs


def cloud_blob(nvert, seed=0):
    m, attrs = exact_cloud(nvert, seed)
    return ca.encode(m, with_normal=False, with_color=False, with_uv=False, attributes=attrs)


# ------------------------------------------------------------------------------------------------------------------------------------
# the span edge: integer coordinates at q = 1 (position_bits = 0), a torus rescaled to a box of exactly `top`

def edge_mesh(top, shift):
    m = synth.torus(24, 12)
    p = np.asarray(m.position, dtype=np.float64)
    q = np.rint((p - p.min(0)) / (p.max(0) - p.min(0)) * top) + shift
    grid = np.stack([q[:, 0], q[:, 1]], 1).astype(np.int32)
    return synth.Mesh(q.astype(np.float32), m.index, m.normal, m.color, m.uv), grid


def edge_blob(top, shift):
    m, grid = edge_mesh(top, shift)
    return ca.encode(m, position_bits=0, position_q=1.0, with_normal=False, with_color=False, with_uv=False,
                     attributes=[("grid", grid, 1.0, ca.PARALLEL)])


EDGES = {"edge_65535": (65535, 0, 65535, 0), "edge_65536": (65536, 0, 65536, 0), "edge_neg": (65535, -40000, 65535, -40000)}   # key: (top, shift, span, minimum)


def assert_edge(key):
    """the case sits where it is meant to, by the oracle's trace - before anything is compared"""
    top, shift, span, mn = EDGES[key]
    tr = traced(key)[1]
    for nm in ("position", "grid"):
        d = tr["_delta_" + nm].astype(np.int64)
        assert (d.max(0) - d.min(0) == span).all() and (d.min(0) == mn).all(), (key, nm, d.min(0), d.max(0))


def enc(mesh, **kw):
    return ca.encode(mesh, **kw)


def golden(name):
    from conftest import load_golden
    return np.ascontiguousarray(load_golden(name)["crt"], dtype=np.uint8)


BLOBS = {
    "edge_65535": lambda: edge_blob(65535, 0), "edge_65536": lambda: edge_blob(65536, 0), "edge_neg": lambda: edge_blob(65535, -40000),
    "fields32": lambda: golden("fields32"),
    "c4_unit": lambda: golden("c4_unit"),
    "icosphere2": lambda: enc(synth.icosphere(2)),
    "holey_disc20": lambda: enc(synth.holey_disc(20)),
    "torus_182": lambda: enc(synth.torus(182, 182)),
    "torus_105": lambda: enc(synth.torus(105, 105)),
    "cloud_40_20": lambda: enc(synth.point_cloud(40, 20)),
    "bare_sphere": lambda: enc(synth.closed_sphere(20, 12, seed=5), with_normal=False),
    "single_vertex": lambda: cloud_blob(1, seed=3),
}


def generic_names(blob):
    return [a["name"] for a in oc.parse_header(blob)["attrs"] if a["codec"] not in (2, 3)]
