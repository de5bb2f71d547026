"""crthip_encode_batch_to_device without a device: the symbols and the argument checks that come before any device work,
crthip_encode_batch_bound against the host encoder's sizes, and the device splice itself - the plan and the mover of
csrc/enc_splice.h - run on the host in the kernel's partition (crthip_encode_splice_model, crthip_splice_copy_model,
crthip_encode_splice_plan_model) and held against crthip_encode_attrs byte for byte.  tests/test_encode_device_out_gpu.py checks
the same bytes on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import corto_amd as ca  # noqa: E402
from corto_amd import synth  # noqa: E402
from conftest import GOLDEN, load_golden  # noqa: E402
from test_encode_batch_gpu import _corpus  # noqa: E402   (a list of seeded meshes: building it needs no device)

E_ARGUMENT = -8
TILE = 4096                                                         # ESP_TILE of csrc/enc_splice.h


@pytest.fixture(scope="module")
def L():
    return ca.lib()


def _cases():
    sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def _attrs(m, seed):
    rng = np.random.default_rng(seed)
    return [("weight", rng.standard_normal((m.nvert, 3)).astype(np.float32), 0.01, ca.CORRELATED),
            ("label", rng.integers(-300, 300, (m.nvert, 1)).astype(np.int16), 1.0, 0)]


def _items():
    """every golden case and every item of the batch corpus, each under entropy NONE and TUNSTALL, each with and without generic attributes"""
    items = []
    for i, (m, k) in enumerate([(m, k) for _, m, k in _cases()] + _corpus()):
        for e in (0, 1):
            items.append((m, dict(k, entropy=e)))
            items.append((m, dict(k, entropy=e, attributes=_attrs(m, i))))
    return items


def _host_encode(m, k):
    if m.nvert == 0:                                                # the host reads position[0] of an empty cloud: give it zeros to read
        backing = np.zeros((4, 3), dtype=np.float32)
        e = synth.Mesh(position=backing[:0])
        e.position = backing[:0]
        for a in ("normal", "color", "uv", "radius"):
            setattr(e, a, getattr(m, a))
        return e, ca.encode(e, **k)
    return m, ca.encode(m, **k)


def _first(m, n, index=None):
    """the first n vertices of m with every attribute it has, as a cloud or with the index given"""
    backing = np.zeros((4, 3), dtype=np.float32)                    # (an empty position array still has an address: the host encoder forms &position[0])
    c = synth.Mesh(position=backing[:0], index=index)
    c.position = np.ascontiguousarray(m.position[:n]) if n else backing[:0]
    for a in ("normal", "color", "uv", "radius"):
        if getattr(m, a) is not None:
            setattr(c, a, np.ascontiguousarray(getattr(m, a)[:n]))
    return c


def _tiny_items():
    """The shapes at which a coded block's header, its payload and the payload's address can disagree, TUNSTALL (1) and NONE (0) side by
    side: a 1-vertex cloud (every stream one symbol: under TUNSTALL header-only blocks, csize 0, no payload address; under NONE 1 byte
    of payload), a 0-vertex cloud (zero-length streams, zero words), a single triangle, a small mesh whose colour is constant (its logs
    are all zero: a one-symbol Tunstall block next to multi-symbol ones), and a small mesh with one generic attribute of 16 PARALLEL
    components (sixteen blocks in one stream)."""
    base = synth.bumpy_sphere(8, 4, seed=7)
    items = []
    for e in (1, 0):
        items.append((_first(base, 1), dict(entropy=e)))
        items.append((_first(base, 0), dict(entropy=e)))
        items.append((_first(base, 3, index=np.array([[0, 1, 2]], dtype=np.uint32)), dict(entropy=e)))
    flat = synth.bumpy_sphere(8, 4, seed=8)
    flat.color[:] = flat.color[0]
    wide = synth.bumpy_sphere(6, 4, seed=9)
    w16 = np.random.default_rng(9).integers(-2000, 2000, (wide.nvert, 16)).astype(np.int16)
    for e in (1, 0):
        items.append((flat, dict(entropy=e)))
        items.append((wide, dict(entropy=e, attributes=[("w16", w16, 1.0, ca.PARALLEL)])))
    return items


def test_symbols_and_header(L):
    hdr = open(os.path.join(ROOT, "include", "corto_hip.h")).read()
    for name in ("crthip_encode_batch_to_device", "crthip_encode_batch_bound", "crthip_ctx_encode_splice_stats"):
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "#define CRTHIP_ENCODE_INPUTS_RESIDENT 1u" in hdr and "crthip_splice_stats;" in hdr
    assert "#define CRTHIP_ABI_VERSION 6" in hdr and L.crthip_abi_version() == 6


def _call(L, ctx, n, meshes, flags, offs, lens, stats=None):
    return L.crthip_encode_batch_to_device(ctx, n, meshes, None, 0, flags, None, 0, offs, lens, None, None, None, stats, None)


def test_argument_checks_without_a_device(L):
    m = ca.MeshDesc()
    offs = np.full(1, 77, dtype=np.uint64)
    lens = np.full(1, 77, dtype=np.uint32)
    po, pl = ca._np_ptr(offs), ca._np_ptr(lens)
    assert _call(L, None, 1, C.byref(m), 0, po, pl) == E_ARGUMENT
    assert b"context" in L.crthip_last_error()
    # n == 0 writes nothing and returns 0: not the arrays, and the statistics are cleared
    stats = ca.EncodeBatchStats()
    stats.value_streams = 5
    assert _call(L, None, 0, None, 0, po, pl, C.byref(stats)) == 0
    assert offs[0] == 77 and lens[0] == 77 and stats.value_streams == 0
    assert _call(L, None, 0, None, 0, None, None) == 0
    # null blob_offset / blob_len (the context is not dereferenced before the arguments have been looked at)
    dummy = C.create_string_buffer(4096)
    ctx = C.cast(dummy, C.c_void_p)
    assert _call(L, ctx, 1, C.byref(m), 0, None, pl) == E_ARGUMENT
    assert _call(L, ctx, 1, C.byref(m), 0, po, None) == E_ARGUMENT
    # an unknown flag bit, with and without the known one
    for flags in (2, 3, 0x80000000):
        assert _call(L, None, 0, None, flags, po, pl) == E_ARGUMENT
        assert _call(L, ctx, 1, C.byref(m), flags, po, pl) == E_ARGUMENT
        assert b"flag" in L.crthip_last_error()
    s = ca.SpliceStats()
    assert L.crthip_ctx_encode_splice_stats(None, C.byref(s)) == E_ARGUMENT


def test_bound_covers_the_host_encoders_sizes():
    items = _items()
    sizes, bounds = [], []
    for m, k in items:
        _, blob = _host_encode(m, k)
        b = ca.encode_batch_bound([m], kw=k)
        _, total = ca.arena_layout([len(blob)])
        assert b >= total > 0, (k, b, total)
        assert b % 16 == 0
        sizes.append(len(blob)); bounds.append(b)
    # additive over items
    _, total = ca.arena_layout(sizes)
    whole = ca.encode_batch_bound([m for m, _ in items], kw=[k for _, k in items])
    assert whole == sum(bounds) and whole >= total
    # loose by design (the Tunstall tables' 512 bytes a block, the CLERS and split caps), but not absurd: within a few times the real size
    print("bound / size over %d items: %.2f" % (len(items), whole / total))


def test_bound_is_zero_for_a_refused_mesh():
    good = synth.bumpy_sphere(12, 6, seed=1)
    ok = ca.encode_batch_bound([good])
    assert ok > 0
    assert ca.encode_batch_bound([good], kw=dict(entropy=7)) == 0                       # an entropy no encoder has
    assert ca.encode_batch_bound([good], kw=dict(attributes=[("position", good.position, 0.1, 0)])) == 0   # a name the mesh already has
    huge = synth.Mesh(position=good.position)
    huge.position = _FakeRows(good.position, (1 << 26) // 3 + 1)                        # beyond the value coder's bound; never read
    assert ca.encode_batch_bound([huge], kw=dict(with_normal=False, with_color=False, with_uv=False)) == 0
    assert ca.encode_batch_bound([good, good], kw=[dict(entropy=7), {}]) == ok          # the neighbour still counts
    assert ca.encode_batch_bound([]) == 0


class _FakeRows:
    """an array that claims more rows than it has: a descriptor whose arrays the bound must not read"""

    def __init__(self, a, rows):
        self.a, self.shape, self.ctypes = a, (rows,) + a.shape[1:], a.ctypes


def test_splice_model_equals_the_host_encoder():
    items = _items()
    assert any(m.nvert == 0 for m, _ in items) and any(m.nface == 0 for m, _ in items) and any("attributes" in k for _, k in items)
    for i, (m, k) in enumerate(items):
        m, expect = _host_encode(m, k)
        for mis in ((0, 1 + i % 15) if i % 8 else (0, 1, 4, 15)):
            blob, pad = ca.encode_splice_model(m, dst_misalign=mis, **k)
            assert blob.tobytes() == expect.tobytes(), (i, mis)
            assert len(pad) == (-len(blob)) % 16 and not pad.any(), (i, mis)


def test_splice_model_equals_the_host_encoder_on_tiny_shapes():
    items = _tiny_items()
    assert sorted({m.nvert for m, _ in items})[:3] == [0, 1, 3] and {k["entropy"] for _, k in items} == {0, 1}
    for i, (m, k) in enumerate(items):
        expect = ca.encode(m, **k)
        for mis in (0, 1, 15):
            blob, pad = ca.encode_splice_model(m, dst_misalign=mis, **k)
            assert blob.tobytes() == expect.tobytes(), (i, mis)
            assert len(pad) == (-len(blob)) % 16 and not pad.any(), (i, mis)


def test_splice_model_equals_the_golden_bytes():
    for name, m, k in _cases():
        blob, _ = ca.encode_splice_model(m, dst_misalign=3, **k)
        assert blob.tobytes() == load_golden(name)["crt"].tobytes(), name


def test_mover_alone_every_alignment_and_length():
    rng = np.random.default_rng(3)
    src0 = rng.integers(0, 256, 3 * TILE + 256, dtype=np.uint8)
    lengths = list(range(0, 81)) + [TILE - 17, TILE - 1, TILE, TILE + 1, TILE + 15, TILE + 16, TILE + 33, 2 * TILE + 7]
    for sa in range(16):
        for da in range(16):
            for n in (lengths if (sa, da) in ((0, 0), (3, 9), (13, 2)) or sa == da else lengths[:81]):
                src_at = 16 + sa
                dst = np.full(n + 64, 0xA5, dtype=np.uint8)
                base = (-dst.ctypes.data) % 16
                dst_at = base + 16 + da
                src_base = (-src0.ctypes.data) % 16
                ca.splice_copy_model(src0, src_base + src_at, dst, dst_at, n, seed=sa * 16 + da)
                assert dst[dst_at:dst_at + n].tobytes() == src0[src_base + src_at:src_base + src_at + n].tobytes(), (sa, da, n)
                assert (dst[:dst_at] == 0xA5).all() and (dst[dst_at + n:] == 0xA5).all(), (sa, da, n)


def test_plan_tiles_the_arena_exactly_once():
    items = _items()
    hosted = [_host_encode(m, k) for m, k in items]
    offs, lens, st, pieces = ca.encode_splice_plan_model([m for m, _ in hosted], kw=[k for _, k in items])
    assert lens.tolist() == [len(b) for _, b in hosted]
    want_offs, total = ca.arena_layout(lens)
    assert offs.tolist() == want_offs.tolist() and st["arena_bytes"] == total
    assert (offs % 16 == 0).all()
    # no gap, no overlap: every piece starts where the one before it ended, the first at 0, the last ends at the total
    at = 0
    for dst, nbytes, literal in pieces.tolist():
        assert dst == at and nbytes > 0 and literal in (0, 1)
        at += nbytes
    assert at == total
    assert st["literal_bytes"] + st["device_bytes"] == total
    assert st["literal_bytes"] == int(pieces[pieces[:, 2] == 1, 1].sum()) and st["device_bytes"] == int(pieces[pieces[:, 2] == 0, 1].sum())
    assert st["pieces"] == len(pieces) and st["jobs"] >= st["pieces"]
    # in chunks, as a batch beyond one device image is planned: every chunk a plan of its own that continues the arena where the last
    # one ended - the same offsets, lengths and bytes' origins, pieces that still tile [0, total) once (a piece never spans two chunks)
    for chunk in (1, 7, 100):
        offs_c, lens_c, st_c, pieces_c = ca.encode_splice_plan_model([m for m, _ in hosted], kw=[k for _, k in items], chunk_items=chunk)
        assert offs_c.tolist() == offs.tolist() and lens_c.tolist() == lens.tolist(), chunk
        assert st_c["launches"] == -(-len(items) // chunk) and st_c["arena_bytes"] == total
        assert st_c["literal_bytes"] == st["literal_bytes"] and st_c["device_bytes"] == st["device_bytes"], chunk
        at = 0
        for dst, nbytes, literal in pieces_c.tolist():
            assert dst == at and nbytes > 0, chunk
            at += nbytes
        assert at == total
        starts = set(pieces_c[:, 0].tolist())
        assert all(int(offs[i]) in starts for i in range(0, len(items), chunk) if lens[i]), chunk        # a chunk's first piece begins at its first blob
    # a refused item takes no room and moves no neighbour
    offs2, lens2, _, _ = ca.encode_splice_plan_model([hosted[0][0], hosted[1][0], hosted[2][0]], kw=[items[0][1], dict(items[1][1], entropy=7), items[2][1]])
    assert lens2.tolist() == [lens[0], 0, lens[2]] and offs2.tolist() == ca.arena_layout(lens2)[0].tolist()
