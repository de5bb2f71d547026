"""The encoder's device topology pass, on the CPU: the source the kernels run (csrc/enc_topology.h, compiled for the host) against the host
encoder's own pass, array by array and count by count (crthip_encode_topology_model), and the additions to the public interface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corto_amd as ca
import topology_corpus as tc

E_ARGUMENT = -8
ARRAYS = ("faces", "group_end", "quads", "clers", "split_words")
COUNTS = ("nvert", "nface", "max_front", "split_bits")


def _same(name, m, kw):
    host = ca.encode_topology_model(m, 0, **kw)
    dev = ca.encode_topology_model(m, 1, **kw)
    for k in ARRAYS:
        assert host[k].shape == dev[k].shape and host[k].tobytes() == dev[k].tobytes(), (name, k)
    for k in COUNTS:
        assert host[k] == dev[k], (name, k, host[k], dev[k])
    assert dev["lds"] == int(ca.encode_topology_fits_lds(m)), name
    info = ca.probe(ca.encode(m, **kw))                             # the hook reports the pass the encoder really runs
    assert (host["nvert"], host["nface"]) == (info.nvert, info.nface), name
    return host, dev


def _run(items):
    n = 0
    for name, m, kw in items:
        if tc.is_mesh(m):
            _same(name, m, kw)
            n += 1
    return n


def test_golden_cases():
    assert _run(tc.golden_cases()) >= 23


def test_mixed_corpus():
    items = tc.mixed_corpus()
    assert {"non_manifold", "all_degenerate", "unreferenced", "short_groups"} <= {n for n, _, _ in items}
    assert _run(items) > 80


def test_pairing_rules():
    items = tc.pairing_cases()
    assert sum(n.startswith("soup") for n, _, _ in items) >= 200
    name, seam, kw = items[0]
    # the second group's smallest vertex is the fan's apex, on 40 faces: a bucket of more than 16 sides that the host leaves unsorted
    second = seam.index[seam.groups[0]:]
    assert second.min() > 0 and (second == second.min()).any(axis=1).sum() == 40
    for n, m, _ in items[1:4]:
        assert np.bincount(m.index.ravel()).max() >= 17, n           # the book's edge
    assert _run(items) == len(items)


def test_two_groups_fixture_takes_the_unsorted_bucket():
    m = [c for c in tc.golden_cases() if c[0] == "two_groups"][0][1]
    assert m.index[m.groups[0]:].min() == 192


def test_links_of_32_bits():
    name, m, kw = tc.wide_mesh()
    assert 3 * m.nface > 65535 and (m.nface, m.nvert) == (65536, 33024)
    host, dev = _same(name, m, kw)
    assert dev["lds"] == 0


def test_lds_rule_is_sizes_alone():
    c4 = [c for c in tc.golden_cases() if c[0] == "c4_unit"][0][1]
    assert ca.encode_topology_fits_lds(c4)
    assert not ca.encode_topology_fits_lds(tc.wide_mesh()[1])
    cloud = [c for c in tc.golden_cases() if c[0] == "cloud_diff"][0][1]
    assert not ca.encode_topology_fits_lds(cloud)
    assert ca.encode_topology_fits_lds(tc.random_soup(1))            # connectivity does not enter
    L = ca.lib()
    for nvert, nface, fits in ((2145, 4096, 1), (65535, 100, 0), (100, 21846, 0), (9000, 4096, 1), (11000, 4096, 0)):
        d = ca.MeshDesc()
        d.nvert, d.nface, d.index = nvert, nface, 1                  # (sizes alone: the index is never read)
        assert L.crthip_encode_topology_fits_lds(C.byref(d)) == fits, (nvert, nface)


def test_unknown_which_is_an_argument_error():
    m = tc.book(17)
    for which in (2, -1):
        with pytest.raises(ca.CortoError) as e:
            ca.encode_topology_model(m, which, with_normal=False, with_color=False, with_uv=False)
        assert e.value.code == E_ARGUMENT


def test_interface_additions():
    L = ca.lib()
    for sym in ("crthip_ctx_set_encode_topology", "crthip_encode_topology_fits_lds", "crthip_encode_topology_model"):
        assert hasattr(L, sym), sym
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "corto_hip.h")).read()
    assert re.search(r"int\s+crthip_ctx_set_encode_topology\s*\(\s*crthip_ctx\s*\*\s*ctx\s*,\s*int\s+where\s*\)", hdr)
    for k, v in (("HOST", 0), ("DEVICE", 1), ("SPLIT", 2)):
        assert re.search(r"#define\s+CRTHIP_TOPOLOGY_%s\s+%d\b" % (k, v), hdr)
    assert L.crthip_ctx_set_encode_topology(None, 0) == E_ARGUMENT  # no context: refused before anything is touched
    assert L.crthip_abi_version() == 6


def test_stats_struct_grows_at_its_end():
    old = [("wall_ms", C.c_float), ("host_topology_ms", C.c_float), ("host_frame_ms", C.c_float), ("clouds_device_sorted", C.c_uint32),
           ("clouds_host_sorted", C.c_uint32), ("value_streams", C.c_uint32), ("bytes_to_device", C.c_uint64), ("bytes_from_device", C.c_uint64),
           ("host_check_ms", C.c_float), ("host_stage_ms", C.c_float), ("sync_wait_ms", C.c_float), ("value_coder_ms", C.c_float),
           ("upload_ms", C.c_float), ("alloc_ms", C.c_float), ("topology_wait_ms", C.c_float)]

    class Old(C.Structure):
        _fields_ = old
    new = ca.EncodeBatchStats
    assert C.sizeof(new) >= C.sizeof(Old)
    for name, _ in old:
        assert getattr(new, name).offset == getattr(Old, name).offset, name
    last = max(getattr(Old, n).offset + getattr(Old, n).size for n, _ in old)
    for name in ("topology_device", "topology_lds", "device_topology_ms"):
        assert getattr(new, name).offset >= last, name
