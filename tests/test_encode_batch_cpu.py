"""crthip_encode_batch on the host side alone: the symbol, the argument checks that come before any device work, and the
Python wrapper's keyword validation (tests/test_encode_batch_gpu.py checks the bytes on the device)."""
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


@pytest.fixture(scope="module")
def L():
    return ca.lib()


def test_encode_batch_is_exported_and_declared(L):
    assert hasattr(L, "crthip_encode_batch")
    hdr = open(os.path.join(ROOT, "include", "corto_hip.h")).read()
    assert "crthip_encode_batch(" in hdr and "crthip_encode_batch_stats;" in hdr
    assert L.crthip_abi_version() == 6


def test_null_context_is_an_argument_error(L):
    offs = np.zeros(2, dtype=np.uint64)
    m = ca.MeshDesc()
    r = L.crthip_encode_batch(None, 1, C.byref(m), 0, None, 0, offs.ctypes.data_as(C.c_void_p), None, None, None, None, None)
    assert r == -8                                          # CRTHIP_E_ARGUMENT
    assert b"context" in L.crthip_last_error()


def test_empty_batch_returns_zero_before_touching_the_device(L):
    offs = np.full(1, 77, dtype=np.uint64)
    stats = ca.EncodeBatchStats()
    stats.value_streams = 5
    dummy = C.create_string_buffer(64)                      # n == 0: the context is never dereferenced
    r = L.crthip_encode_batch(C.cast(dummy, C.c_void_p), 0, None, 0, None, 0, offs.ctypes.data_as(C.c_void_p), None, None, None,
                              C.byref(stats), None)
    assert r == 0 and offs[0] == 0 and stats.value_streams == 0


def test_null_offsets_are_an_argument_error(L):
    dummy = C.create_string_buffer(64)
    assert L.crthip_encode_batch(C.cast(dummy, C.c_void_p), 0, None, 0, None, 0, None, None, None, None, None, None) == -8


def test_encode_batch_checks_the_length_of_a_kw_list():
    meshes = [synth.bumpy_sphere(8, 4, seed=1), synth.bumpy_sphere(8, 4, seed=2)]
    with pytest.raises(ValueError):
        ca.encode_batch(meshes, ctx=None, kw=[{}])
    with pytest.raises(ValueError):
        ca.encode_batch(meshes, ctx=None, kw=[{}, {}, {}])


def test_mesh_desc_factoring_keeps_encode_bytes():
    """encode() builds its crthip_mesh through the helper encode_batch shares: the host encoder's bytes stay the golden ones"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "c4_unit.npz"))
    m = synth.bumpy_sphere(64, 32, seed=0)
    assert ca.encode(m, normal_prediction=ca.BORDER).tobytes() == z["crt"].tobytes()
