"""CPU: computed normals (crthip_batch_bind_computed_normals) - the value's model (tests/computed_normals.py) against the oracle's decode
of a BORDER-encoded twin, bit for bit; the twin decodes to the same positions and index as the blob without normals; the call is exported,
declared, and refuses a NULL batch.  No kernel runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corto_amd as ca
import computed_normals as cn
from conftest import ROOT
from oracle import oracle as oc


@pytest.mark.parametrize("fmt", [ca.FMT_FLOAT, ca.FMT_INT16], ids=["f32", "i16"])
@pytest.mark.parametrize("name", cn.LOOPED)
def test_model_is_what_upstream_leaves_off_the_boundary(name, fmt):
    """at every non-boundary vertex with a non-zero estimate the model equals the oracle's decode of the BORDER twin, raw bytes"""
    e = cn.expected(name)
    got, zero = e.model(fmt)
    ref = oc.decode(e.twin, normal_format=fmt)["normal"]
    where = ~e.bnd & ~zero
    assert where.sum() > 0 and (zero & ~e.bnd == e.degenerate).all(), name
    assert got.dtype == ref.dtype
    assert got[where].tobytes() == ref[where].tobytes(), (name, int((got[where] != ref[where]).any(axis=1).sum()))
    if name in cn.CLOSED:
        assert where.all(), (name, int(e.bnd.sum()), int(zero.sum()))     # no boundary vertex, no degenerate vertex: the oracle alone is the reference
    else:
        assert e.bnd.sum() == {"holey_disc_20": 228, "bumpy_sphere_16_8": 32}[name] and e.nvert == {"holey_disc_20": 439, "bumpy_sphere_16_8": 144}[name]


@pytest.mark.parametrize("name,bits", [(n, 14) for n in cn.LOOPED + ["torus_105_105", "torus_182_182"]] + [("torus_24_12", 4)])
def test_twin_decodes_to_the_same_positions_and_index(name, bits):
    bare, twin = cn.twins(name, bits)
    a, b = oc.decode(bare), oc.decode(twin)
    assert "normal" not in a and "normal" in b
    cn.assert_same(a, b, ["position", "index"], (name, bits))


@pytest.mark.parametrize("case", cn.DEGENERATE, ids=[c[0] for c in cn.DEGENERATE])
def test_degenerate_vertices_get_the_up_vector(case):
    """coarse positions make estimates cancel: upstream's FLOAT path leaves 0/0 there (that is how Expected finds them), the model (0,0,1)"""
    name, bits, nzero, nvert = case
    e = cn.expected(name, bits)
    assert e.nvert == nvert and not e.bnd.any()
    for fmt, up in ((ca.FMT_FLOAT, (0, 0, 1)), (ca.FMT_INT16, (0, 0, 32767))):
        got, zero = e.model(fmt)
        assert zero.sum() == nzero and (zero == e.degenerate).all(), (name, int(zero.sum()))
        assert (got[zero] == np.array(up, dtype=got.dtype)).all()
        assert not np.isnan(got.astype(np.float64)).any()
        exp = e.normal(fmt)
        assert got.tobytes() == exp.tobytes(), name


def test_the_call_is_exported_and_declared():
    L = ca.lib()
    assert hasattr(L, "crthip_batch_bind_computed_normals")
    hdr = open(os.path.join(ROOT, "include", "corto_hip.h")).read()
    assert re.search(r"\bint\s+crthip_batch_bind_computed_normals\s*\(\s*crthip_batch\s*\*b,\s*uint32_t i,\s*void\s*\*buffer,\s*uint32_t format,\s*uint32_t stride\)", hdr)
    assert L.crthip_abi_version() == 6 and re.search(r"#define\s+CRTHIP_ABI_VERSION\s+6\b", hdr)      # additive: the number stays


def test_a_null_batch_is_an_argument_error():
    L = ca.lib()
    buf = np.zeros(16, dtype=np.float32)
    assert L.crthip_batch_bind_computed_normals(None, 0, buf.ctypes.data_as(C.c_void_p), ca.FMT_FLOAT, 0) == -8      # CRTHIP_E_ARGUMENT
    assert L.crthip_batch_bind_computed_normals(None, 0, None, ca.FMT_FLOAT, 0) == -8
