"""CPU: the kernels' source of CRTHIP_BIND_QUANTIZED on the host (corto_amd.quant_out_model: csrc/quant_out.h in k_quant_out.hip's
partitions) on the oracle's delta-decoded integers, against the expectation of tests/quantized_outputs.py.  Tolerance 0; every destination
is pre-filled with 0xA5 and every byte outside the vertices' halfwords must still be 0xA5."""
import numpy as np
import pytest

import corto_amd as ca
import quantized_outputs as qo
from oracle import oracle as oc

FILL = qo.FILL
PATHS = [(0, 0), (1, 1), (1, 2), (1, 3)]                   # (which, seed): one workgroup; the blocks of the two-kernel path in three orders


def run_model(e, stride, offset, which, seed):
    """the model on e's integers into a poisoned destination: every byte against the expectation"""
    N, nv = e.N, e.nvert
    st = stride or 2 * N
    nbytes = offset + (nv - 1) * st + 2 * N + 6            # (a poisoned tail behind the last vertex)
    raw = np.full(nbytes + 16, FILL, np.uint8)
    at = (-raw.ctypes.data) % 16                            # `offset` counts from a 16-byte boundary
    dst = raw[at:at + nbytes]
    _, t = ca.quant_out_model(e.d.astype(np.int32), stride=stride, which=which, seed=seed, q=float(e.q), out=dst, offset=offset)
    e.check_record(t, (e.name, nv, stride, offset, which, seed))
    want = np.full(nbytes, FILL, np.uint8)
    if e.written:
        rows = np.lib.stride_tricks.as_strided(want[offset:], shape=(nv, 2 * N), strides=(st, 1))
        rows[:] = e.out.view(np.uint8).reshape(nv, 2 * N)
    assert dst.tobytes() == want.tobytes(), (e.name, nv, stride, offset, which, seed)
    assert (raw[:at] == FILL).all() and (raw[at + nbytes:] == FILL).all()


def model_sizes():
    m = qo.blob_max()
    return qo.MODEL_NVERT + [m - 1, m, m + 1]


@pytest.fixture(scope="module")
def clouds():
    """nvert -> {N: Expected} from ONE encode and ONE oracle decode a size"""
    out = {}
    for nv in model_sizes():
        blob = ca.aligned_blob(qo.cloud_blob(nv, seed=nv % 7))
        tr = oc.decode(blob, trace=True)
        out[nv] = {N: qo.Expected(blob, tr, "g%d" % N) for N in (1, 2, 3, 4)}
    return out


def test_size_classes_come_from_the_header():
    assert qo.constant("RECORD_BYTES") == 48 == len(bytes(ca.QuantTransform()))
    assert qo.constant("QOUT_BLOCK") == 1024 and qo.constant("QOUT_THREADS") == 256 and qo.constant("QOUT_SPAN_MAX") == qo.SPAN_MAX
    assert qo.blob_max() >= 1025


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_model_matches_the_oracle(clouds, N):
    for nv in model_sizes():
        e = clouds[nv][N]
        assert e.nvert == nv and e.written == 1 and (nv < 256 or (e.base < 0).any())    # (negative bases: from a few hundred vertices on)
        if N >= 3 and nv > 1:
            assert e.span[1] == 0 and e.span[0] > 0                 # a component whose span is 0
        for stride in (0, 2 * N + 2, 16):
            for offset in (0, 2):
                for which, seed in PATHS:
                    run_model(e, stride, offset, which, seed)


def test_packed_stride_is_the_packed_layout(clouds):
    e = clouds[257][3]
    a, ta = ca.quant_out_model(e.d.astype(np.int32), stride=6)
    b, tb = ca.quant_out_model(e.d.astype(np.int32), stride=0)
    assert a.tobytes() == b.tobytes() == e.out.tobytes() and bytes(ta) == bytes(tb)


@pytest.mark.parametrize("key", sorted(qo.EDGES))
def test_span_edge(key):
    qo.assert_edge(key)                                     # the spans and minima the case is about, from the trace, before anything is compared
    for name in ("position", "grid"):
        e = qo.expected(key, name)
        assert e.written == int(qo.EDGES[key][2] <= qo.SPAN_MAX)
        for stride in (0, 2 * e.N + 2):
            for which, seed in PATHS:
                run_model(e, stride, 2, which, seed)


def test_32_bit_fields_do_not_wrap():
    """fixture fields32: values over the whole int32 range - the span is computed in 64 bits, nothing is stored, nothing wraps"""
    blob, tr = qo.traced("fields32")
    names = qo.generic_names(blob)
    wide = [nm for nm in names if (qo.Expected(blob, tr, nm).span > 0x7FFFFFFF).any()]
    assert wide, names
    for nm in names:
        e = qo.Expected(blob, tr, nm)
        if e.N > 4:
            continue
        if nm in wide:
            assert e.written == 0
        for which, seed in PATHS:
            run_model(e, 0, 0, which, seed)


def test_model_refuses_what_a_binding_refuses():
    v = np.zeros((4, 2), np.int32)
    out = np.zeros(64, np.uint8)
    for kw in (dict(stride=2), dict(stride=5), dict(offset=1)):
        with pytest.raises(ca.CortoError) as ei:
            ca.quant_out_model(v, out=out, **kw)
        assert ei.value.code == qo.E_ARGUMENT
