"""The kernel schedule of a decode call, pinned: for each case the records of Batch.kernel_times() - (name, launches), in the order of their first
launch - equal a literal.  Many tests ask whether one kernel's name is among them; this one holds the whole sequence of Planner::launch, shape by
shape (plan_launch.cpp: long streams, forked, one stream) and stage by stage, so that a launch that moves, doubles or goes missing shows here
and not only in a benchmark.  A record that spans several launches is one record (normal_scan x2, delta_tiles, topology_lds, tunstall_decode).
The literals were recorded on an MI355X from the library of the commit BEFORE Planner::launch was split into stage members, selected with
$CORTO_HIP_LIB_PATH in a process of its own - never from the tree under test (profiles/plan_launch.md lists them and says how).
Profiling on, a fresh context per case; crthip_kernel_times holds 32 names and every case stays below that."""
import functools

import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from test_plan_jobs_cpu import corpus_blobs
from test_pool_carry_gpu import c4_item

B_EST, B_BORDER, B_DIFF, B_NONORMAL, B_CLOUD, B_TANBIG, B_UNFUSED, B_BEYOND16, B_SIXCOMP = range(9)     # tests/cpp/plan_dump.cpp's enum
EVERYTHING = dict(computed_normals=True, computed_tangents=True, meshlet_bounds=True, adjacency=True, weld=True)


@functools.lru_cache(maxsize=None)
def corpus():
    return corpus_blobs()


@functools.lru_cache(maxsize=None)
def long_stream_blob():
    """a sphere of the corpus's kind whose batch decode sets Plan::tun_multi_chunk (a Tunstall stream of more than one chunk): 128 000 vertices,
    test_pool_carry_gpu's "blob with long Tunstall streams".  Spheres of 256x128, 300x150, 360x180 and 420x210 (88 200 vertices) do not set it"""
    return ca.aligned_blob(ca.encode(synth.bumpy_sphere(512, 250, seed=1), normal_prediction=ca.BORDER))


def sequence(b):
    return [(name, rec["launches"]) for name, rec in b.kernel_times().items()]


def decode(blobs, single_stream=False, **outputs):
    c = ca.Context(0)
    try:
        if single_stream:
            c.set_single_stream(True)
        c.set_profiling(True)
        b = ca.Batch(c, blobs)
        try:
            b.allocate_outputs(**outputs)
            b.decode()
            assert (b.sync() == 0).all()
            return sequence(b)
        finally:
            b.close()
    finally:
        c.close()


def pipelined(items, single_stream=True):
    """a lane's calls over one or two batches - decode_with_next(None, A), (A, B), (B, None) - and the sequence of each call"""
    c = ca.Context(0)
    objs = []
    try:
        if single_stream:
            c.set_single_stream(True)
        c.set_profiling(True)
        objs = [ca.Batch(c, []) for _ in items]
        for k, (o, blobs) in enumerate(zip(objs, items)):
            o.set_parity(k)
            o.reset(blobs)
            o.allocate_outputs(fill=0)
        objs[0].decode_entropy()
        seqs = [sequence(objs[0])]
        for k, o in enumerate(objs):
            o.decode_with_next(objs[k + 1] if k + 1 < len(objs) else None)
            assert (o.sync() == 0).all()
            seqs.append(sequence(o))
        return seqs
    finally:
        for o in objs:
            o.close()
        c.close()


CASES = {
    "forked": lambda: decode([corpus()[B_EST]]),
    "one_stream_front": lambda: decode([corpus()[B_EST]], single_stream=True),
    "derived_blob_kernels": lambda: decode([corpus()[B_EST], corpus()[B_NONORMAL]], single_stream=True, meshlets=(64, 124, 0), **EVERYTHING),
    "derived_beyond_lds": lambda: decode([corpus()[B_BEYOND16]], meshlets=(64, 124, 4096), **EVERYTHING),
    "cloud": lambda: decode([corpus()[B_CLOUD]]),
    "quantised_40": lambda: decode([corpus()[B_EST]], quantized=("position",)),
    "quantised_2352": lambda: decode([corpus()[B_TANBIG]], quantized=("position",)),
    "long_streams": lambda: decode([long_stream_blob()]),
    "pipelined_pair": lambda: pipelined([c4_item(64, 700), c4_item(64, 8780)]),
    # a schedule without a separate entropy stage is only planned by the call that has it as `next`: Planner::splits() and the branch launch() takes agree
    "pipelined_long_streams": lambda: pipelined([[long_stream_blob()]]),
    "pipelined_forked": lambda: pipelined([[corpus()[B_EST]]], single_stream=False),
}

EXPECTED = {
    "forked": [("tunstall_stream", 2), ("topology_lds", 1), ("unpack_wave", 1), ("delta_lds16", 1), ("normal_blob", 1)],
    "one_stream_front": [("tunstall_stream", 1), ("front", 1), ("delta_lds16", 1), ("normal_blob", 1)],
    "derived_blob_kernels": [("tunstall_stream", 1), ("front", 1), ("delta_lds16", 1), ("normal_blob", 1), ("normal_blob_computed", 1), ("tangent_blob", 1),
                             ("meshlet_blob", 1), ("meshlet_bounds", 1), ("weld_blob", 1), ("adjacency_blob", 1), ("dequantize", 1)],
    "derived_beyond_lds": [("tunstall_stream", 2), ("topology_lds", 1), ("fill", 1), ("unpack_extract", 1), ("delta_tiles", 1), ("normal_faces", 1),
                           ("normal_scan", 2), ("normal_fill", 1), ("normal_flags", 1), ("normal_vertex", 1), ("tangent_faces", 1), ("tangent_vertex", 1),
                           ("meshlet_segments", 1), ("meshlet_place", 1), ("meshlet_bounds", 1), ("weld_insert", 1), ("weld_lookup", 1), ("weld_index", 1),
                           ("adjacency_count", 1), ("adjacency_offsets", 1), ("adjacency_fill", 1), ("adjacency_twin", 1), ("dequantize", 1)],
    "cloud": [("tunstall_stream", 1), ("unpack_wave", 1), ("cloud_sums", 1), ("scan", 1), ("cloud_apply", 1), ("normal_diff", 1), ("dequantize", 1)],
    "quantised_40": [("tunstall_stream", 2), ("topology_lds", 1), ("unpack_wave", 1), ("delta_lds16", 1), ("normal_blob", 1), ("quant_out_blob", 1)],
    "quantised_2352": [("tunstall_stream", 2), ("topology_lds", 1), ("fill", 1), ("unpack_wave", 1), ("delta_lds16", 1), ("normal_blob", 1), ("quant_range", 1),
                       ("quant_store", 1)],
    "long_streams": [("tunstall_tables", 1), ("tunstall_chunk_sums", 1), ("tunstall_decode", 1), ("topology_lds", 1), ("unpack_wave", 1), ("unpack_extract", 1),
                     ("delta_tiles", 1), ("normal_faces", 1), ("normal_scan", 2), ("normal_fill", 1), ("normal_flags", 1), ("normal_vertex", 1), ("dequantize", 1)],
    # the pair is carried: B's K-TAB and K-STREAM ride in A's front and delta_lds16 grids, and no call after the first has a Tunstall launch of its own
    "pipelined_pair": [[("tunstall_tables", 1), ("tunstall_stream", 1)],
                       [("front", 1), ("delta_lds16", 1), ("normal_blob", 1)],
                       [("front", 1), ("delta_lds16", 1), ("normal_blob", 1)]],
    "pipelined_long_streams": [[], [("tunstall_tables", 1), ("tunstall_chunk_sums", 1), ("tunstall_decode", 1), ("topology_lds", 1), ("unpack_wave", 1),
                                    ("unpack_extract", 1), ("delta_tiles", 1), ("normal_faces", 1), ("normal_scan", 2), ("normal_fill", 1), ("normal_flags", 1),
                                    ("normal_vertex", 1), ("dequantize", 1)]],
    "pipelined_forked": [[], [("tunstall_stream", 2), ("topology_lds", 1), ("unpack_wave", 1), ("delta_lds16", 1), ("normal_blob", 1)]],
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence(case):
    got = CASES[case]()
    for seq in (got if case.startswith("pipelined") else [got]):
        assert len(seq) < 32, seq
    assert got == EXPECTED[case]
