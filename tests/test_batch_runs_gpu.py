"""Packed host blobs that lie in several buffers (crthip_ctx_set_packed_host_blobs): the blob list is cut into runs of blobs that follow
one another in host memory in arena layout, and every run goes up with a copy of its own, straight from the caller's memory.  Outputs are
raw-byte equal to the oracle (tolerance 0); crthip_batch_stats' upload_copies / upload_gathered_bytes say which path ran."""
import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from oracle import oracle as oc

pytestmark = pytest.mark.gpu

RUNS_MAX = 8           # batch.cpp: PACKED_RUNS_MAX


def enc(mesh, **kw):
    return ca.aligned_blob(ca.encode(mesh, position_bits=12, uv_bits=10, normal_bits=9, **kw))


@pytest.fixture(scope="module")
def blobs():
    """five small blobs of different sizes and kinds, a stray sixth, and the oracle's arrays of each"""
    bl = [enc(synth.bumpy_sphere(8, 4, seed=1), normal_prediction=ca.BORDER), enc(synth.bumpy_sphere(8, 4, seed=2), normal_prediction=ca.BORDER),
          enc(synth.point_cloud(20, 12, seed=3), normal_prediction=ca.DIFF), enc(synth.bumpy_sphere(10, 5, seed=4), normal_prediction=ca.BORDER),
          enc(synth.bumpy_sphere(8, 4, seed=5), normal_prediction=ca.BORDER), enc(synth.bumpy_sphere(9, 4, seed=6), normal_prediction=ca.BORDER)]
    return bl, [oc.decode(b) for b in bl]


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    c.set_packed_host_blobs(True)
    yield c
    c.close()


def decode_and_check(ctx, views, refs, tag):
    b = ca.Batch(ctx, views)
    try:
        st = b.stats()
        copies, gathered, arena = int(st.upload_copies), int(st.upload_gathered_bytes), int(st.arena_bytes)
        b.allocate_outputs(color_components=4, fill=0xA5)
        b.decode()
        assert (b.sync() == 0).all(), tag
        for i, ref in enumerate(refs):
            got = b.host_outputs(i)
            names = [k for k in ("position", "normal", "color", "uv", "index") if k in ref]
            assert names and set(names) == set(got) - {"nvert", "nface"}, (tag, i)
            for k in names:
                assert got[k].tobytes() == ref[k].tobytes(), (tag, i, k)
        return copies, gathered, arena
    finally:
        b.close()


def test_two_pinned_buffers_are_two_copies(ctx, blobs):
    bl, refs = blobs
    pin_a, va = ca.pinned_host_arena(bl[:3])
    pin_b, vb = ca.pinned_host_arena(bl[3:5])
    copies, gathered, _ = decode_and_check(ctx, va + vb, refs[:5], "3 + 2")
    assert (copies, gathered) == (2, 0)


def test_a_stray_pageable_blob_is_a_run_of_its_own(ctx, blobs):
    """the runs plus the stray: three copies, nothing gathered (the stray's copy reads pageable memory, which the runtime stages)"""
    bl, refs = blobs
    pin_a, va = ca.pinned_host_arena(bl[:3])
    pin_b, vb = ca.pinned_host_arena(bl[3:5])
    stray = bl[5].copy()
    copies, gathered, _ = decode_and_check(ctx, va + vb + [stray], refs, "3 + 2 + stray")
    assert (copies, gathered) == (3, 0)
    # ... and in the middle of a buffer's blobs it cuts that buffer's run in two
    copies, gathered, _ = decode_and_check(ctx, va[:2] + [stray] + va[2:] + vb, [refs[0], refs[1], refs[5], refs[2], refs[3], refs[4]], "stray inside")
    assert (copies, gathered) == (4, 0)


def test_one_buffer_is_one_copy(ctx, blobs):
    bl, refs = blobs
    pin, views = ca.pinned_host_arena(bl[:5])
    copies, gathered, _ = decode_and_check(ctx, views, refs[:5], "one buffer")
    assert (copies, gathered) == (1, 0)


def test_more_runs_than_the_limit_are_gathered(ctx, blobs):
    """RUNS_MAX + 1 blobs, none adjacent to the one before: the documented fallback, one copy of the gathered image"""
    bl, refs = blobs
    pin, views = ca.pinned_host_arena(bl[:5])
    order = [0, 2, 4, 1, 3, 0, 2, 4, 1]                    # (never i, i + 1)
    assert len(order) == RUNS_MAX + 1
    copies, gathered, arena = decode_and_check(ctx, [views[i] for i in order], [refs[i] for i in order], "nine runs")
    assert copies == 1 and gathered == arena > 0


def test_switch_off_gathers(blobs):
    bl, refs = blobs
    c = ca.Context(0)
    try:
        pin, views = ca.pinned_host_arena(bl[:5])
        copies, gathered, arena = decode_and_check(c, views, refs[:5], "switch off")
        assert copies == 1 and gathered == arena > 0
    finally:
        c.close()
