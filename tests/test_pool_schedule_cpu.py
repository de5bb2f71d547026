"""The pool's schedule without a GPU: tests/cpp/pool_fake_backend.cpp defines everything corto_amd/csrc/pool.cpp calls (the crthip_ctx_* /
crthip_batch_* entry points, pool_internal.h, a handful of HIP calls as malloc and a table), logs every call per lane, and asserts from the
log what pool.cpp's comments, corto_hip.h ("Groups", crthip_pool_decode) and DESIGN.md §7 promise: every item settled once, groups of at
most G members that are all resident or all uploaded, one mesh stage between two syncs, a lane's block never moved under a batch, the
poison in front of the last steps and no others, one D2H copy a host-bound member, a device fault that ends the call with everything in
flight synced.  The blobs are real ones from the host encoder; crthip_probe and the output layout are the library's own (host_probe.cpp).
Built twice as a stand-alone program from pool.cpp, host_probe.cpp, crt_format.cpp and the fake alone - no HIP runtime is linked: plain
(every scenario) and with ThreadSanitizer on the host code (two pool devices x two threads, and the 17-item decodes)."""
import os
import subprocess

import numpy as np
import pytest

import corto_amd as ca
from conftest import ROOT
from corto_amd import synth

CLANG = "/opt/rocm/lib/llvm/bin/clang++"       # hipcc's own host compiler: the sources are plain C++ here and nothing links the runtime
CSRC = os.path.join(ROOT, "corto_amd", "csrc")


def enc(mesh, **kw):
    kw.setdefault("normal_prediction", ca.BORDER)
    return ca.aligned_blob(ca.encode(mesh, position_bits=12, uv_bits=10, normal_bits=9, **kw))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """(plain program, ThreadSanitizer program, corpus): four tiny meshes of three sizes and a cloud, as tests/test_pool_group_gpu.py's items"""
    tmp = tmp_path_factory.mktemp("pool_schedule")
    blobs = [enc(synth.bumpy_sphere(8, 4, seed=1)), enc(synth.bumpy_sphere(10, 5, seed=2)), enc(synth.point_cloud(20, 12, seed=3), normal_prediction=ca.DIFF),
             enc(synth.bumpy_sphere(12, 4, seed=4)), enc(synth.bumpy_sphere(8, 4, seed=5))]
    corpus = str(tmp / "corpus.bin")
    with open(corpus, "wb") as f:
        f.write(np.uint32(len(blobs)).tobytes())
        for b in blobs:
            f.write(np.uint32(len(b)).tobytes()); f.write(b.tobytes())
    exes, procs = [], []
    for name, extra in (("pool_fake_backend", []), ("pool_fake_backend_tsan", ["-fsanitize=thread"])):
        exes.append(str(tmp / name))
        procs.append(subprocess.Popen([CLANG, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + extra +
                                      ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pool_fake_backend.cpp"), os.path.join(CSRC, "pool.cpp"),
                                       os.path.join(CSRC, "host_probe.cpp"), os.path.join(CSRC, "crt_format.cpp"), "-o", exes[-1]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out[-4000:]
    return exes[0], exes[1], corpus


def test_every_scenario_keeps_the_invariants(built):
    out = subprocess.run([built[0], built[2]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "pool_fake_backend ok: 17 scenarios" in out.stdout, out.stdout[-2000:]


def test_worker_threads_under_thread_sanitizer(built):
    """four worker threads on twelve lanes with crthip_batch_done answering after a few polls, and the 17-item decodes: the invariants that do
    not depend on the order, and no data race in pool.cpp's host code"""
    out = subprocess.run([built[1], built[2], "--threaded-only"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr, out.stdout[-4000:] + out.stderr[-4000:]
    assert "pool_fake_backend ok: 4 scenarios" in out.stdout, out.stdout[-2000:]
