"""The decode planner without a GPU: tests/cpp/plan_dump.cpp, a stand-alone program with its own main, is built from the planner's stage files
(plan_carve.cpp, plan_jobs.cpp, plan_group.cpp), batch_bind.cpp, meshlet_host.cpp, crt_format.cpp and host_probe.cpp as plain C++ - no HIP
runtime is linked - once plain and once under AddressSanitizer and UBSan, and run directly.  It binds real blobs from the host encoder through the C
ABI's bind calls with constant fake addresses, runs carve(), jobs(), group() and upload() for every scenario and asserts what only the GPU suite saw
before: binding and unbinding every derived output leaves the plan of a batch that never bound them; a batch without derived bindings has no tangent,
meshlet, bounds, adjacency or weld job, no optional array placed and no record behind the status words; after each cascade call (a bind, a normals
call, a meshlets call) the dropped outputs have no jobs; with tangents, bounds or a weld the position's integers last until k_dequant, with one fused
reader and none of them the normal kernel writes the float positions; every id in every id and block map is below its job array's size; the zero
fills of a scratch table cover it exactly; and, of the image upload() stages, no word is a scratch pointer left unresolved and every word upload()
changed lies in the scratch block.  profiles/plan_jobs.md, profiles/plan_launch.md: the same program compares two trees."""
import os
import subprocess

import numpy as np
import pytest

import corto_amd as ca
from conftest import ROOT
from corto_amd import synth

CLANG = "/opt/rocm/lib/llvm/bin/clang++"       # hipcc's own host compiler: the sources are plain C++ here and nothing links the runtime
CSRC = os.path.join(ROOT, "corto_amd", "csrc")
SOURCES = ["plan_carve.cpp", "plan_jobs.cpp", "plan_group.cpp", "batch_bind.cpp", "meshlet_host.cpp", "crt_format.cpp", "host_probe.cpp"]


def enc(mesh, **kw):
    kw.setdefault("normal_prediction", ca.ESTIMATED)
    return ca.aligned_blob(ca.encode(mesh, position_bits=12, uv_bits=10, normal_bits=9, **kw))


def corpus_blobs():
    """the smallest blobs that reach every branch of the planner, in the order of plan_dump.cpp's enum"""
    tiny = synth.bumpy_sphere(8, 4, seed=1)
    six = np.linspace(0.0, 1.0, tiny.nvert * 6, dtype=np.float32).reshape(tiny.nvert, 6)
    return [enc(tiny), enc(tiny, normal_prediction=ca.BORDER), enc(tiny, normal_prediction=ca.DIFF),
            enc(synth.bumpy_sphere(10, 5, seed=2), with_normal=False),                         # a mesh that stores no normals
            enc(synth.point_cloud(20, 12, seed=3), normal_prediction=ca.DIFF),
            enc(synth.bumpy_sphere(48, 48, seed=4), normal_prediction=ca.BORDER),              # 2 352 vertices: just above TANGENT_BLOB_MAX
            enc(synth.bumpy_sphere(128, 86, seed=5)),                                          # 3*nface = 66 048: no fused normal kernel
            enc(synth.bumpy_sphere(256, 128, seed=6)),                                         # 33 024 vertices: beyond DELTA16_NVERT_MAX
            enc(tiny, attributes=[("weights", six, 1.0 / 64, 0)])]                             # an attribute of more than four components


def write_corpus(path):
    blobs = corpus_blobs()
    with open(path, "wb") as f:
        f.write(np.uint32(len(blobs)).tobytes())
        for b in blobs:
            f.write(np.uint32(len(b)).tobytes()); f.write(b.tobytes())


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """(plain program, sanitized program, corpus)"""
    tmp = tmp_path_factory.mktemp("plan_jobs")
    corpus = str(tmp / "corpus.bin")
    write_corpus(corpus)
    exes, procs = [], []
    for name, extra in (("plan_dump", []), ("plan_dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exes.append(str(tmp / name))
        procs.append(subprocess.Popen([CLANG, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function"] + extra +
                                      ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "plan_dump.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", exes[-1]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out[-4000:]
    return exes[0], exes[1], corpus


def test_every_scenario_keeps_the_plan_invariants(built, tmp_path):
    """... and two runs of one build write the same dump, byte for byte"""
    dumps = []
    for k in range(2):
        dumps.append(str(tmp_path / ("dump%d.txt" % k)))
        out = subprocess.run([built[0], built[2], "--dump", dumps[-1]], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
        assert "plan_dump ok: " in out.stdout, out.stdout[-2000:]
    with open(dumps[0], "rb") as a, open(dumps[1], "rb") as b:
        assert a.read() == b.read()


def test_planner_and_bind_calls_under_sanitizers(built):
    out = subprocess.run([built[1], built[2]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "plan_dump ok: " in out.stdout and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
