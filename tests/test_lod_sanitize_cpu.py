"""The method and both partitions of the levels of detail (csrc/lod.h) under AddressSanitizer and UBSan: tests/cpp/lod_check.cpp, a stand-alone
program with its own main, on heap blocks that end exactly at nvert words of remap, at 3*faces words of the level's index (a capacity equal to
the kept count), at the tables' ends and at the 16-byte record, with positions that share cells and indices that hold ids >= nvert.
Host code only: the sources are compiled for the host, no device code is sanitized and nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_lod_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "lod_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "lod_check.cpp"),
                           os.path.join(csrc, "lod_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "lod_check ok" in out.stdout, out.stdout[-2000:]
