"""The method and both partitions of a cloud's levels of detail (csrc/cloud_lod.h) under AddressSanitizer and UBSan:
tests/cpp/cloud_lod_check.cpp, a stand-alone program with its own main, on heap blocks that end exactly at nvert words of remap, at `cells`
words of points and weight (capacities equal to the kept count), at ceil(cells / K) chunk records, at the table's end and at the 16-byte
record, with positions that share cells.  Host code only: the sources are compiled for the host, no device code is sanitized and nothing of
it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_cloud_lod_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "cloud_lod_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "cloud_lod_check.cpp"),
                           os.path.join(csrc, "cloud_lod_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "cloud_lod_check ok" in out.stdout, out.stdout[-2000:]
