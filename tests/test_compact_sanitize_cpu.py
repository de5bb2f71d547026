"""The method, both partitions and the gather of the compaction (csrc/compact.h) under AddressSanitizer and UBSan:
tests/cpp/compact_check.cpp, a stand-alone program with its own main, on heap blocks that end exactly at nvert words of newid, at
vertex_capacity words of order, at index_capacity words of index (capacities equal to what is written, one less, and 0), at the last
gathered byte, at the mask's end and at the 16-byte record.  Host code only: the sources are compiled for the host, no device code is
sanitized and nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_compact_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "compact_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "compact_check.cpp"),
                           os.path.join(csrc, "compact_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "compact_check ok" in out.stdout, out.stdout[-2000:]
