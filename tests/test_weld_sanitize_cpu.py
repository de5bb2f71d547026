"""The method and both partitions of the weld (csrc/weld.h) under AddressSanitizer and UBSan: tests/cpp/weld_check.cpp, a stand-alone program
with its own main, on heap blocks that end exactly at nvert words of remap, at 3*nface words of the welded index, at T words of the table and at
the 16-byte record, with positions that coincide and indices that hold ids >= nvert.
Host code only: the sources are compiled for the host, no device code is sanitized and nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_weld_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "weld_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "weld_check.cpp"),
                           os.path.join(csrc, "weld_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "weld_check ok" in out.stdout, out.stdout[-2000:]
