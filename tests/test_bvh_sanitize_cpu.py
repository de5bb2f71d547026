"""Both partitions of the BVH (csrc/bvh.h) under AddressSanitizer and UBSan: tests/cpp/bvh_check.cpp, a stand-alone program with its own
main, on heap blocks that end exactly at 2F - 1 node records, at 2F - 1 words of parent, at F words of order and at the 16-byte record; the
hook's own scratch ends at the kernels' sizes.  Host code only: the sources are compiled for the host, no device code is sanitized and
nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_bvh_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "bvh_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "bvh_check.cpp"),
                           os.path.join(csrc, "bvh_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "bvh_check ok" in out.stdout, out.stdout[-2000:]
