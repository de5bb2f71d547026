"""The closest-face queries (csrc/bvh_closest.h) under AddressSanitizer and UBSan: tests/cpp/bvh_closest_check.cpp, a stand-alone program
with its own main, on heap blocks that end exactly at the last node, at the last vertex's sixth byte (stride 8 included), at the last index
entry, at the transform's 48th byte and at the last point and hit record, on trees of both partitions, in both child orders, and on corrupt
ones; the hook's own stack block ends at the kernel's LDS size.  Host code only: the sources are compiled for the host, no device code is
sanitized and nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_bvh_closest_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "bvh_closest_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "bvh_closest_check.cpp"),
                           os.path.join(csrc, "bvh_closest_host.cpp"), os.path.join(csrc, "bvh_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "bvh_closest_check ok" in out.stdout, out.stdout[-2000:]
