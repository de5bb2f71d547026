"""The host side of crthip_mesh_layout under AddressSanitizer and UBSan: tests/cpp/enc_layout_check.cpp, a stand-alone program, with the
three host sources it exercises.  Host code only: the sources are compiled for the host and no device code is sanitized."""
import os
import subprocess

from conftest import ROOT


def test_layout_host_code_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "enc_layout_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "enc_layout_check.cpp"),
                           os.path.join(csrc, "encoder.cpp"), os.path.join(csrc, "enc_input_host.cpp"), os.path.join(csrc, "enc_topology_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "enc_layout_check ok" in out.stdout, out.stdout[-2000:]
