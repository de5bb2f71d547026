"""The arithmetic and the two partitions of CRTHIP_BIND_QUANTIZED (csrc/quant_out.h) under AddressSanitizer and UBSan:
tests/cpp/quant_out_check.cpp, a stand-alone program with its own main, on heap blocks that end exactly with the last vertex's halfwords.
Host code only: the sources are compiled for the host, no device code is sanitized and nothing of it is loaded into python."""
import os
import subprocess

from conftest import ROOT


def test_quant_out_partitions_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "quant_out_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "quant_out_check.cpp"),
                           os.path.join(csrc, "quant_out_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "quant_out_check ok" in out.stdout, out.stdout[-2000:]
