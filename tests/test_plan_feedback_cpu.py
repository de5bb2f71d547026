"""What a decode context learns from a batch's flags (corto_amd/csrc/plan_feedback.h) - K-DELTA's narrow / wide layout and the CLERS
automaton's LDS edge slots, each with its back-off - as a stand-alone host program under AddressSanitizer and UBSan.  The trajectories are
in tests/cpp/plan_feedback_check.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feedback_trajectories_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "corto_amd", "csrc")
    exe = str(tmp_path / "plan_feedback_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "cpp", "plan_feedback_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "plan_feedback_check ok" in out.stdout, out.stdout[-2000:]
