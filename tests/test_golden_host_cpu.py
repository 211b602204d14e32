"""The host passes of fi_golden_run (fi_golden_host.h: snapshot page dedupe,
register liveness at the snapshots, first-access index) on hand-made inputs,
in a stand-alone host program under AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_golden_host_passes_sanitized(tmp_path):
    """tools/golden_host_check.cpp: the three functions as the engine calls
    them, against values derived by hand in its comments."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    exe = str(tmp_path / "golden_host_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tools", "golden_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "golden_host_check ok" in r.stdout
