"""CPU checks of the literal tick contract (fi_set_tick_contract): the library
exports its entry point, the command-line driver and FaultCampaign refuse bad
values before a device is asked for, and the two statements of the literal
map (fi_tick.cpp map_tick_site, fi_tick_map.h tick_map_site) agree on random
attempt tables -- tools/tick_map_check.cpp in its literal mode, as a
stand-alone host program under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


def test_library_exports_tick_contract():
    from shrewd_amd import build_library
    lib = ctypes.CDLL(build_library())
    assert hasattr(lib, "fi_set_tick_contract")


def test_cli_rejects_unknown_tick_contract():
    """Refused while the arguments are read: before an engine (a device) is asked for."""
    from shrewd_amd import build as b
    exe = b.build_cli()
    r = subprocess.run([exe, "--workload", os.path.join(ROOT, "workloads", "hello.elf"), "--trials", "8",
                        "--cpu-type", "timing", "--tick-contract", "bogus"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--tick-contract" in r.stderr and "bogus" in r.stderr
    assert "no HIP device" not in r.stderr


def test_fault_campaign_rejects_tick_contract_without_timing(tmp_path):
    """tick_contract needs cpu_type='timing': refused before the engine is made."""
    from shrewd_amd import FaultCampaign
    for kw in ({"cpu_type": "atomic", "tick_contract": "literal"}, {"cpu_type": "timing", "tick_contract": "bogus"}):
        with pytest.raises(ValueError, match="tick_contract"):
            FaultCampaign(str(tmp_path / "absent.elf"), **kw)


def test_literal_maps_agree(tmp_path):
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "tick_map_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I" + os.path.join(csrc, "hip"),
                    os.path.join(ROOT, "tools", "tick_map_check.cpp"), os.path.join(csrc, "fi_tick.cpp"),
                    "-o", exe], check=True, timeout=300)
    for seed in ("1", "7"):
        r = subprocess.run([exe, seed, "literal"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
