"""CPU checks of the device tick map: the library exports its entry points,
the command-line driver knows --tick-map, and the map function shared by the
host and the kernel (fi_tick_map.h over pack_tick_table's table) equals
fi_tick.cpp map_tick_site on random attempt tables -- as a stand-alone host
program under AddressSanitizer and UBSan (tools/tick_map_check.cpp)."""
import ctypes
import os
import subprocess

from conftest import ROOT


def test_library_exports_device_tick_map():
    from shrewd_amd import build_library
    lib = ctypes.CDLL(build_library())
    for f in ("fi_set_tick_map", "fi_map_tick_sites_device", "fi_run_tick_trials_device"):
        assert hasattr(lib, f), f


def test_cli_rejects_unknown_tick_map():
    """Refused while the arguments are read: before an engine (a device) is asked for."""
    from shrewd_amd import build as b
    exe = b.build_cli()
    r = subprocess.run([exe, "--workload", os.path.join(ROOT, "workloads", "hello.elf"), "--trials", "8",
                        "--cpu-type", "timing", "--tick-map", "bogus"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--tick-map" in r.stderr and "bogus" in r.stderr
    assert "no HIP device" not in r.stderr


def test_fault_campaign_rejects_tick_map_without_timing(tmp_path):
    """tick_map needs cpu_type='timing': refused before the engine is made."""
    import pytest
    from shrewd_amd import FaultCampaign
    for kw in ({"cpu_type": "atomic", "tick_map": "device"}, {"cpu_type": "timing", "tick_map": "bogus"}):
        with pytest.raises(ValueError, match="tick_map"):
            FaultCampaign(str(tmp_path / "absent.elf"), **kw)


def test_shared_map_function_equals_host_map(tmp_path):
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "tick_map_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I" + os.path.join(csrc, "hip"),
                    os.path.join(ROOT, "tools", "tick_map_check.cpp"), os.path.join(csrc, "fi_tick.cpp"),
                    "-o", exe], check=True, timeout=300)
    for seed in ("1", "7"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
