"""CPU checks of the literal tick contract (fi_set_tick_contract): the library
exports its entry point, the command-line driver and FaultCampaign refuse bad
values before a device is asked for, and the literal map (fi_tick_map.h
tick_map_site) gives the recorded results on random attempt tables
(tests/golden/tick_map.json) -- tools/tick_map_check.cpp in its literal mode,
as a stand-alone host program under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_tick_device_cpu import build_tick_map_check, recorded_tick_map


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


def test_literal_tick_map_equals_recorded_host_map(tmp_path):
    """As test_tick_device_cpu.py test_tick_map_equals_recorded_host_map, under
    the literal contract: the recording is the former host statement's
    (fi_tick.cpp's, with literal set), with which the packed-table map agreed
    on the tick descriptors too.  The tool itself asserts that the only escapes
    left are FI_TK_MACRO and sites past FI_SITE_TK_SKIP_MAX attempts and that
    each kind of descriptor occurred."""
    exe = build_tick_map_check(tmp_path)
    for seed, want in recorded_tick_map("literal").items():
        assert len(want) == 41 and want[-1].startswith("ok 160000 sites")
        r = subprocess.run([exe, seed, "literal"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.splitlines() == want
