"""CPU checks of the tick map and the site draw: the library exports the
device map's entry points, the command-line driver knows --tick-map, the map
function shared by the host and the kernel (fi_tick_map.h over
pack_tick_table's table) gives the recorded results on random attempt tables
(tests/golden/tick_map.json), and the shared draw (fi_site_draw.h) equals the
oracle's samplers -- both through tools/tick_map_check.cpp, a stand-alone
host program under AddressSanitizer and UBSan."""
import ctypes
import json
import os
import subprocess

import pytest

from conftest import ROOT, workload_elf


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
    from shrewd_amd import FaultCampaign
    for kw in ({"cpu_type": "atomic", "tick_map": "device"}, {"cpu_type": "timing", "tick_map": "bogus"}):
        with pytest.raises(ValueError, match="tick_map"):
            FaultCampaign(str(tmp_path / "absent.elf"), **kw)


def build_tick_map_check(out_dir):
    """tools/tick_map_check.cpp as a stand-alone host program under AddressSanitizer and UBSan."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(out_dir / "tick_map_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I" + os.path.join(csrc, "hip"),
                    os.path.join(ROOT, "tools", "tick_map_check.cpp"), os.path.join(csrc, "fi_tick.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


def recorded_tick_map(contract):
    with open(os.path.join(ROOT, "tests", "golden", "tick_map.json")) as f:
        rec = json.load(f)
    return {seed: rec[f"seed {seed} {contract}"] for seed in ("1", "7")}


@pytest.fixture(scope="module")
def tick_map_check(tmp_path_factory):
    return build_tick_map_check(tmp_path_factory.mktemp("tick_map_check"))


def test_tick_map_equals_recorded_host_map(tick_map_check):
    """The one map (tick_map_site over pack_tick_table's table) on 40 random
    attempt tables per seed, 4000 sites each: its per-table hashes and counts
    equal tests/golden/tick_map.json, recorded from the former host statement
    of the map (over the unpacked attempts, in fi_tick.cpp) before it was
    deleted -- the packed-table map printed the same lines then."""
    for seed, want in recorded_tick_map("numinst").items():
        assert len(want) == 41 and want[-1].startswith("ok 160000 sites")
        r = subprocess.run([tick_map_check, seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.splitlines() == want


REGS, PC, RESULT = (1 << 32) - 2, 1 << 32, 1 << 34
DRAW_CASES = [(REGS | PC, 1, 2**64 - 1), (REGS | PC | RESULT, 1, 2**64 - 1), (REGS, 4, 2**64 - 1),
              (REGS | PC, 1, 0x00FF00FF00FF00FF), (REGS | PC, 8, 0x00FF00FF00FF00FF), (PC, 64, 1)]


@pytest.fixture(scope="module")
def hello_oracle(oracle_mod):
    o = oracle_mod.Oracle(workload_elf("hello"), "hello")
    ninst = o.run_golden().ninst
    return o, ninst, o.tick_setup()


@pytest.mark.parametrize("structures,burst,bits", DRAW_CASES)
def test_shared_draw_equals_oracle_samplers(tick_map_check, hello_oracle, structures, burst, bits):
    """fi_site_draw.h (the engine's one draw: both device samplers and the
    host tick sampler call it) against the oracle's own two samplers, over
    hello's numInst and its golden ticks, trials 1000 .. 5999.  Memory words
    are left out (they need the engine's page list); every case keeps an
    eligible bit position."""
    o, ninst, ticks = hello_oracle
    seed, first, n = 0x5EED7101, 1000, 5000
    for rng, ref, when in ((ninst, o.sample(seed, first, n, structures, burst, bits), "inst"),
                           (ticks, o.tick_sample(seed, first, n, structures, burst, bits), "tick")):
        r = subprocess.run([tick_map_check, "draw", str(seed), str(first), str(n), str(rng), str(structures),
                            str(burst), hex(bits)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [ln.split() for ln in r.stdout.splitlines()]
        assert len(got) == n
        want = [[str(int(s[when])), str(int(s["target"])), format(int(s["mask"]), "x"), str(int(s["trial"]))]
                for s in ref]
        assert got == want
