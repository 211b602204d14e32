"""CPU checks of exact campaigns in the tick domain (fi_exact_tick.h,
DESIGN.md §4j "Tick domain"): the library exports the entry points;
tools/exact_tick_host_check.cpp -- a stand-alone host program under
AddressSanitizer and UBSan -- walks every tick of random small attempt tables
under both tick contracts; hand-made tables whose classes are written out
here; FaultCampaign's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_library_exports_exact_tick():
    from shrewd_amd import build_library
    lib = ctypes.CDLL(build_library())
    for f in ("fi_exact_tick_get_info", "fi_exact_tick_sites", "fi_run_exact_ticks", "fi_exact_tick_locate",
              "fi_exact_tick_classes", "fi_exact_tick_attempts"):
        assert hasattr(lib, f), f


def test_host_check_every_tick_of_random_tables(tmp_path):
    """60 random tables x both contracts: over every tick, x1..x31, the pc and
    the result, the map followed by a linear interval lookup lands in the class
    exact_tick_locate names, that class runs the site the tick maps to, and
    class weights + dead + golden + escaped ticks = T per structure."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "exact_tick_host_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I" + os.path.join(csrc, "hip"),
                    os.path.join(ROOT, "tools", "exact_tick_host_check.cpp"), os.path.join(csrc, "fi_tick.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- hand-made tables
def _table(rows):
    """rows: (done, n, exec, flags, g, done_rd); one fetch, 4-byte instructions at 0x10000 + 4 j."""
    from shrewd_amd.fi import TICK_ATTEMPT_DT
    att = np.zeros(len(rows), TICK_ATTEMPT_DT)
    for j, (done, n, ex, flags, g, done_rd) in enumerate(rows):
        att[j] = (done, 0x10000 + 4 * j, n, ex, ex, 0, g, 4, 1, 0, 0, 0, 0, done_rd, flags)
    return att


def _index(entries):
    """entries: {reg: [(numInst, is_ecall, reads)]} -> (off33, ev) of the first-access index."""
    off, ev = [0] * 33, []
    for r in range(1, 32):
        off[r] = len(ev)
        ev += [((2 * n + (0 if ecall else 1)) << 1) | int(reads) for n, ecall, reads in entries.get(r, [])]
    off[32] = len(ev)
    return np.array(off, np.uint32), np.array(ev, np.uint32)


def _classes(att, T, ninst, off, ev, reg, contract="numinst"):
    from shrewd_amd import exact_tick_classes
    cls, tot = exact_tick_classes(att, T, ninst, off, ev, reg, contract)
    return [(int(c["weight"]), int(c["tick"]), int(c["inst"])) for c in cls], tot


def test_load_whose_completion_writes_the_flipped_register():
    """alu [0,10] | load x5: fetch [11,20], data [21,50] | alu [51,60] | exit
    ecall [61,69]; T = 70, ninst = 3.  x5 is written by the load (numInst 1) and
    read at numInst 2; x6 is read at numInst 2 only."""
    from shrewd_amd.fi import TA_COMMITS, TA_ECALL, TA_END
    att = _table([(10, 0, 10, TA_COMMITS, 0, 0), (50, 1, 20, TA_COMMITS, 1, 5), (60, 2, 60, TA_COMMITS, 2, 0),
                  (70, 3, 70, TA_ECALL | TA_END, 3, 0)])
    off, ev = _index({5: [(1, False, False), (2, False, True)], 6: [(2, False, True)]})
    for contract in ("numinst", "literal"):
        # x5: [0,20] dies at the load's write; the data phase is golden-equal (the completion overwrites
        # the flip); [51,60] maps to numInst 2, the read; the exit ecall's ticks have no access after them
        cls, tot = _classes(att, 70, 3, off, ev, 5, contract)
        assert cls == [(10, 51, 2)]
        assert tot == {"dead": 11 + 10 + 9, "golden": 30, "escaped": 0, "esc_insts": 0}
        # x6: fetch phases map to their own numInst, the load's data phase to numInst 2: all before the read
        cls, tot = _classes(att, 70, 3, off, ev, 6, contract)
        assert cls == [(11 + 10 + 30 + 10, 0, 2)]
        assert tot == {"dead": 9, "golden": 0, "escaped": 0, "esc_insts": 0}
        # x7: never accessed
        cls, tot = _classes(att, 70, 3, off, ev, 7, contract)
        assert cls == [] and tot["dead"] == 70


def test_ecall_then_retry_for_a0_and_the_exit_ecall_interval():
    """alu [0,10] | ecall at numInst 1 [11,20] (commits nothing) | the next
    attempt at numInst 1 [21,30] | exit ecall [31,39]; T = 40, ninst = 2.  a0 is
    read by both ecalls.  A flip while the attempt after the ecall is fetched
    lands after the ecall read a0: not a numInst site."""
    from shrewd_amd.fi import TA_COMMITS, TA_ECALL, TA_END, XT_MAPPED
    att = _table([(10, 0, 10, TA_COMMITS, 0, 0), (20, 1, 20, TA_ECALL, 1, 0), (30, 1, 30, TA_COMMITS, 1, 0),
                  (40, 2, 40, TA_ECALL | TA_END, 3, 0)])
    off, ev = _index({10: [(1, True, True), (2, True, True)], 5: [(1, False, True)]})
    # the exit ecall's interval stands at numInst == ninst, unclipped: 9 ticks, inst 2
    cls, tot = _classes(att, 40, 2, off, ev, 10, "numinst")
    assert cls == [(11 + 10, 0, 1), (9, 31, 2)]
    assert tot == {"dead": 0, "golden": 0, "escaped": 10, "esc_insts": 10 * 1}
    cls, tot = _classes(att, 40, 2, off, ev, 10, "literal")
    assert cls == [(11 + 10, 0, 1), (9, 31, 2), (10, 21, XT_MAPPED)]   # the descriptor class comes last
    assert tot == {"dead": 0, "golden": 0, "escaped": 0, "esc_insts": 0}
    # x5 is no syscall argument: the ticks after the ecall are plain sites at numInst 1
    cls, tot = _classes(att, 40, 2, off, ev, 5, "numinst")
    assert cls == [(11 + 10 + 10, 0, 1)] and tot["dead"] == 9 and tot["escaped"] == 0
    # the atomic classes of the same index clip the exit ecall to ninst - 1 = 1: no class of its own
    from shrewd_amd import exact_classes
    acls, dead = exact_classes(off, ev, 2, 10)
    assert [(int(c["inst"]), int(c["weight"])) for c in acls] == [(1, 2)] and dead == 0


def test_exact_tick_classes_rejects_bad_arguments():
    from shrewd_amd import EngineError, exact_tick_classes
    from shrewd_amd.fi import TA_COMMITS
    att = _table([(10, 0, 10, TA_COMMITS, 0, 0)])
    off, ev = _index({})
    with pytest.raises(EngineError):
        exact_tick_classes(att, 10, 1, off, ev, 0)
    with pytest.raises(EngineError):
        exact_tick_classes(att, 0, 1, off, ev, 5)
    with pytest.raises(EngineError):
        exact_tick_classes(att, 10, 1, off, ev, 5, contract=7)


def test_fault_campaign_refuses_profile_and_memory_with_timing(tmp_path):
    """Refused in __init__ with a message, before the engine is made."""
    from shrewd_amd import FaultCampaign
    for kw, what in (({"profile": True}, "profile"), ({"exact_memory": True}, "exact_memory")):
        with pytest.raises(ValueError, match=what):
            FaultCampaign(str(tmp_path / "absent.elf"), cpu_type="timing", **kw)
