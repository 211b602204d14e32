"""The profile of exact campaigns without a device (DESIGN.md 4j "Profile"):
the consumer rule and the host tables in a sanitized stand-alone program, and
fi_exact_class_consumers against a numpy restatement of the definitions on the
oracle's golden runs and on hand-made traces.

The numpy model below (np_tables, np_reg_consumers) is also what
tests/test_gpu_profile.py checks the device against."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, workload_elf
from test_exact_cpu import index_from_ops, np_classes

ECALL = 1 << 31


def test_profile_host_passes_sanitized(tmp_path):
    """tools/profile_host_check.cpp: fi_exact.h's consumer rule, the rows and the
    two tables on a hand-made trace, against values derived in its comments."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    exe = str(tmp_path / "profile_host_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tools", "profile_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "profile_host_check ok" in r.stdout


# ---- the numpy model, written from the definitions
def np_tables(trace):
    """-> (inst_val: the trace word of the instruction that commits as numInst
    t, t in [0, ninst); ecall_val: {numInst: the word of the first ecall entry
    there}).  An ecall commits nothing: its entry sits at the numInst of the
    instruction after it."""
    trace = np.asarray(trace, np.uint32)
    ecall = (trace >> 31) == 1
    t = np.cumsum(~ecall) - (~ecall)               # numInst before the entry
    ecall_val = {}
    for i in np.flatnonzero(ecall):
        ecall_val.setdefault(int(t[i]), int(trace[i]))
    return trace[~ecall], ecall_val


def np_reg_consumers(trace, off, ev, ninst, r):
    """The consumer of each of register r's classes, as a trace word: the
    entry that heads the class (it reads, u' > prev'); key ev >> 1 even (an
    ecall) -> the first ecall entry at the unclipped numInst ev >> 2, else the
    instruction that commits there."""
    inst_val, ecall_val = np_tables(trace)
    e = ev[off[r]:off[r + 1]].astype(np.int64)
    u = np.minimum(e >> 2, ninst - 1)
    prev = np.concatenate([[-1], u[:-1]])
    head = ((e & 1) == 1) & (u > prev)
    return np.array([ecall_val[x >> 2] if (x >> 1) & 1 == 0 else int(inst_val[x >> 2]) for x in e[head].tolist()],
                    np.uint32)


def synthetic_trace(ops):
    """A golden trace for the oracle's golden_ops(): the ecall bit from kind ==
    3, halfword ids that repeat so that entries share rows (instructions: the
    event index mod 37; ecalls: 100 + the event index mod 3)."""
    ecall = ops["kind"] == 3
    i = np.arange(len(ops))
    return np.where(ecall, ECALL | (100 + i % 3), i % 37).astype(np.uint32)


@pytest.mark.parametrize("name", ["hello", "fpamo", "crc32"])
def test_class_consumers_match_model(oracle_mod, name):
    from shrewd_amd import exact_class_consumers, exact_classes
    o = oracle_mod.Oracle(workload_elf(name), name)
    ninst = int(o.run_golden().ninst)
    ops = o.golden_ops()
    off, ev = index_from_ops(ops)
    trace = synthetic_trace(ops)
    assert int(((trace >> 31) == 0).sum()) == ninst
    total = to_ecall = 0
    for r in range(1, 32):
        got = exact_class_consumers(trace, off, ev, ninst, r)
        want = np_reg_consumers(trace, off, ev, ninst, r)
        assert np.array_equal(got, want), r
        c, _ = exact_classes(off, ev, ninst, r)
        assert len(got) == len(c), r
        total += len(got)
        to_ecall += int((got >> 31).sum())
    print(f"{name}: {total} classes over x1..x31, {to_ecall} charged to an ecall")
    assert total > 0 and to_ecall > 0            # (every workload's exit ecall reads a0 and a7)


# An index entry: (2 * numInst + !ecall) << 1 | reads
def E(t, ecall, reads):
    return ((2 * t + (0 if ecall else 1)) << 1) | int(reads)


# ninst = 10, every entry its own halfword: instructions 20 .. 29 commit as numInst 0 .. 9; an ecall
# (40) at numInst 3, two (41, 42) at numInst 6, the exit ecall (43) at numInst 10 == ninst
HAND_TRACE = np.array([20, 21, 22, ECALL | 40, 23, 24, 25, ECALL | 41, ECALL | 42, 26, 27, 28, 29, ECALL | 43],
                      np.uint32)
HAND = {
    # an ecall heads a class at the same numInst as an instruction that reads too; a write; the
    # exit ecall clipped to ninst - 1 heads the second class and is still charged to the ecall
    10: ([E(3, True, True), E(3, False, True), E(6, False, False), E(10, True, True)], [ECALL | 40, ECALL | 43]),
    # the last instruction heads the class; the exit ecall, clipped onto it, heads nothing
    11: ([E(9, False, True), E(10, True, True)], [29]),
    # a register whose only class is headed by the exit ecall
    12: ([E(10, True, True)], [ECALL | 43]),
    # two consecutive ecalls at one numInst: the first heads the class
    13: ([E(6, True, True), E(6, True, True)], [ECALL | 41]),
    # ... and a class headed by the second is charged to the first as well (the known imprecision)
    14: ([E(5, False, False), E(6, True, True)], [ECALL | 41]),
    # (x5: an empty register)
}


def hand_index():
    off, ev = [0], []
    for r in range(32):
        ev += HAND.get(r, ([], []))[0]
        off.append(len(ev))
    return np.array(off, np.uint32), np.array(ev, np.uint32)


def test_class_consumers_hand_made():
    from shrewd_amd import exact_class_consumers, exact_classes
    off, ev = hand_index()
    inst_val, ecall_val = np_tables(HAND_TRACE)
    assert inst_val.tolist() == list(range(20, 30)) and ecall_val == {3: ECALL | 40, 6: ECALL | 41, 10: ECALL | 43}
    for r in range(1, 32):
        got = exact_class_consumers(HAND_TRACE, off, ev, 10, r)
        assert got.tolist() == HAND.get(r, ([], []))[1], r
        assert np.array_equal(got, np_reg_consumers(HAND_TRACE, off, ev, 10, r)), r
        c, _ = exact_classes(off, ev, 10, r)
        inst, _, _ = np_classes(off, ev, 10, r)
        assert len(got) == len(c) and np.array_equal(c["inst"], inst)
        # the order is the classes': a consumer's numInst, clipped, is its class's instant
        when = {int(w): t for t, w in enumerate(inst_val)} | {w: t for t, w in ecall_val.items()}
        assert [min(when[int(g)], 9) for g in got] == c["inst"].tolist(), r
    assert len(exact_class_consumers(HAND_TRACE, off, ev, 10, 5)) == 0


def test_class_consumers_rejects_bad_arguments():
    from shrewd_amd import EngineError, exact_class_consumers
    off, ev = hand_index()
    for reg in (0, 32):
        with pytest.raises(EngineError):
            exact_class_consumers(HAND_TRACE, off, ev, 10, reg)
    with pytest.raises(EngineError):               # the trace holds 10 committing entries, not 11
        exact_class_consumers(HAND_TRACE, off, ev, 11, 10)


def test_python_names_import_without_a_device():
    import shrewd_amd
    from shrewd_amd import Engine, FaultCampaign
    from shrewd_amd.fi import N_PROFILE_GROUP, PROFILE_GROUP_NAMES, PROFILE_ROW_DT, allreduce_profile
    assert callable(shrewd_amd.exact_class_consumers) and callable(allreduce_profile)
    for n in ("profile_rows", "exact_consumers", "run_exact"):
        assert callable(getattr(Engine, n))
    assert callable(FaultCampaign.profile)
    assert PROFILE_ROW_DT.itemsize == 24 and N_PROFILE_GROUP == len(PROFILE_GROUP_NAMES) == 4


def test_allreduce_profile_keeps_shape_and_values():
    """One rank (gloo): the all-reduce of a profile is the profile, uint64
    values past 2^63 included."""
    import socket
    import torch.distributed as dist
    from shrewd_amd.fi import allreduce_profile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    prof = (np.arange(5 * 4 * 6, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)).reshape(5, 4, 6)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        got = allreduce_profile(prof)
    finally:
        dist.destroy_process_group()
    assert got.dtype == np.uint64 and got.shape == prof.shape and np.array_equal(got, prof)


def test_config_script_profile_argument(monkeypatch, tmp_path):
    """configs/fi_campaign.py --profile FILE: only with --exact; reaches the
    ctypes FaultCampaign as profile=True and writes its profile() as JSON."""
    import importlib.util
    import json
    import shrewd_amd
    spec = importlib.util.spec_from_file_location("fi_campaign_cfg", os.path.join(ROOT, "configs", "fi_campaign.py"))
    cfg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfg)
    with pytest.raises(SystemExit):
        cfg.parse(["--workload", "w.elf", "--profile", "p.json"])
    assert cfg.parse(["--workload", "w.elf", "--exact"]).profile == ""
    seen = {}
    rows = [{"pc": 65536, "raw": 0x73, "inst_group": "system", "execs": 1, "ecall": 1,
             "counts": {"int_reg": {"sdc": 3}}, "share": {"int_reg": {"sdc": 0.5}}}]

    class FakeCampaign:
        def __init__(self, workload, **kw):
            seen.update(kw, workload=workload)

        def run_exact(self):
            seen["ran_exact"] = True

        def summary(self):
            return {"trials": 6}

        def vulnerability(self):
            return {}

        def profile(self):
            return rows

    monkeypatch.setattr(shrewd_amd, "FaultCampaign", FakeCampaign)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "p.json"
    cfg.run_ctypes(cfg.parse(["--workload", "w.elf", "--exact", "--profile", str(out)]))
    assert seen["ran_exact"] and seen["profile"] is True
    assert json.loads(out.read_text()) == rows
    seen.clear()
    cfg.run_ctypes(cfg.parse(["--workload", "w.elf", "--exact"]))
    assert seen["profile"] is False
