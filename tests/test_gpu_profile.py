"""The profile of exact campaigns on the device (fi_run_exact_profile, DESIGN.md
4j "Profile"): the fault space attributed to the static instructions that
consume the faults, against numpy recomputations from the definitions.  Integer
equality throughout."""
import ctypes

import numpy as np
import pytest

from conftest import workload_elf
from test_exact_cpu import ALL_BITS, REGS, index_from_ops
from test_gpu_exact import CRC_BITS, CRC_STRUCT, MEM, PC, RESULT, campaign, oracle_for, same_hist, same_outcomes
from test_profile_cpu import ECALL, np_reg_consumers, np_tables

pytestmark = pytest.mark.gpu

BITS3 = (1 << 0) | (1 << 12) | (1 << 63)


def groups_of(sites):
    """0 = x1..x31, 1 = the pc (32), 2 = memory words (33), 3 = a result (34)"""
    t = sites["target"].astype(np.int64)
    return np.where(t < 32, 0, t - 31)


def np_profile(n_rows, cons, sites, weights, outcomes):
    prof = np.zeros((n_rows, 4, 6), np.uint64)
    cls = np.where(outcomes["cls"] < 6, outcomes["cls"], 5).astype(np.int64)
    np.add.at(prof, (cons.astype(np.int64), groups_of(sites), cls), weights.astype(np.uint64))
    return prof


def row_trace(e):
    """The golden trace with each entry's row in place of its halfword (bit 31
    stays the ecall flag) -> (that, the rows' halfwords ascending)"""
    _, tr, _ = e.debug_golden_trace()
    half = np.unique(tr & 0x7FFFFFFF)
    return (np.searchsorted(half, tr & 0x7FFFFFFF) | (tr & ECALL)).astype(np.uint32), half


def np_consumers(e, o, structures, nbits):
    """exact_consumers over a whole campaign without memory words, from the
    golden trace and the definitions: per selected structure ascending, per
    class in time order, nbits trials each."""
    rt, _ = row_trace(e)
    ninst = int(e.golden.ninst)
    off, ev = index_from_ops(o.golden_ops())
    inst_row, _ = np_tables(rt)
    per = []
    for s in range(1, 35):
        if not (structures >> s) & 1:
            continue
        per.append(np_reg_consumers(rt, off, ev, ninst, s) if s < 32 else inst_row[:ninst])
    return np.repeat(np.concatenate(per) & 0x7FFFFFFF, nbits).astype(np.uint32)


def invariant(prof, hist, dead):
    """Per group g and class c: the rows' counts summed + (masked: g's dead
    sites) == the histogram over g's structures and all bits.  dead = {group: sites}"""
    h = hist["counts"]
    per_group = {0: h[1:32].sum(axis=(0, 1)), 1: h[32].sum(axis=0), 2: h[33].sum(axis=0), 3: h[34].sum(axis=0)}
    for g in range(4):
        want = per_group[g].astype(np.int64).copy()
        got = prof[:, g, :].sum(axis=0).astype(np.int64)
        got[0] += dead.get(g, 0)
        assert np.array_equal(got, want), (g, got, want)


def profiled(e, n):
    """run_exact(profile=True) over the whole campaign with its sites, weights
    and consumers -> (outcomes, hist, prof, sites, weights, consumers, rows)"""
    out, h, prof = e.run_exact(0, n, profile=True)
    sites, w = e.exact_sites(0, n)
    cons = e.exact_consumers(0, n)
    rows = e.profile_rows()
    assert prof.shape == (len(rows), 4, 6) and prof.dtype == np.uint64
    assert int(cons.max()) < len(rows)
    return out, h, prof, sites, w, cons, rows


def test_hello_whole_space(engine_factory, oracle_mod):
    """x1..x31 | pc | result, every bit: about 1.9 k trials, a 256-thread block
    spans several structures and groups."""
    e = engine_factory("hello")
    o = oracle_for(oracle_mod, "hello")
    structures = REGS | PC | RESULT
    x = campaign(e, structures)
    n, ninst = int(x.trials), int(e.golden.ninst)
    plain_out, plain_h = e.run_exact(0, n)
    out, h, prof, sites, w, cons, rows = profiled(e, n)
    same_outcomes(out, plain_out, sites, "profile=True vs run_exact")
    same_hist(h, plain_h, "profile=True vs run_exact")
    assert np.array_equal(prof, np_profile(len(rows), cons, sites, w, out))
    assert np.array_equal(cons, np_consumers(e, o, structures, 64))
    invariant(prof, h, {0: int(x.dead_sites)})
    # the rows
    _, tr, lo = e.debug_golden_trace()
    assert (np.diff(rows["pc"].astype(np.int64)) > 0).all()
    assert int(rows["execs"].sum()) == len(tr)
    assert np.array_equal(rows["pc"], lo + 2 * np.unique(tr & 0x7FFFFFFF).astype(np.uint64))
    assert rows["ecall"].any() and (rows["raw"][rows["ecall"] == 1] == 0x73).all()
    assert np.isin(rows["len"], (2, 4)).all()
    # at least one register class is charged to an ecall row
    reg = sites["target"] < 32
    assert rows["ecall"][cons[reg]].any()
    # a result trial is charged to the instruction that commits at its t, also when that one writes no
    # integer register (flags bit 0 clear: nothing was flipped)
    rt, _ = row_trace(e)
    inst_row, _ = np_tables(rt)
    res = sites["target"] == 34
    assert np.array_equal(cons[res], inst_row[sites["inst"][res].astype(np.int64)])
    none = res & ((out["flags"] & 1) == 0)
    assert (out["cls"][none] == 0).all()
    print(f"hello: {len(rows)} rows, {n} trials, {int(prof.sum())} live sites, "
          f"{int(prof[rows['ecall'] == 1].sum())} charged to ecalls")


def test_hello_chunks_and_ranges(engine_factory):
    """Chunks of 1000 trials (a boundary inside a class) and three ranges sum to
    the one-call profile; an empty range at 0 adds the dead sites to the
    histogram and nothing to the profile."""
    e = engine_factory("hello")
    c = engine_factory("hello", max_trials_per_launch=1000)
    structures = REGS | PC | RESULT
    n = int(campaign(e, structures).trials)
    assert int(campaign(c, structures).trials) == n and n > 1201 and 1000 % 64
    _, h, prof = e.run_exact(0, n, profile=True)
    _, ch, cprof = c.run_exact(0, n, profile=True)
    same_hist(ch, h, "chunked vs one launch")
    assert np.array_equal(cprof, prof)
    total = np.zeros_like(prof)
    for lo, hi in ((0, 333), (333, 1201), (1201, n)):
        _, _, p = c.run_exact(lo, hi - lo, want_outcomes=False, profile=True)
        total += p
    assert np.array_equal(total, prof)
    _, h0, p0 = e.run_exact(0, 0, profile=True)
    assert int(h0["trials"]) > 0 and not p0.any()


@pytest.mark.parametrize("bits,burst", [(BITS3, 1), (ALL_BITS, 4)])
def test_fpamo_runs_straddle_waves(engine_factory, bits, burst):
    """{sp, s0, a0, a5}: nbits = 3 and 61, neither divides 64: a class's lanes
    straddle waves and workgroups."""
    e = engine_factory("fpamo")
    x = campaign(e, (1 << 2) | (1 << 8) | (1 << 10) | (1 << 15), bits, burst)
    assert 64 % int(x.nbits)
    out, h, prof, sites, w, cons, rows = profiled(e, int(x.trials))
    assert np.array_equal(prof, np_profile(len(rows), cons, sites, w, out))
    invariant(prof, h, {0: int(x.dead_sites)})


def test_crc32_many_rows_per_block(engine_factory):
    """pc | result, the single bit 12: consecutive lanes hit consecutive,
    different instructions, and some workgroup meets more rows than the
    kernel's LDS table holds, so the direct-to-global path runs."""
    from shrewd_amd.fi import lib
    e = engine_factory("crc32")
    x = campaign(e, PC | RESULT, 1 << 12)
    n = int(x.trials)
    assert int(x.nbits) == 1 and n == 2 * int(e.golden.ninst)
    out, h, prof, sites, w, cons, rows = profiled(e, n)
    assert np.array_equal(prof, np_profile(len(rows), cons, sites, w, out))
    invariant(prof, h, {})
    # a result trial at a store or a branch -- no integer register written (the pre-decoded text: flag
    # kPreRd = 16 with rd != 0) -- flips nothing: masked, and still charged to that instruction
    pre, tr, _ = e.debug_golden_trace()
    rt, _ = row_trace(e)
    inst_row, _ = np_tables(rt)
    half = tr[(tr >> 31) == 0].astype(np.int64)                  # the halfword of the instruction at numInst t
    writes = ((pre[half, 13] & 16) != 0) & (pre[half, 5] != 0)
    res = sites["target"] == 34
    t = sites["inst"].astype(np.int64)
    none = res & ~writes[np.minimum(t, len(writes) - 1)]
    assert none.any() and (out["cls"][none] == 0).all()
    assert ((out["flags"][res & ~none] & 1) == 1).all()
    assert (out["cls"][res & ((out["flags"] & 1) == 0)] == 0).all()
    assert np.array_equal(cons[res], inst_row[t[res]])
    assert (prof[np.unique(cons[none]), 3, 0] > 0).all()
    slots = int(lib().fi_debug_profile_slots())
    assert e.config()["max_trials_per_launch"] % 256 == 0      # a workgroup's 256 trials: an aligned window
    most = max(len(np.unique(cons[i:i + 256])) for i in range(0, n, 256))
    print(f"crc32 pc | result: {len(rows)} rows, at most {most} in a workgroup, {slots} table slots")
    assert slots > 0 and most > slots


def test_crc32_hot_rows(engine_factory):
    """{a0, a1, t6} x bits {0, 12, 40}: the loops' few instructions take almost
    all the weight."""
    e = engine_factory("crc32")
    x = campaign(e, CRC_STRUCT, CRC_BITS)
    out, h, prof, sites, w, cons, rows = profiled(e, int(x.trials))
    assert np.array_equal(prof, np_profile(len(rows), cons, sites, w, out))
    invariant(prof, h, {0: int(x.dead_sites)})
    per_row = prof.sum(axis=(1, 2))
    top = np.sort(per_row)[::-1]
    print(f"crc32 three registers: {int(x.trials)} trials, top 4 rows hold {int(top[:4].sum())} of {int(top.sum())}")
    assert int(top[:8].sum()) * 10 > int(top.sum()) * 9


def test_hello_memory(engine_factory):
    """mem | x1..x31: memory classes carry their consumer; the memory index is
    what an engine that never profiled returns."""
    from shrewd_amd import Engine
    e = Engine()
    try:
        e.load_elf(workload_elf("hello"), ["hello"])
        e.golden_run()
        e.set_exact_memory(True)
        before = e.golden_mem_index()                   # (nothing was profiled yet)
        x = campaign(e, MEM | REGS)
        n = int(x.trials)
        plain_out, plain_h = e.run_exact(0, n)          # (the classes are first built unprofiled, then again)
        out, h, prof, sites, w, cons, rows = profiled(e, n)
        same_outcomes(out, plain_out, sites, "profile=True vs run_exact")
        same_hist(h, plain_h, "profile=True vs run_exact")
        assert np.array_equal(prof, np_profile(len(rows), cons, sites, w, out))
        mi = e.exact_mem_info()
        mem_dead = sum(int(mi.set[g].dead_sites) for g in range(int(mi.byte_sets)))
        invariant(prof, h, {0: int(x.dead_sites) - mem_dead, 2: mem_dead})
        # a memory class's consumer: the instruction at the heading event's numInst, or an ecall row
        # standing there; the former where no ecall entry stands at that numInst
        rt, _ = row_trace(e)
        inst_row, ecall_row = np_tables(rt)
        addr, off, ev = e.golden_mem_index()
        ninst = int(e.golden.ninst)
        mem = np.flatnonzero(sites["target"] == 33)
        assert len(mem) and prof[:, 2].any()
        to_ecall = 0
        for k in mem.tolist():
            wd = int(np.searchsorted(addr, sites["addr"][k]))
            assert addr[wd] == sites["addr"][k]
            us = (ev[off[wd]:off[wd + 1]] >> np.uint64(16)).astype(np.int64)
            heads = np.unique(us[np.minimum(us, ninst - 1) == int(sites["inst"][k])])
            ok = set()
            for u in heads.tolist():
                if u < ninst:
                    ok.add(int(inst_row[u]))
                if u in ecall_row:
                    ok.add(ecall_row[u] & 0x7FFFFFFF)
                else:
                    assert u < ninst
            assert int(cons[k]) in ok, (k, sites[k], cons[k], ok)
            if not any(u in ecall_row for u in heads.tolist()):
                assert rows["ecall"][cons[k]] == 0
            to_ecall += int(rows["ecall"][cons[k]])
        print(f"hello memory: {len(mem)} memory trials, {to_ecall} charged to an ecall")
        assert to_ecall > 0                              # write(1, msg, n) reads the message
        for a, b, c in zip(e.golden_mem_index(), before, engine_factory("hello").golden_mem_index()):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    finally:
        e.close()


def test_refusals(engine_factory):
    from shrewd_amd import HIST_DT, Engine
    from shrewd_amd.fi import FI_E_ARG, FI_E_STATE, FI_OK
    e = engine_factory("hello")
    x = campaign(e, REGS)
    rows = len(e.profile_rows())
    hist = np.zeros(1, HIST_DT)
    prof = np.zeros((rows + 1, 4, 6), np.uint64)
    for bad in (rows + 1, rows - 1, 0):
        assert e.L.fi_run_exact_profile(e.h, 0, 0, None, hist.ctypes.data, prof.ctypes.data, bad) == FI_E_ARG
        assert e.L.fi_last_error(e.h).decode().strip()
    assert e.L.fi_run_exact_profile(e.h, 0, 0, None, hist.ctypes.data, None, rows) == FI_E_ARG
    assert e.L.fi_run_exact_profile(e.h, 0, int(x.trials) + 1, None, None, prof.ctypes.data, rows) == FI_E_ARG
    assert e.L.fi_exact_consumers(e.h, int(x.trials), 1, prof.ctypes.data) == FI_E_ARG
    assert e.L.fi_run_exact_profile(e.h, 0, 0, None, hist.ctypes.data, prof.ctypes.data, rows) == FI_OK
    assert not prof.any()
    timing = Engine()
    try:
        timing.load_elf(workload_elf("hello"), ["hello"])
        timing.set_cpu_model("timing")
        timing.golden_run()
        timing.set_campaign(0xE8AC7, REGS, 1)
        n = ctypes.c_uint64()
        assert timing.L.fi_profile_rows(timing.h, None, 0, ctypes.byref(n)) == FI_E_STATE
        assert timing.L.fi_exact_consumers(timing.h, 0, 0, None) == FI_E_STATE
        assert timing.L.fi_run_exact_profile(timing.h, 0, 0, None, None, prof.ctypes.data, rows) == FI_E_STATE
        assert timing.L.fi_run_exact(timing.h, 0, 0, None, None) == FI_E_STATE
    finally:
        timing.close()


def test_fault_campaign_profile(tmp_path):
    """FaultCampaign(profile=True): run_exact() keeps the profile; profile() is
    sorted by the chosen class, carries counts and shares of the space, and
    sums with the dead sites to the histogram.  The config script writes the
    same list."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from shrewd_amd import FaultCampaign
    from shrewd_amd.fi import inst_group
    elf = os.path.join(ROOT, "workloads", "hello.elf")
    c = FaultCampaign(elf, cmd=["hello"], structures=("int_reg", "pc"), profile=True)
    try:
        with pytest.raises(ValueError):
            c.profile()
        c.run_exact()
        x = c.engine.exact_info()
        rows = c.profile()
        assert rows and len(c.profile(sort="crash")) == len(rows)
        key = [sum(g.get("sdc", 0) for g in r["counts"].values()) for r in rows]
        assert key == sorted(key, reverse=True)
        total = np.zeros(6, np.int64)
        for r in rows:
            assert r["inst_group"] == inst_group(r["raw"]) and r["execs"] >= 1 and set(r["counts"]) <= {"int_reg", "pc"}
            for g, d in r["counts"].items():
                total += np.array([d[k] for k in ("masked", "sdc", "crash", "hang", "detected", "escape")])
                assert all(abs(r["share"][g][k] * int(x.space) - v) < 1e-3 for k, v in d.items())
        total[0] += int(x.dead_sites)
        assert np.array_equal(total, c.histogram()["counts"].sum(axis=(0, 1)).astype(np.int64))
        assert any(r["ecall"] and r["raw"] == 0x73 for r in rows)
    finally:
        c.engine.close()
    out = tmp_path / "prof.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "configs", "fi_campaign.py"), "--workload", elf, "--cmd", "hello",
                        "--structures", "int_reg,pc", "--exact", "--profile", str(out)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(out.read_text()) == json.loads(json.dumps(rows))
