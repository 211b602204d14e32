"""Exact campaigns over memory words on the device (fi_set_exact_memory,
DESIGN.md 4j "Memory words"): one trial per byte-liveness class, weighted,
against the engine's and the oracle's brute force, the numpy model of
tests/test_exact_mem_cpu.py and the sampled path."""
import contextlib
import os

import numpy as np
import pytest

from conftest import ROOT, np_histogram, workload_elf
from test_exact_cpu import ALL_BITS, REGS, all_sites, index_from_ops, np_exact_sites, np_weighted_histogram, positions
from test_exact_mem_cpu import (FPAMO_BITS, MEM, T_MEM, add_mem_dead, all_mem_sites, byte_sets, golden_index, mem_class_of,
                                np_mem_exact_sites, np_mem_intervals, space_words)

pytestmark = pytest.mark.gpu

PC, RESULT = 1 << 32, 1 << 34
FIELDS = ("counts", "crash_sub", "escape_sub", "trials", "guest_insts")
SEED = 0xE8AC7
THREADS = min(16, os.cpu_count() or 1)


def oracle_for(oracle_mod, name):
    o = oracle_mod.Oracle(workload_elf(name), name)
    o.run_golden()
    return o


def same_hist(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f"{what}: {f} differs"


def same_outcomes(dev, ref, sites, what):
    bad = np.flatnonzero(dev != ref)
    assert not len(bad), (f"{what}: {len(bad)} of {len(sites)} outcomes differ; first: site={sites[bad[0]]} "
                          f"got={dev[bad[0]]} want={ref[bad[0]]}")


def select(e, structures, bits=ALL_BITS, burst=1):
    e.set_campaign(SEED, structures, burst)
    e.set_bits(bits)
    e.set_protect(0)


def campaign(e, structures, bits=ALL_BITS, burst=1):
    select(e, structures, bits, burst)
    return e.exact_info()


@contextlib.contextmanager
def brute_engine(name):
    """An engine of its own for a brute force over millions of sites, closed
    afterwards: an engine's work buffers grow to its largest launch (64 KiB of
    private pages per trial slot) and stay until it is closed, and the
    session's cached engines must leave room for the tests that start other
    processes on the same device."""
    from shrewd_amd import Engine
    e = Engine(max_trials_per_launch=1 << 17)
    try:
        e.load_elf(workload_elf(name), [name])
        e.golden_run()
        yield e
    finally:
        e.close()


def pages_of(e):
    """The memory-fault candidate pages, as the sampler draws them."""
    e.set_campaign(SEED, MEM, 1)
    e.set_bits(ALL_BITS)
    return sorted(set((e.sample(0, 20000)["addr"] & ~np.uint64(4095)).tolist()))


def model(e, o, structures, bits, burst):
    """The numpy model's exact trials of a campaign with memory on, in trial-id
    order -> (sites, weights, register dead {r: t}, memory dead {b: pairs},
    the trials before memory, memory's trials)"""
    ninst = int(e.golden.ninst)
    off, ev = index_from_ops(o.golden_ops())
    base, bw, rdead = np_exact_sites(off, ev, ninst, structures & ~MEM, bits, burst)
    nres = ninst * len(positions(bits, burst)) if structures & RESULT else 0
    cut = len(base) - nres
    ms, mw, mdead, _ = np_mem_exact_sites(e.golden_mem_index(), ninst, pages_of(e), bits, burst)
    sites = np.concatenate([base[:cut], ms, base[cut:]])
    sites["trial"] = np.arange(len(sites)) & 0xFFFFFFFF
    return sites, np.concatenate([bw[:cut], mw, bw[cut:]]), rdead, mdead, cut, len(ms)


@pytest.mark.parametrize("name", ["hello", "fpamo"])
def test_recorded_index_is_the_engines(engine_factory, name):
    """tests/golden/mem_index_*.npz (what the CPU premise tests run on) is
    still exactly the engine's memory index and candidate pages."""
    e = engine_factory(name)
    (addr, off, ev), pages = golden_index(name)
    a, o, v = e.golden_mem_index()
    assert np.array_equal(a, addr) and np.array_equal(o, off) and np.array_equal(v, ev)
    assert pages_of(e) == pages


@pytest.mark.parametrize("bits,burst", [(ALL_BITS, 1), (ALL_BITS, 4), ((1 << 0) | (1 << 7) | (1 << 12) | (1 << 63), 2)])
def test_hello_whole_space(engine_factory, oracle_mod, bits, burst):
    """x1..x31 | pc | memory | result: run_exact equals the engine's and the
    oracle's brute force over every site; exact_sites equals the model's sites
    and weights; register, pc and result trials are those of the campaign
    without memory.  Burst 2 at position 7 spans two bytes."""
    e = engine_factory("hello")
    o = oracle_for(oracle_mod, "hello")
    structures = REGS | PC | MEM | RESULT
    ninst = int(e.golden.ninst)
    try:
        e.set_exact_memory(True)
        sites, w, rdead, mdead, cut, nmem = model(e, o, structures, bits, burst)
        x = campaign(e, structures, bits, burst)
        m = e.exact_mem_info()
        nb = len(positions(bits, burst))
        assert int(x.trials) == len(sites) and int(x.nbits) == nb and nmem > 0
        assert int(m.text_words) == 0 and int(m.words) == 1024 and int(m.byte_sets) == len(byte_sets(bits, burst))
        assert int(x.classes[T_MEM]) == sum(int(g.classes) for g in m.set[:m.byte_sets])
        assert int(x.dead_sites) == nb * sum(rdead.values()) + sum(mdead.values())
        assert sum(int(g.dead_sites) for g in m.set[:m.byte_sets]) == sum(mdead.values())
        got, gw = e.exact_sites(0, len(sites))
        assert np.array_equal(got, sites) and np.array_equal(gw, w)
        lo = cut + 3                                   # a range that starts inside a memory class
        got, gw = e.exact_sites(lo, nmem - 3 + 5)      # ... and ends in the result's trials
        assert np.array_equal(got, sites[lo:cut + nmem + 5]) and np.array_equal(gw, w[lo:cut + nmem + 5])
        out, h = e.run_exact(0, int(x.trials))
        space = np.concatenate([all_sites(ninst, structures & ~MEM, bits, burst),
                                all_mem_sites(space_words(pages_of(e)), ninst, bits, burst)])
        assert int(x.space) == len(space)
        with brute_engine("hello") as b:
            select(b, structures, bits, burst)
            _, bh = b.run_sites(space)
        same_hist(h, bh, "exact vs the engine's brute force")
        assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
        same_hist(h, np_histogram(space, o.run_trials(space, threads=THREADS)), "exact vs the oracle's brute force")
        same_outcomes(out, o.run_trials(sites, threads=THREADS), sites, "exact trials vs the oracle at the representatives")
        hw = add_mem_dead(np_weighted_histogram(sites, out, w, rdead, bits, burst, ninst), mdead, ninst)
        same_hist(h, hw, "device vs numpy weighted histogram")
    finally:
        e.set_exact_memory(False)
    # the same campaign without memory: the same sites under the same ids, the result's moved down
    y = campaign(e, structures & ~MEM, bits, burst)
    assert int(y.trials) == len(sites) - nmem
    off_sites, off_w = e.exact_sites(0, int(y.trials))
    on = np.concatenate([sites[:cut], sites[cut + nmem:]])
    for f in ("inst", "mask", "addr", "target"):
        assert np.array_equal(off_sites[f], on[f]), f
    assert np.array_equal(off_sites["trial"][:cut], on["trial"][:cut])
    assert np.array_equal(off_w, np.concatenate([w[:cut], w[cut + nmem:]]))
    print(f"hello burst {burst}: {x.space} sites, {x.trials} exact trials ({nmem} memory), {x.dead_sites} dead")


def test_hello_chunks_and_ranges(engine_factory):
    """Chunks of 1000 trials and three ranges cut inside memory classes give
    the one-call result, the dead sites once; an empty range at 0 adds exactly
    the dead sites."""
    from shrewd_amd.fi import HIST_DT
    e = engine_factory("hello")
    c = engine_factory("hello", max_trials_per_launch=1000)
    structures = REGS | PC | MEM | RESULT
    try:
        e.set_exact_memory(True)
        c.set_exact_memory(True)
        x = campaign(e, structures)
        n = int(x.trials)
        m0 = 64 * sum(int(v) for v in x.classes[1:33])         # memory's first trial
        nmem = n - m0 - 64 * int(e.golden.ninst)
        cuts = (m0 + 13, m0 + (nmem // 2 | 1), m0 + nmem - 3)  # burst 1: a memory class is 8 trials from m0 on
        assert n > 1000 and all((k - m0) % 8 for k in cuts) and m0 < cuts[0] < cuts[1] < cuts[2] < m0 + nmem
        out, h = e.run_exact(0, n)
        assert int(campaign(c, structures).trials) == n
        cout, ch = c.run_exact(0, n)
        same_outcomes(cout, out, cout, "chunked vs one launch")
        same_hist(ch, h, "chunked vs one launch")
        parts, total = [], np.zeros(1, HIST_DT)[0]
        for lo, hi in zip((0,) + cuts, cuts + (n,)):
            po, ph = c.run_exact(lo, hi - lo)
            parts.append(po)
            for f in FIELDS:
                total[f] += ph[f]
        same_outcomes(np.concatenate(parts), out, out, "ranges vs one call")
        same_hist(total, h, "ranges vs one call")
        _, h0 = e.run_exact(0, 0)
        dead, ninst = int(x.dead_sites), int(e.golden.ninst)
        assert dead > 0 and int(h0["trials"]) == dead and int(h0["guest_insts"]) == dead * ninst
        assert int(h0["counts"][:, :, 0].sum()) == dead == int(h0["counts"].sum())
        assert int(h0["counts"][T_MEM].sum()) == sum(int(g.dead_sites) for g in e.exact_mem_info().set) > 0
        _, h1 = e.run_exact(1, 0)
        assert int(h1["trials"]) == 0 and not h1["counts"].any()
    finally:
        e.set_exact_memory(False)
        c.set_exact_memory(False)


def test_fpamo_memory_alone(engine_factory, oracle_mod):
    """Memory words alone at eight positions, through FP and AMO code: exact
    equals the engine's brute force over 2 x 512 x 848 x 8 sites, the
    representatives equal the oracle, and an AMO's event heads a live class."""
    e = engine_factory("fpamo")
    o = oracle_for(oracle_mod, "fpamo")
    ninst = int(e.golden.ninst)
    try:
        e.set_exact_memory(True)
        pages = pages_of(e)
        x = campaign(e, MEM, FPAMO_BITS)
        assert int(x.space) == 2 * 512 * 848 * 8 and int(e.exact_mem_info().text_words) == 0
        out, h = e.run_exact(0, int(x.trials))
        sites, w = e.exact_sites(0, int(x.trials))
        space = all_mem_sites(space_words(pages), ninst, FPAMO_BITS)
        assert len(space) == int(x.space)
        with brute_engine("fpamo") as b:
            select(b, MEM, FPAMO_BITS)
            _, bh = b.run_sites(space)
        same_hist(h, bh, "exact vs the engine's brute force")
        assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
        same_outcomes(out, o.run_trials(sites, threads=THREADS), sites, "exact trials vs the oracle")
        ms, mw, _, _ = np_mem_exact_sites(e.golden_mem_index(), ninst, pages, FPAMO_BITS)
        assert np.array_equal(sites, ms) and np.array_equal(w, mw)
    finally:
        e.set_exact_memory(False)
    addr, off, ev = e.golden_mem_index()
    both = (ev >> np.uint64(8)) & ev & np.uint64(0xFF)
    hits = 0
    for i in np.flatnonzero(both):                     # events that read and write the same bytes
        word = addr[np.searchsorted(off, i, side="right") - 1]
        t = min(int(ev[i] >> np.uint64(16)), ninst - 1)
        for b in positions(FPAMO_BITS, 1):
            if (int(both[i]) >> (b // 8)) & 1:
                hits += int(((sites["addr"] == word) & (sites["inst"] == t) & (sites["mask"] == np.uint64(1 << b))).any())
    assert both.any() and hits > 0


CRC_BITS = (1 << 0) | (1 << 12) | (1 << 40)


@pytest.fixture(scope="module")
def crc32_mem(engine_factory):
    """The crc32 memory campaign, run once for the tests below."""
    e = engine_factory("crc32")
    try:
        e.set_exact_memory(True)
        pages = pages_of(e)
        x = campaign(e, MEM, CRC_BITS)
        out, h = e.run_exact(0, int(x.trials))
        sites, w = e.exact_sites(0, int(x.trials))
        info = e.exact_mem_info().as_dict()
    finally:
        e.set_exact_memory(False)
    return e, x, pages, sites, w, out, h, info


def test_crc32_memory(crc32_mem, engine_factory, oracle_mod):
    """The whole space cannot be brute-forced: sites at a random t inside 300
    classes and 300 dead intervals equal the representative or the masked
    golden run; an engine without forwarding gives identical outcomes; the
    oracle agrees on 3,000 representatives."""
    e, x, pages, sites, w, out, h, info = crc32_mem
    ninst = int(e.golden.ninst)
    index = e.golden_mem_index()
    addr, off, ev = index
    ms, mw, mdead, n_words = np_mem_exact_sites(index, ninst, pages, CRC_BITS)
    assert np.array_equal(sites, ms) and np.array_equal(w, mw)
    assert info["text_words"] == 0 and info["words"] == n_words and int(x.space) == n_words * ninst * 3
    assert int(x.dead_sites) == sum(mdead.values()) and int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
    rng = np.random.default_rng(SEED)
    # 300 classes spread over the trial range, a random t of each
    pick = np.linspace(0, len(sites) - 1, 300).astype(np.int64)
    inside = sites[pick].copy()
    inside["inst"] = (inside["inst"].astype(np.int64) - rng.integers(0, w[pick].astype(np.int64))).astype(np.uint64)
    # 300 dead intervals: of the words the index lists (before a store, after the last access) and of others
    dead = []
    words = space_words(pages)
    listed = np.flatnonzero(np.isin(addr, words))
    for f, pos in byte_sets(CRC_BITS, 1):
        for i in listed[np.linspace(0, len(listed) - 1, 400).astype(np.int64)]:
            u, prev, cls = np_mem_intervals(ev[off[i]:off[i + 1]], ninst, f)
            lo, hi = list(prev[~cls]), list(u[~cls])
            if (u[-1] if len(u) else -1) < ninst - 1:
                lo.append(u[-1] if len(u) else -1)
                hi.append(ninst - 1)
            dead += [(int(addr[i]), pos[0], int(a), int(b)) for a, b in zip(lo, hi)]
    rest = words[~np.isin(words, addr)]
    dead += [(int(a), 12, -1, ninst - 1) for a in rest[np.linspace(0, len(rest) - 1, 20).astype(np.int64)]]
    assert len(dead) >= 300
    dead = [dead[i] for i in np.linspace(0, len(dead) - 1, 300).astype(np.int64)]
    ds = inside[:len(dead)].copy()
    ds["addr"] = [d[0] for d in dead]
    ds["mask"] = [1 << d[1] for d in dead]
    ds["inst"] = [int(rng.integers(d[2] + 1, d[3] + 1)) for d in dead]
    assert (mem_class_of(sites, w, ds) < 0).all() and np.array_equal(mem_class_of(sites, w, inside), pick)
    select(e, MEM, CRC_BITS)
    got, _ = e.run_sites(np.concatenate([inside, ds]))
    same_outcomes(got[:300], out[pick], inside, "a site inside a class vs its representative")
    d = got[300:]
    assert (d["cls"] == 0).all() and (d["ninst"] == ninst).all()
    f = engine_factory("crc32", flags=512)                 # FI_CFG_NO_FORWARD
    try:
        f.set_exact_memory(True)
        assert int(campaign(f, MEM, CRC_BITS).trials) == int(x.trials)
        fout, fh = f.run_exact(0, int(x.trials))
    finally:
        f.set_exact_memory(False)
    same_outcomes(fout, out, sites, "FI_CFG_NO_FORWARD vs default")
    same_hist(fh, h, "FI_CFG_NO_FORWARD vs default")
    pick = np.linspace(0, len(sites) - 1, 3000).astype(np.int64)
    o = oracle_for(oracle_mod, "crc32")
    same_outcomes(out[pick], o.run_trials(sites[pick], threads=THREADS), sites[pick], "exact trials vs the oracle")
    print(f"crc32 memory: {x.space} sites, {x.trials} exact trials, {x.dead_sites} dead, "
          f"{info['index_words']} index words, build {info['build_ms']:.2f} ms")


def test_sampled_memory_sites_fall_into_their_classes(crc32_mem):
    """3,000 sampled memory sites of the same campaign: each one's outcome is
    the exact outcome of the class that contains it; a site in no class is a
    masked golden run.  At least 500 of each."""
    e, x, pages, sites, w, out, _, _ = crc32_mem
    select(e, MEM, CRC_BITS)
    s = e.sample(0, 3000)
    assert (s["target"] == T_MEM).all()
    so, _ = e.run_trials(0, 3000)
    cl = mem_class_of(sites, w, s)
    live = cl >= 0
    print(f"sampled: {int(live.sum())} in a class, {int((~live).sum())} dead, {int((so['cls'] != 0).sum())} not masked")
    assert int(live.sum()) >= 500 and int((~live).sum()) >= 500
    same_outcomes(so[live], out[cl[live]], s[live], "sampled sites vs their classes")
    d = so[~live]
    assert (d["cls"] == 0).all() and (d["ninst"] == e.golden.ninst).all()


def test_refusals_and_neutrality(engine_factory):
    from shrewd_amd import Engine, EngineError, FaultCampaign
    from shrewd_amd.fi import FI_E_ARG, FI_E_STATE, FI_OK
    e = engine_factory("hello")
    e.set_campaign(SEED, REGS | MEM, 1)
    assert e.L.fi_run_exact(e.h, 0, 0, None, None) == FI_E_ARG       # off: as before
    with pytest.raises(EngineError, match="memory"):
        e.exact_info()
    with pytest.raises(EngineError, match="off"):
        e.exact_mem_info()
    x = campaign(e, REGS | PC | RESULT)
    sites, w = e.exact_sites(0, int(x.trials))
    try:
        e.set_exact_memory(True)
        y = campaign(e, REGS | PC | RESULT)                           # on, memory not selected: the same campaign
        assert bytes(x) == bytes(y)
        s2, w2 = e.exact_sites(0, int(y.trials))
        assert np.array_equal(s2, sites) and np.array_equal(w2, w)
        z = campaign(e, REGS | MEM)
        assert int(z.classes[T_MEM]) > 0 and int(e.exact_mem_info().text_words) == 0
        assert e.L.fi_run_exact(e.h, int(z.trials), 1, None, None) == FI_E_ARG
    finally:
        e.set_exact_memory(False)
    fresh = Engine()
    try:
        fresh.load_elf(workload_elf("hello"), ["hello"])
        assert fresh.L.fi_set_exact_memory(fresh.h, 1) == FI_E_STATE  # no golden run
        assert fresh.L.fi_set_exact_memory(fresh.h, 0) == FI_OK
    finally:
        fresh.close()
    timing = Engine()
    try:
        timing.load_elf(workload_elf("hello"), ["hello"])
        timing.set_cpu_model("timing")
        timing.golden_run()
        assert timing.L.fi_set_exact_memory(timing.h, 1) == FI_E_STATE
        assert "Timing" in timing.L.fi_last_error(timing.h).decode()
    finally:
        timing.close()
    c = FaultCampaign(os.path.join(ROOT, "workloads", "hello.elf"), cmd=["hello"], structures=("int_reg", "mem"),
                      exact_memory=True)
    try:
        c.run_exact()
        v = c.vulnerability()
        assert set(v) == set(range(1, 32)) | {T_MEM}
        for s, shares in v.items():
            assert abs(sum(shares.values()) - 1) < 1e-12, s
        assert v[T_MEM]["masked"] < 1
    finally:
        c.engine.close()
