"""Exact campaigns on the device (fi_run_exact): one trial per
first-access class, weighted, against the engine's and the oracle's brute
force over every site of the same space."""
import os

import numpy as np
import pytest

from conftest import np_histogram, workload_elf
from test_exact_cpu import (ALL_BITS, REGS, all_sites, class_of, index_from_ops, np_exact_sites,
                            np_weighted_histogram)

pytestmark = pytest.mark.gpu

PC, RESULT, MEM = 1 << 32, 1 << 34, 1 << 33
FIELDS = ("counts", "crash_sub", "escape_sub", "trials", "guest_insts")
SEED = 0xE8AC7
THREADS = min(16, os.cpu_count() or 1)       # the oracle's brute force: no more threads than it gets cores


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


def campaign(e, structures, bits=ALL_BITS, burst=1):
    e.set_campaign(SEED, structures, burst)
    e.set_bits(bits)
    e.set_protect(0)
    return e.exact_info()


def exact_vs_brute(e, o, structures, bits=ALL_BITS, burst=1):
    """run_exact over the whole campaign against the engine's brute force and
    the oracle's over every site -> (info, exact outcomes, histogram, the sites of the space)"""
    x = campaign(e, structures, bits, burst)
    ninst = int(e.golden.ninst)
    out, h = e.run_exact(0, int(x.trials))
    space = all_sites(ninst, structures, bits, burst)
    assert int(x.space) == len(space)
    _, bh = e.run_sites(space)
    same_hist(h, bh, "exact vs the engine's brute force")
    assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
    same_hist(h, np_histogram(space, o.run_trials(space, threads=THREADS)), "exact vs the oracle's brute force")
    return x, out, h, space


def test_hello_whole_space(engine_factory, oracle_mod):
    """x1..x31 | pc | result, every bit: a 256-thread block of either exact
    kernel spans several structures; the escapes are counted like any class."""
    e = engine_factory("hello")
    o = oracle_for(oracle_mod, "hello")
    structures = REGS | PC | RESULT
    x, out, h, _ = exact_vs_brute(e, o, structures)
    ninst = int(e.golden.ninst)
    off, ev = index_from_ops(o.golden_ops())
    sites, w, dead = np_exact_sites(off, ev, ninst, structures)
    assert int(x.trials) == len(sites) and int(x.nbits) == 64
    assert int(x.dead_sites) == 64 * sum(dead.values())
    assert sum(int(c) for c in x.classes[1:32]) == 16 and x.classes[32] == x.classes[34] == ninst
    got, gw = e.exact_sites(0, len(sites))
    assert np.array_equal(got, sites) and np.array_equal(gw, w)
    # a range that starts inside a class
    got, gw = e.exact_sites(70, 300)
    assert np.array_equal(got, sites[70:370]) and np.array_equal(gw, w[70:370])
    same_outcomes(out, o.run_trials(sites), sites, "exact trials vs the oracle at the representatives")
    same_hist(h, np_weighted_histogram(sites, out, w, dead, golden_ninst=ninst), "device vs numpy weighted histogram")
    esc = int(h["counts"][:, :, 5].sum())
    print(f"hello: {x.space} sites, {x.trials} exact trials, {x.dead_sites} dead, {esc} escapes")
    assert esc > 0


def test_hello_chunks_and_ranges(engine_factory):
    """Chunks of 1000 trials (a boundary inside a class) and three ranges cut
    off the multiples of nbits give the one-call result, the dead sites once;
    an empty range at 0 adds exactly the dead sites."""
    from shrewd_amd.fi import HIST_DT
    e = engine_factory("hello")
    c = engine_factory("hello", max_trials_per_launch=1000)
    structures = REGS | PC | RESULT
    x = campaign(e, structures)
    n = int(x.trials)
    assert n > 1000 and 1000 % int(x.nbits)
    out, h = e.run_exact(0, n)
    assert int(campaign(c, structures).trials) == n
    cout, ch = c.run_exact(0, n)
    same_outcomes(cout, out, cout, "chunked vs one launch")
    same_hist(ch, h, "chunked vs one launch")
    parts, total = [], np.zeros(1, HIST_DT)[0]
    for lo, hi in ((0, 333), (333, 1201), (1201, n)):
        po, ph = c.run_exact(lo, hi - lo)
        parts.append(po)
        for f in FIELDS:
            total[f] += ph[f]
    same_outcomes(np.concatenate(parts), out, out, "three ranges vs one call")
    same_hist(total, h, "three ranges vs one call")
    _, h0 = e.run_exact(0, 0)
    dead, ninst = int(x.dead_sites), int(e.golden.ninst)
    assert dead > 0 and int(h0["trials"]) == dead and int(h0["guest_insts"]) == dead * ninst
    assert int(h0["counts"][:, :, 0].sum()) == dead == int(h0["counts"].sum())
    assert not h0["crash_sub"].any() and not h0["escape_sub"].any()
    _, h1 = e.run_exact(1, 0)     # not the range that starts at 0: nothing
    assert int(h1["trials"]) == 0 and not h1["counts"].any()


@pytest.mark.parametrize("bits,burst", [(ALL_BITS, 4), ((1 << 0) | (1 << 12) | (1 << 63), 1)])
def test_hello_burst_and_bit_mask(engine_factory, oracle_mod, bits, burst):
    e = engine_factory("hello")
    x, *_ = exact_vs_brute(e, oracle_for(oracle_mod, "hello"), REGS | PC | RESULT, bits, burst)
    assert int(x.nbits) == (61 if burst == 4 else 3)


def test_fpamo_four_registers_and_protect(engine_factory, oracle_mod):
    """{sp, s0, a0, a5}, every bit, through FP and AMO code; once more with
    a0..a7 protected: the detected class is weighted like the others."""
    e = engine_factory("fpamo")
    o = oracle_for(oracle_mod, "fpamo")
    structures = (1 << 2) | (1 << 8) | (1 << 10) | (1 << 15)
    x, out, h, space = exact_vs_brute(e, o, structures)
    assert int(x.space) == 4 * 64 * int(e.golden.ninst)
    sites, _ = e.exact_sites(0, int(x.trials))
    same_outcomes(out, o.run_trials(sites), sites, "exact trials vs the oracle")
    prot = 0xFF << 10
    try:
        e.set_protect(prot)
        pout, ph = e.run_exact(0, int(x.trials))
        _, bh = e.run_sites(space)
    finally:
        e.set_protect(0)
    same_hist(ph, bh, "protected: exact vs brute force")
    same_outcomes(pout, o.run_trials(sites, protect_mask=prot), sites, "protected exact trials vs the oracle")
    assert int(ph["counts"][:, :, 4].sum()) > 0 and int(ph["counts"][:, :, 4].sum()) == int(bh["counts"][:, :, 4].sum())


CRC_STRUCT = (1 << 10) | (1 << 11) | (1 << 31)          # a0, a1, t6
CRC_BITS = (1 << 0) | (1 << 12) | (1 << 40)


@pytest.fixture(scope="module")
def crc32_exact(engine_factory):
    """The crc32 exact campaign, run once for the tests below."""
    e = engine_factory("crc32")
    x = campaign(e, CRC_STRUCT, CRC_BITS)
    out, h = e.run_exact(0, int(x.trials))
    sites, w = e.exact_sites(0, int(x.trials))
    return e, x, sites, w, out, h


def test_crc32_three_registers(crc32_exact, engine_factory, oracle_mod):
    """Through the translated kernels and the loop proofs: the weighted
    histogram is the brute force's; an engine without forwarding runs the
    representatives where they stand, with identical outcomes; the oracle
    agrees on 3,000 of them."""
    e, x, sites, w, out, h = crc32_exact
    campaign(e, CRC_STRUCT, CRC_BITS)
    space = all_sites(int(e.golden.ninst), CRC_STRUCT, CRC_BITS)
    assert int(x.space) == len(space) and int(x.trials) < len(space) // 8
    _, bh = e.run_sites(space)
    same_hist(h, bh, "exact vs the engine's brute force")
    assert int(h["counts"].sum()) == int(h["trials"]) == len(space)
    f = engine_factory("crc32", flags=512)               # FI_CFG_NO_FORWARD
    assert int(campaign(f, CRC_STRUCT, CRC_BITS).trials) == int(x.trials)
    fout, fh = f.run_exact(0, int(x.trials))
    same_outcomes(fout, out, sites, "FI_CFG_NO_FORWARD vs default")
    same_hist(fh, h, "FI_CFG_NO_FORWARD vs default")
    pick = np.linspace(0, len(sites) - 1, 3000).astype(np.int64)
    o = oracle_for(oracle_mod, "crc32")
    same_outcomes(out[pick], o.run_trials(sites[pick]), sites[pick], "exact trials vs the oracle")
    print(f"crc32: {x.space} sites, {x.trials} exact trials, {x.dead_sites} dead")


def test_sampled_sites_fall_into_their_classes(crc32_exact):
    """3,000 sampled sites of the same campaign: each one's outcome is the
    exact outcome of the class that contains it; a site in no class is a
    masked golden run."""
    e, x, sites, w, out, _ = crc32_exact
    campaign(e, CRC_STRUCT, CRC_BITS)
    s = e.sample(0, 3000)
    so, _ = e.run_trials(0, 3000)
    cl = class_of(sites, w, s)
    live = cl >= 0
    assert live.any() and (~live).any()
    same_outcomes(so[live], out[cl[live]], s[live], "sampled sites vs their classes")
    d = so[~live]
    assert (d["cls"] == 0).all() and (d["ninst"] == e.golden.ninst).all()


def test_refusals(engine_factory):
    from shrewd_amd import Engine, EngineError
    from shrewd_amd.fi import FI_E_ARG, FI_E_STATE, FI_OK

    def refused(eng, first, n, want=None):
        rc = eng.L.fi_run_exact(eng.h, first, n, None, None)
        assert rc != FI_OK and (want is None or rc == want), rc
        assert eng.L.fi_last_error(eng.h).decode().strip()

    e = engine_factory("hello")
    e.set_campaign(SEED, REGS | MEM, 1)               # (set_campaign takes it: sampled campaigns have memory sites)
    refused(e, 0, 0, FI_E_ARG)
    with pytest.raises(EngineError, match="memory"):
        e.exact_info()
    x = campaign(e, REGS)
    refused(e, 0, int(x.trials) + 1, FI_E_ARG)
    refused(e, int(x.trials), 1, FI_E_ARG)
    refused(e, 2**64 - 1, 2, FI_E_ARG)                # first + n wraps
    assert e.L.fi_run_exact(e.h, int(x.trials), 0, None, None) == FI_OK
    fresh = Engine()
    try:
        fresh.load_elf(workload_elf("hello"), ["hello"])
        refused(fresh, 0, 0, FI_E_STATE)              # no golden run
        fresh.golden_run()
        refused(fresh, 0, 0, FI_E_STATE)              # no campaign
    finally:
        fresh.close()
    timing = Engine()
    try:
        timing.load_elf(workload_elf("hello"), ["hello"])
        timing.set_cpu_model("timing")
        timing.golden_run()
        timing.set_campaign(SEED, REGS, 1)
        refused(timing, 0, 0)
    finally:
        timing.close()
