"""Exact campaigns in the tick domain (fi_run_exact_ticks, DESIGN.md §4j "Tick
domain"): every tick of a TimingSimpleCPU golden run covered by one trial per
class, weighted by the class's ticks.

Bar, integer-exact throughout: the map is constant over a segment (every tick
of hello against its segment's representative); the weighted histogram and
every trial's outcome equal a brute force that runs one representative tick
site per (segment, structure, bit) through the existing fi_run_tick_sites and
weights it by the segment's length in numpy -- the segments computed here from
the exported attempt table, not taken from the engine; ranges sum to the
whole; weights past 2^32 (hello on a board 20,000 times slower); sampled tick
sites -- run by the engine and, literally, by the oracle -- have the outcome of
the trial fi_exact_tick_locate names.
"""
import numpy as np
import pytest

from conftest import workload_elf

pytestmark = pytest.mark.gpu

REGS = (1 << 32) - 2
PC, MEM, RESULT = 1 << 32, 1 << 33, 1 << 34
SP, S0, A0, A1, A5, T6 = 2, 8, 10, 11, 15, 31
SEED = 0x5EED7201
ALL_BITS = 2**64 - 1
HIST_FIELDS = ("counts", "crash_sub", "escape_sub", "trials", "guest_insts")
MASKED, CRASH, ESCAPE, ESC_TIMING = 0, 2, 5, 7
# cpu_period and every controller / DRAM time of the board (fi_timing_params)
TIME_FIELDS = ("cpu_period", "mc_frontend", "mc_backend", "mc_command_window", "tCK", "tBURST", "tRCD", "tCL", "tRP",
               "tRAS", "tRRD", "tXAW", "tRFC", "tWR", "tWTR", "tRTP", "tRTW", "tCS", "tREFI")


def _timing_engine(name, params=None):
    import torch  # noqa: F401  (before the engine library: one HIP runtime for both)
    from shrewd_amd import Engine, build_library
    build_library()
    e = Engine()
    e.load_elf(workload_elf(name), [name])
    e.set_cpu_model("timing", params)
    e.golden_run()
    e.set_tick_map("device")   # the brute force maps its sites where the exact campaign does
    return e


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def make(name):
        if name not in cache:
            cache[name] = _timing_engine(name)
        e = cache[name]
        e.set_protect(0)
        e.set_tick_contract("numinst")
        return e

    yield make
    for e in cache.values():
        e.close()


def _segments(e):
    """(first tick, length) of the golden run's segments, from the attempt table alone."""
    att = e.exact_tick_attempts()
    T = int(e.tick_info()["golden_ticks"])
    first, length = [], []
    for j in range(len(att)):
        a = int(att["done"][j - 1]) + 1 if j else 0
        hi = T - 1 if j + 1 == len(att) else min(int(att["done"][j]), T - 1)
        ends = ([int(att["fetch_done0"][j])] if att["nfetch"][j] == 2 else []) + [int(att["exec"][j]), hi]
        for end in ends:
            end = min(end, hi)
            if end >= a:
                first.append(a)
                length.append(end - a + 1)
                a = end + 1
    first, length = np.array(first, np.uint64), np.array(length, np.uint64)
    assert int(length.sum()) == T
    return first, length


def _bits(mask):
    return [b for b in range(64) if (mask >> b) & 1]


def _brute_sites(e, structures, bits_mask):
    """One representative tick site per (structure, segment, bit) and its weight."""
    from shrewd_amd.fi import TICK_SITE_DT
    first, length = _segments(e)
    bits = np.array(_bits(bits_mask), np.uint64)
    targets = [t for t in range(1, 35) if (structures >> t) & 1]
    n = len(targets) * len(first) * len(bits)
    ts = np.zeros(n, TICK_SITE_DT)
    ts["target"] = np.repeat(np.array(targets, np.uint32), len(first) * len(bits))
    ts["tick"] = np.tile(np.repeat(first, len(bits)), len(targets))
    ts["mask"] = np.tile(np.uint64(1) << bits, len(targets) * len(first))
    ts["trial"] = np.arange(n, dtype=np.uint64).astype(np.uint32)
    w = np.tile(np.repeat(length, len(bits)), len(targets))
    return ts, w


def _bit_of(masks):
    """The position of each single-bit mask."""
    u, inv = np.unique(masks, return_inverse=True)
    return np.array([int(m).bit_length() - 1 for m in u], np.int64)[inv.reshape(-1)]


def _weighted_hist(ts, out, w):
    """fi_run_tick_sites' histogram with each trial counted w times (sums modulo 2^64)."""
    from shrewd_amd import HIST_DT
    h = np.zeros((), HIST_DT)
    w = w.astype(np.uint64)
    cls = np.minimum(out["cls"], ESCAPE).astype(np.int64)
    np.add.at(h["counts"], (ts["target"].astype(np.int64), _bit_of(ts["mask"]), cls), w)
    np.add.at(h["crash_sub"], (out["sub"][cls == CRASH] & 15).astype(np.int64), w[cls == CRASH])
    np.add.at(h["escape_sub"], (out["sub"][cls == ESCAPE] & 7).astype(np.int64), w[cls == ESCAPE])
    h["trials"] = w.sum(dtype=np.uint64)
    with np.errstate(over="ignore"):
        h["guest_insts"] = (w * out["ninst"]).sum(dtype=np.uint64)
    return h


def _same_hist(got, want):
    for f in HIST_FIELDS:
        assert np.array_equal(got[f], want[f]), f


def _campaign(e, structures, bits=ALL_BITS):
    e.set_campaign(SEED, structures, 1)
    e.set_bits(bits)
    return e.exact_tick_info()


def _check_against_brute_force(e, structures, bits=ALL_BITS):
    """The exact campaign's histogram = the weighted brute force's; every exact
    trial's outcome = the outcome of its representative's brute-force site."""
    x = _campaign(e, structures, bits)
    T = int(e.tick_info()["golden_ticks"])
    nsel = bin(structures).count("1")
    assert x.space == T * x.nbits * nsel and x.nbits == len(_bits(bits))
    out, hist = e.run_exact_ticks(0, int(x.trials))
    assert int(hist["counts"].sum()) == int(hist["trials"]) == int(x.space)
    ts, w = _brute_sites(e, structures, bits)
    bout, _ = e.run_tick_sites(ts)
    _same_hist(hist, _weighted_hist(ts, bout, w))
    # each exact trial against the brute-force site of its representative (same tick, structure, mask)
    sites, rep, wt = e.exact_tick_sites(0, int(x.trials))
    key = lambda a: (a["target"].astype(np.uint64) << np.uint64(56)) ^ (a["tick"] << np.uint64(6)) ^ \
        _bit_of(a["mask"]).astype(np.uint64)   # noqa: E731
    kb = key(ts)
    order = np.argsort(kb)
    at = order[np.searchsorted(kb[order], key(rep))]
    assert np.array_equal(kb[at], key(rep)), "a representative is no segment's first tick"
    bad = np.nonzero(out != bout[at])[0]
    assert not len(bad), f"{len(bad)} of {len(out)} outcomes differ; first: trial {bad[0]} site {sites[bad[0]]} " \
                         f"rep {rep[bad[0]]} got {out[bad[0]]} want {bout[at][bad[0]]}"
    assert int(wt.sum()) + (int(x.dead_ticks) + int(x.escaped_ticks)) * int(x.nbits) == int(x.space)
    return x, out, hist, wt


# ---- 1. hello: representatives, the whole campaign, ranges, 64-bit weights
@pytest.mark.parametrize("contract", ["numinst", "literal"])
def test_hello_every_tick_maps_as_its_segment(engines, contract):
    """All 577,089 ticks x {a0, a5, sp, pc, result} x one bit through the device
    map: site, disposition and host outcome equal those of the segment's first tick."""
    from shrewd_amd.fi import TICK_SITE_DT
    e = engines("hello")
    e.set_tick_contract(contract)
    T = int(e.tick_info()["golden_ticks"])
    assert T == 577089
    first, length = _segments(e)
    assert len(first) == 13 and len(e.exact_tick_attempts()) == 9
    ticks = np.arange(T, dtype=np.uint64)
    seg = np.searchsorted(first, ticks, side="right") - 1
    for target, bit in ((A0, 3), (A5, 63), (SP, 0), (32, 12), (34, 40)):
        ts = np.zeros(T, TICK_SITE_DT)
        ts["tick"], ts["mask"], ts["target"] = ticks, 1 << bit, target
        _, sites, disp, ho = e.map_tick_sites_device(ts)
        rs = np.zeros(len(first), TICK_SITE_DT)
        rs["tick"], rs["mask"], rs["target"] = first, 1 << bit, target
        _, rsites, rdisp, rho = e.map_tick_sites_device(rs)
        for f in ("inst", "mask", "addr", "target"):
            assert np.array_equal(sites[f], rsites[f][seg]), (target, f)
        assert np.array_equal(disp, rdisp[seg]) and np.array_equal(ho, rho[seg]), target


@pytest.mark.parametrize("contract", ["numinst", "literal"])
def test_hello_whole_campaign_equals_brute_force(engines, contract):
    """x1..x31 + pc, 64 bits: 13 segments x 32 structures x 64 bits brute-force sites."""
    e = engines("hello")
    e.set_tick_contract(contract)
    x, out, hist, wt = _check_against_brute_force(e, REGS | PC)
    assert x.segments == 13 and x.classes[32] == 13
    assert int(hist["trials"]) == 577089 * 64 * 32


def test_hello_ranges_sum_to_the_whole(engines):
    from shrewd_amd import HIST_DT
    e = engines("hello")
    x = _campaign(e, REGS | PC | RESULT)
    n = int(x.trials)
    assert n > 1100
    whole_out, whole = e.run_exact_ticks(0, n)
    cuts = [0, 7, 7, 1033, n - 1, n]   # odd cuts, n == 0, a cut inside a class (1033 % 64 != 0)
    acc = np.zeros((), HIST_DT)
    outs = []
    for lo, hi in zip(cuts, cuts[1:]):
        o, h = e.run_exact_ticks(lo, hi - lo)
        outs.append(o)
        for f in HIST_FIELDS:
            acc[f] += h[f]
    _same_hist(acc, whole)
    assert np.array_equal(np.concatenate(outs), whole_out)
    assert int(whole["counts"].sum()) == int(whole["trials"]) == 577089 * 64 * 33 == int(x.space)
    # the dead and escaped ticks come with first == 0 only, also when n == 0
    _, h0 = e.run_exact_ticks(0, 0)
    _, h1 = e.run_exact_ticks(5, 0)
    assert int(h0["trials"]) == (int(x.dead_ticks) + int(x.escaped_ticks)) * 64 and int(h1["trials"]) == 0
    assert int(h0["escape_sub"][ESC_TIMING]) == int(x.escaped_ticks) * 64


def test_hello_weights_past_32_bits():
    """hello on a board whose cpu_period and controller / DRAM times are 20,000
    times longer: the model scales exactly, class weights pass 2^32."""
    from shrewd_amd.fi import timing_params
    d = timing_params()
    e = _timing_engine("hello", timing_params(**{k: getattr(d, k) * 20000 for k in TIME_FIELDS}))
    try:
        assert int(e.tick_info()["golden_ticks"]) == 11_541_780_000
        x, out, hist, wt = _check_against_brute_force(e, REGS | PC)
        assert int(wt.max()) > 2**32
        assert int(hist["trials"]) == 11_541_780_000 * 64 * 32 > 2**44
    finally:
        e.close()


# ---- 2. fpamo: AMO / LR / SC macro-ops
@pytest.mark.parametrize("contract", ["numinst", "literal"])
def test_fpamo_equals_brute_force(engines, contract):
    e = engines("fpamo")
    e.set_tick_contract(contract)
    assert len(e.exact_tick_attempts()) == 850
    sel = sum(1 << t for t in (SP, S0, A0, A5)) | PC | RESULT
    bits = sum(1 << b for b in (0, 1, 7, 12, 31, 32, 40, 63))
    _check_against_brute_force(e, sel, bits)


# ---- 3. crc32
CRC_SEL = (1 << A0) | (1 << A1) | (1 << T6) | PC | RESULT
CRC_BITS = (1 << 0) | (1 << 12) | (1 << 40)


@pytest.fixture(scope="module")
def crc32_exact(engines):
    e = engines("crc32")
    x, out, hist, wt = _check_against_brute_force(e, CRC_SEL, CRC_BITS)
    out.flags.writeable = False
    return e, x, out


def test_crc32_equals_brute_force(crc32_exact):
    e, x, out = crc32_exact
    assert x.segments == 89246 and len(e.exact_tick_attempts()) == 64620
    assert x.classes[32] == x.segments


def test_crc32_sampled_sites_have_their_trials_outcome(crc32_exact, oracle_mod):
    """3,000 sampled tick sites, run by the engine and literally by the oracle:
    both equal the outcome of the exact trial fi_exact_tick_locate names, or
    masked (the golden run) / FI_ESC_TIMING where it names none."""
    from shrewd_amd.fi import XT_DEAD, XT_ESCAPE, XT_GOLDEN, XT_TRIAL
    e, x, out = crc32_exact
    _campaign(e, CRC_SEL, CRC_BITS)
    ts = e.sample_tick_sites(0, 3000)
    dev, _ = e.run_tick_sites(ts)
    o = oracle_mod.Oracle(workload_elf("crc32"), "crc32")
    try:
        ninst = o.run_golden().ninst
        assert o.tick_setup() == int(e.tick_info()["golden_ticks"])
        ref = o.run_tick_trials(ts)
    finally:
        o.close()
    trial, kind = e.exact_tick_locate(ts)
    live = kind == XT_TRIAL
    assert live.any() and (kind == XT_DEAD).any()
    want = np.zeros_like(dev)
    want[live] = out[trial[live].astype(np.int64)]
    gone = (kind == XT_DEAD) | (kind == XT_GOLDEN)
    for got in (dev, ref):
        assert np.array_equal(got[live], want[live])
        assert (got["cls"][gone] == MASKED).all() and (got["ninst"][gone] == ninst).all()
        esc = kind == XT_ESCAPE
        assert (got["cls"][esc] == ESCAPE).all() and (got["sub"][esc] == ESC_TIMING).all()


def test_class_runs_across_workgroups_and_structures(engines):
    """x31 and the pc, 64 bits: a range that starts inside x31's classes and ends
    inside the pc's, so that a 256-thread block of the histogram kernel holds
    both structures and 64-lane class runs cross block boundaries."""
    e = engines("crc32")
    x = _campaign(e, (1 << T6) | PC)
    n31 = int(x.classes[T6]) * 64
    assert n31 > 300
    first, n = n31 - 300, 300 + 900   # 300 % 256 != 0: the boundary falls inside a block
    sites, rep, wt = e.exact_tick_sites(first, n)
    assert set(np.unique(rep["target"])) == {T6, 32}
    out, hist = e.run_exact_ticks(first, n)
    bout, _ = e.run_tick_sites(rep)
    assert np.array_equal(out, bout)
    _same_hist(hist, _weighted_hist(rep, bout, wt))


# ---- 4. refusals
def test_refusals(engines, engine_factory):
    from shrewd_amd import EngineError
    from shrewd_amd.fi import FI_E_ARG, FI_E_STATE, FI_OK

    def refused(eng, want, first=0, n=0):
        rc = eng.L.fi_run_exact_ticks(eng.h, first, n, None, None)
        assert rc == want, rc
        assert eng.L.fi_last_error(eng.h).decode().strip()

    a = engine_factory("hello")   # the atomic CPU model
    a.set_campaign(SEED, REGS | PC, 1)
    refused(a, FI_E_STATE)
    with pytest.raises(EngineError, match="TimingSimpleCPU"):
        a.exact_tick_info()
    e = engines("hello")
    x = _campaign(e, REGS | PC)
    e.set_protect(1 << 10)
    refused(e, FI_E_ARG)
    e.set_protect(0)
    e.set_protect_opclasses(2)
    refused(e, FI_E_ARG)
    e.set_protect_opclasses(0)
    e.set_campaign(SEED, REGS | MEM, 1)
    refused(e, FI_E_ARG)
    with pytest.raises(EngineError, match="memory"):
        e.exact_tick_info()
    _campaign(e, REGS | PC)
    refused(e, FI_E_ARG, 0, int(x.trials) + 1)
    refused(e, FI_E_ARG, 2**64 - 1, 2)
    assert e.L.fi_run_exact_ticks(e.h, int(x.trials), 0, None, None) == FI_OK
    # a site outside the space has no place
    ts = np.array([(5, 3, 10, 0)], dtype=[("tick", "<u8"), ("mask", "<u8"), ("target", "<u4"), ("trial", "<u4")])
    with pytest.raises(EngineError, match="outside"):
        e.exact_tick_locate(ts)
    # the atomic exact entry points still refuse a timing engine
    rc = e.L.fi_run_exact(e.h, 0, 0, None, None)
    assert rc == FI_E_STATE
    with pytest.raises(EngineError):
        e.exact_info()


def test_fault_campaign_run_exact_dispatches_on_cpu_type(tmp_path):
    import os

    from conftest import ROOT
    from shrewd_amd import FaultCampaign
    c = FaultCampaign(os.path.join(ROOT, "workloads", "hello.elf"), cmd=["hello"], structures=REGS | PC,
                      cpu_type="timing", tick_map="device")
    try:
        c.run_exact()
        T = int(c.engine.tick_info()["golden_ticks"])
        assert int(c._hist["trials"]) == T * 64 * 32
        v = c.vulnerability()
        assert set(v) == set(range(1, 33))
        for s in v.values():
            assert abs(sum(s.values()) - 1.0) < 1e-12   # the shares of T x nbits sites
    finally:
        c.engine.close()
