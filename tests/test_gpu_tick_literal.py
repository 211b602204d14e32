"""GPU parity of the literal tick contract (fi_set_tick_contract).

Under FI_TICK_CONTRACT_LITERAL the sites the numInst contract reports as
escape/timing with reasons FI_TK_NONCOUNT .. FI_TK_FAULTOP (1-6) run on the
device: the fetch override, the stale decoder half and the attempt offset of
a TimingSimpleCPU pc / register flip.  The reference is the oracle's literal
run of every tick site (or_run_tick_trials' `truth` records); the oracle's
contract output says which reason each site has.  Bar: bit-exact outcomes on
every site whose reason is not FI_TK_MACRO (7), the contract's escape record
where it is, with both map locations.
"""
import numpy as np
import pytest

from conftest import np_histogram, workload_elf

pytestmark = pytest.mark.gpu

REGS = (1 << 32) - 2
PC = 1 << 32
RESULT = 1 << 34
SEED = 0x5EED7101
MAPS = ["host", "device"]
BURST_PC_MASKS = [0x6, 0x7, 0xE, 0x1E, 0x1006, 0x1800]
# reasons that occur in the oracle's contract output on the boundary sites
BOUNDARY_REASONS = {"crc32": {2, 4}, "qsort": {2, 4, 5}, "hello": {1, 2, 4, 5, 6}}

CFG_NO_SNAPSHOT_START, CFG_NO_EARLY_EXIT, CFG_NO_TRANSLATE, CFG_NO_EPOCHS, CFG_SOLO_ALL = 1, 2, 4, 8, 128


def _boundary_sites(o, rng, n):
    """Tick sites on the edges of attempts (first / last tick of each phase),
    every target kind, across the run (tests/test_gpu_tick.py's recipe)."""
    ops, ticks = o.tick_trace()
    end = int(ticks["exec"][-1])   # sites lie in [0, golden ticks)
    out = []
    for j in rng.integers(0, len(ops), n):
        T = ticks[j]
        cand = [int(T["fetch_send"][0]), int(T["fetch_send"][0]) + 1, int(T["exec"]), int(T["exec"]) + 1,
                int(T["done"])]
        if ops["nfetch"][j] == 2:
            cand += [int(T["fetch_done"][0]), int(T["fetch_done"][0]) + 1]
        t = int(rng.choice(cand))
        tgt = int(rng.choice([32, 32, 34, int(rng.integers(1, 32))]))
        b = int(rng.integers(0, 64)) if tgt != 32 else int(rng.choice([1, 2, 3, 5, 12, 20, 40]))
        out.append((min(t, end - 1), 1 << b, tgt, len(out)))
    return np.array(out, dtype=[("tick", "<u8"), ("mask", "<u8"), ("target", "<u4"), ("trial", "<u4")])


def _reasons(contract):
    """The FI_TK_* reason of each site in the oracle's contract output (0: none)."""
    esc = (contract["cls"] == 5) & (contract["sub"] == 7)
    return np.where(esc, contract["exit_code"], 0)


@pytest.fixture(scope="module")
def lit(oracle_mod):
    """Engines (timing CPU model, golden run done) and oracles per workload and
    configuration, and the reference sets: each computed once and left alone."""
    from shrewd_amd import Engine, build_library
    build_library()
    engines, oracles, refs = {}, {}, {}

    class Lit:
        def oracle(self, name):
            if name not in oracles:
                o = oracle_mod.Oracle(workload_elf(name), name)
                o.run_golden()
                o.tick_setup()
                oracles[name] = o
            return oracles[name]

        def engine(self, name, **cfg):
            key = (name, tuple(sorted(cfg.items())))
            if key not in engines:
                e = Engine(**cfg)
                e.load_elf(workload_elf(name), [name])
                e.set_cpu_model("timing")
                e.golden_run()
                engines[key] = e
            return engines[key]

        def ref(self, name, kind):
            """(tick sites, the oracle's contract outcomes, its literal outcomes)"""
            if (name, kind) not in refs:
                o = self.oracle(name)
                if kind == "boundary":
                    ts = _boundary_sites(o, np.random.default_rng(5), 6000)
                elif kind == "burst":
                    ts = _boundary_sites(o, np.random.default_rng(11), 3000)
                    pc = ts["target"] == 32
                    ts["mask"][pc] = np.random.default_rng(12).choice(BURST_PC_MASKS, int(pc.sum()))
                else:
                    ts = o.tick_sample(SEED, 0, 6000, REGS | PC | RESULT)
                contract, truth = o.run_tick_trials(ts, threads=16, truth=True)
                for a in (ts, contract, truth):
                    a.setflags(write=False)
                refs[(name, kind)] = (ts, contract, truth)
            return refs[(name, kind)]

    yield Lit()
    for e in engines.values():
        e.close()
    for o in oracles.values():
        o.close()


class _literal:
    """The engine under the literal contract and the given map; the defaults again on the way out."""

    def __init__(self, e, where="host"):
        self.e, self.where = e, where

    def __enter__(self):
        self.e.set_tick_map(self.where)
        self.e.set_tick_contract("literal")
        return self.e

    def __exit__(self, *exc):
        self.e.set_tick_contract("numinst")
        self.e.set_tick_map("host")


def _compare(dev, ref, sites, what):
    bad = np.nonzero(dev != ref)[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(sites)} outcomes differ; first: site={sites[i]} "
                             f"gpu={dev[i]} oracle={ref[i]}")


def _no_resolved_escape(dev):
    esc = (dev["cls"] == 5) & (dev["sub"] == 7) & (dev["exit_code"] >= 1) & (dev["exit_code"] <= 6)
    assert not esc.any(), f"{int(esc.sum())} escape/timing records with a reason 1-6; first: {dev[esc][0]}"


@pytest.mark.parametrize("where", MAPS)
@pytest.mark.parametrize("name", ["crc32", "qsort", "hello"])
def test_boundary_sites_equal_truth(lit, name, where):
    """Every boundary site's outcome is the oracle's literal one; nothing is left an escape."""
    ts, contract, truth = lit.ref(name, "boundary")
    why = _reasons(contract)
    assert not ((why == 7) | (why == 8)).any()
    for r in BOUNDARY_REASONS[name]:   # (else the test checks nothing the numInst contract does not)
        assert (why == r).any(), f"reason {r} does not occur"
    with _literal(lit.engine(name), where) as e:
        dev, _ = e.run_tick_sites(ts)
    _compare(dev, truth, ts, f"{name}/{where}")
    _no_resolved_escape(dev)


@pytest.mark.parametrize("where", MAPS)
@pytest.mark.parametrize("name", ["crc32", "fpamo"])
def test_burst_pc_masks_equal_truth(lit, name, where):
    """Burst pc masks reach FI_TK_ALIGN (the decoder re-slices the old word);
    fpamo's AMO / LR / SC data phases stay FI_TK_MACRO escapes."""
    ts, contract, truth = lit.ref(name, "burst")
    why = _reasons(contract)
    assert (why == 3).any() and not (why == 8).any()
    macro = why == 7
    assert macro.sum() <= 0.01 * len(ts)
    with _literal(lit.engine(name), where) as e:
        dev, _ = e.run_tick_sites(ts)
    _compare(dev[~macro], truth[~macro], ts[~macro], f"{name}/{where}")
    _compare(dev[macro], contract[macro], ts[macro], f"{name}/{where} (FI_TK_MACRO)")
    _no_resolved_escape(dev)


@pytest.mark.parametrize("where", MAPS)
@pytest.mark.parametrize("name", ["hello", "qsort"])
def test_sampled_campaign_equals_truth(lit, name, where):
    ts, contract, truth = lit.ref(name, "sampled")
    why = _reasons(contract)
    kept = int(((why == 7) | (why == 8)).sum())
    assert kept == 0
    assert (why != 0).sum() >= 10   # (sites the numInst contract leaves as escapes)
    with _literal(lit.engine(name), where) as e:
        e.set_campaign(SEED, REGS | PC | RESULT, 1)
        e.set_bits(2**64 - 1)
        dev, hist = e.run_tick_trials(0, len(ts))
    _compare(dev, truth, ts, f"{name}/{where}")
    assert hist["trials"] == len(ts)
    assert hist["escape_sub"][7] == kept
    # the histogram files each trial under its tick site's target / lowest bit
    h = np_histogram(np.array([(0, int(s["mask"]), 0, int(s["target"]), 0) for s in ts],
                              dtype=[("inst", "<u8"), ("mask", "<u8"), ("addr", "<u8"), ("target", "<u4"),
                                     ("trial", "<u4")]), truth)
    assert (hist["counts"] == h["counts"]).all()


STALE_CONFIGS = {
    "solo_all": dict(flags=CFG_SOLO_ALL),
    "no_translate": dict(flags=CFG_NO_TRANSLATE),
    "no_epochs": dict(flags=CFG_NO_EPOCHS),
    "no_snapshots": dict(flags=CFG_NO_SNAPSHOT_START | CFG_NO_EARLY_EXIT),
    "chunked": dict(max_trials_per_launch=128),
}


@pytest.mark.parametrize("where", MAPS)
@pytest.mark.parametrize("cfg", sorted(STALE_CONFIGS))
def test_stale_half_through_every_path(lit, cfg, where):
    """crc32's FI_TK_STRADDLE2 (the trial carries a stale decoder half) and
    FI_TK_STRADDLE1 sites under each kernel selection, with and without epochs,
    snapshots and chunking: the outcomes of the default configuration, = truth."""
    ts, contract, truth = lit.ref("crc32", "boundary")
    why = _reasons(contract)
    pick = (why == 4) | (why == 2)
    assert (why == 4).sum() >= 20 and (why == 2).sum() >= 100
    sub = ts[pick]
    with _literal(lit.engine("crc32"), where) as e:
        base, _ = e.run_tick_sites(sub)
    with _literal(lit.engine("crc32", **STALE_CONFIGS[cfg]), where) as e:
        dev, _ = e.run_tick_sites(sub)
    _compare(base, truth[pick], sub, f"default/{where}")
    _compare(dev, base, sub, f"{cfg}/{where}")


@pytest.mark.parametrize("name", ["crc32", "qsort", "hello"])
def test_host_and_device_maps_agree(lit, name):
    ts, contract, truth = lit.ref(name, "boundary")
    with _literal(lit.engine(name)) as e:
        sites, disp, ho = e.map_tick_sites(ts)
        ts_d, sites_d, disp_d, ho_d = e.map_tick_sites_device(ts)
        assert (ts_d == ts).all() and (disp_d == disp).all() and (ho_d == ho).all()
        run = disp == 0
        assert (sites_d[run] == sites[run]).all()
        assert (sites["addr"][run] != 0).any()   # tick descriptors: the literal contract's sites
        # the mapped sites are plain fi_run_sites input
        out, _ = e.run_sites(sites[run])
        dev, _ = e.run_tick_sites(ts)
    _compare(out, dev[run], ts[run], name)
    _compare(dev[run], truth[run], ts[run], name)


@pytest.mark.parametrize("where", MAPS)
def test_default_contract_untouched(lit, where):
    """Left at its default, or set back to it, the contract is the numInst one: the oracle's contract output."""
    ts, contract, truth = lit.ref("crc32", "boundary")
    e = lit.engine("crc32", max_trials_per_launch=65536)   # (an engine no other test sets to literal)
    e.set_tick_map(where)
    try:
        dev, _ = e.run_tick_sites(ts)
        _compare(dev, contract, ts, f"default/{where}")
        e.set_tick_contract("literal")
        e.set_tick_contract("numinst")
        dev, _ = e.run_tick_sites(ts)
        _compare(dev, contract, ts, f"set back/{where}")
        with pytest.raises(Exception):
            e.set_tick_contract(2)
    finally:
        e.set_tick_contract("numinst")
        e.set_tick_map("host")
