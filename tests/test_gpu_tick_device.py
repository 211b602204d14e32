"""The device map of tick-domain campaigns (fi_set_tick_map FI_TICK_MAP_DEVICE,
fi_map_tick_sites_device, fi_run_tick_trials_device).

A kernel draws and maps every tick site from a packed copy of the golden
attempts, golden-equal and escape trials keep their slot (parked: dead at
injection) and the histogram is built on the device.  Bar: the mapper = the
host mapper (fi_map_tick_sites) site for site, the sampler = the host sampler,
and a device-map campaign = the host-map campaign and = the oracle's literal
tick trials, byte for byte, under every configuration that changes the
plumbing (chunks, no forwarding, no early exit, 64-lane epochs, interpreter).
"""
import os

import numpy as np
import pytest

from conftest import ROOT, workload_elf

pytestmark = pytest.mark.gpu

REGS = (1 << 32) - 2
PC = 1 << 32
MEM = 1 << 33
RESULT = 1 << 34
SEED = 0x5EED7101
ALL_BITS = 2**64 - 1
HIST_FIELDS = ("counts", "crash_sub", "escape_sub", "trials", "guest_insts")
STRUCTS = {"crc32": REGS | PC | RESULT, "qsort": REGS | PC | RESULT, "hello": REGS | PC, "intmix": REGS | PC}


def _timing_engine(name, **kw):
    import torch  # noqa: F401  (before the engine library, as conftest's engine_factory: one HIP runtime for both)
    from shrewd_amd import Engine
    e = Engine(**kw)
    e.load_elf(workload_elf(name), [name])
    e.set_cpu_model("timing")
    e.golden_run()
    return e


@pytest.fixture(scope="module")
def tick_pair(oracle_mod):
    import torch  # noqa: F401
    from shrewd_amd import build_library
    build_library()
    cache = {}

    def make(name):
        if name not in cache:
            o = oracle_mod.Oracle(workload_elf(name), name)
            o.run_golden()
            o.tick_setup()
            cache[name] = (_timing_engine(name), o)
        e = cache[name][0]
        e.set_tick_map("host")
        e.set_protect(0)   # (set_campaign, which every sampling test calls, makes every bit eligible again)
        return cache[name]

    yield make
    for e, o in cache.values():
        e.close()
        o.close()


def _compare(dev, ref, sites, what="outcomes"):
    bad = np.nonzero(dev != ref)[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{len(bad)} of {len(sites)} {what} differ; first: [{i}] site={sites[i]} "
                             f"got={dev[i]} want={ref[i]}")


def _same_hist(a, b):
    for f in HIST_FIELDS:
        assert np.array_equal(a[f], b[f]), f


_SITES = {}   # (workload, seed, n) -> boundary set: made once, shared, never written to


def _boundary_sites(name, o, seed, n):
    if (name, seed, n) not in _SITES:
        ts = _make_boundary_sites(o, np.random.default_rng(seed), n)
        ts.flags.writeable = False
        _SITES[name, seed, n] = ts
    return _SITES[name, seed, n]


def _make_boundary_sites(o, rng, n):
    """Tick sites on the edges of attempts (first / last tick of each phase),
    every target kind, across the run (tests/test_gpu_tick.py's generator)."""
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


def _load_dest_sites(o, dtype):
    """Flips of a load's destination while its data is outstanding: golden-equal."""
    ops, ticks = o.tick_trace()
    gops = o.golden_ops()
    loads = np.nonzero((ops["kind"] == 0) & (ops["nfrag"] > 0) & (ops["cmd"] == 0))[0]
    extra = [(int(ticks["done"][j]), 1 << 7, (int(gops["dst"][j]) & 0xFFFFFFFE).bit_length() - 1, 0)
             for j in loads[::max(1, len(loads) // 200)] if bin(int(gops["dst"][j]) & 0xFFFFFFFE).count("1") == 1]
    return np.array(extra, dtype)


# ---- 1. the mapper
@pytest.mark.parametrize("name", ["crc32", "qsort", "hello"])
def test_device_map_equals_host_map(tick_pair, name):
    e, o = tick_pair(name)
    for seed, n in ((5, 6000), (9, 3000)):
        ts = _boundary_sites(name, o, seed, n)
        if name == "crc32":
            ts = np.concatenate([ts, _load_dest_sites(o, ts.dtype)])
            ts["trial"] = np.arange(len(ts))
        hs, hd, ho = e.map_tick_sites(ts)
        ts_out, ds, dd, do = e.map_tick_sites_device(ts)
        assert np.array_equal(ts_out, ts)
        _compare(dd, hd, ts, "dispositions")
        _compare(ds[hd == 0], hs[hd == 0], ts[hd == 0], "mapped sites")
        _compare(do[hd != 0], ho[hd != 0], ts[hd != 0], "host outcomes")
        if name == "crc32":
            assert set(np.unique(dd).tolist()) == {0, 1, 2}


# ---- 2. the sampler
@pytest.mark.parametrize("name", ["crc32", "qsort"])
def test_device_sampler_equals_host_sampler(tick_pair, name):
    e, _ = tick_pair(name)
    for structs, burst, bits in ((REGS | PC, 1, ALL_BITS), (REGS | PC | RESULT, 1, ALL_BITS), (REGS, 4, ALL_BITS),
                                 (REGS | PC, 1, 0x00FF00F0000F0A05), (REGS, 4, 0xF0000000000000F1)):
        e.set_campaign(SEED, structs, burst)
        e.set_bits(bits)
        want = e.sample_tick_sites(1000, 5000)
        got, sites, disp, _ = e.map_tick_sites_device(None, 1000, 5000)
        assert np.array_equal(got, want), (structs, burst, hex(bits))
        hs, hd, _ = e.map_tick_sites(want)
        assert np.array_equal(disp, hd)
        assert np.array_equal(sites[hd == 0], hs[hd == 0])
    e.set_bits(ALL_BITS)


# ---- 3. campaigns: device map = host map
@pytest.mark.parametrize("name", ["crc32", "qsort", "hello", "intmix"])
def test_device_campaign_equals_host_campaign(tick_pair, name):
    e, _ = tick_pair(name)
    e.set_campaign(SEED, STRUCTS[name], 1)
    ref, rh = e.run_tick_trials(0, 6000)
    e.set_tick_map("device")
    dev, dh = e.run_tick_trials(0, 6000)
    e.set_tick_map("host")
    _compare(dev, ref, np.arange(6000))
    _same_hist(dh, rh)


@pytest.mark.parametrize("name", ["crc32", "qsort", "hello"])
def test_device_sites_equal_host_sites(tick_pair, name):
    e, o = tick_pair(name)
    ts = _boundary_sites(name, o, 5, 6000)
    ref, rh = e.run_tick_sites(ts)
    e.set_tick_map("device")
    dev, dh = e.run_tick_sites(ts)
    e.set_tick_map("host")
    _compare(dev, ref, ts)
    _same_hist(dh, rh)
    esc = (dev["cls"] == 5) & (dev["sub"] == 7)
    assert esc.any() and (~esc).sum() > 0.5 * len(ts)


# ---- 4. against the oracle's literal tick trials
def test_device_campaign_matches_oracle(tick_pair):
    e, o = tick_pair("crc32")
    structs = REGS | PC | RESULT
    e.set_campaign(SEED, structs, 1)
    e.set_tick_map("device")
    dev, hist = e.run_tick_trials(0, 6000)
    e.set_tick_map("host")
    ts = o.tick_sample(SEED, 0, 6000, structs)
    _compare(dev, o.run_tick_trials(ts, threads=16), ts)
    assert hist["trials"] == 6000 and hist["guest_insts"] == int(dev["ninst"].sum())


def test_device_boundary_sites_match_oracle(tick_pair):
    e, o = tick_pair("qsort")
    ts = _boundary_sites("qsort", o, 5, 6000)
    e.set_tick_map("device")
    dev, _ = e.run_tick_sites(ts)
    e.set_tick_map("host")
    _compare(dev, o.run_tick_trials(ts, threads=16), ts)


# ---- 5. configurations that change the eff / chunk plumbing
@pytest.fixture(scope="module")
def crc32_host_ref(tick_pair):
    e, _ = tick_pair("crc32")
    e.set_campaign(SEED, REGS | PC | RESULT, 1)
    return e.run_tick_trials(0, 6000)


@pytest.mark.parametrize("kw,n", [({"max_trials_per_launch": 4096}, 6000), ({"flags": 512}, 2000),
                                  ({"flags": 2}, 2000), ({"flags": 64}, 2000), ({"flags": 4}, 2000)],
                         ids=["two_chunks", "no_forward", "no_early_exit", "no_solo", "no_translate"])
def test_device_map_under_configurations(crc32_host_ref, kw, n):
    ref, rh = crc32_host_ref
    e = _timing_engine("crc32", **kw)
    try:
        e.set_campaign(SEED, REGS | PC | RESULT, 1)
        e.set_tick_map("device")
        dev, dh = e.run_tick_trials(0, n)
    finally:
        e.close()
    _compare(dev, ref[:n], np.arange(n))
    assert dh["trials"] == n and dh["guest_insts"] == int(ref[:n]["ninst"].sum())
    if n == len(ref):
        _same_hist(dh, rh)


# ---- 6. the device-resident entry
def test_run_tick_trials_device_entry(oracle_mod, crc32_host_ref):
    import torch
    from shrewd_amd import HIST_DT, OUTCOME_DT
    from test_isa_vectors import clk_branch_sites, clk_program_elf
    n = 3000
    ref, _ = crc32_host_ref
    e = _timing_engine("crc32")
    try:
        e.set_campaign(SEED, REGS | PC | RESULT, 1)
        _, rh = e.run_tick_trials(0, n)
        d_out = torch.zeros(n * OUTCOME_DT.itemsize, dtype=torch.uint8, device="cuda")
        d_hist = torch.zeros(HIST_DT.itemsize, dtype=torch.uint8, device="cuda")
        e.run_tick_trials_device(0, n, d_out.data_ptr(), d_hist.data_ptr())
        e.sync()
        dev = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=OUTCOME_DT)
        hd = np.frombuffer(d_hist.cpu().numpy().tobytes(), dtype=HIST_DT)[0]
        _compare(dev, ref[:n], np.arange(n))
        _same_hist(hd, rh)
        e.run_tick_trials_device(0, n, d_out.data_ptr(), d_hist.data_ptr())   # the histogram accumulates
        e.sync()
        hd2 = np.frombuffer(d_hist.cpu().numpy().tobytes(), dtype=HIST_DT)[0]
        for f in HIST_FIELDS:
            assert np.array_equal(hd2[f], 2 * rh[f]), f
        assert np.array_equal(np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=OUTCOME_DT), ref[:n])
        # the clock escape of tick trials is off again: the same engine, reloaded
        # with a program that reads curTick, runs plain numInst trials as the oracle does
        e.load_elf(clk_program_elf(), ["clk"])
        e.set_cpu_model("atomic")
        e.golden_run()
        o = oracle_mod.Oracle(clk_program_elf(), "clk")
        o.run_golden()
        sites = clk_branch_sites()
        got, _ = e.run_sites(sites)
        want = o.run_trials(sites, protect_mask=0)
        o.close()
        _compare(got, want, sites)
        assert not ((got["cls"] == 5) & (got["sub"] == 7)).any()
    finally:
        e.close()


# ---- 7. refusals: the host path's error, word for word
def _refusal(fn):
    from shrewd_amd.fi import EngineError
    with pytest.raises(EngineError) as ei:
        fn()
    return str(ei.value)


def _both(e, call):
    """The EngineError text of call(e) under the host map and under the device map."""
    e.set_tick_map("host")
    host = _refusal(lambda: call(e))
    e.set_tick_map("device")
    try:
        dev = _refusal(lambda: call(e))
    finally:
        e.set_tick_map("host")
    return host, dev


def test_device_map_refusals(tick_pair):
    import torch
    from shrewd_amd import HIST_DT, Engine
    e, _ = tick_pair("crc32")
    buf = torch.zeros(16 * 64 + HIST_DT.itemsize, dtype=torch.uint8, device="cuda")
    entry = lambda x: x.run_tick_trials_device(0, 64, buf.data_ptr(), buf.data_ptr() + 16 * 64)   # noqa: E731
    # memory words among the structures
    e.set_campaign(SEED, REGS | MEM, 1)
    host, dev = _both(e, lambda x: x.run_tick_trials(0, 64))
    assert host == dev and "memory words" in dev
    assert _refusal(lambda: entry(e)).replace("fi_run_tick_trials_device", "fi_run_tick_trials") == host
    assert "memory words" in _refusal(lambda: e.map_tick_sites_device(None, 0, 64))
    # selective replication on
    e.set_campaign(SEED, REGS | PC, 1)
    e.set_protect(1 << 10)
    host, dev = _both(e, lambda x: x.run_tick_trials(0, 64))
    assert host == dev and "fi_set_protect" in dev
    assert _refusal(lambda: entry(e)).replace("fi_run_tick_trials_device", "fi_run_tick_trials") == host
    e.set_protect(0)
    # explicit sites: tick == golden_ticks, mask == 0
    end = e.tick_info()["golden_ticks"]
    for bad in ((end, 1, 5, 0), (end - 1, 0, 5, 0)):
        ts = np.array([(100, 1, 5, 0), bad], dtype=[("tick", "<u8"), ("mask", "<u8"), ("target", "<u4"),
                                                     ("trial", "<u4")])
        ts["trial"] = np.arange(len(ts))
        host, dev = _both(e, lambda x: x.run_tick_sites(ts))
        assert host == dev and "tick site 1" in dev
        assert "tick site 1" in _refusal(lambda: e.map_tick_sites_device(ts))
    # n == 0: nothing to do
    e.set_tick_map("device")
    out, hist = e.run_tick_trials(0, 0)
    assert len(out) == 0 and hist["trials"] == 0
    out, hist = e.run_tick_sites(np.zeros(0, ts.dtype))
    assert len(out) == 0 and hist["trials"] == 0
    assert all(len(a) == 0 for a in e.map_tick_sites_device(None, 0, 0))
    e.set_tick_map("host")
    # the atomic CPU model has no tick model
    a = Engine()
    try:
        a.load_elf(workload_elf("crc32"), ["crc32"])
        a.golden_run()
        a.set_campaign(SEED, REGS | PC, 1)
        host, dev = _both(a, lambda x: x.run_tick_trials(0, 64))
        assert host == dev and "AtomicSimpleCPU" in dev
        assert _refusal(lambda: entry(a)).replace("fi_run_tick_trials_device", "fi_run_tick_trials") == host
    finally:
        a.close()


# ---- 8. the drivers
def test_fault_campaign_device_map(tmp_path, tick_pair):
    from shrewd_amd import FaultCampaign
    _, o = tick_pair("crc32")
    path = tmp_path / "crc32.elf"
    path.write_bytes(workload_elf("crc32"))
    fc = FaultCampaign(str(path), cmd=["crc32"], trials=3000, seed=SEED, structures=("int_reg", "pc"),
                       cpu_type="timing", tick_map="device")
    try:
        out = fc.run()
        ts = o.tick_sample(SEED, 0, 3000, REGS | PC)
        _compare(out, o.run_tick_trials(ts, threads=16), ts)
        assert fc.summary()["trials"] == 3000
    finally:
        fc.engine.close()
    with pytest.raises(ValueError, match="tick_map"):
        FaultCampaign(str(path), cmd=["crc32"], trials=10, cpu_type="atomic", tick_map="device")


def test_native_cli_device_map(tick_pair, tmp_path):
    import subprocess
    from shrewd_amd import HIST_DT, OUTCOME_DT
    from shrewd_amd import build as b
    exe = b.build_cli()
    e, _ = tick_pair("crc32")
    n = 4000
    e.set_campaign(SEED, REGS | PC, 1)
    ref, rh = e.run_tick_trials(0, n)
    for devices in ("0", "0,0"):
        prefix = str(tmp_path / f"t{devices.count(',')}")
        r = subprocess.run([exe, "--workload", os.path.join(ROOT, "workloads", "crc32.elf"), "--cmd", "crc32",
                            "--trials", str(n), "--seed", hex(SEED), "--structures", "int_reg,pc",
                            "--cpu-type", "timing", "--tick-map", "device", "--devices", devices,
                            "--output", prefix], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = np.fromfile(prefix + ".outcomes.bin", OUTCOME_DT)
        hist = np.fromfile(prefix + ".hist.bin", HIST_DT)[0]
        assert out.tobytes() == ref.tobytes()
        assert hist["counts"].tobytes() == rh["counts"].tobytes()
