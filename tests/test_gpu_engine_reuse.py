"""An engine that has been through something else equals a fresh engine.

The other GPU tests pin the engine against the oracle.  These pin it against
itself: whatever an engine loaded, ran or grew before, the next load and golden
run must leave it where a new engine would be -- the golden facts, the golden
streams, the sampled sites, every outcome and every histogram field.  Each case
uses the smallest workloads the repository has (hello, fpamo, and the rnd / vm
known-answer programs) and 512 trials over registers, the pc and memory words.

GoldenInfo.translate_us is a wall-clock duration of the background build (0 from
a warm cache), not engine state: it is the one field left out of the comparison.
"""
import numpy as np
import pytest

from conftest import workload_elf

pytestmark = pytest.mark.gpu

N = 512
REGS_PC = ((1 << 32) - 2) | (1 << 32)
MEM = 1 << 33
SEED = 0x5EED2E05
GOLDEN_FIELDS = ("ninst", "ncycles", "exit_code", "stdout_len", "stderr_len", "fetch_bytes", "data_bytes", "snapshots",
                 "snapshot_interval", "snapshot_frames", "translated_blocks", "translated_insts")


def _kat(name):
    import test_isa_vectors as kat
    return {"vm": kat.vm_program_elf, "rnd": kat.rnd_program_elf}[name]()


def _engine(**kw):
    from shrewd_amd import Engine
    from shrewd_amd.fi import CFG_NO_TRANSLATE
    kw.setdefault("flags", CFG_NO_TRANSLATE)
    return Engine(**kw)


def _hist_dict(h):
    return {f: np.array(h[f]) for f in h.dtype.names}


def _observe(e, g, n=N, structs=REGS_PC | MEM):
    """Everything every case compares: golden facts and streams, the sampled
    sites, their outcomes and the histogram."""
    e.set_campaign(SEED, structs, 1)
    sites = e.sample(0, n)
    out, hist = e.run_sites(sites)
    return {"golden": {f: int(getattr(g, f)) for f in GOLDEN_FIELDS}, "stdout": e.golden_stdout(),
            "stderr": e.golden_stderr(), "sites": sites, "out": out, "hist": _hist_dict(hist)}


def _same(used, fresh, path=""):
    assert type(used) is type(fresh), path
    if isinstance(used, dict):
        assert used.keys() == fresh.keys(), path
        for k in used:
            _same(used[k], fresh[k], f"{path}/{k}")
    elif isinstance(used, np.ndarray):
        assert used.shape == fresh.shape, f"{path}: shape {used.shape} != {fresh.shape}"
        bad = np.argwhere(used != fresh)
        assert not len(bad), f"{path}: {len(bad)} differ, first at {tuple(bad[0])}: " \
                             f"{used[tuple(bad[0])]} != {fresh[tuple(bad[0])]}"
    else:
        assert used == fresh, f"{path}: {used!r} != {fresh!r}"


def _fresh_hello(extra=None, **kw):
    e = _engine(**kw)
    e.load_elf(workload_elf("hello"), ["hello"])
    g = e.golden_run()
    obs = _observe(e, g)
    if extra:
        obs.update(extra(e))
    e.close()
    return obs


def _mem_info(e):
    d = e.exact_mem_info().as_dict()
    d.pop("build_ms")
    return d


def test_fp_golden_state_does_not_reach_the_next_image():
    """fpamo's golden run writes FP state (no snapshot start, no early exit);
    hello's must not inherit it."""
    def exact(e):
        e.set_campaign(SEED, REGS_PC, 1)
        return {"exact": e.exact_info().as_dict()}
    e = _engine()
    e.load_elf(workload_elf("fpamo"), ["fpamo"])
    e.golden_run()
    e.set_campaign(SEED, REGS_PC | MEM, 1)
    e.run_sites(e.sample(0, N))
    e.load_elf(workload_elf("hello"), ["hello"])
    g = e.golden_run()
    used = _observe(e, g)
    used.update(exact(e))
    e.close()
    _same(used, _fresh_hello(exact))


def test_checkpoint_start_state_does_not_reach_a_plain_load(oracle_mod, tmp_path):
    """A checkpoint's FP registers, fcsr, VMA list and tick leave with it."""
    elf = workload_elf("fpamo")
    o = oracle_mod.Oracle(elf, "fpamo")
    k = max(1, int(o.run_golden().ninst * 0.6))
    d = str(tmp_path / "fp_cpt")
    o.write_checkpoint(k, d)
    e = _engine(private_pages=64)
    e.load_checkpoint(d, elf)
    e.golden_run()
    e.set_campaign(SEED, REGS_PC | MEM, 1)
    e.run_sites(e.sample(0, N))
    e.load_elf(workload_elf("hello"), ["hello"])
    g = e.golden_run()
    used = _observe(e, g)
    e.close()
    _same(used, _fresh_hello(private_pages=64))


def test_curtick_reader_does_not_reach_the_next_tick_model():
    """rnd's golden run reads curTick, which refuses the tick model; hello's
    tick model on the same engine is a fresh engine's."""
    def tick(e):
        e.set_campaign(SEED, REGS_PC, 1)
        out, hist = e.run_tick_trials(0, N)
        return {"tick_info": e.tick_info(), "tick_out": out, "tick_hist": _hist_dict(hist)}

    def run(e):
        e.load_elf(workload_elf("hello"), ["hello"])
        e.set_cpu_model("timing")
        g = e.golden_run()
        obs = _observe(e, g)
        obs.update(tick(e))
        e.close()
        return obs
    e = _engine(private_pages=64)
    e.load_elf(_kat("rnd"), ["rnd"])
    e.golden_run()
    used = run(e)
    assert used["tick_info"]["status"] == ""
    _same(used, run(_engine(private_pages=64)))


def test_unmapping_golden_run_does_not_reach_exact_memory():
    """vm's golden run unmaps memory, which refuses exact memory classes;
    hello's on the same engine are accepted and a fresh engine's."""
    def mem(e):
        e.set_exact_memory(True)
        e.set_campaign(SEED, REGS_PC | MEM, 1)
        return {"exact_mem": _mem_info(e)}
    e = _engine(private_pages=64)
    e.load_elf(_kat("vm"), ["vm"])
    e.golden_run()
    e.load_elf(workload_elf("hello"), ["hello"])
    g = e.golden_run()
    used = _observe(e, g)
    used.update(mem(e))
    e.close()
    _same(used, _fresh_hello(mem, private_pages=64))


def test_second_golden_run_equals_the_first():
    """atomic, timing, atomic golden runs of hello on one engine, each taken
    twice: the last is a single atomic one, and the tick model says so.
    (fi_set_cpu_model is refused once an image has a golden run, so the image
    is loaded again before the model changes; the repeated golden_run() is the
    second golden run of one image.)"""
    def tick(e):
        return {"tick_info": e.tick_info()}
    e = _engine()
    for model in (None, "timing", "atomic"):
        e.load_elf(workload_elf("hello"), ["hello"])
        if model:
            e.set_cpu_model(model)
        e.golden_run()
        g = e.golden_run()
    used = _observe(e, g)
    used.update(tick(e))
    e.close()
    assert "AtomicSimpleCPU" in used["tick_info"]["status"]
    _same(used, _fresh_hello(tick))


def test_translated_kernels_do_not_cross_a_load():
    """hello's translated kernels are unloaded by the next load; fpamo runs on
    its own."""
    def run(e):
        e.load_elf(workload_elf("fpamo"), ["fpamo"])
        g = e.golden_run(wait_translation=True)
        obs = _observe(e, g)
        obs["translate_status"] = e.translate_status()
        e.close()
        return obs
    e = _engine(flags=0)
    e.load_elf(workload_elf("hello"), ["hello"])
    e.golden_run(wait_translation=True)
    e.set_campaign(SEED, REGS_PC | MEM, 1)
    e.run_sites(e.sample(0, N))
    _same(run(e), run(_engine(flags=0)))


def _fresh_each(make, steps):
    """Each step on an engine of its own."""
    fresh = {}
    for name, step in steps:
        e = make()
        fresh[name] = step(e)
        e.close()
    return fresh


def test_sources_do_not_leak_across_slots():
    """Every kind of run leaves the two chunk slots (sites, outcomes, weights,
    the tick map's and the capture's buffers) as the next kind expects them:
    runs of different sources in a row on one engine equal the same calls on
    fresh engines.  hello's exact campaign over x1..x31 | pc | result is 1,920
    trials; chunks of 1,000 use both slots and end on a partial chunk."""
    RESULT = 1 << 34

    def exact(e, profile=False):
        e.set_campaign(SEED, REGS_PC | RESULT, 1)
        n = int(e.exact_info().trials)
        assert n > 1000 and n % 1000
        r = e.run_exact(0, n, profile=profile)
        obs = {"out": r[0], "hist": _hist_dict(r[1])}
        if profile:
            obs["prof"] = r[2]
        return obs

    def capture(e):
        e.set_campaign(SEED, REGS_PC | MEM, 1)
        out, hist, cap = e.run_sites_capture(e.sample(0, 1500), cap_bytes=64)
        return {"out": out, "hist": _hist_dict(hist), "stdout": cap.out, "stderr": cap.err, "out_len": cap.out_len,
                "err_len": cap.err_len}

    def trials(e):
        e.set_campaign(SEED, REGS_PC | MEM, 1)
        out, hist = e.run_trials(0, 2500)
        return {"out": out, "hist": _hist_dict(hist)}

    def atomic():
        e = _engine(max_trials_per_launch=1000)
        e.load_elf(workload_elf("hello"), ["hello"])
        e.golden_run()
        return e
    steps = [("exact", exact), ("capture", capture), ("profile", lambda e: exact(e, True)), ("trials", trials),
             ("exact again", exact)]
    e = atomic()
    used = {name: step(e) for name, step in steps}
    e.close()
    _same(used, _fresh_each(atomic, steps))
    _same(used["exact again"], used["exact"])

    # the timing model with the device map: the tick map's buffers and the 64-bit weights are made on
    # first use and dropped when the work buffers grow -- from the exact tick campaign's trials to
    # 1,500 to 3,000 slots here
    def exact_ticks(e):
        e.set_campaign(SEED, REGS_PC | RESULT, 1)
        e.set_bits(0xFFFF)
        n = int(e.exact_tick_info().trials)
        assert 0 < n < 1500
        out, hist = e.run_exact_ticks(0, n)
        return {"out": out, "hist": _hist_dict(hist)}

    def tick_trials(e):
        e.set_campaign(SEED, REGS_PC, 1)
        out, hist = e.run_tick_trials(0, 1500)
        return {"out": out, "hist": _hist_dict(hist)}

    def sites(e):
        e.set_campaign(SEED, REGS_PC | MEM, 1)
        out, hist = e.run_sites(e.sample(0, 3000))
        return {"out": out, "hist": _hist_dict(hist)}

    def timing():
        e = _engine(max_trials_per_launch=4096)
        e.load_elf(workload_elf("hello"), ["hello"])
        e.set_cpu_model("timing")
        e.golden_run()
        e.set_tick_map("device")
        return e
    steps = [("exact ticks", exact_ticks), ("tick trials", tick_trials), ("sites", sites),
             ("exact ticks again", exact_ticks)]
    e = timing()
    used = {name: step(e) for name, step in steps}
    e.close()
    _same(used, _fresh_each(timing, steps))
    _same(used["exact ticks again"], used["exact ticks"])


def test_work_growth_equals_a_fresh_engine():
    """Work buffers grown from 64 to 256 slots, with the tick and capture
    buffers already made at 64: three-chunk runs equal a fresh engine's."""
    def make():
        e = _engine(max_trials_per_launch=256)
        e.load_elf(workload_elf("hello"), ["hello"])
        e.set_cpu_model("timing")
        g = e.golden_run()
        e.set_tick_map("device")
        return e, g

    def runs(e, g, n, n_cap):
        obs = _observe(e, g, n)
        e.set_campaign(SEED, REGS_PC, 1)
        out, hist = e.run_tick_trials(0, n)
        obs.update(tick_out=out, tick_hist=_hist_dict(hist))
        e.set_campaign(SEED, REGS_PC | MEM, 1)
        out, hist, cap = e.run_sites_capture(obs["sites"][:n_cap], cap_bytes=64)
        obs.update(cap_out=out, cap_hist=_hist_dict(hist), cap_stdout=cap.out, cap_stderr=cap.err,
                   cap_out_len=cap.out_len, cap_err_len=cap.err_len)
        return obs
    e, g = make()
    runs(e, g, 64, 64)
    used = runs(e, g, 600, 300)
    e.close()
    e, g = make()
    fresh = runs(e, g, 600, 300)
    e.close()
    _same(used, fresh)
