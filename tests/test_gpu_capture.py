"""Output capture on the device (fi_run_sites_capture): every
trial's stdout against the oracle's serial run of the same site, stderr by
self-consistency and by hand-derived cases, and the same streams under every
execution path, cap, launch size and the second pass."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import ROOT, workload_elf
from test_capture_cpu import OUTS_MSG, outs_elf, outs_model
from test_isa_vectors import SYS_STDERR, sys_program_elf, sys_program_expected

pytestmark = pytest.mark.gpu

REGS = (1 << 32) - 2
PC = 1 << 32
MEM = 1 << 33
SEED = 0x5EED0001
CAP = 4096
T_MEM = 33
MASKED, SDC = 0, 1
END_EXIT = 0    # the golden end sub-code of every program here: an exit syscall

# program -> (structures, sites, Engine arguments of its default configuration)
PROGRAMS = {"outs": (REGS | PC | MEM, 1500, {"snapshot_interval": 256}),
            "crc32": (REGS | PC, 1000, {}),
            "qsort": (REGS | PC | MEM, 1000, {}),
            "sys": (REGS | PC | MEM, 1000, {})}


def program_elf(name: str) -> bytes:
    if name == "outs":
        return outs_elf()
    if name == "sys":
        return sys_program_elf()
    return workload_elf(name)


@pytest.fixture(scope="module")
def engines():
    """make(program, wait=True, **Engine arguments on top of the program's own) -> a loaded engine, kept."""
    from shrewd_amd import Engine, build_library
    build_library()
    cache = {}

    def make(name, wait=True, **kw):
        kw = {**PROGRAMS[name][2], **kw}
        key = (name, wait, tuple(sorted(kw.items())))
        if key not in cache:
            e = Engine(**kw)
            e.load_elf(program_elf(name), [name])
            e.golden_run(wait_translation=wait)
            e.set_campaign(SEED, PROGRAMS[name][0], 1)
            cache[key] = e
        return cache[key]

    yield make
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def reference(engines):
    """ref(program) -> (sites, outcomes, hist, capture) of the default configuration, computed once."""
    cache = {}

    def ref(name):
        if name not in cache:
            e = engines(name)
            sites = e.sample(0, PROGRAMS[name][1])
            cache[name] = (sites,) + e.run_sites_capture(sites, cap_bytes=CAP)
        return cache[name]

    return ref


def same_streams(cap, want, what=""):
    for f in ("out_len", "err_len", "out", "err"):
        a, b = getattr(cap, f), getattr(want, f)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {f} differs for {len(bad)} of {len(a)} trials, first {int(bad[0])}: "
                                 f"stdout {cap.stdout(int(bad[0]))!r} / {want.stdout(int(bad[0]))!r}, "
                                 f"lengths {int(cap.out_len[bad[0]])}, {int(cap.err_len[bad[0]])} / "
                                 f"{int(want.out_len[bad[0]])}, {int(want.err_len[bad[0]])}")


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_stdout_equals_oracle_run(reference, oracle_mod, name):
    from concurrent.futures import ThreadPoolExecutor
    sites, out, _, cap = reference(name)
    workers = 4

    def serial_runs(k):   # (an oracle of its own per thread; the calls release the GIL)
        o = oracle_mod.Oracle(program_elf(name), name)
        o.run_golden()
        return [o.run_one(s) for s in sites[k::workers]]

    runs = [None] * len(sites)
    with ThreadPoolExecutor(workers) as ex:
        for k, part in enumerate(ex.map(serial_runs, range(workers))):
            runs[k::workers] = part
    bad = []
    for i in range(len(sites)):
        res, stdout = runs[i]
        assert len(stdout) < 1 << 16    # (run_one's own buffer: the whole stream)
        if out[i] != res or cap.stdout(i) != stdout or int(cap.out_len[i]) != len(stdout):
            bad.append((i, sites[i], out[i], res, cap.stdout(i), int(cap.out_len[i]), stdout))
    assert not bad, f"{len(bad)} of {len(sites)} trials differ from the oracle; first: {bad[0]}"


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_outcomes_equal_run_sites(engines, reference, name):
    sites, out, hist, _ = reference(name)
    out2, hist2 = engines(name).run_sites(sites)
    assert np.array_equal(out, out2)
    assert hist.tobytes() == hist2.tobytes()


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_streams_are_consistent_with_classes(engines, reference, name):
    sites, out, _, cap = reference(name)
    e = engines(name)
    gout, gerr, gexit = e.golden_stdout(), e.golden_stderr(), e.golden.exit_code & 0xFF
    n_checked = 0
    for i in range(len(sites)):
        if out[i]["cls"] in (MASKED, SDC):
            golden = (cap.stdout(i) == gout and cap.stderr(i) == gerr and int(cap.out_len[i]) == len(gout) and
                      int(cap.err_len[i]) == len(gerr) and out[i]["exit_code"] == gexit and out[i]["sub"] == END_EXIT)
            assert golden == (out[i]["cls"] == MASKED), (i, sites[i], out[i], cap.stdout(i), cap.stderr(i))
            n_checked += 1
        for buf, ln in ((cap.out, cap.out_len), (cap.err, cap.err_len)):
            assert not buf[i, min(int(ln[i]), CAP):].any(), (i, "bytes past the stream's end")
    assert n_checked


def vaddr_of(elf: bytes, needle: bytes) -> int:
    """The address the bytes `needle` of the file are loaded at (PT_LOAD headers)."""
    off = elf.index(needle)
    assert elf.find(needle, off + 1) < 0
    phoff, = struct.unpack_from("<Q", elf, 0x20)
    phentsize, phnum = struct.unpack_from("<HH", elf, 0x36)
    for k in range(phnum):
        p_type, _, p_offset, p_vaddr, _, p_filesz = struct.unpack_from("<IIQQQQ", elf, phoff + k * phentsize)
        if p_type == 1 and p_offset <= off < p_offset + p_filesz:
            return p_vaddr + (off - p_offset)
    raise AssertionError("not in a PT_LOAD segment")


@pytest.mark.parametrize("name,msg", [("sys", SYS_STDERR), ("outs", OUTS_MSG)])
def test_stderr_of_a_flipped_message(engines, name, msg):
    """Bit 0 of the message's first byte flipped in memory before the first
    instruction: every write of it to fd 2 carries the flipped byte."""
    from shrewd_amd import SITE_DT
    e = engines(name)
    a = vaddr_of(program_elf(name), msg)
    site = np.zeros(1, SITE_DT)
    site["inst"], site["target"], site["addr"], site["mask"] = 0, T_MEM, a & ~7, 1 << (8 * (a & 7))
    out, _, cap = e.run_sites_capture(site, cap_bytes=CAP)
    flipped = bytes([msg[0] ^ 1]) + msg[1:]
    if name == "sys":
        want_out, want_err = sys_program_expected(), flipped
    else:
        want_out, want_err = outs_model(flipped)
        assert want_err == flipped * 6
    assert out[0]["cls"] == SDC
    assert cap.stderr(0) == want_err and int(cap.err_len[0]) == len(want_err)
    assert cap.stdout(0) == want_out == e.golden_stdout() and int(cap.out_len[0]) == len(want_out)


def _flags():
    from shrewd_amd import fi
    return {"NO_SNAPSHOT_START|NO_EARLY_EXIT": fi.CFG_NO_SNAPSHOT_START | fi.CFG_NO_EARLY_EXIT,
            "NO_EPOCHS": fi.CFG_NO_EPOCHS, "NO_TRANSLATE": fi.CFG_NO_TRANSLATE, "NO_SOLO": fi.CFG_NO_SOLO,
            "SOLO_ALL": fi.CFG_SOLO_ALL, "SOLO_ALL|NO_TRANSLATE": fi.CFG_SOLO_ALL | fi.CFG_NO_TRANSLATE,
            "PACK_RUNS": fi.CFG_PACK_RUNS, "FIXED_RESUME": fi.CFG_FIXED_RESUME, "SIMT": fi.CFG_SIMT,
            "NO_FORWARD": fi.CFG_NO_FORWARD, "NO_SDC_EXIT": fi.CFG_NO_SDC_EXIT, "NO_HANG_PROOF": fi.CFG_NO_HANG_PROOF,
            "NO_ODD_KERNEL": fi.CFG_NO_ODD_KERNEL}


FLAG_NAMES = ["NO_SNAPSHOT_START|NO_EARLY_EXIT", "NO_EPOCHS", "NO_TRANSLATE", "NO_SOLO", "SOLO_ALL",
              "SOLO_ALL|NO_TRANSLATE", "PACK_RUNS", "FIXED_RESUME", "SIMT", "NO_FORWARD", "NO_SDC_EXIT",
              "NO_HANG_PROOF", "NO_ODD_KERNEL"]


@pytest.mark.parametrize("flag", FLAG_NAMES)
@pytest.mark.parametrize("name", ["outs", "crc32"])
def test_streams_equal_under_every_path(engines, reference, name, flag):
    """(NO_SNAPSHOT_START|NO_EARLY_EXIT composes nothing from the golden
    stream: agreement with it is the check of the prefix and suffix rules.)"""
    sites, out, _, want = reference(name)
    got_out, _, cap = engines(name, flags=_flags()[flag]).run_sites_capture(sites, cap_bytes=CAP)
    same_streams(cap, want, f"{name} {flag}")
    assert np.array_equal(got_out["cls"], out["cls"])


@pytest.mark.parametrize("flags", [0, 4], ids=["translate", "NO_TRANSLATE"])
@pytest.mark.parametrize("name", ["outs", "crc32"])
def test_streams_equal_before_and_after_translation(reference, name, flags):
    """The static kernels (until the load-time build lands) and the translated ones."""
    from shrewd_amd import Engine
    sites, _, _, want = reference(name)
    e = Engine(flags=flags, **PROGRAMS[name][2])
    try:
        e.load_elf(program_elf(name), [name])
        e.golden_run(wait_translation=False)
        same_streams(e.run_sites_capture(sites, cap_bytes=CAP)[2], want, f"{name} before wait_translation")
        e.wait_translation()
        same_streams(e.run_sites_capture(sites, cap_bytes=CAP)[2], want, f"{name} after wait_translation")
    finally:
        e.close()


@pytest.mark.parametrize("cap_bytes", [8, 200])
def test_truncation(engines, reference, cap_bytes):
    sites, out, _, want = reference("outs")
    assert int(want.out_len.max()) > 200 > 192 == len(engines("outs").golden_stdout())
    got_out, _, cap = engines("outs").run_sites_capture(sites, cap_bytes=cap_bytes)
    assert np.array_equal(got_out, out)
    assert cap.out.shape == cap.err.shape == (len(sites), cap_bytes)
    assert np.array_equal(cap.out_len, want.out_len) and np.array_equal(cap.err_len, want.err_len)
    assert np.array_equal(cap.out, want.out[:, :cap_bytes]) and np.array_equal(cap.err, want.err[:, :cap_bytes])
    long = np.nonzero(want.out_len > cap_bytes)[0]
    assert len(long) and all(len(cap.stdout(int(i))) == cap_bytes for i in long)


def test_chunks_and_second_pass(engines):
    """Launch size changes no stream; neither does the second pass of the
    trials that ran out of private pages (P = 1, no overflow pool: every chunk
    has some), which writes into the rows its first pass began."""
    from shrewd_amd import STAT
    from shrewd_amd.fi import CFG_NO_OVERFLOW
    for name in ("outs", "crc32"):
        one = engines(name)
        one.set_campaign(SEED, REGS | PC | MEM, 1)
        sites = one.sample(0, 3000)
        one.set_campaign(SEED, PROGRAMS[name][0], 1)
        out, hist, want = one.run_sites_capture(sites, cap_bytes=CAP)
        small = engines(name, max_trials_per_launch=1024)
        redo = engines(name, max_trials_per_launch=1024, private_pages=1, flags=CFG_NO_OVERFLOW)
        for e, what in ((small, "1024 per launch"), (redo, "second pass")):
            got = e.run_sites_capture(sites, cap_bytes=CAP)
            assert np.array_equal(got[0], out), (name, what)
            for f in ("counts", "crash_sub", "escape_sub", "trials", "guest_insts"):
                assert np.array_equal(got[1][f], hist[f]), (name, what, f)
            same_streams(got[2], want, f"{name} {what}")
        assert int(redo.debug_stats()[STAT.REDO_TRIALS]) > 0, f"{name}: no resource escape to redo"


def test_arguments(engines):
    from shrewd_amd.fi import FI_OK, OUTCOME_DT
    FI_E_ARG = -1
    e = engines("outs")
    sites = e.sample(0, 4)
    out = np.zeros(4, OUTCOME_DT)
    buf = np.zeros((4, 64), np.uint8)

    def call(n, cap_bytes, out_buf):
        return e.L.fi_run_sites_capture(e.h, sites.ctypes.data, n, cap_bytes, out.ctypes.data, None, out_buf, None, None)

    for n, cap_bytes, out_buf, word in ((4, 0, buf.ctypes.data, "cap_bytes"), (4, (1 << 20) + 1, buf.ctypes.data, "cap_bytes"),
                                        (4, 64, None, "out_buf")):
        assert call(n, cap_bytes, out_buf) == FI_E_ARG
        assert word in e.L.fi_last_error(e.h).decode()
    assert call(0, 64, None) == FI_OK
    assert call(4, 64, buf.ctypes.data) == FI_OK     # err_buf, lens and hist NULL
    assert np.array_equal(buf, e.run_sites_capture(sites, cap_bytes=64)[2].out)
    empty = e.run_sites_capture(sites[:0], cap_bytes=64)
    assert len(empty[0]) == 0 and empty[2].out.shape == (0, 64)


def test_campaign_outputs():
    from shrewd_amd import FaultCampaign
    c = FaultCampaign(os.path.join(ROOT, "workloads", "hello.elf"), cmd=["hello"], trials=2000)
    try:
        out = c.run()
        assert c.engine.golden_stdout() == b"Hello world!\n"
        ids = [c.first + int(i) for i in np.nonzero(out["cls"] == SDC)[0]]
        assert ids, "no SDC among the 2,000 trials"
        res = c.outputs(ids)
        assert sorted(res) == ids
        for t in ids:
            o, stdout, stderr = res[t]
            assert o == out[t - c.first]
            assert stdout != b"Hello world!\n" or o["exit_code"] != c.golden.exit_code & 0xFF, (t, o, stdout)
            assert isinstance(stderr, bytes)
        assert c.outputs([]) == {}
    finally:
        c.engine.close()
