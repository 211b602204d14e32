"""Check-free stretches of the clean solo body (fi_translate.cpp)
against the oracle, through the C ABI.

The `stretch` programs run the loop shapes a stretch covers, mix every value
they read into one checksum and print it.  They are two programs, `walks`
(L1..L3) and `reentry` (L4, L5), because the clean body has eight site caches
and every load and store inside a cycle takes one.

 L1  crc32's shape: a byte walk, step +1, across a page boundary, each byte
     indexing a 1 KiB table of words in an initialised page nothing writes
     (a walking site that holds its next value, and a bounded site);
 L2  a word walk, step -4, that crosses the boundary downwards, with a table
     whose base + range straddles the boundary: never a stretch, and the
     bytes walked were written by the trial itself (private frames);
 L3  a counted loop with a bounded site only; a flipped counter runs it to
     the hang cap;
 L4  an inner byte walk whose next run starts where the last one stopped,
     after the outer block has rewritten that byte;
 L5  the same over an initialised .data page nothing wrote before: the outer
     block's first store turns the shared page into a private one.

Sites: sampled register and pc flips (injection points and snapshot
boundaries fall inside the loops), and hand-placed ones at pass boundaries:
single bits of the pointers, bounds and counters; the bound moved so that the
loop's exit is taken on the first and on the last pass of a stretch; the
table's base moved so that its range straddles a page, ends on a page's last
bytes misaligned, lies in an unmapped page and in the zero page.

Every record must equal the oracle's with the stretches on and off
(FI_CFG_NO_LOOP_STRETCH): on the default path, with every trial on the solo
kernel from the start (FI_CFG_SOLO_ALL), there also without the loop proofs
(FI_CFG_NO_HANG_PROOF: long walks are executed, not proved), and with short
epochs and close snapshots (epoch_iters=8: budgets end inside the loops).  The
counters the step's figures are made of must not depend on the flag."""
import re

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
LCG = 1103515245
FILL = 64            # bytes filled on each side of the boundary
L1_SPAN = 60         # L1 reads [pgb - 60, pgb + 60)
L3_PASSES = 40
OUTER = 5            # runs of L4's / L5's inner loop, 8 bytes each
TBL = [(0x9E3779B1 * (i + 1) ^ (i << 20)) & 0xFFFFFFFF for i in range(256)]
DBUF = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0x8796A5B4C3D2E1F0, 0x13579BDF02468ACE,
        0xECA86420FDB97531]
MIX = "add   s6, s6, t1\n    slli  t5, s6, 3\n    xor   s6, s6, t5"
PARTS = {"walks": ("L1", "L2", "L3"), "reentry": ("L4", "L5")}


def _crc_pass(load, ptr, base, step):
    return f"""    {load}   t1, 0({ptr})
    xor   t2, s6, t1
    andi  t2, t2, 255
    slli  t2, t2, 2
    add   t2, t2, {base}
    lwu   t2, 0(t2)
    srli  s6, s6, 8
    xor   s6, s6, t2
    addi  {ptr}, {ptr}, {step}"""


def stretch_program_source(part: str) -> str:
    head = f"""    .text
_start:
    la    s0, pgb
    li    s9, {LCG}
    li    s6, 0
    addi  t2, s0, -{FILL}
    li    t0, {2 * FILL // 8}
    li    t3, 1
fill:
    mul   t3, t3, s9
    addi  t3, t3, 1234
    sd    t3, 0(t2)
    addi  t2, t2, 8
    addi  t0, t0, -1
    bnez  t0, fill
"""
    walks = f"""    la    s2, tbl
    addi  a0, s0, -{L1_SPAN}
    addi  a1, s0, {L1_SPAN}
L1:
{_crc_pass("lbu", "a0", "s2", 1)}
    bne   a0, a1, L1
    li    t0, -512
    add   s3, s0, t0
    addi  a0, s0, 16
    addi  a1, s0, -24
L2:
{_crc_pass("lw ", "a0", "s3", -4)}
    bne   a0, a1, L2
    li    t0, {L3_PASSES}
L3:
    andi  t2, s6, 255
    add   t2, t2, s2
    lbu   t1, 0(t2)
    {MIX}
    addi  t0, t0, -1
    bnez  t0, L3
"""

    def rerun(outer, inner, start):
        return f"""{start}
    mv    a1, a0
    li    s5, {OUTER}
{outer}:
    addi  a1, a1, 8
{inner}:
    lbu   t1, 0(a0)
    {MIX}
    addi  a0, a0, 1
    bne   a0, a1, {inner}
    lbu   t3, 0(a0)
    xori  t3, t3, 0x5a
    sb    t3, 0(a0)
    addi  s5, s5, -1
    bnez  s5, {outer}
"""
    reentry = rerun("O4", "L4", f"    addi  a0, s0, -{FILL}") + rerun("O5", "L5", "    la    a0, dbuf")
    tail = f"""    la    a1, out
    sd    s6, 0(a1)
    li    a0, 1
    li    a2, 8
    li    a7, 64
    ecall
    li    a0, 0
    li    a7, 93
    ecall
    .data
    .balign 4096
tbl:
{chr(10).join(f"    .word {v:#x}" for v in TBL)}
dbuf:
{chr(10).join(f"    .dword {v:#x}" for v in DBUF)}
    .bss
    .balign 4096
pga:
    .zero 4096
pgb:
    .zero 4096
out:
    .zero 8
    .balign 4096
pgz:
    .zero 4096
"""
    return head + {"walks": walks, "reentry": reentry}[part] + tail


def stretch_program_asm(part: str):
    """(elf, labels)"""
    from tools.rvasm.rvasm import Assembler
    a = Assembler(compress=False)
    elf = a.assemble(stretch_program_source(part))
    return elf, dict(a.labels)


def stretch_program_expected(part: str) -> bytes:
    """The program in plain Python: the checksum it prints."""
    mem = bytearray(1024)                # [pgb - 512, pgb + 512)
    t3 = 1
    for k in range(2 * FILL // 8):
        t3 = (t3 * LCG + 1234) & M64
        mem[512 - FILL + 8 * k:512 - FILL + 8 * k + 8] = t3.to_bytes(8, "little")
    s6 = 0

    def mix(v):
        nonlocal s6
        s6 = (s6 + v) & M64
        s6 ^= (s6 << 3) & M64

    def rd(buf, off, size):
        return int.from_bytes(buf[off:off + size], "little")
    if part == "walks":
        for a in range(-L1_SPAN, L1_SPAN):                       # L1
            s6 = (s6 >> 8) ^ TBL[(s6 ^ mem[512 + a]) & 255]
        for a in range(16, -24, -4):                             # L2 (the table: the memory around pgb itself)
            s6 = (s6 >> 8) ^ rd(mem, 4 * ((s6 ^ rd(mem, 512 + a, 4)) & 255), 4)
        tb = b"".join(v.to_bytes(4, "little") for v in TBL)
        for _ in range(L3_PASSES):                               # L3
            mix(tb[s6 & 255])
    else:
        for buf, a in ((mem, 512 - FILL), (bytearray(b"".join(v.to_bytes(8, "little") for v in DBUF)), 0)):   # L4, L5
            for _ in range(OUTER):
                for _ in range(8):
                    mix(buf[a])
                    a += 1
                buf[a] ^= 0x5A
    return s6.to_bytes(8, "little")


# loop -> (pointer or counter register, bound register (0: none), table base register (0: none), passes)
LOOPS = {"L1": (10, 11, 18, 2 * L1_SPAN), "L2": (10, 11, 19, 10), "L3": (5, 0, 18, L3_PASSES),
         "L4": (10, 11, 0, 8 * OUTER), "L5": (10, 11, 0, 8 * OUTER)}
N_RANDOM = 2000
# the stretches each program's text must hold, in block order: (insts a pass, walking sites as
# (step, size, held), bounded sites as (lowest offset, highest offset + size))
STRETCHES = {"walks": [(10, [(1, 1, 1)], [(0, 1024)]), (10, [(-4, 4, 1)], [(0, 1024)]), (8, [], [(0, 256)])],
             "reentry": [(6, [(1, 1, 1)], []), (6, [(1, 1, 1)], [])]}


def _pass_starts(trace, text_lo, lab, part):
    insts = trace[(trace >> 31) == 0]
    pcs = text_lo + 2 * insts.astype(np.int64)
    return {name: np.nonzero(pcs == lab[name])[0] for name in PARTS[part]}


def stretch_sites(o, ninst, starts, lab, part):
    from oracle.pyoracle import SITE_DT
    rnd = o.sample(0x5EED0A4E, 0, N_RANDOM, ((1 << 32) - 2) | (1 << 32))
    ex = []
    for name in PARTS[part]:
        ptr, bound, base, _ = LOOPS[name]
        st = starts[name]
        for k in (0, 1, len(st) // 2, len(st) - 2):
            for bit in (0, 1, 2, 3, 5, 11, 12, 13, 20, 31, 47, 63):
                for reg in (ptr, bound, base):
                    if reg:
                        ex.append((int(st[k]), reg, 1 << bit))
    if part == "walks":
        pgb, tbl, pgz = lab["pgb"], lab["tbl"], lab["pgz"]
        st = starts["L1"]
        for k in (1, 7):
            p, a1 = pgb - L1_SPAN + k, pgb + L1_SPAN
            # the exit on the first pass of a stretch, and on its last (the stretch of a walk that
            # holds its next byte ends one byte before the page's last)
            for to in (p + 1, pgb - 1, pgb - 2, pgb):
                ex.append((int(st[k]), 11, a1 ^ to))
            # the table's base: straddling, onto a page's last bytes and misaligned, misaligned
            # inside its page, in an unmapped page, in the zero page
            for to in (tbl + 3584, tbl + 3075, tbl + 3072, tbl + 1, 0x2000, 0x2FFC, pgz, pgz + 3072, pgz + 3073):
                ex.append((int(st[k]), 18, tbl ^ to))
        st = starts["L2"]
        for to in (pgb - 1024, pgb, tbl, pgz, 0x2000):           # L2's base into one page
            ex.append((int(st[1]), 19, (pgb - 512) ^ to))
        for to in (pgb + 12 - 4, pgb, pgb + 4, pgb - 4):          # L2's exit: first pass, at the page's edge
            ex.append((int(st[1]), 11, (pgb - 24) ^ to))
        st = starts["L3"]
        for bit in (40, 50, 62):                                 # L3 to the hang cap
            ex.append((int(st[2]), 5, 1 << bit))
    s = np.zeros(len(ex), SITE_DT)
    for i, (inst, target, mask) in enumerate(ex):
        s["inst"][i], s["target"][i], s["mask"][i] = min(inst, ninst - 1), target, mask & M64
    s = np.concatenate([rnd, s])
    s["trial"] = np.arange(len(s))
    return s


_REF = {}


@pytest.fixture(scope="module")
def stretch_ref(oracle_mod):
    """part -> (elf, sites, the oracle's outcomes): computed once per program."""
    def get(part):
        if part in _REF:
            return _REF[part]
        from shrewd_amd import Engine
        elf, lab = stretch_program_asm(part)
        o = oracle_mod.Oracle(elf, "stretch")
        g = o.run_golden()
        assert o.golden_stdout() == stretch_program_expected(part)
        assert 600 <= g.ninst <= 4000, g.ninst
        e = Engine()
        try:
            e.load_elf(elf, ["stretch"])
            e.golden_run()
            _, tr, lo = e.debug_golden_trace()
        finally:
            e.close()
        starts = _pass_starts(np.asarray(tr).reshape(-1), int(lo), lab, part)
        assert [len(starts[n]) for n in PARTS[part]] == [LOOPS[n][3] for n in PARTS[part]]
        sites = stretch_sites(o, g.ninst, starts, lab, part)
        ref = o.run_trials(sites, protect_mask=0)
        cls = np.bincount(ref["cls"], minlength=6)
        assert cls[0] > 0 and cls[1] > 50 and cls[2] > 50, cls.tolist()
        _REF[part] = (elf, sites, ref)
        return _REF[part]
    yield get
    _REF.clear()


def _compare(dev, ref, sites):
    bad = np.nonzero(dev != ref)[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{len(bad)} of {len(sites)} outcomes differ; first: site={sites[i]} "
                             f"gpu={dev[i]} oracle={ref[i]}")


def _modes():
    from shrewd_amd.fi import CFG_NO_HANG_PROOF, CFG_SOLO_ALL
    return {"default": {}, "solo": {"flags": CFG_SOLO_ALL}, "solo_noproof": {"flags": CFG_SOLO_ALL | CFG_NO_HANG_PROOF},
            "short_epochs": {"epoch_iters": 8, "snapshot_interval": 256}}


def _totals(e, hist):
    """The counters a step's figures are made of."""
    from shrewd_amd.fi import STAT
    st = e.debug_stats()
    d = {k: int(st[getattr(STAT, k)]) for k in ("TX_INSTS", "FETCH_BYTES", "DATA_BYTES", "PAGES", "DEVICE_INSTS",
                                                 "SOLO_FETCH_BYTES", "SOLO_DATA_BYTES", "SOLO_PAGES", "SOLO_DEVICE_INSTS")}
    for k in ("guest_insts", "fetch_bytes", "data_bytes", "cow_pages", "device_insts"):
        d["hist_" + k] = int(hist[k])
    return d


def _run(elf, part, sites, ref, kw, want):
    """One engine: the text holds the stretches `want`, the records are the oracle's; its totals."""
    from shrewd_amd import Engine
    e = Engine(**kw)
    try:
        e.load_elf(elf, ["stretch"])
        e.golden_run()
        assert e.translate_status() == ""
        assert e.golden_stdout() == stretch_program_expected(part)
        clean = e.debug_translation().split("/*@TX_SPLIT@*/")[-1]
        got = [int(n) for n in re.findall(r"^T_\d+: \{ // stretch of pc 0x[0-9a-f]+, (\d+) insts a pass\n", clean, re.M)]
        walks = re.findall(r"SWALK\(\d+, X\d+ \+ \(uint64_t\)\(int64_t\)-?\d+LL, (-?\d+), (\d+)u, ([01])\)", clean)
        bounds = re.findall(r"SBOUND\(\d+, X\d+, (-?\d+)LL, (-?\d+)LL\)", clean)
        assert got == [n for n, _, _ in want], got
        assert [tuple(int(x) for x in w) for w in walks] == [w for _, ws, _ in want for w in ws], walks
        assert [tuple(int(x) for x in b) for b in bounds] == [b for _, _, bs in want for b in bs], bounds
        dev, hist = e.run_sites(sites)
        _compare(dev, ref, sites)
        return _totals(e, hist)
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["default", "solo", "solo_noproof", "short_epochs"])
@pytest.mark.parametrize("part", ["walks", "reentry"])
def test_stretch_program_parity(stretch_ref, part, mode):
    """The oracle's records with the stretches on and with them off, and the
    same totals either way.  (Nothing on the device counts stretch passes:
    that the stretches run is shown by the instruction counters and timings
    in profiles/README.md, not here.)"""
    from shrewd_amd.fi import CFG_NO_LOOP_STRETCH
    elf, sites, ref = stretch_ref(part)
    kw = dict(_modes()[mode])
    on = _run(elf, part, sites, ref, kw, STRETCHES[part])
    kw["flags"] = kw.get("flags", 0) | CFG_NO_LOOP_STRETCH
    off = _run(elf, part, sites, ref, kw, [])
    assert on == off


def test_crc32_stretch_on_off(engine_factory, oracle_mod):
    """crc32, 4,096 sampled trials in one launch, on the default path: the
    same records and totals with the stretches on and off, and the oracle's."""
    from conftest import workload_elf
    from shrewd_amd.fi import CFG_NO_LOOP_STRETCH
    n = 4096
    on = engine_factory("crc32", max_trials_per_launch=4096)
    off = engine_factory("crc32", max_trials_per_launch=4096, flags=CFG_NO_LOOP_STRETCH)
    assert "// stretch of pc 0x1016c" in on.debug_translation() and "// stretch" not in off.debug_translation()
    on.set_campaign(0x5EED0AD2, ((1 << 32) - 2) | (1 << 32) | (1 << 33), 1)
    sites = on.sample(0, n)
    a, ha = on.run_sites(sites)
    ta = _totals(on, ha)
    b, hb = off.run_sites(sites)
    assert np.array_equal(a, b)
    assert ta == _totals(off, hb)
    assert ta["TX_INSTS"] > 0 and ta["SOLO_DEVICE_INSTS"] > 0
    o = oracle_mod.Oracle(workload_elf("crc32"), "crc32")
    o.run_golden()
    _compare(a, o.run_trials(sites), sites)
