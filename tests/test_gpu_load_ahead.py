"""Loads issued one pass ahead in the clean solo body (fi_translate.cpp,
DESIGN.md 4h) against the oracle, through the C ABI.

The `ahead` programs below walk memory in eight loops, each the smallest
shape a wrong implementation of the held load gets wrong, mix every value
they read into one checksum and print it.  They are two programs, `walks`
(L1..L5) and `reentry` (L6..L8), because the clean body has eight site caches
and every load and store inside a cycle takes one: in one program the later
loops would get none and so hold nothing.

 L1  a byte walk, step +1, across a page boundary (the held load is skipped
     on a page's last byte and resumes on the next page);
 L2  a word walk, step -4, that crosses the boundary downwards;
 L3  a doubleword walk, step +8, at an induction register (t2) beside a
     separate down-counter (t0);
 L4  a halfword walk, step +2, from an odd address that reaches the page's
     last byte (the site's misaligned-page-end leave fires there);
 L5  a self-loop that stores to p + 1 before its next pass reads it (the
     translator must not hold this load);
 L6  an inner read loop whose next run starts at the byte its last run
     loaded ahead, after the outer block has rewritten that byte (a tag that
     survived the re-entry would return the old byte);
 L7  the same over an initialised .data page that nothing wrote before: the
     outer block's first store turns the shared page into a private one;
 L8  a doubleword walk over two stack pages nobody has written (the zero
     page).

Every record must equal the oracle's with the ahead loads on and off
(FI_CFG_NO_LOAD_AHEAD), on the default path, with every trial on the solo
kernel from the start (FI_CFG_SOLO_ALL) and there also without the loop
proofs (FI_CFG_NO_HANG_PROOF: long walks are executed, not proved)."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
LCG = 1103515245
FILL = 64            # bytes filled on each side of the boundary
L1_SPAN = 60         # L1 reads [pgb - 60, pgb + 60)
OUTER = 5            # runs of L6's / L7's inner loop, 8 bytes each
DBUF = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0x8796A5B4C3D2E1F0, 0x13579BDF02468ACE,
        0xECA86420FDB97531]

MIX = "add   s6, s6, t1\n    slli  t5, s6, 3\n    xor   s6, s6, t5"


PARTS = {"walks": ("L1", "L2", "L3", "L4", "L5"), "reentry": ("L6", "L7", "L8")}


def ahead_program_source(part: str) -> str:
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
    walks = f"""    addi  a0, s0, -{L1_SPAN}
    addi  a1, s0, {L1_SPAN}
L1:
    lbu   t1, 0(a0)
    {MIX}
    addi  a0, a0, 1
    bne   a0, a1, L1
    addi  a0, s0, 16
    addi  a1, s0, -24
L2:
    lw    t1, 0(a0)
    {MIX}
    addi  a0, a0, -4
    bne   a0, a1, L2
    addi  t2, s0, -24
    li    t0, 6
L3:
    ld    t1, 0(t2)
    {MIX}
    addi  t2, t2, 8
    addi  t0, t0, -1
    bnez  t0, L3
    addi  a0, s0, -9
    addi  a1, s0, 9
L4:
    lhu   t1, 0(a0)
    {MIX}
    addi  a0, a0, 2
    bne   a0, a1, L4
    addi  a0, s0, 32
    addi  a1, s0, 48
L5:
    lbu   t1, 0(a0)
    {MIX}
    sb    s6, 1(a0)
    addi  a0, a0, 1
    bne   a0, a1, L5
"""
    reentry = f"""    addi  a0, s0, -{FILL}
    mv    a1, a0
    li    s5, {OUTER}
O6:
    addi  a1, a1, 8
L6:
    lbu   t1, 0(a0)
    {MIX}
    addi  a0, a0, 1
    bne   a0, a1, L6
    lbu   t3, 0(a0)
    xori  t3, t3, 0x5a
    sb    t3, 0(a0)
    addi  s5, s5, -1
    bnez  s5, O6
    la    a0, dbuf
    mv    a1, a0
    li    s5, {OUTER}
O7:
    addi  a1, a1, 8
L7:
    lbu   t1, 0(a0)
    {MIX}
    addi  a0, a0, 1
    bne   a0, a1, L7
    lbu   t3, 0(a0)
    xori  t3, t3, 0x5a
    sb    t3, 0(a0)
    addi  s5, s5, -1
    bnez  s5, O7
    li    t0, -12288
    add   a0, sp, t0
    srli  a0, a0, 12
    slli  a0, a0, 12
    addi  a0, a0, -32
    addi  a1, a0, 64
L8:
    ld    t1, 0(a0)
    {MIX}
    addi  a0, a0, 8
    bne   a0, a1, L8
"""
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
    .balign 8
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
"""
    return head + {"walks": walks, "reentry": reentry}[part] + tail


def ahead_program_asm(part: str):
    """(elf, labels)"""
    from tools.rvasm.rvasm import Assembler
    a = Assembler(compress=False)
    elf = a.assemble(ahead_program_source(part))
    return elf, dict(a.labels)


def ahead_program_expected(part: str) -> bytes:
    """The program in plain Python: the checksum it prints."""
    mem = bytearray(2 * FILL)            # [pgb - FILL, pgb + FILL)
    t3 = 1
    for k in range(2 * FILL // 8):
        t3 = (t3 * LCG + 1234) & M64
        mem[8 * k:8 * k + 8] = t3.to_bytes(8, "little")
    s6 = 0

    def mix(v):
        nonlocal s6
        s6 = (s6 + v) & M64
        s6 ^= (s6 << 3) & M64

    def rd(buf, off, size):
        return int.from_bytes(buf[off:off + size], "little")
    if part == "walks":
        for a in range(-L1_SPAN, L1_SPAN):                       # L1
            mix(mem[FILL + a])
        for a in range(16, -24, -4):                             # L2 (lw sign-extends)
            w = rd(mem, FILL + a, 4)
            mix((w - (1 << 32)) & M64 if w >> 31 else w)
        for k in range(6):                                       # L3
            mix(rd(mem, FILL - 24 + 8 * k, 8))
        for a in range(-9, 9, 2):                                # L4
            mix(rd(mem, FILL + a, 2))
        for a in range(32, 48):                                  # L5: reads what the pass before stored
            mix(mem[FILL + a])
            mem[FILL + a + 1] = s6 & 255
    else:
        for buf in (mem, bytearray(b"".join(v.to_bytes(8, "little") for v in DBUF))):   # L6, L7
            a = 0
            for _ in range(OUTER):
                for _ in range(8):
                    mix(buf[a])
                    a += 1
                buf[a] ^= 0x5A
        for _ in range(8):                                       # L8: zeroes
            mix(0)
    return s6.to_bytes(8, "little")


# loop -> (pointer register, bound / counter register, step, access size, passes,
#          the pointer at its first pass as label + offset; None: not a fixed address)
LOOPS = {"L1": (10, 11, 1, 1, 2 * L1_SPAN, ("pgb", -L1_SPAN)), "L2": (10, 11, -4, 4, 10, ("pgb", 16)),
         "L3": (7, 5, 8, 8, 6, ("pgb", -24)), "L4": (10, 11, 2, 2, 9, ("pgb", -9)), "L5": (10, 11, 1, 1, 16, ("pgb", 32)),
         "L6": (10, 11, 1, 1, 8 * OUTER, ("pgb", -FILL)), "L7": (10, 11, 1, 1, 8 * OUTER, ("dbuf", 0)),
         "L8": (10, 11, 8, 8, 8, None)}
N_RANDOM = 2000
# what the held text of each program must be: (type, step) per site, in block order (L5 holds none)
HELD = {"walks": [("u8", "1"), ("u32", "-4"), ("u64", "8"), ("u16", "2")],
        "reentry": [("u8", "1"), ("u8", "1"), ("u64", "8")]}


def _pass_starts(trace, text_lo, lab, part):
    """loop -> the counts (instructions committed before it) of each pass's
    first instruction, from the engine's golden trace (ecalls are events, not
    counted, as in the oracle's numInst)."""
    insts = trace[(trace >> 31) == 0]
    pcs = text_lo + 2 * insts.astype(np.int64)
    return {name: np.nonzero(pcs == lab[name])[0] for name in PARTS[part]}


def ahead_sites(o, ninst, starts, lab, part):
    """N_RANDOM sampled register and pc sites, then hand-placed flips at pass
    boundaries: single bits of each loop's pointer and bound (low bits move
    the walk inside its pages and misalign it, bit 12 and up move it to other
    pages, mapped or not), and the pointer moved to the unmapped page 0x2000,
    onto the last element of its page and onto its page's first byte."""
    from oracle.pyoracle import SITE_DT
    rnd = o.sample(0x5EED0A4D, 0, N_RANDOM, ((1 << 32) - 2) | (1 << 32))
    ex = []
    for name in PARTS[part]:
        ptr, bound, step, size, _, first = LOOPS[name]
        st = starts[name]
        for k in (1, len(st) // 2, len(st) - 2):
            for bit in (0, 1, 2, 3, 5, 11, 12, 13, 20, 31, 47, 63):
                ex.append((int(st[k]), ptr, 1 << bit))
                ex.append((int(st[k]), bound, 1 << bit))
        if first is not None:
            k = 2
            p = lab[first[0]] + first[1] + k * step      # the pointer at the start of pass k
            for to in (0x2000 | (p & 4095), (p | 4095) + 1 - size, p & ~4095):
                if to != p:
                    ex.append((int(st[k]), ptr, p ^ to))
    s = np.zeros(len(ex), SITE_DT)
    for i, (inst, target, mask) in enumerate(ex):
        s["inst"][i], s["target"][i], s["mask"][i] = min(inst, ninst - 1), target, mask
    s = np.concatenate([rnd, s])
    s["trial"] = np.arange(len(s))
    return s


_REF = {}


@pytest.fixture(scope="module")
def ahead_ref(oracle_mod):
    """part -> (elf, sites, the oracle's outcomes): computed once per program."""
    def get(part):
        if part in _REF:
            return _REF[part]
        from shrewd_amd import Engine
        elf, lab = ahead_program_asm(part)
        o = oracle_mod.Oracle(elf, "ahead")
        g = o.run_golden()
        assert o.golden_stdout() == ahead_program_expected(part)
        assert 600 <= g.ninst <= 4000, g.ninst
        e = Engine()
        try:
            e.load_elf(elf, ["ahead"])
            e.golden_run()
            _, tr, lo = e.debug_golden_trace()
        finally:
            e.close()
        starts = _pass_starts(np.asarray(tr).reshape(-1), int(lo), lab, part)
        assert [len(starts[n]) for n in PARTS[part]] == [LOOPS[n][4] for n in PARTS[part]]
        sites = ahead_sites(o, g.ninst, starts, lab, part)
        ref = o.run_trials(sites, protect_mask=0)
        # the site set reaches what it is for: walks onto unmapped pages (crashes)
        # and corrupted checksums besides the benign ones
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
    from shrewd_amd.fi import CFG_NO_HANG_PROOF, CFG_NO_LOAD_AHEAD, CFG_SOLO_ALL
    return {"default": 0, "solo": CFG_SOLO_ALL, "solo_noproof": CFG_SOLO_ALL | CFG_NO_HANG_PROOF}, CFG_NO_LOAD_AHEAD


@pytest.mark.parametrize("ahead", ["ahead_on", "ahead_off"])
@pytest.mark.parametrize("mode", ["default", "solo", "solo_noproof"])
@pytest.mark.parametrize("part", ["walks", "reentry"])
def test_ahead_program_parity(ahead_ref, part, mode, ahead):
    import re
    from shrewd_amd import Engine
    elf, sites, ref = ahead_ref(part)
    modes, off = _modes()
    e = Engine(flags=modes[mode] | (off if ahead == "ahead_off" else 0))
    try:
        e.load_elf(elf, ["ahead"])
        e.golden_run()
        assert e.translate_status() == ""
        assert e.golden_stdout() == ahead_program_expected(part)
        # the generated text holds every read loop's load but L5's
        clean = e.debug_translation().split("/*@TX_SPLIT@*/")[-1]
        held = re.findall(r"HV\d+ = \*\(const g_(\w+) \*\)\(p_ \+ (-?\d+)\)", clean)
        assert held == (HELD[part] if ahead == "ahead_on" else []), held
        dev, _ = e.run_sites(sites)
        _compare(dev, ref, sites)
    finally:
        e.close()


def test_crc32_solo_all_ahead_on_off(engine_factory, oracle_mod):
    """crc32, 4,096 sampled trials, every one on the solo kernel from its
    start: the same records with the ahead loads on and off, and the oracle's."""
    from conftest import workload_elf
    from shrewd_amd.fi import CFG_NO_LOAD_AHEAD, CFG_SOLO_ALL
    n = 4096
    on = engine_factory("crc32", flags=CFG_SOLO_ALL)
    off = engine_factory("crc32", flags=CFG_SOLO_ALL | CFG_NO_LOAD_AHEAD)
    assert "HV" in on.debug_translation() and "HV" not in off.debug_translation()
    on.set_campaign(0x5EED0AD1, ((1 << 32) - 2) | (1 << 32) | (1 << 33), 1)
    sites = on.sample(0, n)
    a, _ = on.run_sites(sites)
    b, _ = off.run_sites(sites)
    assert np.array_equal(a, b)
    o = oracle_mod.Oracle(workload_elf("crc32"), "crc32")
    o.run_golden()
    _compare(a, o.run_trials(sites), sites)
