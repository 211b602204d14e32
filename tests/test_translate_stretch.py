"""The translator's check-free stretches on the CPU (fi_translate.cpp, DESIGN.md
4h; no GPU: fi_debug_translate_flags runs on the host), on the fixtures of
tests/test_translate.py.  The device side is tested against the oracle in
tests/test_gpu_loop_stretch.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SPLIT = "/*@TX_SPLIT@*/"
BLOCK = re.compile(r"^S_(\d+): \{ // pc (0x[0-9a-f]+), (\d+) insts\n(.*?)^\}\n", re.S | re.M)
STRETCH = re.compile(r"^T_(\d+): \{ // stretch of pc (0x[0-9a-f]+), (\d+) insts a pass\n(.*?)^\}\n", re.S | re.M)
# the entry's tests: a walking site (site cache, register, offset, step, size, held) and a
# bounded one (site cache, base register, lowest offset, highest offset + size)
WALK = re.compile(r"  k_ = SMINU\(k_, SWALK\((\d+), X(\d+) \+ \(uint64_t\)\(int64_t\)(-?\d+)LL, (-?\d+), (\d+)u, ([01])\)\);\n")
BOUND = re.compile(r"  if \(!SBOUND\((\d+), X(\d+), (-?\d+)LL, (-?\d+)LL\)\) k_ = 0u;\n")
STORE = re.compile(r"\*\(g_u\d+ \*\)p_ = ")
SIZE = {"u8": 1, "u16": 2, "u32": 4, "u64": 8}


def _translate(name, flags):
    from shrewd_amd.fi import lib
    L = lib()
    z = np.load(os.path.join(ROOT, "tests", "golden", f"tx_inputs_{name}.npz"))
    pre, tr, lo = np.ascontiguousarray(z["pre"]), np.ascontiguousarray(z["trace"]), int(z["text_lo"])
    n = C.c_uint64()
    assert L.fi_debug_translate_flags(pre.ctypes.data, len(pre), lo, tr.ctypes.data, len(tr), flags, None, 0,
                                      C.byref(n)) == 0
    buf = C.create_string_buffer(n.value + 1)
    assert L.fi_debug_translate_flags(pre.ctypes.data, len(pre), lo, tr.ctypes.data, len(tr), flags, buf, n.value + 1,
                                      C.byref(n)) == 0
    return buf.value.decode()


def _strip_stretch(text):
    """The text with everything the stretches add taken out again."""
    text = re.sub(r"  uint(?:32|64)_t WV\d+; uint64_t WP\d+;\n", "", text)
    text = re.sub(r"^S_\d+_K: ;\n", "", text, flags=re.M)
    text = re.sub(r"  k_ = (?:brem|\(brem - \d+u\)) / \d+u;\n(?:  k_ = SMINU\([^\n]*\n|  if \(!SBOUND\([^\n]*\n)+  if \(SHOT\(k_ >= 2u\)\) goto T_\d+;\n",
                  "", text)
    return STRETCH.sub("", text)


def _stretches(clean):
    """leader -> (pc, insts a pass, the block's text, the stretch's text)"""
    blocks = {int(h): (int(pc, 16), int(n), text) for h, pc, n, text in BLOCK.findall(clean)}
    out = {}
    for h, pc, n, text in STRETCH.findall(clean):
        bpc, bn, btext = blocks[int(h)]
        assert (bpc, bn) == (int(pc, 16), int(n))
        out[int(h)] = (bpc, bn, btext, text)
    return out


def test_crc32_has_one_stretch_at_the_crc_loop():
    """crc32's crc loop (pc 0x1016c: lbu t1, 0(a0); xor; andi 255; slli 2; add
    s2; lwu; srli; xor; addi a0, a0, 1; bne a0, a1) is the one stretch: the
    byte load a walking site (u8, step 1) that holds the next pass's value, the
    table load a bounded site (u32 at s2 = X18 plus 0..1020).  The buffer fill
    stores, the table's loops store or are several blocks, the hex loop
    stores: none of them has one."""
    from shrewd_amd.fi import CFG_NO_LOOP_STRETCH
    on, off = _translate("crc32", 0), _translate("crc32", CFG_NO_LOOP_STRETCH)
    assert on.split(SPLIT)[:-1] == off.split(SPLIT)[:-1]     # nothing outside the clean body changed
    clean = on.split(SPLIT)[-1]
    st = _stretches(clean)
    assert [pc for pc, _, _, _ in st.values()] == [0x1016C] and len(re.findall(r"^T_\d+: ", clean, re.M)) == 1
    (h, (pc, n, block, body)), = st.items()
    assert n == 10
    walks, bounds = WALK.findall(block), BOUND.findall(block)
    assert len(walks) == 1 and len(bounds) == 1
    site, reg, offs, step, size, held = (int(x) for x in walks[0])
    assert (reg, offs, step, size, held) == (10, 0, 1, 1, 1)
    # the held value: loaded once before the first pass, then taken and loaded a pass ahead
    assert f"  WV{site} = *(const g_u8 *)SC_PTR({site}, X10 + (uint64_t)(int64_t)0LL);\n" in body
    assert f"  WP{site} = SC_BASE({site}) + (uint64_t)(int64_t)1LL; SOPAQUE(WP{site});\n" in body
    assert f"  v_ = WV{site}; WV{site} = *(const g_u8 *)(uintptr_t)(WP{site} + X10);\n  X6 = v_;\n" in body
    assert f"  uint32_t WV{site}; uint64_t WP{site};\n" in clean.split("S_entry:")[0]
    bsite, base, lo, end = (int(x) for x in bounds[0])
    assert (base, lo, end) == (18, 0, 1020 + 4) and bsite != site
    assert f"  v_ = *(const g_u32 *)SC_PTR({bsite}, X7 + ((uint64_t)(int64_t)0LL));\n  X7 = v_;\n" in body
    # the normal block keeps both sites as they were, in the same site caches
    assert f"CV{site})" in block and f"CV{bsite})" in block
    # the stretch has no test but its own exit and pass count, and commits what it ran
    for word in ("SOVER", "SCOLD", "tlb_find", "CV", "S_out", "HT", "HV"):
        assert word not in body, word
    commit = "SKEEP(WV%d); SADD(10u * d_); xt += 1u * d_; fb += 34u * d_; db += 5u * d_; " % site
    assert body.count(commit) == 2
    assert f"  k_ -= 1u;\n  if (SCOND(!(X10 != X11))) {{ d_ = ks_ - k_; {commit}goto S_199; }}\n" in body
    assert body.endswith(f"  if (SHOT(k_ != 0u)) goto T_{h}_P;\n  d_ = ks_; {commit}goto S_{h}_K;\n")
    # entered after the budget test, left to the label below the tags' reset
    assert re.search(rf"^  HT\d+ = ~0ULL;\nS_{h}_L: ;\nS_{h}_K: ;\n", block, re.M)
    assert re.search(r"  if \(SOVER\(10u\)\) [^\n]*\n  k_ = brem / 10u;\n", block)
    assert block.count(f"goto T_{h};") == 1 and clean.count(f"goto T_{h};") == 1
    # blocks with a store have none
    for _, bpc, _, text in BLOCK.findall(clean):
        if STORE.search(text):
            assert "goto T_" not in text and "SWALK" not in text, bpc


@pytest.mark.parametrize("name", ["crc32", "intmix", "region"])
def test_flag_gives_the_text_without_stretches(name):
    """With FI_CFG_NO_LOOP_STRETCH the text holds no stretch, and it is the
    default text with what the stretches add taken out again, line for line;
    the ahead loads' flag composes with it."""
    from shrewd_amd.fi import CFG_NO_LOAD_AHEAD, CFG_NO_LOOP_STRETCH
    on, off = _translate(name, 0), _translate(name, CFG_NO_LOOP_STRETCH)
    assert not re.search(r"\bT_\d+", off)                     # no stretch label
    for word in ("_K:", "WV", "WP", "SWALK", "SBOUND", "SHOT", " k_ ", "ks_", "// stretch"):
        assert word not in off, word
    assert on != off and _strip_stretch(on) == off
    assert _strip_stretch(_translate(name, CFG_NO_LOAD_AHEAD)) == _translate(name, CFG_NO_LOAD_AHEAD | CFG_NO_LOOP_STRETCH)


@pytest.mark.parametrize("name", ["crc32", "intmix", "region"])
def test_stretches_lie_in_store_free_self_loops(name):
    """Every stretch belongs to a clean-body block that branches to itself,
    stores nothing and leaves only through its last branch; every load of the
    block is a walking site (at a register the block steps once, by the site's
    step) or a bounded site (at a register the block never writes), each with
    a site cache of its own; the stretch repeats the block's register writes."""
    body = _translate(name, 0)
    parts = body.split(SPLIT)
    assert not any(STRETCH.search(p) for p in parts[:-1])
    st = _stretches(parts[-1])
    assert st
    for h, (pc, n, block, text) in st.items():
        assert not STORE.search(block) and not STORE.search(text), hex(pc)
        assert re.search(rf"goto S_{h}(?:_L)?;", block), hex(pc)
        assert "S_dispatch" not in block.split("goto T_")[1], hex(pc)      # no indirect jump, one exit branch
        # the pass count leaves the budget's share of the blocks after the exit that the
        # block's own budget test covers
        m = re.search(r"  if \(SOVER\((\d+)u\)\) [^\n]*\n  k_ = (?:brem|\(brem - (\d+)u\)) / (\d+)u;\n", block)
        assert m and int(m.group(3)) == n and int(m.group(1)) == n + int(m.group(2) or 0), hex(pc)
        walks, bounds = WALK.findall(block), BOUND.findall(block)
        loads = re.findall(r"ea_ = X(\d+) \+ [^\n]*\n[^\n]*CV(\d+)\)", block)
        assert len(loads) == len(walks) + len(bounds) and "tx_probe_ld" not in block, hex(pc)
        assert sorted(int(s) for _, s in loads) == sorted([int(w[0]) for w in walks] + [int(b[0]) for b in bounds]), hex(pc)

        def writes(r):
            return len(re.findall(rf"  SX\({r}, ", block)) + len(re.findall(rf"    X{r} = ", block))
        for site, reg, offs, step, size, held in walks:
            steps = re.findall(rf"  SX\({reg}, X{reg} \+ \(\(uint64_t\)\(int64_t\)(-?\d+)LL\)\);", block)
            assert steps == [step] and writes(reg) == 1, (hex(pc), reg, steps)
            assert (f"WV{site} = " in text) == (held == "1"), hex(pc)
        for site, reg, lo, end in bounds:
            assert writes(reg) == 0 and int(lo) < int(end), (hex(pc), reg)
        # the same register writes, in the same order
        order = re.compile(r"^  (?:SX\((\d+), |  X(\d+) = |X(\d+) = )", re.M)
        assert [a or b or c for a, b, c in order.findall(block)] == [a or b or c for a, b, c in order.findall(text)], hex(pc)
    if name == "crc32":
        assert len(st) == 1
