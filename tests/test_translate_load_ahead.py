"""The translator's loads one pass ahead on the CPU (fi_translate.cpp, DESIGN.md
4h; no GPU: fi_debug_translate_flags runs on the host), on the fixtures of
tests/test_translate.py.  The device side is tested against the oracle in
tests/test_gpu_load_ahead.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SPLIT = "/*@TX_SPLIT@*/"
# a site's ahead load: HV<i> = *(const g_<type> *)(p_ + <step>); HT<i> = ea_ + ...
HELD = re.compile(r"HV(\d+) = \*\(const g_(\w+) \*\)\(p_ \+ (-?\d+)\); HT(\d+) = ea_ \+ \(uint64_t\)\(int64_t\)(-?\d+);")
BLOCK = re.compile(r"^S_(\d+): \{ // pc (0x[0-9a-f]+), \d+ insts\n(.*?)^\}\n", re.S | re.M)


def _inputs(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"tx_inputs_{name}.npz"))
    return np.ascontiguousarray(z["pre"]), np.ascontiguousarray(z["trace"]), int(z["text_lo"])


def _translate(name, flags=None):
    """The generated text: through fi_debug_translate (flags None) or
    fi_debug_translate_flags."""
    from shrewd_amd.fi import lib
    L = lib()
    pre, tr, lo = _inputs(name)

    def call(buf, cap, n):
        if flags is None:
            return L.fi_debug_translate(pre.ctypes.data, len(pre), lo, tr.ctypes.data, len(tr), buf, cap, C.byref(n))
        return L.fi_debug_translate_flags(pre.ctypes.data, len(pre), lo, tr.ctypes.data, len(tr), flags, buf, cap,
                                          C.byref(n))
    n = C.c_uint64()
    assert call(None, 0, n) == 0
    buf = C.create_string_buffer(n.value + 1)
    assert call(buf, n.value + 1, n) == 0
    return buf.value.decode()


def _blocks(clean):
    """pc -> (leader index, text) of the clean body's blocks."""
    return {int(pc, 16): (int(h), text) for h, pc, text in BLOCK.findall(clean)}


def _strip_ahead(text):
    """The text with everything the ahead loads add taken out again."""
    text = re.sub(r"  uint(?:32|64)_t HV\d+; uint64_t HT\d+;\n", "", text)
    text = re.sub(r"  HT\d+ = ~0ULL;\n", "", text)
    text = re.sub(r"S_\d+_L: ;\n", "", text)
    text = re.sub(r"SC_SET\((\d+), vp_, e_\); HT\d+ = ~0ULL; \}", r"SC_SET(\1, vp_, e_); }", text)
    size = {"u8": 1, "u16": 2, "u32": 4, "u64": 8}
    text = re.sub(r"    if \(HT\d+ == ea_\) v_ = HV\d+; else v_ = \*\(const g_(\w+) \*\)p_;\n"
                  r"    if \(SCOLD\(\(\(uint32_t\)ea_ & 4095u\) \+ \(uint32_t\)-?\d+ > \d+u\)\) HT\d+ = ~0ULL;\n"
                  r"    else \{ HV\d+ = [^\n]*\n",
                  lambda m: f"    if (SPRIV(pv_)) v_ = *(const g_{m.group(1)} *)p_; else v_ = tx_sload(p_, "
                            f"{size[m.group(1)]}u);\n", text)
    return re.sub(r"goto S_(\d+)_L;", r"goto S_\1;", text)


def test_crc32_ahead_sites():
    """crc32's crc loop (pc 0x1016c: lbu t1, 0(a0) ... lwu t2, 0(t2) ... addi a0,
    a0, 1; bne a0, a1) holds its byte load, step 1, and not its table load,
    whose address depends on the byte; the buffer fill (gen) and the hex
    loop store and hold nothing; nothing outside the clean body does."""
    body = _translate("crc32", 0)
    parts = body.split(SPLIT)
    clean = parts[-1]
    for p in parts[:-1]:
        assert "HV" not in p and "HT" not in p and "_L:" not in p
    held = HELD.findall(clean)
    assert len(held) == 1 and clean.count("HV") == 3, held   # one site: declared, taken, loaded
    site, typ, step, site2, step2 = held[0]
    assert (typ, step, step2) == ("u8", "1", "1") and site == site2
    h, loop = _blocks(clean)[0x1016C]
    assert HELD.search(loop) and "ea_ = X10 + " in loop.split("HV")[0]
    assert loop.count("*(const g_u32 *)p_") == 1             # the table load, as it was
    assert f"S_{h}_L: ;" in loop and f"goto S_{h}_L;" in loop and f"goto S_{h};" not in loop
    # the tag is dropped on every entry but the back edge, and by a refill
    assert re.search(rf"^  HT{site} = ~0ULL;\nS_{h}_L: ;\n", loop, re.M)
    assert f"SC_SET({site}, vp_, e_); HT{site} = ~0ULL; }}" in loop
    assert f"  uint32_t HV{site}; uint64_t HT{site};\n" in clean.split("S_entry:")[0]
    # every other entry goes to the block's own label: the dispatch, other blocks
    assert f"goto S_{h};" in clean and clean.count(f"goto S_{h}_L;") == 1
    # blocks with a store hold nothing
    for pc, (_, text) in _blocks(clean).items():
        if re.search(r"\*\(g_u\d+ \*\)p_ = ", text):
            assert "HV" not in text, hex(pc)


@pytest.mark.parametrize("name", ["crc32", "intmix", "region"])
def test_flag_gives_the_text_without_ahead_loads(name):
    """fi_debug_translate is fi_debug_translate_flags(0); with
    FI_CFG_NO_LOAD_AHEAD the text is the one without ahead loads: the
    default text with what they add taken out again, line for line."""
    from shrewd_amd.fi import CFG_NO_LOAD_AHEAD
    on, off = _translate(name, 0), _translate(name, CFG_NO_LOAD_AHEAD)
    assert _translate(name) == on
    assert "HV" not in off and "HT" not in off and "_L:" not in off
    assert _strip_ahead(on) == off
    assert (on == off) == (not HELD.search(on))


@pytest.mark.parametrize("name", ["crc32", "intmix", "region"])
def test_ahead_sites_lie_in_store_free_self_loops(name):
    """Every ahead site is in the clean body, in a block that branches to
    itself (through its back-edge label) and stores nothing; its load is at a
    register plus an immediate that the block steps once, by the site's step,
    and the loaded register is another one."""
    from shrewd_amd.fi import CFG_NO_LOAD_AHEAD  # noqa: F401
    body = _translate(name, 0)
    parts = body.split(SPLIT)
    assert not any(HELD.search(p) for p in parts[:-1])
    clean = parts[-1]
    n = 0
    for pc, (h, text) in _blocks(clean).items():
        for site, typ, step, _, _ in HELD.findall(text):
            n += 1
            assert f"goto S_{h}_L;" in text, hex(pc)
            assert not re.search(r"\*\(g_u\d+ \*\)p_ = ", text), hex(pc)
            m = re.search(rf"ea_ = X(\d+) \+ [^\n]*\n[^\n]*CV{site}\)", text)
            assert m, hex(pc)
            r = m.group(1)
            steps = re.findall(rf"  SX\({r}, X{r} \+ \(\(uint64_t\)\(int64_t\)(-?\d+)LL\)\);", text)
            writes = len(re.findall(rf"  SX\({r}, ", text)) + len(re.findall(rf"    X{r} = ", text))
            assert steps == [step] and writes == 1, (hex(pc), steps, writes)
    assert n == len(HELD.findall(clean))
    if name == "crc32":
        assert n == 1
