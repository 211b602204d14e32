"""The load-time translator's loop proofs on the CPU (fi_translate.cpp; no GPU:
fi_debug_translate runs on the host).  Inputs: crc32's pre-decoded text and
golden block trace, as the engine dumps them (tools/gpu/dump_golden.py ->
tests/golden/tx_inputs_{crc32,intmix,region}.npz, the engine's own output, not
reference data).  The device side of the same proofs is tested against the oracle in
tests/test_gpu_parity.py (test_counted_loop_hang_proofs,
test_runoff_loop_proofs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _translate(env=None, name="crc32"):
    from shrewd_amd.fi import lib
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        L = lib()
        L.fi_debug_translate.restype = C.c_int
        z = np.load(os.path.join(ROOT, "tests", "golden", f"tx_inputs_{name}.npz"))
        pre, tr = np.ascontiguousarray(z["pre"]), np.ascontiguousarray(z["trace"])
        n = C.c_uint64()
        L.fi_debug_translate(pre.ctypes.data, len(pre), int(z["text_lo"]), tr.ctypes.data, len(tr), None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        L.fi_debug_translate(pre.ctypes.data, len(pre), int(z["text_lo"]), tr.ctypes.data, len(tr), buf, n.value + 1,
                             C.byref(n))
        return buf.value.decode()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_crc32_loop_proofs():
    body = _translate()
    # the table's inner bit loop (addi t6, t6, -1; bnez t6): a counted loop of
    # three blocks, no memory access -- a hang proof without loads, at every
    # block of the cycle (tested on dispatch entries)
    hang = re.findall(r"TXHANG\(X31, -1, 5u\).*?TXLOOP\((\d+)u, 5u, 0u\)", body)
    assert len(hang) == 3 and all(int(c) & 0xFF == 31 for c in hang)
    assert "goto SR_" not in body
    # the crc loop (lbu t1, 0(a0) ... addi a0, a0, 1; bne a0, a1): a run-off
    # block against a1, a counter load at a0 and a table load at s2 + [0, 1020]
    m = re.search(r"TXHANG\(X10 - X11, 1, 10u\).*?TXLOOP\((\d+)u, 10u, 2u\); TXLD\(0, (\d+)u, (-?\d+), (\d+)u\); "
                  r"TXLD\(1, (\d+)u, (-?\d+), (\d+)u\);", body)
    assert m, "crc loop has no run-off proof"
    cnt, d0, o0, s0, d1, o1, s1 = (int(x) for x in m.groups())
    assert cnt == 10 | 11 << 8 | 1 << 16
    assert (d0 & 0xFF, (d0 >> 8) & 15, (d0 >> 12) & 15, d0 >> 16, o0, s0) == (10, 0, 1, 0, 0, 0)   # lbu at a0
    assert (d1 & 0xFF, (d1 >> 8) & 15, (d1 >> 12) & 15, d1 >> 16, o1, s1) == (18, 1, 4, 5, 0, 1020)   # lwu at s2+
    # the buffer fill: sw t0, 0(t2) walks with t2 (+4 per pass), a store at
    # another induction register (kind 4, the step in the span field)
    m = re.search(r"TXHANG\(X9, -1, 10u\).*?TXLOOP\((\d+)u, 10u, 1u\); TXLD\(0, (\d+)u, (-?\d+), (\d+)u\);", body)
    assert m, "buffer fill has no run-off proof"
    d, o, st = int(m.group(2)), int(m.group(3)), int(m.group(4))
    assert (d & 0xFF, (d >> 8) & 15, (d >> 12) & 15, o, st) == (7, 4, 4, 0, 4)


def test_clean_body_shape():
    """The clean body is generated in one shape (the A/B variants of round 4
    are gone): the budget counts down, the cold hints are on, and the
    translator reads no variant switch from the environment."""
    base = _translate()
    clean = base.split("/*@TX_SPLIT@*/")[-1]
    assert "#define SADD(n_) (brem -= (n_))" in clean and "#define SCOLD(x)" in clean
    assert "SCOLD(" in clean and "SPRIV(x) __builtin_expect" not in clean
    assert _translate({"SHREWD_FI_TXV": "47"}) == base


def test_crc32_loop_estimates():
    """The counted loops the translator exports for the solo order's work-left
    estimate (fi_types.h LoopEst, fi_kernels.hip solo_work_left): the loops
    its hang proofs recognise -- crc32's buffer fill (s1 counts down), table
    inner bit loop (t6 counts down) and crc loop (a0 runs up to a1) -- each
    with its instructions per pass and a text span around its blocks."""
    from shrewd_amd.fi import lib
    L = lib()
    L.fi_debug_loop_est.restype = C.c_int
    L.fi_debug_loop_est.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "tx_inputs_crc32.npz"))
    pre, tr = np.ascontiguousarray(z["pre"]), np.ascontiguousarray(z["trace"])
    dt = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("reg", "u1"), ("treg", "u1"), ("step", "i1"), ("pad", "u1"),
                   ("m", "<u4")])
    n = C.c_uint64()
    assert L.fi_debug_loop_est(pre.ctypes.data, len(pre), int(z["text_lo"]), tr.ctypes.data, len(tr), None, 0,
                               C.byref(n)) == 0
    out = np.zeros(n.value, dt)
    L.fi_debug_loop_est(pre.ctypes.data, len(pre), int(z["text_lo"]), tr.ctypes.data, len(tr), out.ctypes.data,
                        n.value, C.byref(n))
    loops = {(int(r["reg"]), int(r["treg"]), int(r["step"]), int(r["m"])): (int(r["lo"]), int(r["hi"])) for r in out}
    assert (10, 11, 1, 10) in loops     # crc_loop: lbu .. addi a0, a0, 1; bne a0, a1
    assert (31, 0, -1, 5) in loops      # tbl_inner: addi t6, t6, -1; bnez t6 (shortest pass: 5)
    # the buffer fill (gen: sw t0, 0(t2); addi t2, t2, 4; addi s1, s1, -1;
    # bnez s1): its store walks with the pointer t2, an induction register of
    # its own (round 6: run-off proofs with stores)
    assert (9, 0, -1, 10) in loops and len(loops) == 3
    lo, hi = loops[(10, 11, 1, 10)]
    assert lo == 0x16C and hi == 0x16C + 0x22   # the crc loop's one block (pc 0x1016c, 34 bytes)


def test_clean_body_temporaries_at_function_scope():
    """The clean body declares no block-scope temporaries (a goto out of such
    a block leaves through clang's lifetime cleanup switch: DESIGN.md 4h);
    solo_tx_clean_run declares them (TX_TEMPS)."""
    clean = _translate().split("/*@TX_SPLIT@*/")[-1]
    for decl in ("uint8_t *p_;", "bool pv_;", "uint64_t v_;", "const uint64_t ea_", "const uint64_t e_ ",
                 "const uint64_t t_ ", "const uint64_t off_"):
        assert decl not in clean, decl
    assert "ea_ = X10 + " in clean
    src = open(os.path.join(ROOT, "shrewd_amd", "csrc", "hip", "fi_trial.hip")).read()
    fn = src[src.index("void solo_tx_clean_run("):src.index("/*@TX_SOLO_CLEAN@*/")]
    assert "TX_TEMPS();" in fn


def test_intmix_region_proof():
    """intmix's main loop (loop: ... call popcnt ... sd t3, 0(t2) ... skip:
    addi s2, s2, 1; bltu s2, s3, loop) is a region proof (round 6,
    fi_translate.cpp): it runs while s2 < s3, s2 grows by one per pass, the
    pass calls a leaf (popcnt, its own counted inner loop) and reads / writes
    the acc table at s1 + [0, 4088] and pctab at s0 + [0, 255] -- bounded
    accesses at registers the region never writes (kinds 1 and 5).  The
    shortest pass (callee included) is 30 instructions; the test sits at the
    loop's own blocks only (the callee's are shared with its other callers)."""
    body = _translate(name="intmix")
    clean = body.split("/*@TX_SPLIT@*/")[-1]
    tests = re.findall(r"case (\d+): if \(TXHANGU\(X18, X19, 1, 30u\)\).*?TXLOOP\((\d+)u, 30u, 3u\); "
                       r"TXLD\(0, (\d+)u, 0, 4088u\); TXLD\(1, (\d+)u, 0, 4088u\); TXLD\(2, (\d+)u, 0, 255u\);", clean)
    assert len(tests) == 4, tests
    for _, lp, d0, d1, d2 in tests:
        assert int(lp) == 18 | 19 << 8 | 1 << 16 | 1 << 24
        assert [(int(d) & 0xFF, (int(d) >> 8) & 15, (int(d) >> 12) & 15) for d in (d0, d1, d2)] == [(9, 1, 8), (9, 5, 8), (8, 1, 1)]
    assert "TXHANGU" not in body.split("/*@TX_SPLIT@*/")[1]   # the full solo body has no proofs


# ---- region proofs on the region program (tests/test_isa_vectors.py): three
# valid loops and the near-miss twins the region walk must refuse
REGION_TEST = re.compile(r"case (\d+): if \(TXHANGU\(X(\d+), X(\d+), (-?\d+), (\d+)u\)\) \{.*?"
                         r"TXLOOP\((\d+)u, (\d+)u, (\d+)u\); "
                         r"((?:TXLD\(\d+, \d+u, -?\d+, \d+u\); )*)goto S_out;")
# why each near-miss loop is no region (fi_translate.cpp, the region walk)
REGION_REFUSED = {
    "V1": "the leaf returns with c.jalr ra, which links ra (the OP_c_jalr exclusion)",
    "V2": "the leaf calls on through t4 (another link register / a nested call)",
    "V3": "the leaf writes the bound (writes[rl] != 0)",
    "V4": "ra is written by more than the call (writes[1] != jals)",
    "V5": "an indirect call in the loop's own blocks (C_JALR outside a callee)",
    "V5b": "a ret in the loop's own blocks (C_JALR outside a callee)",
    "V6": "a store whose base the region writes from loaded data (A.k != AV_BND)",
    "V7": "the counter is written twice (writes[rc] != 1)",
    "V8a": "the exit test is bne, not bltu",
    "V8b": "the exit test is blt (signed), not bltu",
    "V9": "an ecall in the loop (no block holds it: the walk falls off translated code, as for C_STOP)",
}


def test_region_rejection_rules():
    """The region walk on the region program.  The valid loops V0 (step 1),
    V0c8 (step 8) and V0c3 (step 3) carry TXHANGU(Xrc, Xrl, c, 26) at their own
    two blocks (the header and the call's return site) and nowhere else.
    The shortest pass, counted by hand from the source: 7 instructions from
    the header to the call (xor, slli, xor, srli, xor, mv, jal), the leaf's
    2 + 7 + 2 (li, li; one turn of its inner loop; mv, ret), 8 from the return
    site to the exit test (andi, slli, add, lw, addw, sw, addi, bltu): m = 26.
    The accesses are the word table at s1 + [0, 252] as a load (kind 1) and a
    store (kind 5) and the leaf's byte table at s0 + [0, 255] (kind 1).  No
    block of a near-miss variant, its callees included, carries a region test
    (REGION_REFUSED says why), and V8a / V8b carry no counted-loop proof
    (TXHANG) either: their cycle goes through the callee's `ret`, an indirect
    jump, so the structurer that feeds the counted proofs sees no cycle of
    direct edges, and with a call inside it would be refused there anyway
    (C_JALR in the cycle)."""
    import test_isa_vectors as kat
    z = np.load(os.path.join(ROOT, "tests", "golden", "tx_inputs_region.npz"))
    text_lo = int(z["text_lo"])
    _, lab = kat.region_program_asm()
    body = _translate(name="region")
    parts = body.split("/*@TX_SPLIT@*/")
    clean = parts[-1]
    assert "TXHANGU" not in parts[1]                        # the full solo body has no proofs
    tests = {}
    for t in REGION_TEST.findall(clean):
        tests[text_lo + 2 * int(t[0])] = t
    # (every test parsed; none outside the clean body)
    assert len(tests) == clean.count("TXHANGU(X") == body.count("TXHANGU(X")
    loops = {name: (rc, rl, c) for name, rc, rl, c, _ in kat.REGION_LOOPS}
    want = {}
    for name in kat.REGION_VALID:
        want[lab[name]] = want[lab[name + "_r"]] = name
    for pc, name in want.items():
        assert pc in tests, f"{name}: no region proof at {pc:#x}"
        rc, rl, c = loops[name]
        _, xrc, xrl, step, m, lp, m2, nld, lds = tests[pc]
        assert (int(xrc), int(xrl), int(step), int(m), int(m2)) == (rc, rl, c, 26, 26), (name, tests[pc])
        assert int(lp) == rc | rl << 8 | c << 16 | 1 << 24, (name, lp)
        acc = [(int(d) & 0xFF, (int(d) >> 8) & 15, (int(d) >> 12) & 15, int(o), int(s))
               for d, o, s in re.findall(r"TXLD\(\d+, (\d+)u, (-?\d+), (\d+)u\)", lds)]
        assert int(nld) == 3 and sorted(acc) == [(8, 1, 1, 0, 255), (9, 1, 4, 0, 252), (9, 5, 4, 0, 252)], (name, acc)
        assert {k for _, k, _, _, _ in acc} == {1, 5}
    # the near misses: nothing in their span or their callees'
    spans = {name: [(lab[name + "_lo"], lab[name + "_hi"])] for name in REGION_REFUSED}
    for name, leaf in (("V1", "f1"), ("V2", "f2"), ("V2", "f2b"), ("V3", "f3"), ("V4", "f4")):
        spans[name].append((lab[leaf], lab[leaf + "_end"]))
    for name in ("V5", "V5b", "V6", "V7", "V8a", "V8b", "V9"):
        spans[name].append((lab["fs"], lab["fs_end"]))
    spans["V5b"].append((lab["V5b_ret"], lab["V5b_ret"] + 2))
    assert set(spans) == {n for n, *_ in kat.REGION_LOOPS} - set(kat.REGION_VALID)
    for name, why in REGION_REFUSED.items():
        hit = [hex(pc) for pc in tests if any(lo <= pc < hi for lo, hi in spans[name])]
        assert not hit, f"{name} got a region proof at {hit}: {why}"
    assert set(tests) == set(want), sorted(hex(pc) for pc in set(tests) ^ set(want))
    # the counted-loop proofs (TXHANG): the leaves' inner loops and the fills only
    counted = {text_lo + 2 * int(i) for i in re.findall(r"case (\d+): if \(TXHANG\(", clean)}
    for name in ("V8a", "V8b"):
        lo, hi = spans[name][0]
        assert not [pc for pc in counted if lo <= pc < hi], name
    assert counted and not [pc for pc in counted if any(lab[n + "_lo"] <= pc < lab[n + "_hi"] for n in loops)]


def _region_fixture():
    """(raw word and length of the instruction at a pc, pc of the k-th
    committed instruction) from the region fixture: the pre-decoded text and
    the golden trace (ecalls, bit 31, are events and not counted, as in the
    oracle's and the engine's numInst)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "tx_inputs_region.npz"))
    text_lo, pre, tr = int(z["text_lo"]), z["pre"], z["trace"]
    insts = tr[(tr >> 31) == 0]

    def at(pc):
        r = pre[(pc - text_lo) // 2]
        return int.from_bytes(bytes(r[0:4]), "little"), int(r[12])
    return at, lambda k: text_lo + 2 * int(insts[k]), len(insts)


def test_region_program_rvc_forms():
    """The RVC forms the region variants exist for are in the text the
    translator sees: f1 returns with c.jalr ra (0x9082), V5 calls with
    c.jalr tp (0x9202), f4's `addi ra, ra, 0` is c.mv ra, ra (0x8086), V7's
    second write of rc is c.mv s10, s10, the valid leaf f0 and V5b's stray
    return end in c.jr ra (0x8082).  Were the assembler to stop compressing
    them, V1 would still be refused (jalr ra links: rd != 0), and the
    c.jalr path of the region walk would go untested without this."""
    import test_isa_vectors as kat
    _, lab = kat.region_program_asm()
    at, _, _ = _region_fixture()
    for what, pc, half in (("f1's return", lab["f1_end"] - 2, 0x9082), ("V5's call", lab["V5_r"] - 2, 0x9202),
                           ("f0's return", lab["f0_end"] - 2, 0x8082), ("V5b's stray return", lab["V5b_ret"], 0x8082),
                           ("V7's second write of rc", lab["V7"], 0x8000 | 26 << 7 | 26 << 2 | 2)):
        raw, ln = at(pc)
        assert (raw & 0xFFFF, ln) == (half, 2), (what, hex(raw), ln)
    raw, ln = at(lab["f4_end"] - 6)   # f4 ends: c.mv ra, ra; c.mv a0, t0; c.jr ra
    assert (raw & 0xFFFF, ln) == (0x8086, 2), ("f4's write of ra", hex(raw), ln)


def test_region_layout_on_golden_trace():
    """region_program_model's instruction counts, on which every fault site
    stands, against the golden trace: each variant's set-up starts at NAME_lo,
    each of its passes (all 32) at NAME, its end is the first instruction
    after the loop, and the hand-placed sites stand on the instructions they name (V0's
    `sub s3, t0, s1`; V6's `add t4, s1, t1` in eight passes; the middle pass's
    first instruction for the bound flips)."""
    import test_isa_vectors as kat
    from test_isa_vectors import enc_r
    _, lab = kat.region_program_asm()
    _, lay = kat.region_program_model()
    at, pc_of, n = _region_fixture()
    assert n == lay["end"]
    for name, *_ in kat.REGION_LOOPS:
        first, end, starts = lay[name]
        assert pc_of(first) == lab[name + "_lo"] and pc_of(end) == lab[name + "_hi"], name
        assert len(starts) == kat.REGION_PASSES and all(pc_of(k) == lab[name] for k in starts), name
    sub = enc_r(0x33, 0, 0x20, 19, 5, 9)     # sub s3, t0, s1
    add = enc_r(0x33, 0, 0, 29, 9, 6)        # add t4, s1, t1
    for tag, inst, target, _ in kat.region_explicit_sites():
        raw, _ = at(pc_of(inst))
        if tag.startswith("base_"):
            assert (raw, target) == (sub, 9), tag
        elif tag == "v6_off":
            assert (raw, target) == (add, 6), tag
        else:
            name, rl = {"v0_rl": ("V0", 19), "v3_rl": ("V3", 13)}[tag]
            assert (pc_of(inst), target) == (lab[name], rl), tag


@pytest.mark.gpu
def test_region_fixture_is_current():
    """tests/golden/tx_inputs_region.npz (tools/gpu/dump_golden.py --fixture kat:region)
    is the engine's pre-decode and golden trace of the region program as it
    assembles today: the CPU test above does not run on stale inputs."""
    import test_isa_vectors as kat
    from shrewd_amd import Engine
    e = Engine()
    try:
        e.load_elf(kat.region_program_elf(), ["region"])
        e.golden_run()
        pre, tr, lo = e.debug_golden_trace()
    finally:
        e.close()
    z = np.load(os.path.join(ROOT, "tests", "golden", "tx_inputs_region.npz"))
    assert lo == int(z["text_lo"])
    assert np.array_equal(np.asarray(z["pre"]).reshape(-1), np.asarray(pre).reshape(-1))
    assert np.array_equal(np.asarray(z["trace"]).reshape(-1), np.asarray(tr).reshape(-1))
