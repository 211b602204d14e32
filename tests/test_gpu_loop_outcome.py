"""loop_outcome on the device (fi_trial.hip), the re-check the solo kernel runs
whenever a translated body claims a run-off loop cannot leave before the hang
cap.  The body proves against the instructions left capped at 2^32 - 1
(SoloTxIO::hleft); loop_outcome re-decides against the 64-bit count, so a
loop that leaves after 2^32 + k instructions must come back undecided, not a
hang (gem5: the trial runs on and exits, `BaseCPU::scheduleInstStop`,
cpu/base.cc:764-770, never fires).  Records are synthetic (fi_debug_loop):
no trial has to run billions of instructions to reach those paths.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAGE_TOP = 0x7FFFFFFFFFFFF000   # the stack's top page (kStackTopVpn): in every page set
BEYOND = 0x8000000000000000     # above kStackBase: unmapped, not in a VMA, not stack growth


def cnt(counter, cmp, step):
    return counter | (cmp << 8) | ((step & 0xFF) << 16)


def ld(reg, kind, size, pos, off=0, span=0):
    return (reg | (kind << 8) | (size << 12) | (pos << 16), off & 0xFFFFFFFF, span)


def loop(regs, left, counter, cmp, step, m, loads=()):
    from shrewd_amd.fi import DEBUG_LOOP_DT
    r = np.zeros(1, DEBUG_LOOP_DT)[0]
    for k, v in regs.items():
        r["regs"][k] = v & (2**64 - 1)
    r["left"], r["lp_cnt"], r["lp_m"], r["lp_n"] = left, cnt(counter, cmp, step), m, len(loads)
    for j, t in enumerate(loads):
        r["lp_ld"][j] = t
    return r


def test_loop_outcome_64bit_left(engine_factory):
    from shrewd_amd.fi import DEBUG_LOOP_DT
    e = engine_factory("hello")
    m = 4
    cases = [
        # 0: leaves after (2^30 + 999) * 4 = 2^32 + 3996 instructions, left 2^33:
        #    the capped body proof fires, the 64-bit re-check says undecided
        (loop({5: 2**30 + 1000}, 2**33, 5, 0, -1, m), 0, 1),
        # 1: the same loop with 2^31 + 5 passes: a hang both ways
        (loop({5: 2**31 + 5}, 2**33, 5, 0, -1, m), 1, 1),
        # 2: a loop that leaves after 2^32 + 4 instructions with left exactly
        #    2^32 + 8: still undecided (the cap is not reached)
        (loop({5: 2**30 + 2}, 2**32 + 8, 5, 0, -1, m), 0, 1),
        # 3: left 2^32 + 3, the loop's last pass at 2^32 + 4: a hang
        (loop({5: 2**30 + 2}, 2**32 + 3, 5, 0, -1, m), 1, 1),
        # 4: a counter compared with x6, distance not a multiple of the step: never leaves
        (loop({5: 3, 6: 0}, 2**40, 5, 6, -2, m), 1, 1),
        # 5: a counter load walking up off the stack's top page: the page fault
        #    512 iterations on, at the first address above kStackBase
        (loop({5: PAGE_TOP, 6: PAGE_TOP + 8 * 2**40}, 2**33, 5, 6, 8, m, [ld(5, 0, 8, 2)]), 2, 1),
        # 6: the same walk downward below the stack: fixupFault would grow the
        #    stack there (mem_state.cc:387-447) -- undecided
        (loop({5: PAGE_TOP, 6: PAGE_TOP - 8 * 2**40}, 2**33, 5, 6, -8, m, [ld(5, 0, 8, 2)]), 0, 1),
        # 7: a bounded (table) load whose range is outside the page set: undecided
        (loop({5: 2**31 + 5, 9: 0x1000}, 2**33, 5, 0, -1, m, [ld(9, 1, 4, 1, 0, 64)]), 0, 1),
        # 8: a counter load that could straddle a line (unaligned): undecided
        (loop({5: PAGE_TOP + 4, 6: PAGE_TOP + 8 * 2**40}, 2**33, 5, 6, 8, m, [ld(5, 0, 8, 0)]), 0, 1),
        # 9: a short loop (100 passes): neither proof fires
        (loop({5: 100}, 2**33, 5, 0, -1, m), 0, 0),
    ]
    recs = np.array([c[0] for c in cases], DEBUG_LOOP_DT)
    out = e.debug_loop_outcome(recs)
    for i, (_, verdict, body) in enumerate(cases):
        assert (int(out["verdict"][i]), int(out["body_proof"][i])) == (verdict, body), (i, out[i])
    # the fault: 512 iterations of 4 instructions, the load third in the block
    assert int(out["k"][5]) == 512 * m + 2 and int(out["fva"][5]) == BEYOND
    # no record with a 64-bit loop shorter than `left` is a hang, whatever the capped proof says
    rng = np.random.default_rng(3)
    many = []
    for _ in range(4000):
        mm = int(rng.integers(1, 64))
        passes = int(rng.integers(2**32 // mm - 4, 2**34 // mm))
        left = int(rng.integers(2**32 - 16, 2**35))
        many.append(loop({5: passes}, left, 5, 0, -1, mm))
    many = np.array(many, DEBUG_LOOP_DT)
    o = e.debug_loop_outcome(many)
    passes = many["regs"][:, 5].astype(np.uint64)
    mm = many["lp_m"].astype(np.uint64)
    left = many["left"].astype(np.uint64)
    hang = (passes - 1) >= (left + mm - 1) // mm
    assert ((o["verdict"] == 1) == hang).all()
    assert (o["verdict"][~hang] == 0).all()
    assert (o["body_proof"].astype(bool) & ~hang).sum() > 100   # the capped proof alone would have been wrong


# ---- region records (bit 24 of lp_cnt: the loop runs while x < l, unsigned;
# fi_translate.cpp region proofs, TXHANGU / tx_hang_proof_u in the clean body)
M64 = 2**64 - 1
CAP32 = 2**32 - 1   # SoloTxIO::hleft: the body proves against `left` capped here


def rcnt(rc, rl, c, region=1):
    return rc | (rl << 8) | ((c & 0xFF) << 16) | (region << 24)


def rloop(regs, left, rc, rl, c, m, loads=(), n_loads=None):
    r = loop(regs, left, rc, rl, c, m, loads)
    r["lp_cnt"] = rcnt(rc, rl, c)
    if n_loads is not None:
        r["lp_n"] = n_loads
    return r


def region_model(x, l, c, m, left):
    """(hang, capped body proof) of a region loop in big integers: it passes
    its exit test n = ceil((l - x) / c) more times if x < l (else it may leave
    at the next test), at least m instructions apart."""
    x, l = x & M64, l & M64
    n = -((x - l) // c) if x < l else 0

    def hang(left_):
        return n != 0 and n - 1 >= -(-left_ // m)
    return hang(left), hang(min(left, CAP32))


def elf_code_range(elf: bytes):
    """[lo, hi) of the executable PT_LOAD segments (the engine's code range)."""
    import struct
    phoff, = struct.unpack_from("<Q", elf, 32)
    phentsize, phnum = struct.unpack_from("<HH", elf, 54)
    lo, hi = M64, 0
    for i in range(phnum):
        typ, flags, _, _, paddr, _, memsz, _ = struct.unpack_from("<IIQQQQQQ", elf, phoff + i * phentsize)
        if typ == 1 and flags & 1 and memsz:
            lo, hi = min(lo, paddr), max(hi, paddr + memsz)
    return lo, hi


def test_loop_outcome_region_records(engine_factory):
    """loop_outcome's region branch and the body's TXHANGU proof on synthetic
    records: expected (verdict, body_proof) from region_model; every access of
    a region record is a bounded table (kinds 1 / 5) that must lie on mapped
    pages, a store table also outside the code range -- otherwise, and for any
    malformed record, the verdict is 0 (undecided: the trial runs on)."""
    import os
    from conftest import ROOT
    from shrewd_amd.fi import DEBUG_LOOP_DT
    e = engine_factory("hello")
    code_lo, code_hi = elf_code_range(open(os.path.join(ROOT, "workloads", "hello.elf"), "rb").read())
    assert code_hi - code_lo >= 64 and (code_hi - 1) >> 12 == code_hi >> 12 == (code_hi + 15) >> 12
    m, far, L33 = 4, 2**31 + 5, 2**33
    X = {5: 1000, 6: 1000 + far}           # x < l, far apart: 2^31 + 5 passes of 4 against left 2^33
    Xt = {**X, 9: PAGE_TOP}
    cases = [
        # (record, verdict); the body proof comes from the model unless given
        ("no accesses", rloop(X, L33, 5, 6, 1, m), 1),
        ("load table on the stack's top page", rloop(Xt, L33, 5, 6, 1, m, [ld(9, 1, 4, 0, 0, 64)]), 1),
        ("store table there", rloop(Xt, L33, 5, 6, 1, m, [ld(9, 5, 4, 0, 0, 64)]), 1),
        ("load and store tables", rloop(Xt, L33, 5, 6, 1, m, [ld(9, 1, 8, 0, 8, 256), ld(9, 5, 8, 0, 8, 256)]), 1),
        ("x > l", rloop({5: 2000 + far, 6: 1000}, L33, 5, 6, 1, m), 0),
        ("x == l", rloop({5: 77, 6: 77}, L33, 5, 6, 1, m), 0),
        ("x == l == 0", rloop({5: 0, 6: 0}, L33, 5, 6, 1, m), 0),
        # the loop ends after (2^30 + 999) * 4 = 2^32 + 3996 instructions, left 2^33:
        # the capped body proof fires, the 64-bit re-check does not
        ("past the 32-bit cap, before left", rloop({5: 9, 6: 9 + 2**30 + 1000}, L33, 5, 6, 1, m), 0),
        ("2^32 + 4 instructions, left 2^32 + 8", rloop({5: 9, 6: 9 + 2**30 + 2}, 2**32 + 8, 5, 6, 1, m), 0),
        ("2^32 + 4 instructions, left 2^32 + 3", rloop({5: 9, 6: 9 + 2**30 + 2}, 2**32 + 3, 5, 6, 1, m), 1),
        # steps with (l - x) no multiple of the step: the ceiling.  left 4000, m 4: a
        # hang needs n - 1 >= 1000.  c = 3: l - x = 3001 -> n = 1001 (hang), 3000 -> 1000 (not)
        ("c 3, l - x = 3001", rloop({5: 5, 6: 3006}, 4000, 5, 6, 3, m), 1),
        ("c 3, l - x = 3000", rloop({5: 5, 6: 3005}, 4000, 5, 6, 3, m), 0),
        ("c 8, l - x = 8001", rloop({5: 5, 6: 8006}, 4000, 5, 6, 8, m), 1),
        ("c 8, l - x = 8000", rloop({5: 5, 6: 8005}, 4000, 5, 6, 8, m), 0),
        ("c 1, l - x = 1001", rloop({5: M64 - 2000, 6: M64 - 999}, 4000, 5, 6, 1, m), 1),
        ("c 1, l - x = 1000", rloop({5: M64 - 2000, 6: M64 - 1000}, 4000, 5, 6, 1, m), 0),
        ("c 8 up to 2^64 - 1", rloop({5: M64 - 8001, 6: M64}, 4000, 5, 6, 8, m), 1),
        # the tables' pages
        ("load table on an unmapped page", rloop({**X, 9: 0x1000}, L33, 5, 6, 1, m, [ld(9, 1, 4, 0, 0, 64)]), 0),
        ("load table from the top page to above the stack base",
         rloop({**X, 9: PAGE_TOP + 0xFC0}, L33, 5, 6, 1, m, [ld(9, 1, 8, 0, 0, 0x100)]), 0),
        ("load table ending at the stack base", rloop({**X, 9: PAGE_TOP + 0xF00}, L33, 5, 6, 1, m,
                                                      [ld(9, 1, 8, 0, 0, 0xF8)]), 1),
        ("load table one byte above it", rloop({**X, 9: PAGE_TOP + 0xF00}, L33, 5, 6, 1, m,
                                               [ld(9, 1, 8, 0, 1, 0xF8)]), 0),
        ("store table in the code range", rloop({**X, 9: code_lo + 8}, L33, 5, 6, 1, m, [ld(9, 5, 4, 0, 0, 16)]), 0),
        ("load table in the code range", rloop({**X, 9: code_lo + 8}, L33, 5, 6, 1, m, [ld(9, 1, 4, 0, 0, 16)]), 1),
        ("store table on the code range's last byte",
         rloop({**X, 9: code_hi}, L33, 5, 6, 1, m, [ld(9, 5, 1, 0, -1, 0)]), 0),
        ("store table just above the code range", rloop({**X, 9: code_hi}, L33, 5, 6, 1, m, [ld(9, 5, 8, 0, 0, 8)]), 1),
        ("good load table, store table in the code",
         rloop({**Xt, 10: code_lo}, L33, 5, 6, 1, m, [ld(9, 1, 4, 0, 0, 64), ld(10, 5, 4, 0, 32, 16)]), 0),
        # the next three are checks of the outcome, not of one rule each: hello has no
        # nine contiguous mapped pages to put a long table on, and page 0 and the pages
        # below the start-up stack are unmapped, so the page walk would refuse these
        # records too were the eight-page or the wrap-around test gone (a record that
        # wraps past 2^64 has base + off = 8 here, or a page difference that underflows)
        ("table over more than eight pages", rloop({**X, 9: PAGE_TOP - 0x9000}, L33, 5, 6, 1, m,
                                                   [ld(9, 1, 8, 0, 0, 0x9800)]), 0),
        ("base + span wraps 2^64", rloop({**X, 9: M64 - 15}, L33, 5, 6, 1, m, [ld(9, 1, 8, 0, 0, 64)]), 0),
        ("base + off wraps 2^64", rloop({**X, 9: M64 - 7}, L33, 5, 6, 1, m, [ld(9, 1, 8, 0, 16, 64)]), 0),
    ]
    # a walking access (kinds 0, 2, 3, 4: a run-off loop's) in a region record
    for kind in (0, 2, 3, 4):
        cases.append((f"walking kind {kind}",
                      rloop({**Xt, 7: PAGE_TOP}, L33, 5, 6, 8, m, [ld(7, kind, 8, 1, 0, 8)]), 0))
    cases.append(("good table, then a walking kind",
                  rloop({**Xt, 7: PAGE_TOP}, L33, 5, 6, 8, m, [ld(9, 1, 4, 0, 0, 64), ld(7, 3, 8, 1, 0, 8)]), 0))
    # malformed records: undecided, and no body proof
    bad = [("compared register 0", rloop(X, L33, 5, 0, 1, m)), ("step 0", rloop(X, L33, 5, 6, 0, m)),
           ("negative step", rloop(X, L33, 5, 6, -1, m)), ("m 0", rloop(X, L33, 5, 6, 1, 0)),
           ("counter register 0", rloop(X, L33, 0, 6, 1, m))]
    recs = np.array([c[1] for c in cases] + [b[1] for b in bad] + [rloop(X, L33, 5, 6, 1, m, n_loads=5)], DEBUG_LOOP_DT)
    out = e.debug_loop_outcome(recs)
    for i, (what, r, verdict) in enumerate(cases):
        c = int(r["lp_cnt"]) >> 16 & 0xFF
        hang, body = region_model(int(r["regs"][5]), int(r["regs"][6]), c, int(r["lp_m"]), int(r["left"]))
        assert not verdict or hang, what                      # (the table's own consistency)
        assert (int(out["verdict"][i]), int(out["body_proof"][i])) == (verdict, int(body)), (what, out[i])
    for j, (what, _) in enumerate(bad):
        o = out[len(cases) + j]
        assert (int(o["verdict"]), int(o["body_proof"])) == (0, 0), (what, o)
    assert (int(out["verdict"][-1]), int(out["body_proof"][-1])) == (0, 1), out[-1]   # lp_n == 5
    # a seeded batch around the cap: c in 1..8, m in 1..63, the passes around
    # left / m, x near 0, 2^63 and the top of the range (l = x + d there wraps for
    # some: then x >= l, the loop may leave at once)
    rng = np.random.default_rng(4)
    many, want = [], []
    for i in range(4000):
        mm, c = int(rng.integers(1, 64)), int(rng.integers(1, 9))
        n = int(rng.integers(2**32 // mm - 4, 2**34 // mm))
        left = int(rng.integers(2**32 - 16, 2**35))
        d = (n - 1) * c + int(rng.integers(1, c + 1))       # ceil(d / c) == n
        where = i % 4
        if where == 0:
            x = int(rng.integers(0, 16))
        elif where == 1:
            x = 2**63 - int(rng.integers(0, d + 16))        # x below or across 2^63, l above
        elif where == 2:
            x = (M64 - 8 - d + int(rng.integers(0, 8))) & M64   # l within 8 of 2^64 - 1
        else:
            x = M64 - 8 - int(rng.integers(0, 2 * d))       # l = x + d wraps for about half
        l = (x + d) & M64
        many.append(rloop({5: x, 6: l}, left, 5, 6, c, mm))
        want.append(region_model(x, l, c, mm, left))
    o = e.debug_loop_outcome(np.array(many, DEBUG_LOOP_DT))
    hang = np.array([w[0] for w in want])
    body = np.array([w[1] for w in want])
    assert ((o["verdict"] == 1) == hang).all(), np.flatnonzero((o["verdict"] == 1) != hang)[:8]
    assert (o["verdict"][~hang] == 0).all()
    assert (o["body_proof"].astype(bool) == body).all(), np.flatnonzero(o["body_proof"].astype(bool) != body)[:8]
    assert hang.sum() > 400 and (~hang).sum() > 400
    assert (o["body_proof"].astype(bool) & ~hang).sum() > 100   # the capped proof alone would have been wrong
