"""Exact campaigns over memory words without a device (DESIGN.md 4j "Memory
words"): byte sets, byte liveness, the walk and the trial-id map in a sanitized
stand-alone program, fi_exact_mem_classes against a numpy restatement on random
event lists, and the premise -- every site of a class has its representative's
outcome, every other site is the golden run -- brute-forced on the oracle over
the engine's recorded memory index of hello and fpamo
(tests/golden/mem_index_*.npz; tests/test_gpu_exact_mem.py asserts the engine
still produces exactly these).

The numpy model below is also what tests/test_gpu_exact_mem.py checks the
device against."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, np_histogram, workload_elf
from test_exact_cpu import ALL_BITS, np_weighted_histogram, positions

MEM = 1 << 33
T_MEM = 33
SEED = 0xE8AC7
THREADS = min(16, os.cpu_count() or 1)
FPAMO_BITS = sum(1 << b for b in (0, 9, 18, 27, 36, 45, 54, 63))


def test_exact_mem_host_passes_sanitized(tmp_path):
    """tools/exact_mem_host_check.cpp: the worked example, same-numInst entries,
    an AMO, the clip at ninst, a word without events, the text-word exclusion
    and the k -> (byte set, word, class, position) map for burst 1, 4 and 16."""
    csrc = os.path.join(ROOT, "shrewd_amd", "csrc")
    exe = str(tmp_path / "exact_mem_host_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    os.path.join(ROOT, "tools", "exact_mem_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exact_mem_host_check ok" in r.stdout


# ---- the numpy model
def byte_sets(bits=ALL_BITS, burst=1):
    """The byte sets in their order -> [(F as a bit per byte, its positions ascending)]"""
    sets = []
    for b in positions(bits, burst):
        f = sum(1 << k for k in range(b // 8, (b + burst - 1) // 8 + 1))
        if not sets or sets[-1][0] != f:
            sets.append((f, []))
        sets[-1][1].append(b)
    return sets


def live_before(ev):
    """live_before of a word's events, restated per byte without the
    recurrence: byte k is live before event i iff the first event at or after
    i that touches k reads it (an event that reads and writes reads first)."""
    e = np.asarray(ev, np.uint64).astype(np.int64)
    live = np.zeros(len(e), np.int64)
    for k in range(8):
        touch = np.flatnonzero((((e >> 8) | e) >> k) & 1)
        if not len(touch):
            continue
        j = np.searchsorted(touch, np.arange(len(e)))      # the next event that touches k
        has = j < len(touch)
        nxt = touch[np.minimum(j, len(touch) - 1)]
        live |= (has & (((e[nxt] >> (8 + k)) & 1) == 1)).astype(np.int64) << k
    return live


def np_mem_intervals(ev, ninst, f, live=None):
    """One word's intervals under the byte set f as the issue states them
    -> (u', prev', is a class) per heading entry."""
    e = np.asarray(ev, np.uint64).astype(np.int64)
    live = live_before(e) if live is None else live
    touch = (((e >> 8) | e) & f & 0xFF) != 0
    u = np.minimum(e[touch] >> 16, ninst - 1)
    prev = np.concatenate([[-1], u[:-1]]).astype(np.int64)
    head = u > prev
    return u[head], prev[head], ((live[touch] & f) != 0)[head]


def np_mem_classes(ev, ninst, f, live=None):
    """One word's classes -> (inst, weight, dead t of the word)."""
    u, prev, cls = np_mem_intervals(ev, ninst, f, live)
    w = (u - prev)[cls]
    return u[cls], w, ninst - int(w.sum())


def space_words(pages, text=(0, 0)):
    """Every word of the candidate pages that does not overlap the text, ascending."""
    a = np.concatenate([np.uint64(p) + np.arange(512, dtype=np.uint64) * np.uint64(8) for p in sorted(pages)])
    lo, hi = np.uint64(text[0]), np.uint64(text[1])
    return a[~((a < hi) & (a + np.uint64(8) > lo))]


def np_mem_exact_sites(index, ninst, pages, bits=ALL_BITS, burst=1, text=(0, 0), first_trial=0):
    """Memory's exact trials in trial-id order: byte sets, words by address,
    classes in time order, positions -> (sites SITE_DT, weights, dead (word, t)
    pairs per position {b: count}, words in the space)."""
    from shrewd_amd.fi import SITE_DT
    addr, off, ev = index
    words = space_words(pages, text)
    listed = np.isin(addr, words)
    lives = [live_before(ev[off[i]:off[i + 1]]) for i in range(len(addr))]
    bm = (1 << burst) - 1
    inst, ad, mask, weight, dead = [], [], [], [], {}
    for f, pos in byte_sets(bits, burst):
        live_sum = 0
        masks = np.array([(bm << b) & ALL_BITS for b in pos], np.uint64)
        for i in np.flatnonzero(listed):
            u, w, _ = np_mem_classes(ev[off[i]:off[i + 1]], ninst, f, lives[i])
            live_sum += int(w.sum())
            inst.append(np.repeat(u, len(pos)))
            weight.append(np.repeat(w, len(pos)))
            ad.append(np.full(len(u) * len(pos), addr[i], np.uint64))
            mask.append(np.tile(masks, len(u)))
        for b in pos:
            dead[b] = len(words) * ninst - live_sum
    n = sum(len(x) for x in inst)
    sites = np.zeros(n, SITE_DT)
    if n:
        sites["inst"], sites["addr"], sites["mask"] = np.concatenate(inst), np.concatenate(ad), np.concatenate(mask)
    sites["target"] = T_MEM
    sites["trial"] = (np.arange(n) + first_trial) & 0xFFFFFFFF
    return sites, (np.concatenate(weight) if n else np.zeros(0)).astype(np.uint32), dead, len(words)


def all_mem_sites(words, ninst, bits=ALL_BITS, burst=1, ts=None):
    """The brute-force space of the given words: every (word, t, position)."""
    from shrewd_amd.fi import SITE_DT
    pos = positions(bits, burst)
    ts = np.arange(ninst) if ts is None else np.asarray(ts)
    bm = (1 << burst) - 1
    sites = np.zeros(len(words) * len(ts) * len(pos), SITE_DT)
    sites["addr"] = np.repeat(np.asarray(words, np.uint64), len(ts) * len(pos))
    sites["inst"] = np.tile(np.repeat(ts, len(pos)), len(words))
    sites["mask"] = np.tile(np.array([(bm << b) & ALL_BITS for b in pos], np.uint64), len(words) * len(ts))
    sites["target"] = T_MEM
    sites["trial"] = np.arange(len(sites)) & 0xFFFFFFFF
    return sites


def low_bit(mask):
    m = mask.astype(np.uint64)
    return np.log2((m & (~m + np.uint64(1))).astype(np.float64)).round().astype(np.int64)


def mem_class_of(ex_sites, ex_weights, sites):
    """For each memory site, the index of the exact trial whose class contains
    it (the same word and mask; the first representative at or after its t, if
    its interval of ex_weights sites reaches back to t), or -1 for a dead site."""
    words = np.unique(np.concatenate([ex_sites["addr"], sites["addr"]]))

    def key(s):   # (word, position, t) in one sortable number
        w = np.searchsorted(words, s["addr"]).astype(np.int64)
        return ((w * 64 + low_bit(s["mask"])) << 30) | s["inst"].astype(np.int64)
    ek, sk = key(ex_sites), key(sites)
    order = np.argsort(ek, kind="stable")
    eks = ek[order]
    out = np.full(len(sites), -1, np.int64)
    if not len(eks):
        return out
    j = np.searchsorted(eks, sk)                    # the first representative at or after t ...
    jj = np.minimum(j, len(eks) - 1)
    ok = (j < len(eks)) & ((eks[jj] >> 30) == (sk >> 30))   # ... of the same word and position
    idx = order[jj]
    ok &= sites["inst"].astype(np.int64) > ex_sites["inst"][idx].astype(np.int64) - ex_weights[idx].astype(np.int64)
    out[ok] = idx[ok]
    return out


def add_mem_dead(h, dead, golden_ninst):
    """Memory's dead sites added to a histogram: per position the dead
    (word, t) pairs as masked golden runs."""
    for b, d in dead.items():
        h["counts"][T_MEM, b, 0] += d
    n = sum(dead.values())
    h["trials"] = int(h["trials"]) + n
    h["guest_insts"] = (int(h["guest_insts"]) + n * golden_ninst) & ALL_BITS
    return h


def golden_index(name):
    """The engine's recorded memory index of a workload -> ((addr, off, ev), candidate pages)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", f"mem_index_{name}.npz"))
    return (z["addr"], z["off"], z["ev"]), [int(p) for p in z["pages"]]


# ---- fi_exact_mem_classes against the model
def test_exact_mem_classes_match_model():
    """Random event lists: short and long, dense in time (several events of one
    numInst), with events at numInst == ninst, loads, stores and AMOs of
    1, 2, 4 and 8 bytes; every byte set of burst 1, 4 and 16."""
    from shrewd_amd import exact_mem_classes
    rng = np.random.default_rng(0xE8AC7)
    sets = sorted({f for burst in (1, 4, 16) for f, _ in byte_sets(ALL_BITS, burst)})
    assert len(sets) == 21                         # 8 bytes, 7 pairs, 6 triples
    total = 0
    for trial in range(200):
        ninst = int(rng.integers(1, 40))
        n = int(rng.integers(0, 30))
        t = np.sort(rng.integers(0, ninst + 1, n))
        size = 1 << rng.integers(0, 4, n)
        bm = ((1 << size) - 1) << (rng.integers(0, 8, n) // size * size)
        kind = rng.integers(1, 4, n)               # 1 read, 2 write, 3 both
        ev = (t.astype(np.uint64) << np.uint64(16)) | (np.where(kind & 1, bm, 0).astype(np.uint64) << np.uint64(8)) \
            | np.where(kind & 2, bm, 0).astype(np.uint64)
        for f in sets:
            c, dead = exact_mem_classes(ev, ninst, f)
            inst, w, d = np_mem_classes(ev, ninst, f)
            assert np.array_equal(c["inst"], inst) and np.array_equal(c["weight"], w) and dead == d, (trial, f, ev)
            assert int(c["weight"].sum()) + dead == ninst
            assert (c["inst"] < ninst).all() and (c["weight"] >= 1).all()
            total += len(c)
    assert total > 1000


def test_exact_mem_classes_rejects_bad_arguments():
    from shrewd_amd import EngineError, exact_mem_classes
    ev = np.array([(2 << 16) | (0x0F << 8)], np.uint64)
    for f in (0, 0x100):
        with pytest.raises(EngineError):
            exact_mem_classes(ev, 10, f)
    with pytest.raises(EngineError):
        exact_mem_classes(ev, 1 << 29, 1)
    c, dead = exact_mem_classes(np.zeros(0, np.uint64), 10, 0xFF)      # a word without events: all dead
    assert len(c) == 0 and dead == 10
    c, dead = exact_mem_classes(ev, 10, 0x01)
    assert c["inst"].tolist() == [2] and c["weight"].tolist() == [3] and dead == 7


# ---- the premise, brute-forced on the oracle over the engine's recorded index
def premise(o, index, pages, words, bits, burst):
    """Every site of `words` x t x position: equal to its class's
    representative, or dead and the masked golden run."""
    g = o.golden
    ninst = int(g.ninst)
    ex, w, dead, n_words = np_mem_exact_sites(index, ninst, pages, bits, burst)
    space = all_mem_sites(words, ninst, bits, burst)
    ref_all = o.run_trials(space, threads=THREADS)
    ref_ex = o.run_trials(ex, threads=THREADS)
    cl = mem_class_of(ex, w, space)
    live = cl >= 0
    bad = np.flatnonzero(ref_all[live] != ref_ex[cl[live]])
    assert not len(bad), f"{len(bad)} sites differ from their representative, first {space[live][bad[:3]]}"
    d = ref_all[~live]
    assert (d["cls"] == 0).all() and (d["ninst"] == g.ninst).all() and (d["exit_code"] == g.exit_code).all()
    return ex, w, dead, n_words, space, ref_all, ref_ex, live


def oracle_for(oracle_mod, name):
    o = oracle_mod.Oracle(workload_elf(name), name)
    o.run_golden()
    return o


@pytest.mark.parametrize("burst", [1, 4])
def test_premise_on_oracle_hello(oracle_mod, burst):
    """hello, the whole memory space (2 pages x 512 words x 7 x positions): the
    class-weighted histogram is the brute-force histogram."""
    o = oracle_for(oracle_mod, "hello")
    index, pages = golden_index("hello")
    ninst = int(o.golden.ninst)
    assert ninst == 7 and len(pages) == 2
    sampled = o.sample(SEED, 0, 20000, MEM)
    assert sorted(set((sampled["addr"] & ~np.uint64(4095)).tolist())) == pages      # as the sampler draws them
    words = space_words(pages)
    ex, w, dead, n_words, space, ref_all, ref_ex, live = premise(o, index, pages, words, ALL_BITS, burst)
    assert n_words == 1024 and len(space) == 1024 * 7 * (65 - burst)
    assert int(live.sum()) == int(w.sum()) and int((~live).sum()) == sum(dead.values()) and len(ex) > 0
    hw = add_mem_dead(np_weighted_histogram(ex, ref_ex, w), dead, ninst)
    hb = np_histogram(space, ref_all)
    for f in ("counts", "crash_sub", "escape_sub", "trials", "guest_insts"):
        assert np.array_equal(hw[f], hb[f]), f
    assert int(hw["counts"].sum()) == int(hw["trials"]) == len(space)


def test_premise_on_oracle_fpamo(oracle_mod):
    """fpamo (FP and AMO code, ninst 848): every word the index lists and 8 it
    does not, at positions {0, 9, ..., 63}."""
    o = oracle_for(oracle_mod, "fpamo")
    index, pages = golden_index("fpamo")
    addr, off, ev = index
    assert int(o.golden.ninst) == 848
    every = space_words(pages)
    listed = addr[np.isin(addr, every)]
    rest = every[~np.isin(every, addr)]
    words = np.sort(np.concatenate([listed, rest[np.linspace(0, len(rest) - 1, 8).astype(np.int64)]]))
    assert len(listed) > 0 and len(words) == len(listed) + 8
    amo = ((ev >> np.uint64(8)) & ev & np.uint64(0xFF)) != 0
    assert amo.any()                               # an event that reads and writes the same bytes
    ex, w, *_ , live = premise(o, index, pages, words, FPAMO_BITS, 1)
    assert live.any() and (~live).any() and len(ex) > 0


def test_python_names_import_without_a_device():
    import shrewd_amd
    from shrewd_amd import Engine, FaultCampaign
    from shrewd_amd.fi import ExactMemInfo
    import inspect
    assert callable(shrewd_amd.exact_mem_classes)
    for n in ("set_exact_memory", "exact_mem_info", "golden_mem_index"):
        assert callable(getattr(Engine, n))
    assert inspect.signature(FaultCampaign.__init__).parameters["exact_memory"].default is False
    assert ExactMemInfo().byte_sets == 0 and ExactMemInfo().as_dict()["byte_sets"] == []
