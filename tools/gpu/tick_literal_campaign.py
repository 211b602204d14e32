"""A tick-domain campaign under both tick contracts (Engine.set_tick_contract)
on one GPU: N seeded single-bit register / pc / result tick sites of one
workload, device map, each contract timed (warm-up, then REPS runs: median and
min .. max of the wall time around run_tick_trials), and every trial checked
against the CPU oracle (checker only): the numInst contract's outcomes against
the oracle's contract output, the literal contract's against its literal run
of every site (the contract's record where the reason is FI_TK_MACRO /
FI_TK_CLOCK).  Beside it the cost of the trials that carry a stale decoder
half (reason FI_TK_STRADDLE2, general path only): boundary sites of that
reason against as many sites the numInst contract runs.

python tools/gpu/tick_literal_campaign.py [WORKLOAD] [N] [SEED] [--reps R]  -> one JSON line"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from shrewd_amd import Engine  # noqa: E402
from shrewd_amd.fi import TICK_ESCAPE_NAMES  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

STRUCTS = ((1 << 32) - 2) | (1 << 32) | (1 << 34)
argv, REPS = [], 3
it = iter(sys.argv[1:])
for a in it:
    if a == "--reps":
        REPS = max(3, int(next(it)))
    else:
        argv.append(a)
name = argv[0] if len(argv) > 0 else "crc32"
N = int(argv[1]) if len(argv) > 1 else 100_000
SEED = int(argv[2], 0) if len(argv) > 2 else 0x5EED7101
elf = open(os.path.join(ROOT, "workloads", f"{name}.elf"), "rb").read()
e = Engine()
e.load_elf(elf, [name])
e.set_cpu_model("timing")
e.golden_run()
e.set_campaign(SEED, STRUCTS, 1)
e.set_tick_map("device")


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def reasons(out):
    esc = (out["cls"] == 5) & (out["sub"] == 7)
    return {TICK_ESCAPE_NAMES.get(int(k), str(k)): int(v)
            for k, v in zip(*np.unique(out["exit_code"][esc], return_counts=True))}


runs, outs = {"numinst": [], "literal": []}, {}
for c in ("literal", "numinst"):   # warm-up: buffers, the packed table
    e.set_tick_contract(c)
    e.run_tick_trials(0, N)
for _ in range(REPS):
    for c in ("numinst", "literal"):
        e.set_tick_contract(c)
        dt, (outs[c], _) = timed(lambda: e.run_tick_trials(0, N))
        runs[c].append(dt)
ts = e.sample_tick_sites(0, N)

o = Oracle(elf, name)
o.run_golden()
o.tick_setup()
assert (o.tick_sample(SEED, 0, N, STRUCTS) == ts).all(), "sampled tick sites differ"
bad = {"numinst": 0, "literal": 0}
kept = 0
t1 = time.perf_counter()
for a in range(0, N, 20_000):
    contract, truth = o.run_tick_trials(ts[a:a + 20_000], threads=16, truth=True)
    esc = (contract["cls"] == 5) & (contract["sub"] == 7) & (contract["exit_code"] >= 7)
    kept += int(esc.sum())
    bad["numinst"] += int((outs["numinst"][a:a + 20_000] != contract).sum())
    bad["literal"] += int((outs["literal"][a:a + 20_000] != np.where(esc, contract, truth)).sum())
oracle_s = time.perf_counter() - t1

# the stale decoder half: boundary sites of reason FI_TK_STRADDLE2 beside plain ones
ops, ticks = o.tick_trace()
rng = np.random.default_rng(5)
two = np.nonzero(ops["nfetch"] == 2)[0]
stale = None
if len(two):
    j = rng.choice(two, 4000)
    bs = np.zeros(len(j), ts.dtype)
    bs["tick"] = ticks["fetch_done"][j, 0] + 1   # the first tick of the second fetch
    bs["mask"] = 1 << rng.choice([1, 2, 3, 5, 12, 20], len(j))
    bs["target"] = 32
    bs["trial"] = np.arange(len(j))
    contract = o.run_tick_trials(bs, threads=16)
    why = np.where((contract["cls"] == 5) & (contract["sub"] == 7), contract["exit_code"], 0)
    s4, s0 = bs[why == 4], bs[why == 0]
    k = min(len(s4), len(s0))
    if k:
        e.set_tick_contract("literal")
        e.run_tick_sites(s4[:k]); e.run_tick_sites(s0[:k])
        t4 = min(timed(lambda: e.run_tick_sites(s4[:k]))[0] for _ in range(3))
        t0 = min(timed(lambda: e.run_tick_sites(s0[:k]))[0] for _ in range(3))
        stale = {"sites": int(k), "stale_half_s": round(t4, 4), "plain_s": round(t0, 4),
                 "us_per_trial": [round(1e6 * t4 / k, 2), round(1e6 * t0 / k, 2)]}
e.close()
o.close()

rec = {"workload": name, "trials": N, "seed": hex(SEED), "structures": "int_reg|pc|result", "tick_map": "device"}
for c in ("numinst", "literal"):
    out = outs[c]
    rec[c] = {"median_s": round(float(np.median(runs[c])), 4), "min_s": round(min(runs[c]), 4),
              "max_s": round(max(runs[c]), 4), "trials_per_s": round(N / float(np.median(runs[c]))),
              "classes": dict(zip(["masked", "sdc", "crash", "hang", "detected", "escape"],
                                  np.bincount(out["cls"], minlength=6).tolist())),
              "timing_escape_reasons": reasons(out), "mismatches": bad[c],
              "checked_against": "oracle contract output" if c == "numinst" else "oracle literal run (truth)"}
rec["oracle"] = {"checked": N, "reason_7_8_sites": kept, "oracle_s": round(oracle_s, 1), "threads": 16}
rec["stale_half_cost"] = stale
print(json.dumps(rec), flush=True)
sys.exit(0 if not (bad["numinst"] or bad["literal"]) else 1)
