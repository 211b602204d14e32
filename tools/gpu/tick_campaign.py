"""A tick-domain campaign (cpu_type="timing") on one GPU: N seeded single-bit
register / pc / result tick sites of one workload, timed end to end, every
trial re-run literally on the CPU oracle (checker only) and compared bit for
bit.  The numInst campaign of the same size is timed beside it.

python tools/gpu/tick_campaign.py [WORKLOAD] [N] [SEED] [CHECK] [--tick-map host|device|both] [--reps R]
-> JSON lines

--tick-map host (the default) / device: where the tick sites are sampled and
mapped (Engine.set_tick_map).  --tick-map both: after a warm-up of each path,
host-map and device-map run_tick_trials(0, N) alternate R times each (at least
5) in this one process, with the numInst run_trials of the same size beside
them; per path the median and the spread (min .. max) of the wall time around
the call, which ends in a synchronise.  The two paths' outcomes must be
byte-equal; the oracle check then covers the device-map outcomes."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from shrewd_amd import Engine  # noqa: E402
from shrewd_amd.fi import TICK_ESCAPE_NAMES, escape_breakdown  # noqa: E402

STRUCTS = ((1 << 32) - 2) | (1 << 32) | (1 << 34)
argv, TICK_MAP, REPS = [], "host", 5
it = iter(sys.argv[1:])
for a in it:
    if a == "--tick-map":
        TICK_MAP = next(it)
    elif a == "--reps":
        REPS = max(5, int(next(it)))
    else:
        argv.append(a)
if TICK_MAP not in ("host", "device", "both"):
    sys.exit("--tick-map: host, device or both")
name = argv[0] if len(argv) > 0 else "crc32"
N = int(argv[1]) if len(argv) > 1 else 100_000
SEED = int(argv[2], 0) if len(argv) > 2 else 0x5EED7102
CHECK = int(argv[3]) if len(argv) > 3 else N
elf = open(os.path.join(ROOT, "workloads", f"{name}.elf"), "rb").read()
e = Engine()
e.load_elf(elf, [name])
e.set_cpu_model("timing")
t0 = time.perf_counter()
g = e.golden_run()
info = e.tick_info()
setup = time.perf_counter() - t0
e.set_campaign(SEED, STRUCTS, 1)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def spread(xs):
    return {"median_s": round(float(np.median(xs)), 4), "min_s": round(min(xs), 4), "max_s": round(max(xs), 4),
            "trials_per_s": round(N / float(np.median(xs))), "runs_s": [round(x, 4) for x in xs]}


both = None
if TICK_MAP == "both":
    walls = {"host": [], "device": [], "numinst": []}
    outs = {}
    for w in ("device", "host", "device"):   # warm-up, the timed calls themselves: buffers (the largest
        e.set_tick_map(w)                    # request first), the packed table, the pinned staging
        e.run_tick_trials(0, N)
    e.run_trials(0, N, want_outcomes=False)
    for _ in range(REPS):
        for w in ("host", "device"):
            e.set_tick_map(w)
            dt, (outs[w], h) = timed(lambda: e.run_tick_trials(0, N))
            walls[w].append(dt)
        walls["numinst"].append(timed(lambda: e.run_trials(0, N, want_outcomes=False))[0])
    assert outs["host"].tobytes() == outs["device"].tobytes(), "host-map and device-map outcomes differ"
    both = {k: spread(v) for k, v in walls.items()}
    both["device_over_host"] = round(both["host"]["median_s"] / both["device"]["median_s"], 3)
    both["device_rate_over_numinst"] = round(both["numinst"]["median_s"] / both["device"]["median_s"], 3)
    both["outcomes_byte_equal"] = True
    out, wall = outs["device"], both["device"]["median_s"]
    e.set_tick_map("host")
else:
    e.set_tick_map(TICK_MAP)
    e.run_tick_trials(0, min(N, 20000), want_outcomes=False)   # warm-up (buffers)
    wall, (out, h) = timed(lambda: e.run_tick_trials(0, N))
    e.set_tick_map("host")
ts = e.sample_tick_sites(0, N)
_, disp, _ = e.map_tick_sites(ts)
t0 = time.perf_counter()
e.run_trials(0, N, want_outcomes=False)
wall_num = time.perf_counter() - t0
cls = np.bincount(out["cls"], minlength=6).tolist()
tesc = (out["cls"] == 5) & (out["sub"] == 7)
rec = {"workload": name, "tick_map": TICK_MAP, "trials": N, "seed": hex(SEED), "structures": "int_reg|pc|result",
       "golden_ninst": int(g.ninst), "golden_ticks": info["golden_ticks"], "attempts": info["attempts"],
       "timing_stats": info["stats"], "setup_s": round(setup, 3),
       "wall_s": round(wall, 3), "trials_per_s": round(N / wall),
       "numinst_campaign_trials_per_s": round(N / wall_num),
       "dispositions": {"device": int((disp == 0).sum()), "golden_equal": int((disp == 1).sum()),
                        "timing_escape": int((disp == 2).sum())},
       "classes": dict(zip(["masked", "sdc", "crash", "hang", "detected", "escape"], cls)),
       "escapes": escape_breakdown(out),
       "timing_escape_reasons": {TICK_ESCAPE_NAMES.get(int(k), str(k)): int(v) for k, v in
                                 zip(*np.unique(out["exit_code"][tesc], return_counts=True))}}
if both:
    rec["tick_map_both"] = both
print(json.dumps(rec), flush=True)
e.close()
from oracle.pyoracle import Oracle  # noqa: E402
idx = np.arange(N) if CHECK >= N else np.sort(np.random.default_rng(SEED).choice(N, size=CHECK, replace=False))
o = Oracle(elf, name)
o.run_golden()
o.tick_setup()
osites = o.tick_sample(SEED, 0, N, STRUCTS)
assert (osites == ts).all(), "sampled tick sites differ"
t1 = time.perf_counter()
bad = 0
piece = 20_000
for a in range(0, len(idx), piece):
    ref = o.run_tick_trials(osites[idx[a:a + piece]], threads=16)
    bad += int((ref != out[idx[a:a + piece]]).sum())
    print(json.dumps({"progress": a + len(ref), "of": int(len(idx)), "mismatches": bad,
                      "s": round(time.perf_counter() - t1, 1)}), flush=True)
rec["oracle_check"] = {"checked": int(len(idx)), "mismatches": bad, "oracle_s": round(time.perf_counter() - t1, 2),
                       "threads": 16, "which": "all trials" if CHECK >= N else "seeded sample",
                       "kind": "literal tick injection (rv64se.c tk_trial)"}
print(json.dumps(rec), flush=True)
sys.exit(0 if bad == 0 else 1)
