"""The profile of an exact campaign (fi_run_exact_profile, DESIGN.md 4j
"Profile") timed on one GPU: the x1..x31 x 64-bit register campaign of one
workload with want_outcomes=False, plain or profiled.

python tools/gpu/exact_profile.py [WORKLOAD] [--mode plain|profile] [--variant V]
    [--reps R] [--probe] [--top FILE] [--tree DIR]  -> one JSON line

--mode plain: run_exact(0, trials); profile: run_exact(0, trials, profile=True),
whose profile is checked against the histogram (per class, the rows' counts +
the dead sites == the histogram's).  Wall time around the call (it ends in a
synchronise) and the device time of the whole call, R times after a warm-up
launch.
--variant V: fi_debug_set_profile_variant (0 = wave-combine + LDS table, the
default; 1 = wave-combine only; 2 = one global atomic per trial).
--probe: one campaign after the warm-up, for a kernel trace taken around this
process in a run of its own.
--top FILE: FaultCampaign(profile=True).profile()'s first 12 rows as JSON.
--tree DIR: import shrewd_amd (and its library) from DIR instead of this
tree -- a checkout of another commit, for the parent's side of a comparison
(plain mode only)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
argv, MODE, VARIANT, REPS, PROBE, TOP, TREE = [], "plain", 0, 3, False, "", ROOT
it = iter(sys.argv[1:])
for a in it:
    if a == "--mode":
        MODE = next(it)
    elif a == "--variant":
        VARIANT = int(next(it))
    elif a == "--reps":
        REPS = max(1, int(next(it)))
    elif a == "--probe":
        PROBE = True
    elif a == "--top":
        TOP = next(it)
    elif a == "--tree":
        TREE = os.path.abspath(next(it))
    else:
        argv.append(a)
name = argv[0] if argv else "crc32"
assert MODE in ("plain", "profile")
sys.path.insert(0, TREE)
from shrewd_amd import Engine, FaultCampaign  # noqa: E402

REGS = (1 << 32) - 2
SEED = 0x5EED0E8A
path = os.path.join(ROOT, "workloads", f"{name}.elf")

if TOP:
    c = FaultCampaign(path, cmd=[name], structures=REGS, profile=True)
    c.engine.wait_translation()
    c.run_exact()
    rows = c.profile()
    with open(TOP, "w") as f:
        json.dump({"workload": name, "structures": "x1..x31", "bits": "0-63", "space": int(c.engine.exact_info().space),
                   "rows": len(rows), "sort": "sdc", "top": rows[:12]}, f, indent=1)
    print(json.dumps({"workload": name, "top": TOP, "rows": len(rows)}), flush=True)
    sys.exit(0)

with open(path, "rb") as f:
    elf = f.read()
e = Engine(device=0)
e.load_elf(elf, [name])
g = e.golden_run()
e.set_campaign(SEED, REGS, 1)
x = e.exact_info()
trials, L = int(x.trials), min(int(x.trials), e.config()["max_trials_per_launch"])
if MODE == "profile":
    e.debug_set_profile_variant(VARIANT)


def run(n):
    t0 = time.perf_counter()
    r = e.run_exact(0, n, want_outcomes=False, profile=True) if MODE == "profile" else \
        e.run_exact(0, n, want_outcomes=False)
    return r, (time.perf_counter() - t0) * 1e3, e.last_kernel_ms()


run(L)                                       # warm-up: code objects, work buffers, the profile's tables
runs = [run(trials) for _ in range(1 if PROBE else REPS)]
r = runs[-1][0]
h = r[1]
assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
rec = {"workload": name, "mode": MODE, "tree": os.path.relpath(TREE, ROOT), "exact_trials": trials, "sites": int(x.space),
       "wall_ms": [round(w, 2) for _, w, _ in runs], "device_ms": [round(d, 2) for _, _, d in runs],
       "median_wall_ms": round(statistics.median(w for _, w, _ in runs), 2)}
if MODE == "profile":
    prof = r[2]
    per_class = prof.sum(axis=(0, 1)).astype(int)
    per_class[0] += int(x.dead_sites)
    assert (per_class == h["counts"].sum(axis=(0, 1)).astype(int)).all() and not prof[:, 1:].any()
    rec.update(variant=VARIANT, rows=len(prof), rows_charged=int((prof.sum(axis=(1, 2)) > 0).sum()))
if PROBE:
    rec["probe"] = True
print(json.dumps(rec), flush=True)
e.close()
