"""An exact campaign (fi_run_exact) on one GPU: the whole
x1..x31 x 64-bit fault space of one workload, one trial per first-access class,
timed end to end; the sampled run_trials of one launch's size beside it; then
the exact vulnerability table (x1..x31 and the pc).

python tools/gpu/exact_campaign.py [WORKLOAD] [--reps R] [--probe] [--memory]
-> JSON lines

Whole campaign: wall time around run_exact(0, trials) (it ends in a
synchronise) and the device time of the whole call (fi_last_kernel_ms), R
times after a warm-up launch.  Per trial: run_exact(0, L) and run_trials(0, L)
alternating R times, L = min(trials, the engine's trials per launch).

--probe: for a kernel trace taken around this process in a run of its own.
Only the first launch of the campaign, then fi_run_sites on the same chunk's
sites, so that fi_exact_hist_kernel (its uint32_t instantiation: a numInst
campaign's weights) and fi_hist_kernel each run once on the same sites and
outcomes.

--memory: the memory words (structure 33) alone, by byte-liveness class
(Engine.set_exact_memory): the one-time class build on its own (the first
exact_info(): wall, and the engine's own figure), then the whole campaign R
times."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from shrewd_amd import CLASS_NAMES, Engine  # noqa: E402

REGS, PC, MEM = (1 << 32) - 2, 1 << 32, 1 << 33
SEED = 0x5EED0E8A
argv, REPS, PROBE, MEMORY = [], 3, False, False
it = iter(sys.argv[1:])
for a in it:
    if a == "--reps":
        REPS = max(1, int(next(it)))
    elif a == "--probe":
        PROBE = True
    elif a == "--memory":
        MEMORY = True
    else:
        argv.append(a)
name = argv[0] if argv else "crc32"

with open(os.path.join(ROOT, "workloads", f"{name}.elf"), "rb") as f:
    elf = f.read()
e = Engine(device=0)
e.load_elf(elf, [name])
g = e.golden_run()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3, e.last_kernel_ms()


if MEMORY:
    e.set_exact_memory(True)
    e.set_campaign(SEED, MEM, 1)
    t0 = time.perf_counter()
    x = e.exact_info()                       # builds the classes
    build_wall = (time.perf_counter() - t0) * 1e3
    m = e.exact_mem_info()
    _, off, _ = e.golden_mem_index()
    trials = int(x.trials)
    L = min(trials, e.config()["max_trials_per_launch"])
    print(json.dumps({"workload": name, "what": "memory words, class build", "golden_ninst": int(g.ninst),
                      "translate": e.translate_status(), "sites": int(x.space), "words": int(m.words),
                      "text_words": int(m.text_words), "index_words": int(m.index_words),
                      "index_events": int(off[-1]), "max_events_per_word": int(np.diff(off.astype(np.int64)).max()),
                      "byte_sets": int(m.byte_sets), "classes": int(x.classes[33]), "exact_trials": trials,
                      "dead_sites": int(x.dead_sites), "dead_share": round(int(x.dead_sites) / int(x.space), 9),
                      "build_wall_ms": round(build_wall, 2), "build_ms": round(float(m.build_ms), 2)}), flush=True)
    e.run_exact(0, L, want_outcomes=False)   # warm-up: code objects, work buffers
    whole = []
    for _ in range(REPS):
        (_, h), wall, dev = timed(lambda: e.run_exact(0, trials, want_outcomes=False))
        whole.append((wall, dev))
    assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
    c = h["counts"][33].sum(axis=0)
    print(json.dumps({"workload": name, "what": "whole campaign, memory words", "exact_trials": trials,
                      "sites": int(x.space), "wall_ms": [round(w, 2) for w, _ in whole],
                      "device_ms": [round(d, 2) for _, d in whole],
                      "median_wall_ms": round(statistics.median(w for w, _ in whole), 2),
                      "median_device_ms": round(statistics.median(d for _, d in whole), 2),
                      "counts": {CLASS_NAMES[k]: int(c[k]) for k in range(6)},
                      "device_insts": int(h["device_insts"])}), flush=True)
    e.close()
    sys.exit(0)

e.set_campaign(SEED, REGS, 1)
x = e.exact_info()
trials, L = int(x.trials), min(int(x.trials), e.config()["max_trials_per_launch"])
print(json.dumps({"workload": name, "golden_ninst": int(g.ninst), "translate": e.translate_status(),
                  **{k: v for k, v in x.as_dict().items() if k != "classes"},
                  "classes_x1_x31": sum(x.as_dict()["classes"].values()), "launch": L}), flush=True)

if PROBE:
    e.run_exact(0, L, want_outcomes=False)
    sites, _ = e.exact_sites(0, L)
    e.run_sites(sites)
    print(json.dumps({"probe": name, "chunk": L}), flush=True)
    e.close()
    sys.exit(0)

e.run_exact(0, L, want_outcomes=False)       # warm-up: code objects, work buffers
e.run_trials(0, L, want_outcomes=False)
whole = []
for _ in range(REPS):
    (_, h), wall, dev = timed(lambda: e.run_exact(0, trials, want_outcomes=False))
    whole.append((wall, dev))
assert int(h["counts"].sum()) == int(h["trials"]) == int(x.space)
print(json.dumps({"workload": name, "what": "whole campaign, x1..x31", "exact_trials": trials, "sites": int(x.space),
                  "wall_ms": [round(w, 2) for w, _ in whole], "device_ms": [round(d, 2) for _, d in whole],
                  "median_wall_ms": round(statistics.median(w for w, _ in whole), 2),
                  "median_device_ms": round(statistics.median(d for _, d in whole), 2),
                  "sites_per_s": round(int(x.space) / (statistics.median(w for w, _ in whole) / 1e3)),
                  "device_insts": int(h["device_insts"])}), flush=True)
ex, sa = [], []
for _ in range(REPS):
    _, wall, dev = timed(lambda: e.run_exact(0, L, want_outcomes=False))
    ex.append((wall, dev))
    _, wall, dev = timed(lambda: e.run_trials(0, L, want_outcomes=False))
    sa.append((wall, dev))
med = lambda v, i: statistics.median(t[i] for t in v)   # noqa: E731
print(json.dumps({"workload": name, "what": "one launch, exact against sampled", "trials": L,
                  "exact_wall_ms": [round(w, 2) for w, _ in ex], "exact_device_ms": [round(d, 2) for _, d in ex],
                  "sampled_wall_ms": [round(w, 2) for w, _ in sa], "sampled_device_ms": [round(d, 2) for _, d in sa],
                  "exact_ns_per_trial": round(med(ex, 1) * 1e6 / L, 2),
                  "sampled_ns_per_trial": round(med(sa, 1) * 1e6 / L, 2)}), flush=True)

# the table: x1..x31 and the pc (the space of the sampled C2 campaigns)
e.set_campaign(SEED, REGS | PC, 1)
y = e.exact_info()
(_, h), wall, dev = timed(lambda: e.run_exact(0, int(y.trials), want_outcomes=False))
per = int(g.ninst) * int(y.nbits)
c = h["counts"]
share = lambda v: {CLASS_NAMES[k]: round(int(v[k]) / int(v.sum()), 6) for k in range(6)}   # noqa: E731
print(json.dumps({"workload": name, "what": "exact table, x1..x31 | pc", "sites": int(y.space),
                  "exact_trials": int(y.trials), "wall_ms": round(wall, 2), "device_ms": round(dev, 2),
                  "all": share(c[1:33].sum(axis=(0, 1))), "x1_x31": share(c[1:32].sum(axis=(0, 1))),
                  "counts_all": [int(v) for v in c[1:33].sum(axis=(0, 1))],
                  "per_structure": {str(s): {CLASS_NAMES[k]: round(int(c[s, :, k].sum()) / per, 6) for k in range(6)}
                                    for s in range(1, 33)}}), flush=True)
e.close()
