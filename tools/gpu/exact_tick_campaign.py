"""Exact campaigns in the tick domain (fi_run_exact_ticks, DESIGN.md 4j "Tick
domain") on one GPU: the class build time of crc32 and qsort under both tick
contracts (fi_exact_tick_info.build_ms), the full crc32 x1..x31 + pc + result
campaign three times in the tick domain and three times as the atomic
fi_run_exact campaign of the same structures (wall time around the call, which
ends in a synchronise, and fi_last_kernel_ms), and crc32's time-weighted and
instruction-weighted SDC and masked shares per structure.

python tools/gpu/exact_tick_campaign.py [OUT.jsonl] -> JSON lines (also printed)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa
from shrewd_amd import Engine, CLASS_NAMES
REGS, PC, RESULT = (1 << 32) - 2, 1 << 32, 1 << 34
SEL = REGS | PC | RESULT
ROOT = sys.path[0]
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def emit(**kw):
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)
def elf(n):
    return open(os.path.join(ROOT, "workloads", f"{n}.elf"), "rb").read()
shares = {}
for name in ("crc32", "qsort"):
    e = Engine(); e.load_elf(elf(name), [name]); e.set_cpu_model("timing"); g = e.golden_run()
    e.set_tick_map("device")
    for contract in ("numinst", "literal"):
        e.set_tick_contract(contract); e.set_campaign(1, SEL, 1)
        x = e.exact_tick_info()
        emit(what="class_build", workload=name, contract=contract, build_ms=x.build_ms, segments=int(x.segments),
             attempts=len(e.exact_tick_attempts()), trials=int(x.trials), ninst=int(g.ninst),
             golden_ticks=int(e.tick_info()["golden_ticks"]), dead_ticks=int(x.dead_ticks), escaped_ticks=int(x.escaped_ticks),
             classes_regs=int(sum(x.classes[1:32])), classes_pc=int(x.classes[32]), classes_result=int(x.classes[34]))
    if name == "crc32":
        e.set_tick_contract("numinst"); x = e.exact_tick_info()
        for rep in range(3):
            t0 = time.perf_counter(); _, h = e.run_exact_ticks(0, int(x.trials), want_outcomes=False); dt = time.perf_counter() - t0
            emit(what="campaign", domain="tick", workload=name, rep=rep, wall_s=dt, kernel_ms=e.last_kernel_ms(), trials=int(x.trials),
                 space=int(x.space))
        per = int(e.tick_info()["golden_ticks"]) * 64
        shares["tick"] = {s: [int(v) / per for v in h["counts"][s].sum(axis=0)] for s in list(range(1, 33)) + [34]}
    e.close()
e = Engine(); e.load_elf(elf("crc32"), ["crc32"]); g = e.golden_run(); e.set_campaign(1, SEL, 1)
x = e.exact_info()
for rep in range(3):
    t0 = time.perf_counter(); _, h = e.run_exact(0, int(x.trials), want_outcomes=False); dt = time.perf_counter() - t0
    emit(what="campaign", domain="numinst", workload="crc32", rep=rep, wall_s=dt, kernel_ms=e.last_kernel_ms(), trials=int(x.trials),
         space=int(x.space), classes_regs=int(sum(x.classes[1:32])), classes_pc=int(x.classes[32]), classes_result=int(x.classes[34]))
per = int(g.ninst) * 64
shares["numinst"] = {s: [int(v) / per for v in h["counts"][s].sum(axis=0)] for s in list(range(1, 33)) + [34]}
sdc = CLASS_NAMES.index("sdc") if "sdc" in CLASS_NAMES else 1
for s in shares["tick"]:
    emit(what="sdc_share", workload="crc32", structure=s, time_weighted=shares["tick"][s][sdc], inst_weighted=shares["numinst"][s][sdc],
         masked_time_weighted=shares["tick"][s][0], masked_inst_weighted=shares["numinst"][s][0])
e.close()
