"""Dump a program's pre-decoded text and golden trace (the translator's
inputs) to gpurun_out/golden_NAME.npz, for offline work on the translator
(tools/jit_inspect.py) and for the fixtures tests/golden/tx_inputs_NAME.npz
(the same arrays, compressed).
python tools/gpu/dump_golden.py [--fixture] [NAME | kat:NAME | PATH.elf ...]
python tools/gpu/dump_golden.py --pack golden_NAME.npz ...
NAME is workloads/NAME.elf; kat:NAME the known-answer program NAME of
tests/test_isa_vectors.py (NAME_program_elf, e.g. kat:region); PATH.elf any
ELF file (named after its stem).  --fixture also writes the fixture of each
program dumped; --pack writes the fixtures of dumps made earlier (no engine,
no GPU: for dumps brought over from the GPU machine)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from shrewd_amd import Engine  # noqa: E402


def load(arg):
    """(name, ELF bytes) of one command-line argument."""
    if arg.startswith("kat:"):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_isa_vectors as kat
        return arg[4:], getattr(kat, f"{arg[4:]}_program_elf")()
    path = arg if arg.endswith(".elf") else os.path.join(ROOT, "workloads", f"{arg}.elf")
    return os.path.splitext(os.path.basename(path))[0], open(path, "rb").read()


def write_fixture(name, pre, trace, text_lo):
    path = os.path.join(ROOT, "tests", "golden", f"tx_inputs_{name}.npz")
    np.savez_compressed(path, pre=pre, trace=trace, text_lo=np.uint64(text_lo))
    print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes", flush=True)


argv = [a for a in sys.argv[1:] if a not in ("--fixture", "--pack")]
if "--pack" in sys.argv[1:]:
    for path in argv:
        z = np.load(path)
        write_fixture(os.path.splitext(os.path.basename(path))[0].replace("golden_", "", 1), z["pre"], z["trace"],
                      z["text_lo"])
    sys.exit(0)
os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
for arg in argv or ["hello", "crc32", "qsort", "intmix", "fpamo"]:
    name, elf = load(arg)
    e = Engine()
    e.load_elf(elf, [name])
    e.golden_run()
    pre, tr, lo = e.debug_golden_trace()
    np.savez(os.path.join(ROOT, "gpurun_out", f"golden_{name}.npz"), pre=pre, trace=tr, text_lo=np.uint64(lo))
    print(name, len(pre), len(tr), e.translate_status()[:100], flush=True)
    if "--fixture" in sys.argv[1:]:
        write_fixture(name, pre, tr, lo)
    e.close()
