"""shrewd_amd -- MI355X-native fault-injection campaign engine for SHREWD/gem5.

The hot path (RV64 AtomicSimpleCPU SE-mode trials, one per GPU lane) runs in
hand-written HIP kernels behind the C ABI in include/fi_engine.h; this package
is the host-side mirror of the gem5 FaultCampaign SimObject interface.
"""
from .fi import (CLASS_NAMES, CRASH_NAMES, END_NAMES, ESCAPE_NAMES, HANG_NAMES, Capture, FaultCampaign, Engine,
                 EngineError, HIST_DT, OUTCOME_DT, SITE_DT, WAVE, allreduce_histogram, build_library, library_path,
                 exact_class_consumers, exact_classes, exact_mem_classes, exact_tick_classes, shard_range,
                 structures_mask)

__all__ = ["FaultCampaign", "Engine", "EngineError", "Capture", "OUTCOME_DT", "SITE_DT", "HIST_DT", "CLASS_NAMES",
           "CRASH_NAMES", "ESCAPE_NAMES", "HANG_NAMES", "END_NAMES", "allreduce_histogram", "build_library",
           "library_path", "exact_class_consumers", "exact_classes", "exact_mem_classes", "exact_tick_classes", "shard_range", "structures_mask", "STAT", "WAVE"]


def __getattr__(name):
    if name == "STAT":   # made from the library's table when it loads (fi.py)
        from . import fi
        return fi.STAT
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
