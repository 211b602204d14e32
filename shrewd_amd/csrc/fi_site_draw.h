// The campaign's fault-site draw, as one function for the device samplers
// (fi_kernels.hip fi_sample_kernel, fi_tick_map_kernel) and the host one
// (fi_engine.cpp fi_sample_tick_sites): site = f(seed, trial) only, so it is
// the same on every shard.  The oracle states the same draw on its own
// (oracle/rv64se.c or_sample, or_tick_sample); tests/test_tick_device_cpu.py
// compares the two.
#pragma once
#include "fi_types.h"

namespace fi {

// SplitMix64 (Steele, Lea & Flood 2014)
FI_TM_HD inline uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

FI_TM_HD inline uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The lowest-bit positions a burst of `burst` bits can start at
FI_TM_HD inline uint64_t burst_positions(uint32_t burst) { return burst == 1 ? ~0ULL : ((2ULL << (64 - burst)) - 1); }

// structures: the fault structures to draw from (bit FI_T_*), not empty; the
// draw is undefined when no eligible bit position is left (bits & positions == 0).
inline DrawCtx draw_ctx(uint64_t seed, uint64_t structures, uint64_t first, uint64_t bits, uint32_t burst) {
    DrawCtx d{};
    d.seed = seed; d.structures = structures; d.first = first;
    d.bits = bits & burst_positions(burst);
    d.burst = burst;
    d.n_struct = (uint32_t)__builtin_popcountll(structures);
    return d;
}

struct SiteDraw {
    uint64_t when;     // uniform in [0, range): the numInst or the tick
    uint64_t mask;
    uint64_t r3;       // the fourth word: a memory site's address draw
    uint32_t target, trial;
};

// Trial c.first + i
FI_TM_HD inline SiteDraw draw_site(const DrawCtx &c, uint64_t i, uint64_t range) {
    const uint64_t id = c.first + i;
    uint64_t st = c.seed ^ (id * 0xD6E8FEB86659FD93ULL);
    const uint64_t r0 = splitmix(st), r1 = splitmix(st), r2 = splitmix(st);
    SiteDraw s;
    s.r3 = splitmix(st);
    s.when = mulhi64(r0, range);
    uint64_t m = c.structures;   // the k-th structure
    for (uint64_t k = mulhi64(r1, (uint64_t)c.n_struct); k; k--) m &= m - 1;
    s.target = (uint32_t)__builtin_ctzll(m);
    uint64_t b;
    if (c.bits == burst_positions(c.burst)) {
        b = mulhi64(r2, (uint64_t)(65 - c.burst));   // every position
    } else {                                          // the k-th eligible position
        uint64_t mm = c.bits;
        for (uint64_t k = mulhi64(r2, (uint64_t)__builtin_popcountll(mm)); k; k--) mm &= mm - 1;
        b = (uint64_t)__builtin_ctzll(mm);
    }
    s.mask = (c.burst == 64 ? ~0ULL : ((1ULL << c.burst) - 1)) << b;
    s.trial = (uint32_t)id;
    return s;
}

}  // namespace fi
