// Exact register vulnerability: the fault space of a campaign
// enumerated by first-access class instead of sampled.  One statement for the
// host (fi_engine.cpp fi_exact_classes, the plan of fi_run_exact;
// tools/exact_host_check.cpp) and the device (fi_kernels.hip
// fi_exact_sites_kernel).
//
// Register r's entries ev[off[r] .. off[r + 1]) of the first-access index
// (fi_golden_host.h first_access_index: (2 * numInst + !ecall) << 1 | reads)
// cut its timeline [0, ninst) into intervals that end at an access.  With
// u'_i = min(ev_i >> 2, ninst - 1) and prev'_i = u'_{i-1} (-1 before the first
// entry), entry i heads a class iff it reads and u'_i > prev'_i: a flip at any
// t in (prev'_i, u'_i] is the flip at u'_i (first-access forwarding, DESIGN.md
// §4), so one trial at inst = u'_i stands for all of them with weight
// u'_i - prev'_i.  Every other t is dead -- the next access writes the
// register, or there is none -- and its trial is the golden run.  The clip to
// ninst - 1: the exit ecall reads a0..a7 at numInst == ninst, and sites exist
// only for t < ninst.  The pc and an instruction's result have one class of
// weight 1 per t and no dead sites; they need no table.
#pragma once
#include "fi_site_draw.h"
#include "fi_types.h"

namespace fi {

// A register class in 8 bytes: inst (29 bits: first_access_index exists only
// for ninst < 2^29), register (5), weight (30)
constexpr uint32_t kExactInstBits = 29, kExactRegBits = 5;
FI_TM_HD inline uint64_t exact_pack(uint64_t inst, uint32_t reg, uint64_t weight) {
    return inst | ((uint64_t)reg << kExactInstBits) | (weight << (kExactInstBits + kExactRegBits));
}
FI_TM_HD inline uint64_t exact_word_inst(uint64_t w) { return w & ((1ULL << kExactInstBits) - 1); }
FI_TM_HD inline uint32_t exact_word_reg(uint64_t w) { return (uint32_t)(w >> kExactInstBits) & ((1u << kExactRegBits) - 1); }
FI_TM_HD inline uint32_t exact_word_weight(uint64_t w) { return (uint32_t)(w >> (kExactInstBits + kExactRegBits)); }

// Register reg's classes in time order as packed words: out[0 .. min(count,
// cap)) (out may be NULL); returns the count, *dead = ninst - the weights' sum.
inline uint64_t exact_reg_classes(const uint32_t *off, const uint32_t *ev, uint64_t ninst, uint32_t reg,
                                  uint64_t *out, uint64_t cap, uint64_t *dead) {
    uint64_t n = 0, live = 0;
    int64_t prev = -1;
    for (uint32_t i = off[reg]; ninst && i < off[reg + 1]; i++) {
        const uint64_t t = ev[i] >> 2;
        const int64_t u = (int64_t)(t < ninst - 1 ? t : ninst - 1);
        if ((ev[i] & 1u) && u > prev) {
            if (out && n < cap) out[n] = exact_pack((uint64_t)u, reg, (uint64_t)(u - prev));
            n++;
            live += (uint64_t)(u - prev);
        }
        prev = u;
    }
    if (dead) *dead = ninst - live;
    return n;
}

// The trial ids of an exact campaign.  k counts through the selected
// structures in ascending number, within a structure through its classes in
// time order, within a class through the eligible bit positions ascending:
// k = class index * nbits + bit slot, the class index running on across the
// structures.  A row per selected structure: its first trial, what added to
// the class index gives the class word's index (registers) or the class's t
// (pc, result; modulo 2^32), and the structure (0: a register, the word names it).
constexpr uint32_t kExactMaxRows = 33;        // x1..x31, the pc, an instruction's result
constexpr uint64_t kExactMaxTrials = 1ULL << 40;   // the reciprocal below is exact under it
struct ExactRow {
    uint64_t first;
    uint32_t delta, target;
};
struct ExactPlan {
    ExactRow row[kExactMaxRows];
    uint32_t n_rows, nbits;
    uint32_t burst, shift;     // nbits a power of two: class index = k >> shift; else shift = 64
    uint64_t recip;            //   and class index = mulhi(k, recip), recip = floor(2^64 / nbits) + 1
    uint64_t bits;             // the eligible lowest-bit positions (limited to 0 .. 64 - burst)
    uint64_t trials;
};

// k / nbits without a 64-bit divide.  nbits <= 64 not a power of two:
// recip * nbits = 2^64 + e with 0 < e < nbits, so mulhi(k, recip) =
// floor(k / nbits + k * e / (nbits * 2^64)) is the quotient whenever
// k * e < 2^64 -- far past k < 2^40.
static_assert(kExactMaxTrials * 64 < (1ULL << 63), "exact_class_index: reciprocal exact for every trial id");
FI_TM_HD inline uint64_t exact_class_index(const ExactPlan &p, uint64_t k) {
    return p.shift < 64 ? k >> p.shift : mulhi64(k, p.recip);
}

// The plan of a campaign: structures (bits 1..31, FI_T_PC, FI_T_RESULT), the
// fi_set_bits mask and the burst; cls_off[r] .. cls_off[r + 1] = register r's
// words in the class array.  classes (FI_N_STRUCT entries, may be NULL)
// receives each structure's class count.
inline ExactPlan exact_plan(uint64_t structures, const uint32_t *cls_off, uint64_t ninst, uint64_t bits_mask,
                            uint32_t burst, uint64_t *classes) {
    ExactPlan p{};
    p.burst = burst;
    p.bits = bits_mask & burst_positions(burst);
    p.nbits = (uint32_t)__builtin_popcountll(p.bits);
    p.shift = 64;
    if (p.nbits && !(p.nbits & (p.nbits - 1))) p.shift = (uint32_t)__builtin_ctz(p.nbits);
    else if (p.nbits) p.recip = ~0ULL / p.nbits + 1;
    uint64_t q = 0;   // the class index so far
    for (uint32_t t = 1; t < FI_N_STRUCT; t++) {
        if (classes) classes[t] = 0;
        if (!((structures >> t) & 1) || t == FI_T_MEM) continue;
        ExactRow &r = p.row[p.n_rows++];
        r.first = q * p.nbits;
        r.target = t < 32 ? 0 : t;
        r.delta = (t < 32 ? cls_off[t] : 0u) - (uint32_t)q;
        const uint64_t n = t < 32 ? cls_off[t + 1] - cls_off[t] : ninst;
        if (classes) classes[t] = n;
        q += n;
    }
    p.trials = q * p.nbits;
    return p;
}

// The dead sites of a campaign (fi_exact_dead_kernel)
struct ExactDead {
    uint32_t dead[32];         // per register (0: not selected)
    uint64_t bits, total;      // eligible positions; the sum of dead x the eligible positions
    uint64_t golden_ninst;
};

struct ExactSite {
    uint64_t inst, mask;
    uint32_t target, weight;
};

// Exact trial k (k < p.trials); classes = every register's packed words
FI_TM_HD inline ExactSite exact_site(const ExactPlan &p, const uint64_t *classes, uint64_t k) {
    const uint64_t q = exact_class_index(p, k);
    const uint32_t slot = (uint32_t)(k - q * p.nbits);
    // the last row that starts at or before k (rows ascend; one compare per row, no indexed access)
    uint32_t delta = p.row[0].delta, target = p.row[0].target;
    for (uint32_t r = 1; r < p.n_rows; r++) {
        const bool in = p.row[r].first <= k;
        delta = in ? p.row[r].delta : delta;
        target = in ? p.row[r].target : target;
    }
    const uint32_t x = (uint32_t)q + delta;
    ExactSite s;
    if (target) {
        s.inst = x; s.target = target; s.weight = 1;
    } else {
        const uint64_t w = classes[x];
        s.inst = exact_word_inst(w); s.target = exact_word_reg(w); s.weight = exact_word_weight(w);
    }
    uint64_t b = slot;   // positions 0 .. nbits - 1: the slot is the position
    if (p.bits & (p.bits + 1)) {
        uint64_t mm = p.bits;
        for (uint32_t j = slot; j; j--) mm &= mm - 1;
        b = (uint64_t)__builtin_ctzll(mm);
    }
    s.mask = (p.burst == 64 ? ~0ULL : ((1ULL << p.burst) - 1)) << b;
    return s;
}

}  // namespace fi
