// Exact vulnerability: the fault space of a campaign
// enumerated by first-access class instead of sampled.  One statement for the
// host (fi_engine.cpp fi_exact_classes, fi_exact_mem_classes, the plan of
// fi_run_exact; tools/exact_host_check.cpp, tools/exact_mem_host_check.cpp)
// and the device (fi_kernels.hip fi_exact_sites_kernel, fi_exact_mem_*_kernel;
// the sites without a trial: ExactUntried, fi_exact_untried_kernel).
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
#include <algorithm>
#include <vector>

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

// The entries that head register reg's classes, in time order: f(class number,
// the entry, u', weight) for each; returns their count, *dead = ninst - the
// weights' sum.
template <typename F>
inline uint64_t exact_reg_heads(const uint32_t *off, const uint32_t *ev, uint64_t ninst, uint32_t reg, F f,
                                uint64_t *dead) {
    uint64_t n = 0, live = 0;
    int64_t prev = -1;
    for (uint32_t i = off[reg]; ninst && i < off[reg + 1]; i++) {
        const uint64_t t = ev[i] >> 2;
        const int64_t u = (int64_t)(t < ninst - 1 ? t : ninst - 1);
        if ((ev[i] & 1u) && u > prev) {
            f(n, ev[i], (uint64_t)u, (uint64_t)(u - prev));
            n++;
            live += (uint64_t)(u - prev);
        }
        prev = u;
    }
    if (dead) *dead = ninst - live;
    return n;
}

// Register reg's classes in time order as packed words: out[0 .. min(count,
// cap)) (out may be NULL); returns the count, *dead = ninst - the weights' sum.
inline uint64_t exact_reg_classes(const uint32_t *off, const uint32_t *ev, uint64_t ninst, uint32_t reg,
                                  uint64_t *out, uint64_t cap, uint64_t *dead) {
    return exact_reg_heads(off, ev, ninst, reg, [&](uint64_t n, uint32_t, uint64_t u, uint64_t w) {
        if (out && n < cap) out[n] = exact_pack(u, reg, w);
    }, dead);
}

// ---- Profile: the consumer of a class (DESIGN.md §4j "Profile").
//
// A class is charged to one entry of the golden trace -- a static instruction
// that committed, or an ecall that was attempted -- named here by a value per
// entry: the profile's row (the engine), or the trace word itself (halfword
// index, bit 31 = ecall: fi_exact_class_consumers).  Two tables over the trace
// (exact_consumer_tables): inst_val[t], t in [0, ninst), the value of the
// instruction that commits as numInst t, and the ecalls as (numInst, value)
// pairs ascending in numInst, the first ecall entry at each (an ecall commits
// nothing: its entry sits at the numInst of the instruction after it; a second
// ecall at the same numInst is charged to the first).
//  - Register: the entry that heads the class, at its unclipped numInst
//    ev >> 2: key ev >> 1 even -> that numInst's ecall, else inst_val.
//  - The pc and an instruction's result: inst_val[t].
//  - A memory word: the event that heads the class, at its unclipped numInst;
//    recorded as a syscall's access (proxy) and an ecall stands at that numInst
//    -> the ecall, else inst_val (an M5 op's proxy reads, say).
struct ExactEcall { uint32_t t, val; };
constexpr uint32_t kExactNoConsumer = 0xFFFFFFFFu;

struct ExactConsumers {        // the two tables, the host's or the device's
    const uint32_t *inst_val;
    const ExactEcall *ecall;
    uint64_t ninst;
    uint32_t n_ecall, pad;
};

// The value of numInst t's ecall, kExactNoConsumer without one
FI_TM_HD inline uint32_t exact_ecall_val(const ExactConsumers &c, uint64_t t) {
    uint32_t lo = 0, hi = c.n_ecall;   // first pair with t' >= t
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (c.ecall[mid].t < t) lo = mid + 1; else hi = mid;
    }
    return lo < c.n_ecall && c.ecall[lo].t == t ? c.ecall[lo].val : kExactNoConsumer;
}
// The consumer of an access at numInst t (unclipped) made by an ecall
// (by_ecall) or by the instruction that commits there.  (The index past the
// last instruction is clamped: only an ecall stands there.)
FI_TM_HD inline uint32_t exact_consumer(const ExactConsumers &c, uint64_t t, bool by_ecall) {
    if (by_ecall) {
        const uint32_t v = exact_ecall_val(c, t);
        if (v != kExactNoConsumer) return v;
    }
    if (!c.ninst) return kExactNoConsumer;
    return c.inst_val[t < c.ninst ? t : c.ninst - 1];
}
FI_TM_HD inline uint32_t exact_reg_consumer(const ExactConsumers &c, uint32_t ev) {
    return exact_consumer(c, ev >> 2, !((ev >> 1) & 1u));
}
FI_TM_HD inline uint32_t exact_mem_consumer(const ExactConsumers &c, uint64_t ev, bool proxy) {
    return exact_consumer(c, ev >> 16, proxy);
}

// Register reg's consumers, one per class in exact_reg_classes' order
inline uint64_t exact_reg_consumers(const uint32_t *off, const uint32_t *ev, uint64_t ninst, uint32_t reg,
                                    const ExactConsumers &c, uint32_t *out, uint64_t cap) {
    return exact_reg_heads(off, ev, ninst, reg, [&](uint64_t n, uint32_t e, uint64_t, uint64_t) {
        if (out && n < cap) out[n] = exact_reg_consumer(c, e);
    }, nullptr);
}

// The tables of a trace: val[i] names entry i (NULL: the trace word itself).
// Returns false when the trace does not hold ninst committing entries.
inline bool exact_consumer_tables(const uint32_t *trace, uint64_t n_trace, const uint32_t *val, uint64_t ninst,
                                  std::vector<uint32_t> &inst_val, std::vector<ExactEcall> &ecall) {
    inst_val.clear();
    ecall.clear();
    for (uint64_t i = 0; i < n_trace; i++) {
        const uint32_t v = val ? val[i] : trace[i];
        const uint64_t t = inst_val.size();
        if (!(trace[i] & 0x80000000u)) inst_val.push_back(v);
        else if (ecall.empty() || ecall.back().t != t) ecall.push_back(ExactEcall{(uint32_t)t, v});
    }
    return inst_val.size() == ninst;
}

// The profile's rows: the distinct trace words with bit 31 cleared, ascending
// (so ascending in pc); row_of[i] = entry i's row, execs[row] = its entries,
// is_ecall[row] = its entries are ecalls.
inline void exact_profile_rows(const uint32_t *trace, uint64_t n_trace, std::vector<uint32_t> &half,
                               std::vector<uint64_t> &execs, std::vector<uint8_t> &is_ecall,
                               std::vector<uint32_t> &row_of) {
    half.resize(n_trace);
    for (uint64_t i = 0; i < n_trace; i++) half[i] = trace[i] & 0x7FFFFFFFu;
    std::sort(half.begin(), half.end());
    half.erase(std::unique(half.begin(), half.end()), half.end());
    execs.assign(half.size(), 0);
    is_ecall.assign(half.size(), 0);
    row_of.resize(n_trace);
    for (uint64_t i = 0; i < n_trace; i++) {
        const uint32_t r = (uint32_t)(std::lower_bound(half.begin(), half.end(), trace[i] & 0x7FFFFFFFu) - half.begin());
        row_of[i] = r;
        execs[r]++;
        if (trace[i] & 0x80000000u) is_ecall[r] = 1;
    }
}

// ---- Memory words (FI_T_MEM), by byte-liveness class.
//
// Words.  The space is every 8-byte word of the memory-fault candidate pages
// (512 per page, as fi_sample_kernel draws them) that does not overlap
// [text_lo, text_hi): mem_dead never calls an instruction word dead and
// forwarding never moves one (fetches are not in the index), so they have no
// classes; they are counted (text words) and left out.
//
// Byte sets.  A position b flips the bytes F(b) = { b / 8 .. (b + burst - 1) / 8 }
// -- the fb that fi_forward_kernel and mem_dead compute from the mask.  The
// eligible positions with equal F form a byte set; F's ends do not decrease
// with b, so a byte set is a run of consecutive eligible positions and the
// sets are ordered by their lowest one: at most 15 for burst <= 8, 64 at most.
//
// Byte liveness.  A word's events (DevCtx::mw_ev: numInst << 16 | bytes read
// << 8 | bytes written, in time order) walked backwards: live_after(last) = 0,
// live_before(i) = rd_i | (live_after(i) & ~wr_i), live_after(i - 1) =
// live_before(i); an event that reads and writes (an AMO) reads first.  A flip
// of the bytes F just before event i is dead iff F & live_before(i) == 0 --
// mem_dead's forward walk, for every byte set at once.
//
// Intervals.  For a word and a byte set F, the events that touch F ((rd | wr)
// & F != 0) in time order -- forwarding stops at the first one: u'_i =
// min(ev_i >> 16, ninst - 1), prev'_i = u'_{i-1} (-1 before the first); entry
// i heads an interval iff u'_i > prev'_i, over t in (prev'_i, u'_i].  If F &
// live_before(i) != 0 the interval is a class: one trial per position of the
// byte set at inst = u'_i, addr = the word, weight u'_i - prev'_i.  Otherwise
// every site of it is dead, as are the sites after the last touching event and
// every site of a word the index does not list.
struct ExactMemClass {
    uint32_t word;             // index of the word in DevCtx::mw_addr
    uint32_t inst, weight;
    uint32_t cons;             // its consumer (a profiled build; else 0)
};
struct ExactMemRow {           // a byte set: a row of the plan with its own position count
    uint64_t first;            // its first trial, counted from the plan's mem_first
    uint64_t recip;            // class index within the row = (j - first) >> shift, or mulhi(j - first, recip)
    uint64_t pos;              // its positions
    uint32_t base;             // its first class in the class array
    uint32_t npos, shift, fmask;   // fmask: F, a bit per byte
};
constexpr uint32_t kExactMaxMemRows = 64;

FI_TM_HD inline uint32_t exact_byte_set(uint32_t b, uint32_t burst) {
    const uint32_t lo = b >> 3, hi = (b + burst - 1) >> 3;
    return ((2u << hi) - 1) & ~((1u << lo) - 1) & 0xFF;
}

// The byte sets of (fi_set_bits mask, burst) in their order: fmask, pos, npos
// and the quotient constants of rows[0 .. n); returns n.
inline uint32_t exact_mem_sets(uint64_t bits_mask, uint32_t burst, ExactMemRow *rows) {
    uint32_t n = 0;
    for (uint64_t m = bits_mask & burst_positions(burst); m; m &= m - 1) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m), f = exact_byte_set(b, burst);
        if (!n || rows[n - 1].fmask != f) {
            rows[n] = ExactMemRow{};
            rows[n++].fmask = f;
        }
        rows[n - 1].pos |= 1ULL << b;
    }
    for (uint32_t g = 0; g < n; g++) {
        ExactMemRow &r = rows[g];
        r.npos = (uint32_t)__builtin_popcountll(r.pos);
        r.shift = 64;
        if (!(r.npos & (r.npos - 1))) r.shift = (uint32_t)__builtin_ctz(r.npos);
        else r.recip = ~0ULL / r.npos + 1;
    }
    return n;
}

// Is the word at addr (8-byte aligned) in the space?  pages: the candidate
// pages, sorted.  (Last bytes, not ends: a page at the top of the address
// space has no end in 64 bits.)
FI_TM_HD inline bool exact_mem_in_space(const uint64_t *pages, uint64_t n_pages, uint64_t text_lo, uint64_t text_hi,
                                        uint64_t addr) {
    if (addr < text_hi && addr + 7 >= text_lo) return false;
    uint64_t lo = 0, hi = n_pages;
    const uint64_t pg = addr & ~4095ULL;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pages[mid] < pg) lo = mid + 1; else hi = mid;
    }
    return lo < n_pages && pages[lo] == pg;
}
// The words of the candidate pages that overlap the text
inline uint64_t exact_mem_text_words(const uint64_t *pages, uint64_t n_pages, uint64_t text_lo, uint64_t text_hi) {
    uint64_t n = 0;
    for (uint64_t i = 0; i < n_pages && text_lo < text_hi; i++) {
        // the first and the last word of the page that overlap [text_lo, text_hi)
        const uint64_t tf = text_lo & ~7ULL, tl = (text_hi - 1) & ~7ULL, pl = pages[i] + 4088;
        const uint64_t a = pages[i] > tf ? pages[i] : tf, b = pl < tl ? pl : tl;
        if (a <= b) n += (b - a) / 8 + 1;
    }
    return n;
}

// live_before of a word's n events (one byte each)
FI_TM_HD inline void exact_mem_liveness(const uint64_t *ev, uint32_t n, uint8_t *live) {
    uint32_t l = 0;
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t e = (uint32_t)ev[i];
        l = ((e >> 8) | (l & ~e)) & 0xFF;
        live[i] = (uint8_t)l;
    }
}

// The walk of one (word, byte set): its classes in time order to out[0 ..
// min(count, cap)) (out may be NULL); returns the count, *wsum = the sum of
// their weights (the word's other ninst - *wsum sites of the set are dead).
// With the consumer tables (pc != NULL) and the events' proxy bits (a bit per
// event of the whole index, this word's first at bit ev_base) each class also
// gets its consumer.
FI_TM_HD inline uint64_t exact_mem_walk(const uint64_t *ev, const uint8_t *live, uint32_t n, uint64_t ninst,
                                        uint32_t fmask, uint32_t word, ExactMemClass *out, uint64_t cap,
                                        uint64_t *wsum, const ExactConsumers *pc = nullptr,
                                        const uint32_t *proxy = nullptr, uint64_t ev_base = 0) {
    uint64_t cnt = 0, sum = 0;
    int64_t prev = -1;
    for (uint32_t i = 0; ninst && i < n; i++) {
        const uint64_t e = ev[i];
        if (!(((e >> 8) | e) & fmask & 0xFF)) continue;
        const uint64_t t = e >> 16;
        const int64_t u = (int64_t)(t < ninst - 1 ? t : ninst - 1);
        if (u > prev && (live[i] & fmask)) {
            if (out && cnt < cap) {
                ExactMemClass c;
                c.word = word; c.inst = (uint32_t)u; c.weight = (uint32_t)(u - prev);
                c.cons = pc ? exact_mem_consumer(*pc, e, (proxy[(ev_base + i) >> 5] >> ((ev_base + i) & 31)) & 1u) : 0;
                out[cnt] = c;
            }
            cnt++;
            sum += (uint64_t)(u - prev);
        }
        prev = u;
    }
    if (wsum) *wsum = sum;
    return cnt;
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
    // memory words (exact_plan_mem; mem_trials = 0 without them): trials [mem_first, mem_first +
    // mem_trials) between the pc's and the result's, one row per byte set in a table beside the
    // classes (the rows would not fit a kernel argument); the rows above count past them
    uint64_t mem_first, mem_trials;
    const ExactMemRow *mem_rows;
    const ExactMemClass *mem_cls;
    const uint64_t *mem_addr;  // the index's word addresses (DevCtx::mw_addr)
    uint32_t n_mem_rows, pad;
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
        if (t == FI_T_MEM) p.mem_first = q * p.nbits;   // where exact_plan_mem puts them
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

// Memory's trials added to a plan: rows[g].base and the classes per row give
// each row's first trial; ids: byte sets in their order, within one the words
// by ascending address, within a word its classes in time order, within a
// class the set's positions ascending.  The tables are the device's (or, in a
// host check, the host's).
inline void exact_plan_mem(ExactPlan &p, ExactMemRow *rows, uint32_t n_rows, const uint64_t *row_classes,
                           const ExactMemRow *tab, const ExactMemClass *cls, const uint64_t *addr) {
    uint64_t j = 0, base = 0;
    for (uint32_t g = 0; g < n_rows; g++) {
        rows[g].first = j;
        rows[g].base = (uint32_t)base;
        j += row_classes[g] * rows[g].npos;
        base += row_classes[g];
    }
    p.mem_trials = j;
    p.trials += j;
    p.mem_rows = tab; p.mem_cls = cls; p.mem_addr = addr;
    p.n_mem_rows = n_rows;
}

// What the class kernels read (fi_kernels.hip fi_exact_mem_*_kernel)
struct ExactMemCtx {
    const uint64_t *mw_addr, *mw_ev;   // the memory liveness index (DevCtx::mw_*)
    const uint32_t *mw_off;
    const uint64_t *pages;             // the candidate pages, sorted
    uint64_t n_pages, text_lo, text_hi, ninst;
    uint32_t mw_n, pad;
    // a profiled build (else proxy = NULL): the consumer tables, rows as values, and the events'
    // proxy bits (a bit per mw_ev entry: a syscall's access)
    ExactConsumers cons;
    const uint32_t *proxy;
};

// What a campaign counts without a trial (fi_exact_untried_kernel), numInst or tick domain: per
// register r the sites that end masked (dead; in a tick campaign golden-equal too) and escaped
// (tick campaigns: FI_ESC_TIMING), per position b the dead (word, t) pairs of b's byte set
// (numInst campaigns with memory).  A row of zeros adds nothing.
struct ExactUntried {
    uint64_t bits;                       // eligible positions
    uint64_t masked[32], escaped[32];    // per register (0: not selected)
    uint64_t mem_masked[64];             // per position
    uint64_t total, insts, esc_total;    // sites over the eligible positions; their guest_insts (mod 2^64); the escaped
};

struct ExactSite {
    uint64_t inst, mask, addr;
    uint32_t target, weight;
};

FI_TM_HD inline uint64_t exact_burst_mask(uint32_t burst) { return burst == 64 ? ~0ULL : ((1ULL << burst) - 1); }

// Memory trial j of the plan's memory range (j < p.mem_trials): the last row
// that starts at or before j (rows ascend; a row without classes starts where
// the next one does and is never that one), the row's own quotient -> the
// class's index in the class array, shared by the row's npos consecutive
// trials; *pos = the row's positions, *slot = the trial's among them.
FI_TM_HD inline uint32_t exact_mem_class(const ExactPlan &p, uint64_t j, uint64_t *pos, uint32_t *slot) {
    uint32_t lo = 0, hi = p.n_mem_rows;   // first row with first > j
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p.mem_rows[mid].first <= j) lo = mid + 1; else hi = mid;
    }
    const ExactMemRow r = p.mem_rows[lo - 1];
    const uint64_t jr = j - r.first;
    const uint64_t c = r.shift < 64 ? jr >> r.shift : mulhi64(jr, r.recip);
    *pos = r.pos;
    *slot = (uint32_t)(jr - c * r.npos);
    return r.base + (uint32_t)c;
}
FI_TM_HD inline ExactSite exact_mem_site(const ExactPlan &p, uint64_t j) {
    uint64_t mm;
    uint32_t slot;
    const ExactMemClass m = p.mem_cls[exact_mem_class(p, j, &mm, &slot)];
    for (uint32_t s = slot; s; s--) mm &= mm - 1;
    ExactSite x;
    x.inst = m.inst; x.target = FI_T_MEM; x.weight = m.weight;
    x.addr = p.mem_addr[m.word];
    x.mask = exact_burst_mask(p.burst) << (uint32_t)__builtin_ctzll(mm);
    return x;
}

// Trial k outside the memory range, k counted as without memory: *target = its
// structure (0: a register) -> the class word's index (registers) or the
// class's t (pc, result); *slot = its bit slot.
FI_TM_HD inline uint32_t exact_class(const ExactPlan &p, uint64_t k, uint32_t *target, uint32_t *slot) {
    const uint64_t q = exact_class_index(p, k);
    *slot = (uint32_t)(k - q * p.nbits);
    // the last row that starts at or before k (rows ascend; one compare per row, no indexed access)
    uint32_t delta = p.row[0].delta, tg = p.row[0].target;
    for (uint32_t r = 1; r < p.n_rows; r++) {
        const bool in = p.row[r].first <= k;
        delta = in ? p.row[r].delta : delta;
        tg = in ? p.row[r].target : tg;
    }
    *target = tg;
    return (uint32_t)q + delta;
}

// The mask of a class's bit slot
FI_TM_HD inline uint64_t exact_slot_mask(const ExactPlan &p, uint32_t slot) {
    uint64_t b = slot;   // positions 0 .. nbits - 1: the slot is the position
    if (p.bits & (p.bits + 1)) {
        uint64_t mm = p.bits;
        for (uint32_t j = slot; j; j--) mm &= mm - 1;
        b = (uint64_t)__builtin_ctzll(mm);
    }
    return exact_burst_mask(p.burst) << b;
}

// Exact trial k (k < p.trials); classes = every register's packed words
FI_TM_HD inline ExactSite exact_site(const ExactPlan &p, const uint64_t *classes, uint64_t k) {
    if (k - p.mem_first < p.mem_trials) return exact_mem_site(p, k - p.mem_first);   // (k < mem_first wraps: no)
    if (k >= p.mem_first) k -= p.mem_trials;   // the result's trials: counted as without memory
    uint32_t target, slot;
    const uint32_t x = exact_class(p, k, &target, &slot);
    ExactSite s;
    s.addr = 0;
    if (target) {
        s.inst = x; s.target = target; s.weight = 1;
    } else {
        const uint64_t w = classes[x];
        s.inst = exact_word_inst(w); s.target = exact_word_reg(w); s.weight = exact_word_weight(w);
    }
    s.mask = exact_slot_mask(p, slot);
    return s;
}

// The profile's bins (DESIGN.md §4j "Profile"): per row FI_N_PROFILE_GROUP
// groups x FI_N_CLASS classes; the groups: registers, the pc, memory words,
// an instruction's result.
constexpr uint32_t kProfBins = FI_N_PROFILE_GROUP * FI_N_CLASS;
// fi_exact_profile_kernel's LDS table: rows per workgroup, slots a row tries
constexpr uint32_t kProfSlots = 32, kProfProbes = 4;
// What that kernel reads besides the plan: a chunk's outcomes and weights, the bins
struct ExactProfCtx {
    const uint32_t *reg_cons, *inst_row;
    const fi_outcome *out;
    const uint32_t *weight;
    unsigned long long *prof;   // [n_rows][kProfBins]
    uint32_t n_rows, variant;
};
FI_TM_HD inline uint32_t exact_profile_group(uint32_t target) {
    return target == FI_T_PC ? 1u : target == FI_T_MEM ? 2u : target == FI_T_RESULT ? 3u : 0u;
}
// The row exact trial k is charged to and its group: reg_cons = a row per
// register class word, beside `classes`; memory's in its class records; the pc
// and a result at t: inst_row[t].
FI_TM_HD inline uint32_t exact_trial_consumer(const ExactPlan &p, const uint32_t *reg_cons, const uint32_t *inst_row,
                                              uint64_t k, uint32_t *group) {
    if (k - p.mem_first < p.mem_trials) {
        uint64_t pos;
        uint32_t slot;
        *group = 2;
        return p.mem_cls[exact_mem_class(p, k - p.mem_first, &pos, &slot)].cons;
    }
    if (k >= p.mem_first) k -= p.mem_trials;
    uint32_t target, slot;
    const uint32_t x = exact_class(p, k, &target, &slot);
    *group = exact_profile_group(target);
    return target ? inst_row[x] : reg_cons[x];
}

}  // namespace fi
