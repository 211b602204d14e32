// Exact campaigns in the tick domain (DESIGN.md §4j "Tick domain"): every tick
// of a TimingSimpleCPU golden run covered, one trial per class.  One statement
// for the host (fi_engine.cpp exact_tick_build, fi_exact_tick_classes,
// fi_exact_tick_locate; tools/exact_tick_host_check.cpp) and the device
// (fi_kernels.hip fi_exact_tick_sites_kernel).  The map itself is
// fi_tick_map.h tick_map_site and is only ever called here, never restated.
// The ticks without a trial go into fi_exact.h's ExactUntried, the bit slots'
// masks come from its exact_slot_mask: one of each for both domains.
//
// Segments.  T = golden_ticks.  Attempt j owns the ticks [done[j - 1] + 1,
// min(done[j], T - 1)] (from 0 for j = 0; the last attempt up to T - 1:
// tick_attempt_at's rule).  Inside it tick_map_site tells up to three phases
// apart: [.., fetch_done0] when nfetch == 2, (.., exec], (exec, done].  The
// non-empty ones are the attempt's segments; the map is a function of
// (segment, target, mask), so any tick of a segment stands for all of them --
// its first, here.
//
// Space.  Every (t, structure, b): t < T, structure one of x1..x31, FI_T_PC,
// FI_T_RESULT as selected, b an eligible position (fi_exact.h).
//
// Register r.  For a register the map does not depend on the bit.  A segment
// is exactly one of
//  - a plain numInst site at inst n (descriptor 0, disp 0).  The entry of r's
//    first-access index that heads n's interval is the first with ev >> 2 >= n
//    (unclipped: the exit ecall's reads stand at n == ninst, a legal tick
//    site; fi_forward_kernel's rule).  It reads: the segment's ticks join that
//    entry's class, which runs at inst = ev >> 2 with their sum as its weight.
//    It writes, or there is none: the ticks are dead (masked, golden numInst,
//    no trial).
//  - disp 1 (golden-equal: done_rd == r while the load's data is outstanding,
//    a site past the run's last commit): dead likewise, counted apart.
//  - disp 2 (FI_ESC_TIMING): counted without a trial under FI_ESCAPE, with
//    guest_insts += ticks x A.n (tick_map_outcome).
//  - a site with a tick descriptor (literal contract): a class of its own,
//    weight = the segment's length; it is not forwarded.
// The pc: one class per segment, whatever the map says for it (disp 1 / 2
// trials keep their id and are parked and fixed as sampled tick trials are).
// An instruction's result: one class per distinct A.n, weight = the ticks of
// the attempts with that n.
//
// Ids.  Structures ascending; within a register its interval classes in time
// order, then its descriptor classes in segment order; within a class the
// eligible positions ascending.  k = class index x nbits + bit slot over the
// selected structures (fi_exact.h ExactPlan, exact_class).
#pragma once
#include <algorithm>
#include <vector>

#include "fi_exact.h"
#include "fi_tick_map.h"

namespace fi {

struct TickSeg { uint64_t first, len; };

// Attempt j's segments in tick order: out[0 .. returned count)
FI_TM_HD inline uint32_t tick_segments(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t T,
                                       uint64_t j, TickSeg out[3]) {
    if (!T || j >= n_att) return 0;
    uint64_t a = j ? done[j - 1] + 1 : 0;
    const uint64_t hi = (j + 1 == n_att || done[j] > T - 1) ? T - 1 : done[j];
    const TickRec A = rec[j];
    uint32_t n = 0;
    // the phases' last ticks, as tick_map_site tests them
    const uint64_t end[3] = {A.nfetch == 2 ? A.fetch_done0 : 0, A.exec, hi};
    for (uint32_t p = (A.nfetch == 2 ? 0u : 1u); p < 3 && a <= hi; p++) {
        const uint64_t e = end[p] < hi ? end[p] : hi;
        if (e < a) continue;
        out[n].first = a; out[n].len = e - a + 1;
        n++;
        a = e + 1;
        if (!a) break;   // (e == 2^64 - 1)
    }
    return n;
}

// A class: weight ticks x one position each.  inst != kExactTickMapped: an
// interval class, the plain site (inst, target, mask); else the site is
// tick_map_site(tick, target, mask).  tick: its representative tick site.
constexpr uint32_t kExactTickMapped = 0xFFFFFFFFu;
struct ExactTickClass {
    uint64_t weight, tick;
    uint32_t inst, target;
};

// What a register's ticks without a trial add up to
struct ExactTickTotals {
    uint64_t dead, golden, escaped;   // ticks
    uint64_t esc_insts;               // the escaped ticks' sum of A.n (mod 2^64)
};

// The entry that heads numInst n's interval of a register's entries ev[lo, hi): hi if none
FI_TM_HD inline uint32_t exact_tick_head(const uint32_t *ev, uint32_t lo, uint32_t hi, uint64_t n) {
    const uint64_t key = 4 * n;   // (2n) << 1: before both events of numInst n
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ev[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// What a register segment is (the cases above): *n = the plain site's inst
enum : uint32_t { kXtPlain = 0, kXtGolden = 1, kXtEscape = 2, kXtDesc = 3 };
FI_TM_HD inline uint32_t exact_tick_reg_case(const TickMap &m, uint64_t *n) {
    if (m.disp) return m.disp;
    *n = m.site.inst;
    return m.site.addr ? kXtDesc : kXtPlain;
}

// Register reg's classes over the segments segs[0 .. n_seg): interval classes
// in time order, then descriptor classes in segment order, appended to cls
// (cls_seg, may be NULL: the segment of each one's representative);
// *n_interval = the interval classes.
inline void exact_tick_reg_classes(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t ninst,
                                   uint32_t literal, const TickSeg *segs, uint64_t n_seg, const uint32_t *off,
                                   const uint32_t *ev, uint32_t reg, std::vector<ExactTickClass> &cls,
                                   std::vector<uint32_t> *cls_seg, uint32_t *n_interval, ExactTickTotals *tot) {
    const uint32_t lo = off[reg], hi = off[reg + 1];
    std::vector<uint64_t> w(hi - lo, 0), rep(hi - lo, 0);
    std::vector<uint32_t> rseg(hi - lo, 0), desc;
    ExactTickTotals t{};
    for (uint64_t s = 0; s < n_seg; s++) {
        const TickMap m = tick_map_site(done, rec, n_att, ninst, segs[s].first, reg, 1, 0, literal);
        uint64_t n = 0;
        switch (exact_tick_reg_case(m, &n)) {
        case kXtGolden: t.golden += segs[s].len; break;
        case kXtEscape: t.escaped += segs[s].len; t.esc_insts += segs[s].len * rec[m.attempt].n; break;
        case kXtDesc: desc.push_back((uint32_t)s); break;
        default: {
            const uint32_t i = exact_tick_head(ev, lo, hi, n);
            if (i < hi && (ev[i] & 1u)) {
                if (!w[i - lo]) { rep[i - lo] = segs[s].first; rseg[i - lo] = (uint32_t)s; }
                w[i - lo] += segs[s].len;
            } else {
                t.dead += segs[s].len;
            }
        }
        }
    }
    uint32_t ni = 0;
    for (uint32_t i = 0; i < hi - lo; i++) {
        if (!w[i]) continue;
        cls.push_back(ExactTickClass{w[i], rep[i], ev[lo + i] >> 2, reg});
        if (cls_seg) cls_seg->push_back(rseg[i]);
        ni++;
    }
    for (uint32_t s : desc) {
        cls.push_back(ExactTickClass{segs[s].len, segs[s].first, kExactTickMapped, reg});
        if (cls_seg) cls_seg->push_back(s);
    }
    if (n_interval) *n_interval = ni;
    if (tot) *tot = t;
}

// Everything a golden run's attempt table and first-access index give, under
// one tick contract: the segments, every structure's classes (structure t's
// at off[t] .. off[t + 1]; memory has none) and the registers' totals.
struct ExactTickTable {
    std::vector<TickSeg> segs;
    std::vector<uint32_t> seg_off;        // [n_att + 1]: attempt j's segments
    std::vector<ExactTickClass> cls;
    std::vector<uint32_t> cls_seg;        // beside cls: the representative's segment
    std::vector<uint32_t> res_cls;        // [n_att]: the attempt's result class, counted from off[FI_T_RESULT]
    uint32_t off[FI_N_STRUCT + 1] = {};
    uint32_t n_interval[32] = {};
    ExactTickTotals tot[32] = {};
};

inline void exact_tick_segments(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t T,
                                std::vector<TickSeg> &segs, std::vector<uint32_t> &seg_off) {
    segs.clear();
    seg_off.assign(n_att + 1, 0);
    for (uint64_t j = 0; j < n_att; j++) {
        TickSeg s[3];
        const uint32_t k = tick_segments(done, rec, n_att, T, j, s);
        segs.insert(segs.end(), s, s + k);
        seg_off[j + 1] = (uint32_t)segs.size();
    }
}

inline void exact_tick_table(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t ninst, uint64_t T,
                             uint32_t literal, const uint32_t *fw_off, const uint32_t *fw_ev, ExactTickTable &x) {
    x = ExactTickTable{};
    exact_tick_segments(done, rec, n_att, T, x.segs, x.seg_off);
    for (uint32_t t = 1; t < FI_N_STRUCT; t++) {
        x.off[t] = (uint32_t)x.cls.size();
        if (t < 32) {
            exact_tick_reg_classes(done, rec, n_att, ninst, literal, x.segs.data(), x.segs.size(), fw_off, fw_ev, t, x.cls,
                                   &x.cls_seg, &x.n_interval[t], &x.tot[t]);
        } else if (t == FI_T_PC) {
            for (size_t s = 0; s < x.segs.size(); s++) {
                x.cls.push_back(ExactTickClass{x.segs[s].len, x.segs[s].first, kExactTickMapped, FI_T_PC});
                x.cls_seg.push_back((uint32_t)s);
            }
        } else if (t == FI_T_RESULT) {
            x.res_cls.assign(n_att, 0);
            bool open = false;   // a class for the current n exists
            for (uint64_t j = 0; j < n_att; j++) {
                if (j && rec[j].n != rec[j - 1].n) open = false;
                for (uint32_t s = x.seg_off[j]; s < x.seg_off[j + 1]; s++) {
                    if (!open) {
                        x.cls.push_back(ExactTickClass{0, x.segs[s].first, kExactTickMapped, FI_T_RESULT});
                        x.cls_seg.push_back(s);
                        open = true;
                    }
                    x.cls.back().weight += x.segs[s].len;
                }
                x.res_cls[j] = (uint32_t)x.cls.size() - x.off[t] - (open ? 1u : 0u);
            }
        }
    }
    x.off[0] = 0;
    x.off[FI_N_STRUCT] = (uint32_t)x.cls.size();
}

// The plan of a tick campaign: fi_exact.h's rows over x.off (every row's
// class index is the class record's; the record names the structure).
inline ExactPlan exact_tick_plan(uint64_t structures, const uint32_t *off, uint64_t bits_mask, uint32_t burst,
                                 uint64_t *classes) {
    ExactPlan p{};
    p.burst = burst;
    p.bits = bits_mask & burst_positions(burst);
    p.nbits = (uint32_t)__builtin_popcountll(p.bits);
    p.shift = 64;
    if (p.nbits && !(p.nbits & (p.nbits - 1))) p.shift = (uint32_t)__builtin_ctz(p.nbits);
    else if (p.nbits) p.recip = ~0ULL / p.nbits + 1;
    uint64_t q = 0;
    for (uint32_t t = 1; t < FI_N_STRUCT; t++) {
        if (classes) classes[t] = 0;
        if (!((structures >> t) & 1) || t == FI_T_MEM) continue;
        ExactRow &r = p.row[p.n_rows++];
        r.first = q * p.nbits;
        r.target = 0;
        r.delta = off[t] - (uint32_t)q;
        if (classes) classes[t] = off[t + 1] - off[t];
        q += off[t + 1] - off[t];
    }
    p.trials = q * p.nbits;
    return p;
}

// Exact tick trial k (k < p.trials): the site the trial kernels run, its tick
// site, the map's disposition and a disp 1 / 2 trial's outcome, the ticks it
// stands for.  c: the packed table and the golden outcome (TickMapCtx).
struct ExactTickSite {
    fi_site site;
    fi_tick_site tsite;
    fi_outcome res;
    uint64_t weight;
    uint32_t disp;
};
FI_TM_HD inline ExactTickSite exact_tick_site(const ExactPlan &p, const ExactTickClass *cls, const TickMapCtx &c,
                                              uint64_t k) {
    uint32_t target, slot;
    const ExactTickClass x = cls[exact_class(p, k, &target, &slot)];
    ExactTickSite s{};
    s.weight = x.weight;
    s.tsite.tick = x.tick; s.tsite.mask = exact_slot_mask(p, slot); s.tsite.target = x.target;
    s.tsite.trial = (uint32_t)k;
    if (x.inst != kExactTickMapped) {
        s.site.inst = x.inst; s.site.mask = s.tsite.mask; s.site.addr = 0; s.site.target = x.target;
        s.site.trial = (uint32_t)k;
        return s;
    }
    const TickMap m = tick_map_site(c.done, c.rec, c.n_att, c.golden_ninst, x.tick, x.target, s.tsite.mask,
                                    (uint32_t)k, c.literal);
    s.site = m.site;
    s.disp = m.disp;
    s.res = tick_map_outcome(m, c.rec[m.attempt], c.gsub, c.gexit, c.gdetail, c.golden_ninst);
    return s;
}

// Where a tick site of the space belongs (fi_exact_tick_locate): the class it
// falls into, counted within its structure (*cls_index, from x.off[target]),
// or why it has no trial.  mask: the site's, target: 1..31, FI_T_PC, FI_T_RESULT.
enum : uint8_t { kXtTrial = 0, kXtDeadTick = 1, kXtGoldenTick = 2, kXtEscapeTick = 3 };
inline uint8_t exact_tick_locate(const ExactTickTable &x, const uint64_t *done, const TickRec *rec, uint64_t n_att,
                                 uint64_t ninst, uint64_t T, uint32_t literal, const uint32_t *fw_off,
                                 const uint32_t *fw_ev, uint64_t tick, uint32_t target, uint64_t mask,
                                 uint32_t *cls_index) {
    const uint64_t j = tick_attempt_at(done, n_att, tick);
    if (target == FI_T_RESULT) { *cls_index = x.res_cls[j]; return kXtTrial; }
    TickSeg sg[3];
    const uint32_t ns = tick_segments(done, rec, n_att, T, j, sg);
    uint32_t s = x.seg_off[j];
    for (uint32_t q = 0; q + 1 < ns && tick >= sg[q + 1].first; q++) s++;
    if (target == FI_T_PC) { *cls_index = s; return kXtTrial; }
    const TickMap m = tick_map_site(done, rec, n_att, ninst, tick, target, mask, 0, literal);
    uint64_t n = 0;
    const uint32_t *seg = x.cls_seg.data();
    const uint32_t base = x.off[target], mid = base + x.n_interval[target], end = x.off[target + 1];
    switch (exact_tick_reg_case(m, &n)) {
    case kXtGolden: return kXtGoldenTick;
    case kXtEscape: return kXtEscapeTick;
    case kXtDesc:
        *cls_index = (uint32_t)(std::lower_bound(seg + mid, seg + end, s) - (seg + base));
        return kXtTrial;
    default: {
        const uint32_t i = exact_tick_head(fw_ev, fw_off[target], fw_off[target + 1], n);
        if (i >= fw_off[target + 1] || !(fw_ev[i] & 1u)) return kXtDeadTick;
        const uint32_t u = fw_ev[i] >> 2;
        const ExactTickClass *c = std::lower_bound(x.cls.data() + base, x.cls.data() + mid, u,
                                                   [](const ExactTickClass &a, uint32_t v) { return a.inst < v; });
        *cls_index = (uint32_t)(c - (x.cls.data() + base));
        return kXtTrial;
    }
    }
}

}  // namespace fi
