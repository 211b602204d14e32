// The tick -> numInst site map over the packed attempt table (fi_types.h
// TickRec; fi_tick.cpp pack_tick_table), as one function for the host and
// the device (fi_kernels.hip fi_tick_map_kernel).  It restates
// fi_tick.cpp map_tick_site case for case -- that function stays the
// statement the cases are argued in (and what this one is tested against).
#pragma once
#include "fi_types.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FI_TM_HD __host__ __device__
#else
#define FI_TM_HD
#endif

namespace fi {

// disposition 0 run `site`, 1 golden-equal, 2 escape (reason = FI_TK_*)
struct TickMap {
    uint32_t disp, reason;
    uint64_t attempt;
    fi_site site;
};

// The attempt in flight at tick t: the first whose last event is at or after
// t (t < golden_ticks: there is one; clamped all the same).
FI_TM_HD inline uint64_t tick_attempt_at(const uint64_t *done, uint64_t n_att, uint64_t t) {
    uint64_t lo = 0, hi = n_att;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (done[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo < n_att ? lo : n_att - 1;
}

FI_TM_HD inline TickMap tick_map_done(TickMap r, uint32_t disp, uint32_t reason) {
    r.disp = disp; r.reason = reason;
    return r;
}
FI_TM_HD inline TickMap tick_map_to(TickMap r, uint64_t golden_ninst, uint32_t tg, uint64_t m, uint64_t inst,
                                    uint32_t trial, uint64_t desc = 0) {
    r.site.inst = inst; r.site.mask = m; r.site.addr = desc; r.site.target = tg; r.site.trial = trial;
    r.disp = inst > golden_ninst ? 1u : 0u;   // after the run's last commit: the golden run
    return r;
}

// literal: fi_set_tick_contract FI_TICK_CONTRACT_LITERAL (the FI_TK_NONCOUNT ..
// FI_TK_FAULTOP cases become sites with a tick descriptor, fi_site.addr)
FI_TM_HD inline TickMap tick_map_site(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t golden_ninst,
                                      uint64_t t, uint32_t target, uint64_t mask, uint32_t trial,
                                      uint32_t literal = 0) {
    TickMap r;
    r.disp = 0; r.reason = 0;
    r.site.inst = 0; r.site.mask = 0; r.site.addr = 0; r.site.target = 0; r.site.trial = 0;
    const uint64_t j = tick_attempt_at(done, n_att, t);
    r.attempt = j;
    const TickRec A = rec[j];
    enum { FETCH1, FETCH2, DATA };
    const int ph = (A.nfetch == 2 && t <= A.fetch_done0) ? FETCH1
                   : t <= A.exec                          ? (A.nfetch == 2 ? FETCH2 : FETCH1)
                                                          : DATA;
    const uint64_t g = A.g <= j ? A.g : j;   // the attempts since the last commit (ecalls, page-fault retries)
    const bool lit = literal && j - g <= FI_SITE_TK_SKIP_MAX;
    const uint64_t skip = (j - g) << FI_SITE_TK_SKIP_SHIFT;
    // the literal contract's pc site: the old word at the new pc, after the j - g attempts before it
    const uint64_t refetch = skip | FI_SITE_TK_FETCH | (ph == FETCH2 ? FI_SITE_TK_FETCH2 : 0);
    // a result fault: the first commit at or after t
    if (target == FI_T_RESULT) return tick_map_to(r, golden_ninst, FI_T_RESULT, mask, A.n, trial);
    if (target >= 1 && target <= 31) {
        if (ph == DATA) {
            if (A.done_rd == target) return tick_map_done(r, 1, 0);
            return tick_map_to(r, golden_ninst, target, mask, A.n + 1, trial);
        }
        for (uint64_t q = g; q < j; q++) {   // the flip lands after these: it must commute with them
            const TickRec Q = rec[q];
            if (((Q.flags & kTrEcall) && target >= 10 && target <= 17) ||
                ((Q.flags & kTrPgfault) && (target == Q.rs1 || target == Q.rs2))) {
                if (lit) return tick_map_to(r, golden_ninst, target, mask, A.n, trial, skip);
                return tick_map_done(r, 2, FI_TK_NONCOUNT);
            }
        }
        return tick_map_to(r, golden_ninst, target, mask, A.n, trial);
    }
    // the pc
    if (g != j && !lit) return tick_map_done(r, 2, FI_TK_NONCOUNT);
    const uint64_t pc = A.pc, np = pc ^ mask;
    const bool same_word = ((pc ^ np) & ~3ULL) == 0;
    const bool commits = (A.flags & kTrCommits) != 0, end = (A.flags & kTrEnd) != 0;
    uint64_t m = 0, inst = A.n + 1;
    uint32_t tg = FI_T_PC;
    uint32_t why = 0;   // the numInst contract's escape; the literal contract's refetch site
    if (ph == DATA) {
        if ((A.flags & kTrMacro) && g == j) return tick_map_done(r, 2, FI_TK_MACRO);
        m = (pc + A.len) ^ (np + 4);
    } else if (ph == FETCH1 && same_word) {
        return tick_map_to(r, golden_ninst, FI_T_PC, mask, A.n, trial, skip);
    } else if (!commits || end) {
        why = FI_TK_FAULTOP;
    } else {
        if (ph == FETCH1) {
            if (A.nfetch == 2) why = FI_TK_STRADDLE1;
            else if ((pc & 3) != (np & 3)) why = FI_TK_ALIGN;
        } else if ((np & 3) == 0) {
            why = FI_TK_STRADDLE2;
        }
        if (!why && g != j) why = FI_TK_NONCOUNT;   // (literal only: run as it lands)
        // the golden instruction executed at np: its effect, moved by np - pc
        const uint64_t imm = (uint64_t)(int64_t)A.imm;
        if (!why) switch (A.ctl) {
        case kCtlAuipc: why = FI_TK_TWO; break;
        case kCtlJal:
            if (A.rd) why = FI_TK_TWO;
            m = (pc + imm) ^ (np + imm);
            break;
        case kCtlJalr:
            if (!A.rd) return tick_map_done(r, 1, 0);   // the target comes from rs1
            tg = A.rd;
            m = (pc + A.len) ^ (np + A.len);
            break;
        case kCtlBranch: {
            const uint64_t x = (A.flags & kTrTaken) ? imm : (uint64_t)A.len;
            m = (pc + x) ^ (np + x);
            break;
        }
        default: m = (pc + A.len) ^ (np + A.len); break;
        }
    }
    if (why) {
        if (lit) return tick_map_to(r, golden_ninst, FI_T_PC, mask, A.n, trial, refetch);
        return tick_map_done(r, 2, why);
    }
    return tick_map_to(r, golden_ninst, tg, m, inst, trial);
}

}  // namespace fi
