// The tick -> numInst site map over the packed attempt table (fi_types.h
// TickRec; fi_tick.cpp pack_tick_table), and the outcome of the trials it
// keeps off the device: one function each for the host (fi_engine.cpp
// fi_map_tick_sites) and the device (fi_kernels.hip fi_tick_map_kernel).  The
// independent statement is the oracle, which runs every tick trial literally
// (oracle/rv64se.c tk_*); tests/golden/tick_map.json pins the map on random
// tables (tools/tick_map_check.cpp).
//
// A flip at tick t happens before every event of tick t; the attempt in
// flight is the first whose last event is at or after t.  Before it executes
// (its fetch outstanding) a register flip is a numInst injection at its
// numInst; while its data access is outstanding the sources are read, so the
// flip takes effect from the next instruction on -- unless the completion
// writes that register (TimingSimpleCPU::completeDataAccess -> completeAcc).
// A pc flip while the fetch is outstanding leaves the instruction fetched from
// the old word: executed at the new pc (decode sets npc, decoder.cc:135-173),
// its effect is the golden instruction's with the next pc, a link or a branch
// target moved by the difference -- one numInst site after it; a pc flip
// during the data access goes through PCState::set, npc = pc + 4, which
// advancePC then takes.  The cases that are not one numInst site are
// FI_ESC_TIMING (FI_TK_*) -- or, under the literal contract
// (fi_set_tick_contract), sites with a tick descriptor in fi_site.addr
// (FI_SITE_TK_*) that the trial kernels run as the timing CPU does: the flip
// applied after the non-counting attempts before it, the next fetch reading
// the old pc's word (fi_trial.hip fetch_lane_tk).  FI_TK_MACRO stays an escape
// there, as does FI_TK_CLOCK at run time.
#pragma once
#include "fi_types.h"

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

// literal: fi_set_tick_contract FI_TICK_CONTRACT_LITERAL (the FI_TK_NONCOUNT ..
// FI_TK_FAULTOP cases become sites with a tick descriptor, fi_site.addr)
FI_TM_HD inline TickMap tick_map_site(const uint64_t *done, const TickRec *rec, uint64_t n_att, uint64_t golden_ninst,
                                      uint64_t t, uint32_t target, uint64_t mask, uint32_t trial,
                                      uint32_t literal = 0) {
    TickMap r{};
    const uint64_t j = tick_attempt_at(done, n_att, t);
    r.attempt = j;
    const TickRec A = rec[j];
    enum { FETCH1, FETCH2, DATA };
    const int ph = (A.nfetch == 2 && t <= A.fetch_done0) ? FETCH1
                   : t <= A.exec                          ? (A.nfetch == 2 ? FETCH2 : FETCH1)
                                                          : DATA;
    const uint64_t g = A.g <= j ? A.g : j;   // the attempts since the last commit (ecalls, page-fault retries)
    // the literal contract: the flip applied after the j - g attempts before it
    // (FI_SITE_TK_SKIP); a pc flip whose fetch went out with the old pc
    // (FI_SITE_TK_FETCH: the fetch override, then the decoder's own state)
    const bool lit = literal && j - g <= FI_SITE_TK_SKIP_MAX;
    const uint64_t skip = (j - g) << FI_SITE_TK_SKIP_SHIFT;
    auto site = [&](uint32_t tg, uint64_t m, uint64_t inst, uint64_t desc = 0) {
        r.site.inst = inst; r.site.mask = m; r.site.addr = desc; r.site.target = tg; r.site.trial = trial;
        r.disp = inst > golden_ninst ? 1u : 0u;   // after the run's last commit: the golden run
        return r;
    };
    auto golden = [&]() { r.disp = 1; return r; };
    auto escape = [&](uint32_t why) { r.disp = 2; r.reason = why; return r; };
    // not one numInst site: the numInst contract's escape; the literal
    // contract's pc site -- the old word at the new pc
    auto refetch = [&](uint32_t why) {
        if (!lit) return escape(why);
        return site(FI_T_PC, mask, A.n, skip | FI_SITE_TK_FETCH | (ph == FETCH2 ? FI_SITE_TK_FETCH2 : 0));
    };
    if (target == FI_T_RESULT) return site(FI_T_RESULT, mask, A.n);   // the first commit at or after t
    if (target >= 1 && target <= 31) {
        if (ph == DATA) return A.done_rd == target ? golden() : site(target, mask, A.n + 1);
        for (uint64_t q = g; q < j; q++) {   // the flip lands after these: it must commute with them
            const TickRec Q = rec[q];
            if (((Q.flags & kTrEcall) && target >= 10 && target <= 17) ||
                ((Q.flags & kTrPgfault) && (target == Q.rs1 || target == Q.rs2)))
                return lit ? site(target, mask, A.n, skip) : escape(FI_TK_NONCOUNT);
        }
        return site(target, mask, A.n);
    }
    // the pc
    if (g != j && !lit) return escape(FI_TK_NONCOUNT);
    const uint64_t pc = A.pc, np = pc ^ mask;
    const bool same_word = ((pc ^ np) & ~3ULL) == 0;
    // (after non-counting attempts the literal contract takes the oracle's order: its literal run is the reference)
    if (ph == DATA) {
        if ((A.flags & kTrMacro) && g == j) return escape(FI_TK_MACRO);
        return site(FI_T_PC, (pc + A.len) ^ (np + 4), A.n + 1);
    }
    if (ph == FETCH1 && same_word) return site(FI_T_PC, mask, A.n, skip);
    if (!(A.flags & kTrCommits) || (A.flags & kTrEnd)) return refetch(FI_TK_FAULTOP);
    if (ph == FETCH1) {
        if (A.nfetch == 2) return refetch(FI_TK_STRADDLE1);
        if ((pc & 3) != (np & 3)) return refetch(FI_TK_ALIGN);
    } else if ((np & 3) == 0) {
        return refetch(FI_TK_STRADDLE2);
    }
    if (g != j) return refetch(FI_TK_NONCOUNT);   // (literal only: run as it lands)
    // the golden instruction executed at np: its effect, moved by np - pc
    const uint64_t imm = (uint64_t)(int64_t)A.imm;
    switch (A.ctl) {
    case kCtlAuipc: return refetch(FI_TK_TWO);
    case kCtlJal:
        if (A.rd) return refetch(FI_TK_TWO);
        return site(FI_T_PC, (pc + imm) ^ (np + imm), A.n + 1);
    case kCtlJalr:
        if (!A.rd) return golden();   // the target comes from rs1
        return site(A.rd, (pc + A.len) ^ (np + A.len), A.n + 1);
    case kCtlBranch: {
        const uint64_t x = (A.flags & kTrTaken) ? imm : (uint64_t)A.len;
        return site(FI_T_PC, (pc + x) ^ (np + x), A.n + 1);
    }
    default: return site(FI_T_PC, (pc + A.len) ^ (np + A.len), A.n + 1);
    }
}

// The outcome of a trial the map keeps off the device -- disp 1, the golden
// run's own (gsub, gexit, gdetail, golden_ninst); disp 2, FI_ESC_TIMING at
// the attempt A = rec[m.attempt] -- and zero for disp 0.
FI_TM_HD inline fi_outcome tick_map_outcome(const TickMap &m, const TickRec &A, uint32_t gsub, uint32_t gexit,
                                            uint32_t gdetail, uint64_t golden_ninst) {
    fi_outcome o{};
    if (m.disp == 1) {
        o.cls = FI_MASKED; o.sub = (uint8_t)gsub; o.exit_code = (uint8_t)gexit;
        o.flags = 1; o.detail = gdetail; o.ninst = golden_ninst;
    } else if (m.disp == 2) {
        o.cls = FI_ESCAPE; o.sub = FI_ESC_TIMING; o.exit_code = (uint8_t)m.reason;
        o.flags = 1; o.detail = (uint32_t)A.pc; o.ninst = A.n;
    }
    return o;
}

}  // namespace fi
