// fi_golden_host.h -- the host passes of fi_golden_run between the capture
// launch and the uploads: snapshot page dedupe, register liveness at each
// snapshot and the first-access index.  They decide which registers count as
// dead at a snapshot and where a register fault is forwarded to.  Plain C++
// over vectors with no HIP in it, so that a stand-alone host program can run
// them under the sanitizers (tools/golden_host_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "fi_types.h"

namespace fi {

// Deduplicate the captured pages and build one sorted page table per
// snapshot.  Snapshot k captured rs[k].tab_n pages: page i has vpn
// rv[k * P + i] and bytes rp[(k * P + i) << 12 ...].  A page equal to the
// latest version of its vpn shares that frame; any other is appended to
// `pool` as a new frame.  start_tab[0 .. n_start) is the process-start table
// (frames already in pool).  Out: snaps (rs with tab_off / tab_n set to the
// snapshot's run of `tab`), tab (the tables, each ascending in vpn).
// Returns pre_ok: false when a new frame differs from the original page
// (org_pages) inside [code_lo, code_hi) -- the golden run rewrote its text.
inline bool dedupe_snapshot_pages(const PageEnt *start_tab, uint32_t n_start, std::vector<uint8_t> &pool,
                                  const std::map<uint64_t, std::vector<uint8_t>> &org_pages, uint64_t code_lo,
                                  uint64_t code_hi, const std::vector<SnapState> &rs, const std::vector<uint8_t> &rp,
                                  const std::vector<uint64_t> &rv, uint32_t P, std::vector<SnapState> &snaps,
                                  std::vector<PageEnt> &tab) {
    bool pre_ok = true;
    std::map<uint64_t, uint32_t> cur;   // vpn -> frame of its latest version
    for (uint32_t i = 0; i < n_start; i++) cur[start_tab[i].vpn] = start_tab[i].frame;
    snaps.clear();
    tab.clear();
    for (uint32_t k = 0; k < rs.size(); k++) {
        SnapState S = rs[k];
        for (uint32_t i = 0; i < S.tab_n; i++) {
            const uint64_t vpn = rv[(uint64_t)k * P + i];
            const uint8_t *pg = rp.data() + (((uint64_t)k * P + i) << 12);
            auto it = cur.find(vpn);
            if (it != cur.end() && !memcmp(pool.data() + ((uint64_t)it->second << 12), pg, kPage)) continue;
            const uint32_t f = (uint32_t)(pool.size() / kPage);
            pool.insert(pool.end(), pg, pg + kPage);
            cur[vpn] = f;
            // the pre-decoded text stays valid only if the golden run never rewrites it
            const uint64_t va = vpn << 12;
            if (va < code_hi && va + kPage > code_lo) {   // bytes of the code range in this page
                const uint64_t a = std::max(va, code_lo), b = std::min(va + kPage, code_hi);
                auto org = org_pages.find(vpn);
                if (org == org_pages.end() || memcmp(org->second.data() + (a - va), pg + (a - va), b - a))
                    pre_ok = false;
            }
        }
        S.tab_off = (uint32_t)tab.size();
        S.tab_n = (uint32_t)cur.size();
        for (auto &kv : cur) {
            PageEnt pe{};
            pe.vpn = kv.first;
            pe.frame = kv.second;
            tab.push_back(pe);
        }
        snaps.push_back(S);
    }
    return pre_ok;
}

// Register liveness at each snapshot: backward over the golden trace,
// live = (live - writes) | reads; an ecall (trace bit 31) and an M5Op (op ==
// m5op) read a0..a7 and write nothing.  Out: rmask / wmask, the registers
// each trace event reads / writes, and snaps[k].live.  Returns live_ok: false
// when the trace is unusable (it overflowed: empty with n_events != 0; or an
// entry lies outside the pre-decoded text or at an invalid entry) -- then
// every register but x0 counts as live at every snapshot.
inline bool trace_liveness(const std::vector<PreInst> &pre, const std::vector<uint32_t> &trace, uint64_t n_events,
                           uint8_t m5op, std::vector<uint32_t> &rmask, std::vector<uint32_t> &wmask,
                           std::vector<SnapState> &snaps) {
    bool live_ok = !trace.empty() || n_events == 0;
    rmask.assign(trace.size(), 0);
    wmask.assign(trace.size(), 0);
    for (size_t i = 0; live_ok && i < trace.size(); i++) {
        const uint32_t h = trace[i] & 0x7FFFFFFFu;
        if (h >= pre.size() || !(pre[h].flags & kPreValid)) { live_ok = false; break; }
        const PreInst &p = pre[h];
        uint32_t r = 0, w = 0;
        if ((p.flags & kPreRs1) && p.rs1) r |= 1u << p.rs1;
        if ((p.flags & kPreRs2) && p.rs2) r |= 1u << p.rs2;
        if ((trace[i] & 0x80000000u) || p.op == m5op) r |= 0x3FC00u;   // x10..x17 (an M5Op's ABI arguments)
        else if ((p.flags & kPreRd) && p.rd) w |= 1u << p.rd;
        rmask[i] = r;
        wmask[i] = w;
    }
    uint32_t live = 0;
    int64_t ev = (int64_t)trace.size() - 1;
    for (int64_t k = (int64_t)snaps.size() - 1; k >= 0; k--) {
        if (!live_ok) { snaps[k].live = 0xFFFFFFFEu; continue; }
        for (; ev >= (int64_t)snaps[k].trace_pos; ev--) live = (live & ~wmask[ev]) | rmask[ev];
        snaps[k].live = live & ~1u;
    }
    return live_ok;
}

// First-access index (DESIGN.md §4 "first-access forwarding"): per register
// x1..x31 its accesses in trace order.  off[r] .. off[r + 1] are register r's
// entries of ev (off[0] = off[1] = 0: x0 has none); an entry is
// (2 * numInst + !ecall) << 1 | reads, numInst counting the committed
// instructions before the event (an ecall's trace entry commits nothing).
inline void first_access_index(const std::vector<uint32_t> &trace, const std::vector<uint32_t> &rmask,
                               const std::vector<uint32_t> &wmask, std::vector<uint32_t> &off,
                               std::vector<uint32_t> &ev) {
    off.assign(33, 0);
    for (size_t i = 0; i < trace.size(); i++)
        for (uint32_t m = (rmask[i] | wmask[i]) & ~1u; m; m &= m - 1) off[__builtin_ctz(m) + 1]++;
    for (int r = 0; r < 32; r++) off[r + 1] += off[r];
    ev.assign(off[32], 0);
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    uint64_t t = 0;
    for (size_t i = 0; i < trace.size(); i++) {
        const bool ecall = (trace[i] & 0x80000000u) != 0;
        const uint32_t key = (uint32_t)(2 * t + (ecall ? 0 : 1));
        for (uint32_t m = (rmask[i] | wmask[i]) & ~1u; m; m &= m - 1) {
            const int r = __builtin_ctz(m);
            ev[at[r]++] = (key << 1) | ((rmask[i] >> r) & 1u);
        }
        if (!ecall) t++;
    }
}

}  // namespace fi
