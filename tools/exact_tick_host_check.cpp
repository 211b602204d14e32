// Host check of exact campaigns in the tick domain: stand-alone (no device,
// no engine); build with the host compiler, with sanitizers, e.g.
//   g++ -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude \
//       -Ishrewd_amd/csrc -Ishrewd_amd/csrc/hip tools/exact_tick_host_check.cpp shrewd_amd/csrc/fi_tick.cpp \
//       -o exact_tick_host_check
// (tests/test_exact_tick_cpu.py does).
//   exact_tick_host_check [SEED]
//       Random small attempt tables (tens of attempts, short periods; ecalls, page-fault retries, straddling
//       fetches, loads that write a register at completion) through fi_tick.cpp pack_tick_table, each with a
//       random first-access index, under both tick contracts.  Over EVERY tick of a table:
//        - registers x1..x31 and two masks: tick_map_site followed by the interval lookup, written out here
//          on its own (a linear walk of the index), lands in the class -- or the dead / golden / escape
//          count -- that exact_tick_locate names, that class's site is the one the map and the lookup give,
//          and the ticks that land in a class number its weight;
//        - the pc: the tick's map equals the map of its class's representative, for two masks;
//        - an instruction's result: likewise;
//        - per structure the class weights + dead + golden + escaped ticks sum to T.
//       Prints "ok" and the totals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "fi_exact_tick.h"
#include "fi_tick.h"

using namespace fi;

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return n ? rng() % n : 0; };
    uint64_t ticks_checked = 0, n_cls[4] = {0, 0, 0, 0}, n_desc = 0, n_exit = 0, n_kind[4] = {0, 0, 0, 0};
    for (int table = 0; table < 60; table++) {
        const size_t n = 2 + rnd(60);
        std::vector<TickAttempt> att(n);
        std::vector<fi_timing_ticks> ticks(n);
        uint64_t t = 1 + rnd(20), ninst = 0, pc = 0x10000 + 2 * rnd(64);
        for (size_t i = 0; i < n; i++) {
            TickAttempt &a = att[i];
            a.pc = pc; a.n = ninst;
            a.len = rnd(3) ? 4 : 2;
            a.nfetch = ((pc & 3) == 2 && a.len == 4) ? 2 : 1;
            a.imm = (int64_t)rnd(4096) - 2048;
            a.ctl = (uint8_t)(rnd(3) ? kCtlNone : rnd(5));
            a.rd = (uint8_t)rnd(32); a.rs1 = (uint8_t)rnd(32); a.rs2 = (uint8_t)rnd(32);
            const bool last = i + 1 == n;
            const uint64_t kind = last ? 0 : rnd(8);   // 0 ecall (the last attempt: the exit ecall), 1 page-fault retry
            a.ecall = kind == 0; a.pgfault = kind == 1;
            a.commits = kind > 1;
            a.end = last;
            a.macro = a.commits && rnd(8) == 0;
            const bool data = a.commits && (a.macro || rnd(3) == 0);
            if (data && rnd(2)) a.done_rd = a.rd;
            fi_timing_ticks &k = ticks[i];
            k.fetch_send[0] = t;
            t += 1 + rnd(12); k.fetch_done[0] = t;
            if (a.nfetch == 2) { k.fetch_send[1] = t; t += 1 + rnd(12); k.fetch_done[1] = t; }
            k.exec = t;
            if (data) t += 1 + rnd(20);
            k.done = t;
            t += rnd(3);   // (the next attempt may start at the same tick)
            if (a.commits) ninst++;
            const bool taken = a.commits && rnd(3) == 0;
            const uint64_t next = a.commits ? (taken ? 0x10000 + 2 * rnd(4096) : pc + a.len) : pc;
            a.next_pc = last ? 0 : next;
            pc = next;
        }
        const uint64_t T = ticks[n - 1].exec;
        std::vector<uint64_t> done;
        std::vector<TickRec> rec;
        pack_tick_table(att, ticks, done, rec);
        // a first-access index: per register a few events at ascending numInst in [0, ninst]; an event at
        // numInst == ninst is the exit ecall's (key even)
        std::vector<uint32_t> off(33, 0), ev;
        for (uint32_t r = 1; r < 32; r++) {
            off[r] = (uint32_t)ev.size();
            for (uint64_t m = rnd(3) ? rnd(3) : 0; m <= ninst; m += 1 + rnd(5)) {
                const bool ecall = m == ninst || rnd(6) == 0;
                if (rnd(4) == 0 && m < ninst && !ecall) {   // an ecall and an instruction at one numInst
                    ev.push_back((uint32_t)((2 * m) << 1 | rnd(2)));
                }
                ev.push_back((uint32_t)((2 * m + (ecall ? 0 : 1)) << 1 | (rnd(3) ? 1 : 0)));
            }
        }
        off[32] = (uint32_t)ev.size();
        for (uint32_t literal = 0; literal < 2; literal++) {
            ExactTickTable x;
            exact_tick_table(done.data(), rec.data(), n, ninst, T, literal, off.data(), ev.data(), x);
            uint64_t seg_sum = 0;
            for (const TickSeg &s : x.segs) seg_sum += s.len;
            if (seg_sum != T) { printf("table %d: the segments hold %llu ticks of %llu\n", table, (unsigned long long)seg_sum, (unsigned long long)T); return 1; }
            const uint64_t masks[2] = {1ULL << rnd(64), 3ULL << rnd(63)};
            for (uint32_t tg = 1; tg < FI_N_STRUCT; tg++) {
                if (tg == FI_T_MEM) continue;
                const uint32_t ncls = x.off[tg + 1] - x.off[tg];
                std::vector<uint64_t> landed(ncls, 0);
                uint64_t none[4] = {0, 0, 0, 0};
                for (uint64_t tk = 0; tk < T; tk++) {
                    for (int mi = 0; mi < 2; mi++) {
                        const uint64_t mask = masks[mi];
                        const TickMap m = tick_map_site(done.data(), rec.data(), n, ninst, tk, tg, mask, 0, literal);
                        uint32_t c = ~0u;
                        const uint8_t kind = exact_tick_locate(x, done.data(), rec.data(), n, ninst, T, literal, off.data(),
                                                               ev.data(), tk, tg, mask, &c);
                        if (mi == 0) { n_kind[kind]++; ticks_checked++; }
                        // what the tick is, from the map and a linear walk of the index
                        uint8_t want = kXtTrial;
                        fi_site ws = m.site;
                        uint32_t wdisp = m.disp;
                        if (tg < 32) {
                            if (m.disp == 1) want = kXtGoldenTick;
                            else if (m.disp == 2) want = kXtEscapeTick;
                            else if (!m.site.addr) {
                                want = kXtDeadTick;
                                for (uint32_t i = off[tg]; i < off[tg + 1]; i++) {
                                    if ((uint64_t)(ev[i] >> 2) < m.site.inst) continue;
                                    if (ev[i] & 1u) { want = kXtTrial; ws.inst = ev[i] >> 2; }
                                    break;
                                }
                            }
                        }
                        if (kind != want) {
                            printf("table %d literal %u: tick %llu target %u: located as %u, is %u\n", table, literal,
                                   (unsigned long long)tk, tg, kind, want);
                            return 1;
                        }
                        if (kind != kXtTrial) { if (mi == 0) none[kind]++; continue; }
                        if (c >= ncls) { printf("table %d: class %u of %u\n", table, c, ncls); return 1; }
                        if (mi == 0) landed[c]++;
                        // the class's own site, as the device enumerates it
                        const ExactTickClass k = x.cls[x.off[tg] + c];
                        fi_site cs{};
                        uint32_t cdisp = 0;
                        if (k.inst != kExactTickMapped) {
                            cs.inst = k.inst; cs.mask = mask; cs.target = k.target;
                        } else {
                            const TickMap r = tick_map_site(done.data(), rec.data(), n, ninst, k.tick, k.target, mask, 0, literal);
                            cs = r.site; cdisp = r.disp;
                            if (cdisp == 2 && (r.reason != m.reason || rec[r.attempt].n != rec[m.attempt].n ||
                                               rec[r.attempt].pc != rec[m.attempt].pc)) {
                                printf("table %d: tick %llu target %u: another escape than its class's\n", table,
                                       (unsigned long long)tk, tg);
                                return 1;
                            }
                            if (tg < 32) n_desc++;
                        }
                        if (k.target != tg || cdisp != wdisp ||
                            (cdisp == 0 && (cs.inst != ws.inst || cs.mask != ws.mask || cs.addr != ws.addr || cs.target != ws.target))) {
                            printf("table %d literal %u: tick %llu target %u mask %llx: class %u runs another site\n", table,
                                   literal, (unsigned long long)tk, tg, (unsigned long long)mask, c);
                            return 1;
                        }
                        if (tg < 32 && k.inst == ninst) n_exit++;
                    }
                }
                uint64_t sum = none[kXtDeadTick] + none[kXtGoldenTick] + none[kXtEscapeTick];
                for (uint32_t c = 0; c < ncls; c++) {
                    if (landed[c] != x.cls[x.off[tg] + c].weight || !landed[c]) {
                        printf("table %d literal %u target %u: class %u has weight %llu, %llu ticks land in it\n", table,
                               literal, tg, c, (unsigned long long)x.cls[x.off[tg] + c].weight, (unsigned long long)landed[c]);
                        return 1;
                    }
                    sum += landed[c];
                }
                if (sum != T) { printf("table %d target %u: %llu of %llu ticks\n", table, tg, (unsigned long long)sum, (unsigned long long)T); return 1; }
                if (tg < 32) {
                    const ExactTickTotals &tt = x.tot[tg];
                    if (tt.dead != none[kXtDeadTick] || tt.golden != none[kXtGoldenTick] || tt.escaped != none[kXtEscapeTick]) {
                        printf("table %d target %u: the totals differ from the ticks' count\n", table, tg);
                        return 1;
                    }
                    // ids: interval classes ascending in inst, then descriptor classes ascending in tick
                    for (uint32_t c = 1; c < ncls; c++) {
                        const ExactTickClass &a = x.cls[x.off[tg] + c - 1], &b = x.cls[x.off[tg] + c];
                        const bool ok = c < x.n_interval[tg] ? a.inst < b.inst
                                        : c == x.n_interval[tg] ? b.inst == kExactTickMapped
                                                                : (a.inst == kExactTickMapped && b.inst == kExactTickMapped && a.tick < b.tick);
                        if (!ok) { printf("table %d target %u: class order at %u\n", table, tg, c); return 1; }
                    }
                    n_cls[0] += x.n_interval[tg]; n_cls[1] += ncls - x.n_interval[tg];
                } else {
                    n_cls[tg == FI_T_PC ? 2 : 3] += ncls;
                }
            }
        }
    }
    if (!n_kind[0] || !n_kind[1] || !n_kind[2] || !n_kind[3]) { printf("a kind never occurred\n"); return 1; }
    if (!n_desc) { printf("a descriptor class never occurred\n"); return 1; }
    if (!n_exit) { printf("the exit-ecall interval never occurred\n"); return 1; }
    printf("ok %llu (tick, structure) pairs: trial %llu dead %llu golden %llu escape %llu; classes interval %llu "
           "descriptor %llu pc %llu result %llu\n", (unsigned long long)ticks_checked, (unsigned long long)n_kind[0],
           (unsigned long long)n_kind[1], (unsigned long long)n_kind[2], (unsigned long long)n_kind[3],
           (unsigned long long)n_cls[0], (unsigned long long)n_cls[1], (unsigned long long)n_cls[2],
           (unsigned long long)n_cls[3]);
    return 0;
}
