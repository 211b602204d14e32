// Host check of the tick site map and the site draw: stand-alone (no device,
// no engine); build with the host compiler, with sanitizers if wanted, e.g.
//   g++ -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude \
//       -Ishrewd_amd/csrc -Ishrewd_amd/csrc/hip tools/tick_map_check.cpp shrewd_amd/csrc/fi_tick.cpp -o tick_map_check
// (tests/test_tick_device_cpu.py does).
//   tick_map_check SEED [literal]
//       40 random attempt tables (std::mt19937_64: the stream is fixed by the standard) through
//       fi_tick.cpp pack_tick_table, 4000 tick sites on each through fi_tick_map.h tick_map_site, under the
//       numInst or the literal contract (fi_set_tick_contract).  Per table one line with a 64-bit FNV-1a
//       hash of the packed table, every site and its result, and the dispositions' counts; then "ok" and the
//       totals.  tests/golden/tick_map.json holds these lines as recorded from the map's first statement
//       (fi_tick.cpp's, over the unpacked attempts, since deleted), for seeds 1 and 7.  Asserted here: the
//       pack's sizes; each disposition occurred; no tick descriptor under the numInst contract; under the
//       literal one each kind of descriptor occurred, and the only escapes left are FI_TK_MACRO and sites
//       past FI_SITE_TK_SKIP_MAX attempts.
//   tick_map_check draw SEED FIRST N RANGE STRUCTURES BURST BITS
//       fi_site_draw.h: trials FIRST .. FIRST + N - 1 as lines "when target mask trial" (mask in hex), for
//       comparison with the oracle's sampler.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "fi_site_draw.h"
#include "fi_tick.h"
#include "fi_tick_map.h"

using namespace fi;

// FNV-1a, 64 bits, over the low `bytes` bytes of each value, least significant first
struct Fnv {
    uint64_t h = 0xcbf29ce484222325ULL;
    void add(uint64_t v, int bytes = 8) {
        for (int i = 0; i < bytes; i++) { h ^= (v >> (8 * i)) & 0xFF; h *= 0x100000001b3ULL; }
    }
};
static void hash_table(Fnv &f, const std::vector<uint64_t> &done, const std::vector<TickRec> &rec) {
    f.add(done.size());
    for (uint64_t d : done) f.add(d);
    for (const TickRec &r : rec) {   // field by field: not the padding
        f.add(r.pc); f.add(r.n); f.add(r.fetch_done0); f.add(r.exec);
        f.add((uint32_t)r.imm, 4); f.add(r.g, 4);
        f.add(r.len, 1); f.add(r.nfetch, 1); f.add(r.ctl, 1);
        f.add(r.rd, 1); f.add(r.rs1, 1); f.add(r.rs2, 1); f.add(r.done_rd, 1); f.add(r.flags, 1);
    }
}
static void hash_site(Fnv &f, uint64_t tick, uint32_t target, uint64_t mask, uint32_t trial, const TickMap &m) {
    f.add(tick); f.add(target, 4); f.add(mask); f.add(trial, 4);
    f.add(m.disp, 4); f.add(m.reason, 4); f.add(m.attempt);
    f.add(m.site.inst); f.add(m.site.mask); f.add(m.site.addr); f.add(m.site.target, 4); f.add(m.site.trial, 4);
}

static int draw(char **a) {
    uint64_t v[7];
    for (int i = 0; i < 7; i++) v[i] = strtoull(a[i], nullptr, 0);
    const DrawCtx d = draw_ctx(v[0], v[4], v[1], v[6], (uint32_t)v[5]);
    for (uint64_t i = 0; i < v[2]; i++) {
        const SiteDraw s = draw_site(d, i, v[3]);
        printf("%llu %u %llx %u\n", (unsigned long long)s.when, s.target, (unsigned long long)s.mask, s.trial);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 9 && !strcmp(argv[1], "draw")) return draw(argv + 2);
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
    const bool literal = argc > 2 && !strcmp(argv[2], "literal");
    if (argc > 3 || (argc > 2 && !literal)) {
        printf("usage: tick_map_check [SEED [literal]] | draw SEED FIRST N RANGE STRUCTURES BURST BITS\n");
        return 2;
    }
    uint64_t by_desc[3] = {0, 0, 0};   // literal: sites with a skip count, a fetch override, a second-fetch one
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return n ? rng() % n : 0; };
    uint64_t checked = 0, by_disp[3] = {0, 0, 0};
    for (int table = 0; table < 40; table++) {
        const size_t n = 1 + rnd(400);
        std::vector<TickAttempt> att(n);
        std::vector<fi_timing_ticks> ticks(n);
        uint64_t t = 1 + rnd(1000), ninst = 0, pc = 0x10000 + 2 * rnd(64);
        for (size_t i = 0; i < n; i++) {
            TickAttempt &a = att[i];
            a.pc = pc; a.n = ninst;
            a.len = rnd(3) ? 4 : 2;
            a.nfetch = ((pc & 3) == 2 && a.len == 4) ? 2 : 1;
            a.imm = (int64_t)rnd(4096) - 2048;
            a.ctl = (uint8_t)(rnd(3) ? kCtlNone : rnd(5));
            a.rd = (uint8_t)rnd(32); a.rs1 = (uint8_t)rnd(32); a.rs2 = (uint8_t)rnd(32);
            const uint64_t kind = rnd(10);   // 0 ecall, 1 page-fault retry, else a commit
            const bool last = i + 1 == n;
            a.ecall = kind == 0; a.pgfault = kind == 1;
            a.commits = kind > 1;
            a.end = last;
            a.macro = a.commits && rnd(8) == 0;
            const bool data = a.commits && (a.macro || rnd(3) == 0) && !last;
            if (data && rnd(2)) a.done_rd = a.rd;
            fi_timing_ticks &k = ticks[i];
            k.fetch_send[0] = t;
            t += 1 + rnd(50); k.fetch_done[0] = t;
            if (a.nfetch == 2) { k.fetch_send[1] = t; t += 1 + rnd(50); k.fetch_done[1] = t; }
            k.exec = t;
            if (data) t += 1 + rnd(80);
            k.done = t;
            t += rnd(3);   // (the next attempt may start at the same tick)
            if (a.commits) ninst++;
            const bool taken = a.commits && rnd(3) == 0;
            const uint64_t next = a.commits ? (taken ? 0x10000 + 2 * rnd(4096) : pc + a.len) : pc;
            a.next_pc = last ? 0 : next;
            pc = next;
        }
        const uint64_t golden_ninst = ninst, golden_ticks = ticks[n - 1].exec;
        std::vector<uint64_t> done;
        std::vector<TickRec> rec;
        pack_tick_table(att, ticks, done, rec);
        if (done.size() != n || rec.size() != n) { printf("pack: size\n"); return 1; }
        Fnv f;
        hash_table(f, done, rec);
        uint64_t disp_here[3] = {0, 0, 0};
        for (int s = 0; s < 4000; s++) {
            uint64_t tick = rnd(golden_ticks);
            if (rnd(2)) {   // on and next to an attempt's own ticks
                const fi_timing_ticks &k = ticks[rnd(n)];
                const uint64_t ev[4] = {k.fetch_done[0], k.exec, k.done, k.fetch_send[0]};
                const uint64_t which = rnd(4);
                tick = ev[which] + rnd(3) - 1;
                if (tick >= golden_ticks) tick = golden_ticks - 1;
            }
            const uint64_t tr = rnd(8);
            const uint32_t target = tr == 0 ? FI_T_RESULT : tr < 4 ? FI_T_PC : (uint32_t)(1 + rnd(31));
            const uint64_t mask = rnd(4) ? 1ULL << rnd(64) : (rng() | 1);
            const uint32_t trial = (uint32_t)rng();
            const TickMap b = tick_map_site(done.data(), rec.data(), n, golden_ninst, tick, target, mask, trial,
                                            literal ? 1u : 0u);
            hash_site(f, tick, target, mask, trial, b);
            if (literal) {
                if (b.disp == 2 && b.reason != FI_TK_MACRO &&
                    !(b.reason == FI_TK_NONCOUNT && b.attempt - rec[b.attempt].g > FI_SITE_TK_SKIP_MAX)) {
                    printf("seed %llu table %d: tick %llu target %u: reason %u is still an escape\n",
                           (unsigned long long)seed, table, (unsigned long long)tick, target, b.reason);
                    return 1;
                }
                if (b.disp == 0) {
                    by_desc[0] += (b.site.addr >> FI_SITE_TK_SKIP_SHIFT) != 0;
                    by_desc[1] += (b.site.addr & FI_SITE_TK_FETCH) != 0;
                    by_desc[2] += (b.site.addr & FI_SITE_TK_FETCH2) != 0;
                }
            } else if (b.site.addr) {
                printf("seed %llu table %d: a tick descriptor under the numInst contract\n", (unsigned long long)seed, table);
                return 1;
            }
            checked++;
            by_disp[b.disp]++;
            disp_here[b.disp]++;
        }
        printf("table %d attempts %zu hash %016llx run %llu golden %llu escape %llu\n", table, n,
               (unsigned long long)f.h, (unsigned long long)disp_here[0], (unsigned long long)disp_here[1],
               (unsigned long long)disp_here[2]);
    }
    if (!by_disp[0] || !by_disp[1] || !by_disp[2]) { printf("a disposition never occurred\n"); return 1; }
    if (literal && (!by_desc[0] || !by_desc[1] || !by_desc[2])) { printf("a tick descriptor never occurred\n"); return 1; }
    printf("ok %llu sites (run %llu, golden %llu, escape %llu)\n", (unsigned long long)checked,
           (unsigned long long)by_disp[0], (unsigned long long)by_disp[1], (unsigned long long)by_disp[2]);
    return 0;
}
