// exact_mem_host_check -- the memory-word classes of exact campaigns
// (shrewd_amd/csrc/fi_exact.h "Memory words"): byte sets, byte
// liveness, the per-(word, byte set) walk, the text-word exclusion and the
// trial-id map across row boundaries, on hand-made events with the expected
// values derived by hand below.  A stand-alone host program, so that it runs
// under AddressSanitizer and UBSan; the kernels that call the same functions
// are covered by the GPU suite.  Build (no HIP needed):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ishrewd_amd/csrc tools/exact_mem_host_check.cpp -o exact_mem_host_check
// Prints "exact_mem_host_check ok" and exits 0, or names what failed.
#include <cstdio>
#include <vector>

#include "fi_exact.h"

using namespace fi;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #x);         \
            fails++;                                              \
        }                                                         \
    } while (0)

// An index event: numInst << 16 | bytes read << 8 | bytes written
static uint64_t E(uint64_t t, uint32_t rd, uint32_t wr) { return (t << 16) | ((uint64_t)rd << 8) | wr; }

struct Cls { uint32_t inst, weight; };

// One word's classes under one byte set, and its dead t
static std::vector<Cls> classes(const std::vector<uint64_t> &ev, uint64_t ninst, uint32_t f, uint64_t &dead) {
    std::vector<uint8_t> live(ev.size() + 1);   // (+1: data() of an empty vector may be null)
    exact_mem_liveness(ev.data(), (uint32_t)ev.size(), live.data());
    uint64_t sum = 0;
    const uint64_t n = exact_mem_walk(ev.data(), live.data(), (uint32_t)ev.size(), ninst, f, 7, nullptr, 0, &sum);
    std::vector<ExactMemClass> c(n + 1);
    uint64_t sum2 = 0;
    CHECK(exact_mem_walk(ev.data(), live.data(), (uint32_t)ev.size(), ninst, f, 7, c.data(), n, &sum2) == n);
    CHECK(sum == sum2);
    std::vector<Cls> out;
    for (uint64_t i = 0; i < n; i++) {
        CHECK(c[i].word == 7);
        out.push_back({c[i].inst, c[i].weight});
    }
    dead = ninst - sum;
    return out;
}
static bool same(const std::vector<Cls> &a, std::vector<Cls> b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].inst != b[i].inst || a[i].weight != b[i].weight) return false;
    return true;
}

static void check_classes() {
    uint64_t dead = 0;
    // The worked example.  ninst = 10; t = 2: rd 0x0F, t = 4: wr 0x03, t = 7: rd 0xFF.
    //   live_before: t = 7: 0xFF; t = 4: 0xFF & ~0x03 = 0xFC; t = 2: 0x0F | 0xFC = 0xFF
    //   F = 0x01: all three events touch it.  (−1, 2] live: (2, 3); (2, 4] the store, 0xFC & 1 = 0:
    //             dead (t = 3, 4); (4, 7] live: (7, 3); t = 8, 9 after the last event: dead.  dead = 4
    //   F = 0x06: (2, 3); the store touches byte 1, 0xFC & 6 != 0 (byte 2 is read at t = 7): (4, 2);
    //             (7, 3); dead = 2
    //   F = 0x10: only t = 7 touches byte 4: (7, 8); dead = 2
    const std::vector<uint64_t> ex = {E(2, 0x0F, 0), E(4, 0, 0x03), E(7, 0xFF, 0)};
    {
        std::vector<uint8_t> live(3);
        exact_mem_liveness(ex.data(), 3, live.data());
        CHECK(live[0] == 0xFF && live[1] == 0xFC && live[2] == 0xFF);
    }
    CHECK(same(classes(ex, 10, 0x01, dead), {{2, 3}, {7, 3}}) && dead == 4);
    CHECK(same(classes(ex, 10, 0x06, dead), {{2, 3}, {4, 2}, {7, 3}}) && dead == 2);
    CHECK(same(classes(ex, 10, 0x10, dead), {{7, 8}}) && dead == 2);
    // Entries of the same numInst: only the first heads an interval.  A store of byte 0 then a
    // load of it at t = 5 (one instruction's two accesses): the store heads (−1, 5], dead (byte 0 is
    // overwritten before it is read); the load has u' = prev' and heads nothing.  dead = 10
    CHECK(same(classes({E(5, 0, 0x01), E(5, 0x01, 0)}, 10, 0x01, dead), {}) && dead == 10);
    // ... the other way round the load heads it and it is live: (5, 6); dead = 4
    CHECK(same(classes({E(5, 0x01, 0), E(5, 0, 0x01)}, 10, 0x01, dead), {{5, 6}}) && dead == 4);
    // An AMO: reads and writes the same bytes in one event, the read first: live.  Then a plain
    // store: (3, 6] dead.  dead = 10 - 4
    CHECK(same(classes({E(3, 0x0F, 0x0F), E(6, 0, 0x0F)}, 10, 0x02, dead), {{3, 4}}) && dead == 6);
    // An event at numInst == ninst (a read by the exit call) is clipped to ninst - 1 = 9: after the
    // store at t = 4 it heads (4, 9]: (9, 5); dead = t 0..4
    CHECK(same(classes({E(4, 0, 0xFF), E(10, 0x80, 0)}, 10, 0x80, dead), {{9, 5}}) && dead == 5);
    // ... and with an event at t = 9 before it, clipped to 9 = prev': heads nothing; the event at
    // t = 9 is live through its own read
    CHECK(same(classes({E(9, 0x80, 0), E(10, 0x80, 0)}, 10, 0x80, dead), {{9, 10}}) && dead == 0);
    // A word with no events, and events that do not touch the set: all dead
    CHECK(same(classes({}, 10, 0xFF, dead), {}) && dead == 10);
    CHECK(same(classes(ex, 10, 0x80, dead), {{7, 8}}) && dead == 2);
    CHECK(same(classes({E(2, 0x0F, 0)}, 10, 0xF0, dead), {}) && dead == 10);
    // no instructions: nothing
    CHECK(same(classes(ex, 0, 0x01, dead), {}) && dead == 0);
}

static void check_byte_sets() {
    ExactMemRow r[kExactMaxMemRows];
    // burst 1, every position: a set per byte, 8 positions each
    CHECK(exact_mem_sets(~0ULL, 1, r) == 8);
    for (uint32_t g = 0; g < 8; g++)
        CHECK(r[g].fmask == (1u << g) && r[g].pos == (0xFFULL << (8 * g)) && r[g].npos == 8 && r[g].shift == 3);
    // burst 4, every position (0..60): per byte g < 7 the positions 8g..8g+4 stay inside it (5) and
    // 8g+5..8g+7 cross into the next (3); byte 7: 56..60 (5).  15 sets
    CHECK(exact_mem_sets(~0ULL, 4, r) == 15);
    for (uint32_t g = 0; g < 15; g++) {
        const uint32_t by = g / 2;
        if (g % 2 == 0) CHECK(r[g].fmask == (1u << by) && r[g].pos == (0x1FULL << (8 * by)) && r[g].npos == 5 && r[g].shift == 64);
        else CHECK(r[g].fmask == (3u << by) && r[g].pos == (0xE0ULL << (8 * by)) && r[g].npos == 3);
    }
    // burst 2, positions {0, 7, 12, 63}: 63 is past 64 - burst; 7 spans bytes 0-1
    CHECK(exact_mem_sets((1ULL << 0) | (1ULL << 7) | (1ULL << 12) | (1ULL << 63), 2, r) == 3);
    CHECK(r[0].fmask == 0x01 && r[0].pos == 1 && r[1].fmask == 0x03 && r[1].pos == (1ULL << 7) && r[2].fmask == 0x02 &&
          r[2].pos == (1ULL << 12));
    // burst 16: a position covers bytes b/8 .. (b+15)/8: {0}: 0x03, {1..8}: bytes 0-2 / 1-2 ...
    CHECK(exact_byte_set(0, 16) == 0x03 && exact_byte_set(1, 16) == 0x07 && exact_byte_set(8, 16) == 0x06 &&
          exact_byte_set(48, 16) == 0xC0 && exact_byte_set(63, 1) == 0x80 && exact_byte_set(0, 64) == 0xFF);
    CHECK(exact_mem_sets(~0ULL, 64, r) == 1 && r[0].fmask == 0xFF && r[0].pos == 1);
    CHECK(exact_mem_sets(0, 1, r) == 0);
}

static void check_text_words() {
    // Pages 0x10000, 0x12000, 0x7f000.  Text [0x10ff4, 0x12010): in page 0x10000 the words from
    // 0x10ff0 (it overlaps the text's first 4 bytes) to the page's end: 2; page 0x11000 is no
    // candidate; in page 0x12000 the words 0x12000 and 0x12008: 2.
    const uint64_t pages[] = {0x10000, 0x12000, 0x7f000};
    CHECK(exact_mem_text_words(pages, 3, 0x10ff4, 0x12010) == 4);
    CHECK(exact_mem_text_words(pages, 3, 0x10ff4, 0x12011) == 5);   // one byte into 0x12010
    CHECK(exact_mem_text_words(pages, 3, 0x20000, 0x30000) == 0);
    CHECK(exact_mem_text_words(pages, 3, 0x7f000, 0x80000) == 512);
    CHECK(exact_mem_text_words(pages, 0, 0x10000, 0x20000) == 0);
    // the last page of the address space (its end is not a 64-bit number): text from its middle to
    // 7 bytes before the end overlaps its upper 256 words, the last one included
    const uint64_t top[] = {0x7ffffffffffff000ULL, 0xfffffffffffff000ULL};
    CHECK(exact_mem_text_words(top, 2, 0xfffffffffffff800ULL, 0xfffffffffffffff9ULL) == 256);
    CHECK(exact_mem_text_words(top, 2, 0x7ffffffffffffff0ULL, 0x8000000000000004ULL) == 2);
    CHECK(!exact_mem_in_space(top, 2, 0xfffffffffffff800ULL, 0xfffffffffffffff9ULL, 0xfffffffffffffff8ULL) &&
          exact_mem_in_space(top, 2, 0xfffffffffffff800ULL, 0xfffffffffffffff9ULL, 0xfffffffffffff7f8ULL) &&
          exact_mem_in_space(top, 2, 0, 0, 0xfffffffffffffff8ULL) && exact_mem_in_space(top, 2, 0, 0, 0x7ffffffffffffff8ULL));
    uint64_t in = 0;
    for (uint64_t a = 0x10000; a < 0x13000; a += 8) in += exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, a);
    CHECK(in == 2 * 512 - 4);
    CHECK(!exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, 0x10ff0) && exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, 0x10fe8));
    CHECK(!exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, 0x12008) && exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, 0x12010));
    CHECK(!exact_mem_in_space(pages, 3, 0x10ff4, 0x12010, 0x11800) && exact_mem_in_space(pages, 3, 0, 0, 0x7fff8) &&
          !exact_mem_in_space(pages, 3, 0, 0, 0x80000) && !exact_mem_in_space(pages, 3, 0, 0, 0x8));
}

// The trial ids of {x6, pc, memory, result} over two words, restated with
// plain loops: byte sets, then words, then classes, then positions; the
// register, pc and result trials keep the ids of the plan without memory,
// the result's moved up by the memory trials.
static void check_map(uint64_t bits_mask, uint32_t burst) {
    constexpr uint64_t kNinst = 10;
    const std::vector<std::vector<uint64_t>> words = {
        {E(2, 0x0F, 0), E(4, 0, 0x03), E(7, 0xFF, 0)},     // the worked example
        {E(1, 0, 0xFF), E(3, 0xF0, 0), E(10, 0x01, 0)}};   // a store, an upper-half load, a clipped read
    const uint64_t addr[2] = {0x7f000, 0x7f040};
    // the register part: x6 written at t = 2, read at t = 5 (tools/exact_host_check.cpp): one class
    std::vector<uint32_t> off(33, 0), ev = {((2 * 2 + 1) << 1), ((2 * 5 + 1) << 1) | 1};
    for (int r = 7; r <= 32; r++) off[r] = 2;
    uint64_t rw[2];
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 6, rw, 2, nullptr) == 1);
    uint32_t cls_off[33] = {};
    for (int r = 7; r <= 32; r++) cls_off[r] = 1;
    const uint64_t structures = (1ULL << 6) | (1ULL << FI_T_PC) | (1ULL << FI_T_MEM) | (1ULL << FI_T_RESULT);
    const ExactPlan p0 = exact_plan(structures, cls_off, kNinst, bits_mask, burst, nullptr);
    CHECK(p0.mem_trials == 0 && p0.mem_first == 11ull * p0.nbits && p0.trials == 21ull * p0.nbits);

    ExactMemRow rows[kExactMaxMemRows];
    const uint32_t n_rows = exact_mem_sets(bits_mask, burst, rows);
    std::vector<ExactMemClass> cls;
    uint64_t per_row[kExactMaxMemRows] = {};
    struct Want { uint64_t inst, addr, mask; uint32_t weight; };
    std::vector<Want> want;
    uint32_t npos_sum = 0;
    for (uint32_t g = 0; g < n_rows; g++) {
        npos_sum += rows[g].npos;
        for (uint32_t w = 0; w < 2; w++) {
            std::vector<uint8_t> live(words[w].size());
            exact_mem_liveness(words[w].data(), (uint32_t)words[w].size(), live.data());
            ExactMemClass c[4];
            const uint64_t n = exact_mem_walk(words[w].data(), live.data(), (uint32_t)words[w].size(), kNinst, rows[g].fmask,
                                              w, c, 4, nullptr);
            CHECK(n <= 3);
            per_row[g] += n;
            for (uint64_t i = 0; i < n; i++) {
                cls.push_back(c[i]);
                for (uint64_t m = rows[g].pos; m; m &= m - 1)
                    want.push_back({c[i].inst, addr[w], exact_burst_mask(burst) << __builtin_ctzll(m), c[i].weight});
            }
        }
    }
    CHECK(npos_sum == p0.nbits);
    ExactPlan p = p0;
    exact_plan_mem(p, rows, n_rows, per_row, rows, cls.data(), addr);
    CHECK(p.mem_trials == want.size() && p.trials == p0.trials + want.size());
    for (uint64_t k = 0; k < p.trials; k++) {
        const ExactSite s = exact_site(p, rw, k);
        if (k >= p.mem_first && k < p.mem_first + p.mem_trials) {
            const Want &w = want[k - p.mem_first];
            CHECK(s.target == FI_T_MEM && s.inst == w.inst && s.addr == w.addr && s.mask == w.mask && s.weight == w.weight);
        } else {   // as without memory
            const ExactSite r = exact_site(p0, rw, k < p.mem_first ? k : k - p.mem_trials);
            CHECK(s.target == r.target && s.inst == r.inst && s.mask == r.mask && s.weight == r.weight && s.addr == 0);
            CHECK(s.target == (k < p0.nbits ? 6u : k < p.mem_first ? (uint32_t)FI_T_PC : (uint32_t)FI_T_RESULT));
        }
    }
    // memory alone: the ids start at 0
    ExactPlan q = exact_plan(1ULL << FI_T_MEM, cls_off, kNinst, bits_mask, burst, nullptr);
    CHECK(q.trials == 0 && q.mem_first == 0);
    exact_plan_mem(q, rows, n_rows, per_row, rows, cls.data(), addr);
    CHECK(q.trials == want.size());
    for (uint64_t k = 0; k < q.trials; k++) {
        const ExactSite s = exact_site(q, rw, k);
        CHECK(s.target == FI_T_MEM && s.inst == want[k].inst && s.addr == want[k].addr && s.mask == want[k].mask);
    }
}

int main() {
    check_classes();
    check_byte_sets();
    check_text_words();
    check_map(~0ULL, 1);
    check_map(0x8000100000021081ULL, 1);    // sparse: bytes 0, 1, 2, 5 and 7; byte 0 holds two positions
    check_map(~0ULL, 4);
    check_map(0x8000100000021081ULL, 4);    // bit 63 is past 64 - burst
    check_map(~0ULL, 16);
    check_map(0x0000100000021081ULL, 16);
    if (fails) {
        printf("exact_mem_host_check: %d check(s) failed\n", fails);
        return 1;
    }
    printf("exact_mem_host_check ok\n");
    return 0;
}
