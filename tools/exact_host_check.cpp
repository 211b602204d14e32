// exact_host_check -- the class builder and the trial-id map of exact
// campaigns (shrewd_amd/csrc/fi_exact.h) on a hand-made
// first-access index, with the expected values derived by hand below: a
// stand-alone host program, so that it runs under AddressSanitizer and UBSan.
// The kernels that call the same functions need a device and are covered by
// the GPU suite.  Build (no HIP needed):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ishrewd_amd/csrc tools/exact_host_check.cpp -o exact_host_check
// Prints "exact_host_check ok" and exits 0, or names what failed.
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

// An index entry: (2 * numInst + !ecall) << 1 | reads
static uint32_t E(uint32_t t, bool ecall, bool reads) { return ((2 * t + (ecall ? 0 : 1)) << 1) | (reads ? 1u : 0u); }

// A golden run of ninst = 10 instructions.  Four registers:
//   x5   never accessed                     no class, dead = 10
//   x6   written at t = 2, read at t = 5    the write heads nothing (t = 0..2 dead); the read heads a
//                                           class over t in (2, 5]: inst 5, weight 3; t = 6..9 have no
//                                           access left: dead = 10 - 3 = 7
//   x10  read by an ecall at numInst 3 and by the instruction at numInst 3, written at t = 6, read by
//        the exit ecall at numInst 10 == ninst
//                                           the ecall heads (-1, 3]: inst 3, weight 4; the instruction's
//                                           entry has u' = 3 = prev': no class; the write: t = 4..6 dead;
//                                           the exit ecall is clipped to u' = 9 and heads (6, 9]: inst 9,
//                                           weight 3; dead = 10 - 7 = 3
//   x11  read by the last instruction (t = 9) and by the exit ecall (numInst 10)
//                                           the instruction heads (-1, 9]: inst 9, weight 10; the exit
//                                           ecall, clipped to 9 = prev', heads nothing; dead = 0
constexpr uint64_t kNinst = 10;
static void index(std::vector<uint32_t> &off, std::vector<uint32_t> &ev) {
    ev = {E(2, false, false), E(5, false, true),                                       // x6
          E(3, true, true), E(3, false, true), E(6, false, false), E(10, true, true),   // x10
          E(9, false, true), E(10, true, true)};                                       // x11
    off.assign(33, 0);
    for (int r = 7; r <= 10; r++) off[r] = 2;
    off[11] = 6;
    for (int r = 12; r <= 32; r++) off[r] = 8;
}

struct Cls { uint64_t inst; uint32_t reg, weight; };

static void check_classes() {
    std::vector<uint32_t> off, ev;
    index(off, ev);
    uint64_t w[4], dead = ~0ULL;
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 5, w, 4, &dead) == 0 && dead == 10);
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 6, w, 4, &dead) == 1 && dead == 7);
    CHECK(exact_word_inst(w[0]) == 5 && exact_word_reg(w[0]) == 6 && exact_word_weight(w[0]) == 3);
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 10, w, 4, &dead) == 2 && dead == 3);
    CHECK(exact_word_inst(w[0]) == 3 && exact_word_reg(w[0]) == 10 && exact_word_weight(w[0]) == 4);
    CHECK(exact_word_inst(w[1]) == 9 && exact_word_reg(w[1]) == 10 && exact_word_weight(w[1]) == 3);
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 11, w, 4, &dead) == 1 && dead == 0);
    CHECK(exact_word_inst(w[0]) == 9 && exact_word_reg(w[0]) == 11 && exact_word_weight(w[0]) == 10);
    // counting only (no array), and an array shorter than the count: nothing past cap is written
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 10, nullptr, 0, nullptr) == 2);
    uint64_t one[1] = {0};
    CHECK(exact_reg_classes(off.data(), ev.data(), kNinst, 10, one, 1, &dead) == 2 && exact_word_inst(one[0]) == 3);
    // the field limits: inst < 2^29, weight < 2^30
    const uint64_t big = exact_pack((1ULL << 29) - 1, 31, (1ULL << 29));
    CHECK(exact_word_inst(big) == (1ULL << 29) - 1 && exact_word_reg(big) == 31 && exact_word_weight(big) == (1u << 29));
    // a run of one instruction: every read clips to t = 0
    std::vector<uint32_t> off1(33, 0), ev1 = {E(0, false, true), E(1, true, true)};
    for (int r = 11; r <= 32; r++) off1[r] = 2;
    CHECK(exact_reg_classes(off1.data(), ev1.data(), 1, 10, w, 4, &dead) == 1 && dead == 0);
    CHECK(exact_word_inst(w[0]) == 0 && exact_word_weight(w[0]) == 1);
}

// Every register's words as the engine lays them out, and the plan over them
static void layout(std::vector<uint64_t> &words, uint32_t cls_off[33]) {
    std::vector<uint32_t> off, ev;
    index(off, ev);
    for (uint32_t r = 1; r < 32; r++) {
        cls_off[r] = (uint32_t)words.size();
        uint64_t w[8];
        const uint64_t n = exact_reg_classes(off.data(), ev.data(), kNinst, r, w, 8, nullptr);
        words.insert(words.end(), w, w + n);
    }
    cls_off[0] = 0;
    cls_off[32] = (uint32_t)words.size();
}

// The trial ids of {x5, x6, x10, x11, pc, result}: the classes in order are
//   x6: (5, w 3)   x10: (3, w 4), (9, w 3)   x11: (9, w 10)   pc: t = 0..9   result: t = 0..9
// (x5 has none: its row starts where x6's does and is never the last row at or
// before a trial), 24 classes; k = class index * nbits + slot.
static void check_map(uint64_t bits_mask, uint32_t burst, std::vector<uint32_t> positions) {
    std::vector<uint64_t> words;
    uint32_t cls_off[33];
    layout(words, cls_off);
    CHECK(words.size() == 4);
    const uint64_t structures = (1ULL << 5) | (1ULL << 6) | (1ULL << 10) | (1ULL << 11) | (1ULL << FI_T_PC) |
                                (1ULL << FI_T_RESULT);
    uint64_t per[FI_N_STRUCT];
    const ExactPlan p = exact_plan(structures, cls_off, kNinst, bits_mask, burst, per);
    const uint32_t nb = (uint32_t)positions.size();
    CHECK(p.nbits == nb && p.n_rows == 6 && p.trials == 24ull * nb);
    CHECK(per[5] == 0 && per[6] == 1 && per[10] == 2 && per[11] == 1 && per[FI_T_PC] == 10 && per[FI_T_RESULT] == 10 &&
          per[7] == 0 && per[FI_T_MEM] == 0);
    std::vector<Cls> want = {{5, 6, 3}, {3, 10, 4}, {9, 10, 3}, {9, 11, 10}};
    for (uint32_t t = 0; t < 10; t++) want.push_back({t, FI_T_PC, 1});
    for (uint32_t t = 0; t < 10; t++) want.push_back({t, FI_T_RESULT, 1});
    const uint64_t bm = burst == 64 ? ~0ULL : ((1ULL << burst) - 1);
    uint64_t weight_sum = 0;
    for (uint64_t k = 0; k < p.trials; k++) {
        const ExactSite s = exact_site(p, words.data(), k);
        const Cls &c = want[k / nb];
        CHECK(exact_class_index(p, k) == k / nb);
        CHECK(s.inst == c.inst && s.target == c.reg && s.weight == c.weight);
        CHECK(s.mask == bm << positions[k % nb]);
        weight_sum += s.weight;
    }
    // the live sites: (3 + 7 + 10) register sites and 20 pc / result sites per position
    CHECK(weight_sum == 40ull * nb);
}

// The reciprocal against the divide, at the ends of the trial-id range
static void check_recip() {
    uint32_t cls_off[33] = {};
    for (uint32_t nb = 1; nb <= 64; nb++) {
        const ExactPlan p = exact_plan(1ULL << FI_T_PC, cls_off, 1, nb == 64 ? ~0ULL : (1ULL << nb) - 1, 1, nullptr);
        CHECK(p.nbits == nb);
        uint64_t x = 0x9E3779B97F4A7C15ULL;
        for (int i = 0; i < 2000; i++) {
            x = x * 6364136223846793005ULL + 1442695040888963407ULL;
            const uint64_t ks[] = {(uint64_t)i, (x >> 24) % kExactMaxTrials, kExactMaxTrials - 1 - (uint64_t)i,
                                   ((x >> 30) % (kExactMaxTrials / nb)) * nb, ((x >> 30) % (kExactMaxTrials / nb)) * nb + nb - 1};
            for (uint64_t k : ks) CHECK(exact_class_index(p, k) == k / nb);
        }
    }
}

int main() {
    check_classes();
    {   // nbits 64: every position, burst 1
        std::vector<uint32_t> pos;
        for (uint32_t b = 0; b < 64; b++) pos.push_back(b);
        check_map(~0ULL, 1, pos);
    }
    check_map(1ULL << 17, 1, {17});                                  // nbits 1
    check_map((1ULL << 0) | (1ULL << 12) | (1ULL << 63), 1, {0, 12, 63});   // nbits 3, not contiguous
    {   // a burst of 4 cuts positions 61..63: 61 left
        std::vector<uint32_t> pos;
        for (uint32_t b = 0; b <= 60; b++) pos.push_back(b);
        check_map(~0ULL, 4, pos);
    }
    check_map((1ULL << 3) | (1ULL << 60) | (1ULL << 62), 4, {3, 60});   // the mask's bit 62 is past 64 - burst
    check_map(~0ULL, 64, {0});                                       // only position 0 holds a 64-bit burst
    check_recip();
    if (fails) {
        printf("exact_host_check: %d check(s) failed\n", fails);
        return 1;
    }
    printf("exact_host_check ok\n");
    return 0;
}
