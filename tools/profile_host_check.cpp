// profile_host_check -- the consumer rule and the host tables of an exact
// campaign's profile (shrewd_amd/csrc/fi_exact.h "Profile") on
// a hand-made golden trace, with the expected values derived by hand below: a
// stand-alone host program, so that it runs under AddressSanitizer and UBSan.
// The kernels that call the same functions need a device and are covered by
// the GPU suite.  Build (no HIP needed):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ishrewd_amd/csrc tools/profile_host_check.cpp -o profile_host_check
// Prints "profile_host_check ok" and exits 0, or names what failed.
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

constexpr uint32_t kE = 0x80000000u;   // a trace word's ecall bit
// An index entry: (2 * numInst + !ecall) << 1 | reads
static uint32_t E(uint32_t t, bool ecall, bool reads) { return ((2 * t + (ecall ? 0 : 1)) << 1) | (reads ? 1u : 0u); }

// A golden run of ninst = 10 instructions at the halfwords 20, 22, 24, 30, 32,
// 34, 40, 22, 24, 50 (the instructions at 22 and 24 run twice) with four
// ecalls: one at halfword 26 attempted at numInst 3, two at 36 and 38 both at
// numInst 6, the exit ecall at 52 at numInst 10 == ninst.
//   entry:   0   1   2   3    4   5   6   7    8    9   10  11  12  13
//   word:    20  22  24  26e  30  32  34  36e  38e  40  22  24  50  52e
//   numInst: 0   1   2   3    3   4   5   6    6    6   7   8   9   10
// Rows (ascending halfword): 20 22 24 26 30 32 34 36 38 40 50 52 -> 0 .. 11;
// execs 1 2 2 1 1 1 1 1 1 1 1 1; ecall rows 3, 7, 8, 11.
// inst_row = {0, 1, 2, 4, 5, 6, 9, 1, 2, 10}; ecalls (3, row 3), (6, row 7) --
// the second ecall at numInst 6 is not listed -- and (10, row 11).
constexpr uint64_t kNinst = 10;
static const std::vector<uint32_t> kTrace = {20, 22, 24, 26 | kE, 30, 32, 34, 36 | kE, 38 | kE, 40, 22, 24, 50, 52 | kE};

static void check_tables() {
    std::vector<uint32_t> half, row_of, inst_row;
    std::vector<uint64_t> execs;
    std::vector<uint8_t> is_ecall;
    std::vector<ExactEcall> ec;
    exact_profile_rows(kTrace.data(), kTrace.size(), half, execs, is_ecall, row_of);
    CHECK((half == std::vector<uint32_t>{20, 22, 24, 26, 30, 32, 34, 36, 38, 40, 50, 52}));
    CHECK((execs == std::vector<uint64_t>{1, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
    CHECK((is_ecall == std::vector<uint8_t>{0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1}));
    CHECK((row_of == std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2, 10, 11}));
    CHECK(exact_consumer_tables(kTrace.data(), kTrace.size(), row_of.data(), kNinst, inst_row, ec));
    CHECK((inst_row == std::vector<uint32_t>{0, 1, 2, 4, 5, 6, 9, 1, 2, 10}));
    CHECK(ec.size() == 3 && ec[0].t == 3 && ec[0].val == 3 && ec[1].t == 6 && ec[1].val == 7 && ec[2].t == 10 &&
          ec[2].val == 11);
    // a trace that does not hold ninst committing entries is refused; an empty one holds 0
    CHECK(!exact_consumer_tables(kTrace.data(), kTrace.size(), row_of.data(), kNinst + 1, inst_row, ec));
    CHECK(exact_consumer_tables(nullptr, 0, nullptr, 0, inst_row, ec) && inst_row.empty() && ec.empty());
    exact_profile_rows(nullptr, 0, half, execs, is_ecall, row_of);
    CHECK(half.empty() && row_of.empty());
}

// The register consumers, as trace words (val = NULL).
//   x5   never accessed: no class.
//   x10  read by the ecall at numInst 3, by the instruction at 3, written at 6, read by the exit ecall:
//        classes (inst 3, w 4) charged to the ecall 26e -- not to the instruction 30 at the same
//        numInst -- and (inst 9, w 3), headed by the exit ecall clipped to 9: charged to 52e.
//   x11  read by the last instruction (t = 9) and the exit ecall: one class, charged to 50.
//   x12  read by the exit ecall only: one class (inst 9, w 10), charged to 52e.
//   x13  read by both ecalls at numInst 6: the first heads (inst 6, w 7): 36e; the second heads nothing.
//   x14  written at t = 5, read by the second ecall at numInst 6 only: its class (inst 6, w 1) is
//        charged to the first ecall there, 36e (the imprecision DESIGN.md §4j names).
//   x15  read at t = 7 (the second run of halfword 22): charged to 22.
static void index(std::vector<uint32_t> &off, std::vector<uint32_t> &ev) {
    const std::vector<std::vector<uint32_t>> per = {
        {E(3, true, true), E(3, false, true), E(6, false, false), E(10, true, true)},   // x10
        {E(9, false, true), E(10, true, true)},                                         // x11
        {E(10, true, true)},                                                            // x12
        {E(6, true, true), E(6, true, true)},                                           // x13
        {E(5, false, false), E(6, true, true)},                                         // x14
        {E(7, false, true)}};                                                           // x15
    off.assign(33, 0);
    ev.clear();
    for (uint32_t r = 1; r < 32; r++) {
        off[r] = (uint32_t)ev.size();
        if (r >= 10 && r < 10 + per.size()) ev.insert(ev.end(), per[r - 10].begin(), per[r - 10].end());
    }
    off[32] = (uint32_t)ev.size();
}

static void check_registers() {
    std::vector<uint32_t> off, ev, inst_val;
    std::vector<ExactEcall> ec;
    index(off, ev);
    CHECK(exact_consumer_tables(kTrace.data(), kTrace.size(), nullptr, kNinst, inst_val, ec));
    const ExactConsumers c{inst_val.data(), ec.data(), kNinst, (uint32_t)ec.size(), 0};
    const std::vector<std::vector<uint32_t>> want = {{26 | kE, 52 | kE}, {50}, {52 | kE}, {36 | kE}, {36 | kE}, {22}};
    for (uint32_t r = 1; r < 32; r++) {
        uint32_t out[4] = {7, 7, 7, 7};
        uint64_t cls[4];
        const uint64_t n = exact_reg_consumers(off.data(), ev.data(), kNinst, r, c, out, 4);
        CHECK(n == exact_reg_classes(off.data(), ev.data(), kNinst, r, cls, 4, nullptr));
        const std::vector<uint32_t> w = r >= 10 && r < 16 ? want[r - 10] : std::vector<uint32_t>{};
        CHECK(n == w.size());
        for (uint64_t i = 0; i < n && i < w.size(); i++) CHECK(out[i] == w[i]);
        CHECK(out[n < 4 ? n : 3] == 7 || n == 4);   // nothing past the count
    }
    // counting only, and an array shorter than the count
    CHECK(exact_reg_consumers(off.data(), ev.data(), kNinst, 10, c, nullptr, 0) == 2);
    uint32_t one[2] = {7, 7};
    CHECK(exact_reg_consumers(off.data(), ev.data(), kNinst, 10, c, one, 1) == 2 && one[0] == (26 | kE) && one[1] == 7);
    // the pieces: no ecall at numInst 4 -> the instruction; past the last instruction only the ecall
    CHECK(exact_ecall_val(c, 4) == kExactNoConsumer && exact_ecall_val(c, 10) == (52 | kE));
    CHECK(exact_consumer(c, 4, true) == 32 && exact_consumer(c, 10, false) == 50);
    const ExactConsumers none{nullptr, nullptr, 0, 0, 0};
    CHECK(exact_consumer(none, 0, true) == kExactNoConsumer);
}

// A memory word's events (numInst << 16 | read << 8 | written), byte set 0x01, with the proxy bits of
// the whole index starting at bit 3 (ev_base = 3):
//   write at t = 1 (dead interval), read at t = 4 by an instruction     -> (inst 4, w 3): inst_val[4] = 32
//   read at numInst 6 recorded as a syscall's access                    -> (inst 6, w 2): the ecall 36e
//   read at numInst 8 recorded as a syscall's access, no ecall there    -> (inst 8, w 2): inst_val[8] = 24
//   read at numInst 10 by the exit ecall (proxy), clipped to 9          -> (inst 9, w 1): 52e
static void check_memory() {
    std::vector<uint32_t> inst_val;
    std::vector<ExactEcall> ec;
    CHECK(exact_consumer_tables(kTrace.data(), kTrace.size(), nullptr, kNinst, inst_val, ec));
    const ExactConsumers c{inst_val.data(), ec.data(), kNinst, (uint32_t)ec.size(), 0};
    const std::vector<uint64_t> ev = {(1ULL << 16) | 0x01, (4ULL << 16) | 0x0100, (6ULL << 16) | 0x0100,
                                      (8ULL << 16) | 0x0100, (10ULL << 16) | 0x0100};
    const uint32_t proxy[1] = {(1u << (3 + 2)) | (1u << (3 + 3)) | (1u << (3 + 4))};
    std::vector<uint8_t> live(ev.size());
    exact_mem_liveness(ev.data(), (uint32_t)ev.size(), live.data());
    ExactMemClass out[5];
    uint64_t sum = 0;
    CHECK(exact_mem_walk(ev.data(), live.data(), (uint32_t)ev.size(), kNinst, 0x01, 0, out, 5, &sum, &c, proxy, 3) == 4);
    CHECK(sum == 8);
    CHECK(out[0].inst == 4 && out[0].weight == 3 && out[0].cons == 32);
    CHECK(out[1].inst == 6 && out[1].weight == 2 && out[1].cons == (36 | kE));
    CHECK(out[2].inst == 8 && out[2].weight == 2 && out[2].cons == 24);
    CHECK(out[3].inst == 9 && out[3].weight == 1 && out[3].cons == (52 | kE));
    // without the tables the classes are the same and carry no consumer
    ExactMemClass plain[5];
    CHECK(exact_mem_walk(ev.data(), live.data(), (uint32_t)ev.size(), kNinst, 0x01, 0, plain, 5, nullptr) == 4);
    for (int i = 0; i < 4; i++)
        CHECK(plain[i].inst == out[i].inst && plain[i].weight == out[i].weight && plain[i].cons == 0);
}

// The trials of {x10, x12, pc, result} under bits {0, 12, 63}: every trial of a class has the class's
// row, the group follows the structure.
static void check_trials() {
    std::vector<uint32_t> off, ev, half, row_of, inst_row;
    std::vector<uint64_t> execs, words;
    std::vector<uint8_t> is_ecall;
    std::vector<ExactEcall> ec;
    index(off, ev);
    exact_profile_rows(kTrace.data(), kTrace.size(), half, execs, is_ecall, row_of);
    CHECK(exact_consumer_tables(kTrace.data(), kTrace.size(), row_of.data(), kNinst, inst_row, ec));
    const ExactConsumers c{inst_row.data(), ec.data(), kNinst, (uint32_t)ec.size(), 0};
    uint32_t cls_off[33];
    std::vector<uint32_t> cons;
    for (uint32_t r = 1; r < 32; r++) {
        cls_off[r] = (uint32_t)words.size();
        uint64_t w[4];
        uint32_t k[4];
        const uint64_t n = exact_reg_classes(off.data(), ev.data(), kNinst, r, w, 4, nullptr);
        exact_reg_consumers(off.data(), ev.data(), kNinst, r, c, k, 4);
        words.insert(words.end(), w, w + n);
        cons.insert(cons.end(), k, k + n);
    }
    cls_off[0] = 0;
    cls_off[32] = (uint32_t)words.size();
    const uint64_t structures = (1ULL << 10) | (1ULL << 12) | (1ULL << FI_T_PC) | (1ULL << FI_T_RESULT);
    const ExactPlan p = exact_plan(structures, cls_off, kNinst, (1ULL << 0) | (1ULL << 12) | (1ULL << 63), 1, nullptr);
    CHECK(p.nbits == 3 && p.trials == 23 * 3);
    // classes in order: x10 -> rows 3, 11; x12 -> row 11; pc t = 0..9; result t = 0..9
    std::vector<uint32_t> want_row = {3, 11, 11}, want_group = {0, 0, 0};
    for (int g : {1, 3})
        for (uint32_t t = 0; t < kNinst; t++) { want_row.push_back(inst_row[t]); want_group.push_back((uint32_t)g); }
    for (uint64_t k = 0; k < p.trials; k++) {
        uint32_t group = 9;
        CHECK(exact_trial_consumer(p, cons.data(), inst_row.data(), k, &group) == want_row[k / 3]);
        CHECK(group == want_group[k / 3]);
    }
    CHECK(exact_profile_group(5) == 0 && exact_profile_group(FI_T_PC) == 1 && exact_profile_group(FI_T_MEM) == 2 &&
          exact_profile_group(FI_T_RESULT) == 3);
}

int main() {
    check_tables();
    check_registers();
    check_memory();
    check_trials();
    if (fails) {
        printf("profile_host_check: %d check(s) failed\n", fails);
        return 1;
    }
    printf("profile_host_check ok\n");
    return 0;
}
