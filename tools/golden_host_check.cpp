// golden_host_check -- the host passes of fi_golden_run
// (shrewd_amd/csrc/fi_golden_host.h: snapshot page dedupe, register liveness,
// first-access index) on hand-made inputs, with the expected values derived by
// hand below: a stand-alone host program, so that it runs under
// AddressSanitizer and UBSan.  The launches, downloads and uploads around
// these passes need a device and are covered by the GPU suite.  Build (no HIP
// needed):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ishrewd_amd/csrc tools/golden_host_check.cpp -o golden_host_check
// Prints "golden_host_check ok" and exits 0, or names what failed.
#include <cstdio>
#include <vector>

#include "fi_golden_host.h"

using namespace fi;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #x);         \
            fails++;                                              \
        }                                                         \
    } while (0)

constexpr uint8_t kOpAny = 1, kOpM5 = 200;   // (the passes look at no other op value than the M5Op's)

static PreInst inst(uint8_t op, uint8_t rd, uint8_t rs1, uint8_t rs2, uint8_t flags) {
    PreInst p{};
    p.op = op; p.rd = rd; p.rs1 = rs1; p.rs2 = rs2; p.flags = flags; p.len = 4;
    return p;
}

// Six entries of text (index = halfword):
//   0: addi x5, x6, 1      reads x6          writes x5
//   1: add  x7, x5, x7     reads x5, x7      writes x7   (reads and writes the same register)
//   2: ecall               no register fields; its syscall event (bit 31) reads x10..x17, writes nothing
//   3: addi x6, x0, 3      reads nothing (rs1 = x0)      writes x6
//   4: add  x10, x6, x5    reads x6, x5      writes x10
//   5: not an instruction  (flags 0: invalid)
static std::vector<PreInst> text() {
    const uint8_t V = kPreValid;
    return {inst(kOpAny, 5, 6, 0, V | kPreRs1 | kPreRd),  inst(kOpAny, 7, 5, 7, V | kPreRs1 | kPreRs2 | kPreRd),
            inst(kOpAny, 0, 0, 0, V),                     inst(kOpAny, 6, 0, 0, V | kPreRs1 | kPreRd),
            inst(kOpAny, 10, 6, 5, V | kPreRs1 | kPreRs2 | kPreRd), inst(0, 0, 0, 0, 0)};
}

static std::vector<SnapState> snaps_at(std::initializer_list<uint32_t> pos) {
    std::vector<SnapState> s;
    for (uint32_t p : pos) {
        SnapState S{};
        S.trace_pos = p;
        S.live = 0x12345678u;   // (to be overwritten)
        s.push_back(S);
    }
    return s;
}

// The trace, with numInst t before each event and key = 2 * t + !ecall:
//   i  entry       t  key  reads        writes
//   0  0           0   1   x6           x5
//   1  1           1   3   x5 x7        x7
//   2  3           2   5   -            x6
//   3  2 | ecall   3   6   x10..x17     -      (the syscall: commits nothing)
//   4  2           3   7   -            -      (the ecall instruction commits)
//   5  4           4   9   x5 x6        x10
//   6  0           5  11   x6           x5
//   7  1           6  13   x5 x7        x7
// Liveness, backward (live = (live - writes) | reads), sets written as {registers}:
//   after i7 {5,7}; i6 {6,7}; i5 {5,6,7}                    -> snapshot at 5: 0xE0
//   i4 {5,6,7}; i3 {5,6,7,10..17}; i2 {5,7,10..17}           -> snapshot at 2: 0x3FCA0
//     (x6 is written at i2 before its next read: dead there; x10 is read by the syscall first: live)
//   i1 {5,7,10..17}; i0 {6,7,10..17}                         -> snapshot at 0: 0x3FCC0
// First-access entries, key << 1 | reads:
//   x5:  i0 w 2, i1 r 7, i5 r 19, i6 w 22, i7 r 27
//   x6:  i0 r 3, i2 w 10, i5 r 19, i6 r 23
//   x7:  i1 rw 7, i7 rw 27       (read and written: the read bit is set)
//   x10: i3 r 13, i5 w 18;  x11..x17: i3 r 13
//   off: x5 starts at 0, x6 at 5, x7 at 9, x8..x10 at 11, x11 at 13, ... x17 at 19, the end 20
static void check_liveness_and_index() {
    const std::vector<PreInst> pre = text();
    const uint32_t E = 0x80000000u;
    const std::vector<uint32_t> trace = {0, 1, 3, 2 | E, 2, 4, 0, 1};
    std::vector<SnapState> snaps = snaps_at({0, 2, 5});
    std::vector<uint32_t> rm, wm;
    CHECK(trace_liveness(pre, trace, trace.size(), kOpM5, rm, wm, snaps));
    CHECK(rm == (std::vector<uint32_t>{1u << 6, 1u << 5 | 1u << 7, 0, 0x3FC00u, 0, 1u << 5 | 1u << 6, 1u << 6,
                                       1u << 5 | 1u << 7}));
    CHECK(wm == (std::vector<uint32_t>{1u << 5, 1u << 7, 1u << 6, 0, 0, 1u << 10, 1u << 5, 1u << 7}));
    CHECK(snaps[2].live == 0xE0u);
    CHECK(snaps[1].live == 0x3FCA0u);
    CHECK(snaps[0].live == 0x3FCC0u);
    std::vector<uint32_t> off, ev;
    first_access_index(trace, rm, wm, off, ev);
    std::vector<uint32_t> want_off(33, 20);
    for (int r = 0; r <= 5; r++) want_off[r] = 0;
    want_off[6] = 5; want_off[7] = 9;
    want_off[8] = want_off[9] = want_off[10] = 11;
    for (int r = 11; r <= 17; r++) want_off[r] = 13 + (r - 11);
    CHECK(off == want_off);
    CHECK(ev == (std::vector<uint32_t>{2, 7, 19, 22, 27, 3, 10, 19, 23, 7, 27, 13, 18, 13, 13, 13, 13, 13, 13, 13}));
    CHECK(std::vector<uint32_t>(ev.begin() + off[5], ev.begin() + off[6]) == (std::vector<uint32_t>{2, 7, 19, 22, 27}));
    CHECK(std::vector<uint32_t>(ev.begin() + off[6], ev.begin() + off[7]) == (std::vector<uint32_t>{3, 10, 19, 23}));

    // an M5Op reads x10..x17 and writes nothing, whatever its rd field says
    std::vector<PreInst> p2 = {inst(kOpM5, 10, 0, 0, kPreValid | kPreRd)};
    std::vector<SnapState> s2 = snaps_at({0});
    CHECK(trace_liveness(p2, {0}, 1, kOpM5, rm, wm, s2));
    CHECK(rm == std::vector<uint32_t>{0x3FC00u} && wm == std::vector<uint32_t>{0} && s2[0].live == 0x3FC00u);
    // no events at all: usable, nothing live, an empty index
    s2 = snaps_at({0});
    CHECK(trace_liveness(pre, {}, 0, kOpM5, rm, wm, s2) && s2[0].live == 0);
    first_access_index({}, rm, wm, off, ev);
    CHECK(off == std::vector<uint32_t>(33, 0) && ev.empty());
}

// An entry past the text (6), the invalid entry (5), a trace that overflowed
// (empty with events counted): live_ok is false and every register but x0
// counts as live at every snapshot.
static void check_unusable_trace() {
    const std::vector<PreInst> pre = text();
    const std::vector<std::vector<uint32_t>> bad = {{0, 1, 6, 4}, {0, 5, 1}, {0, 1, 0x80000000u | 6}, {}};
    for (const auto &trace : bad) {
        std::vector<SnapState> snaps = snaps_at({0, 1, 2});
        std::vector<uint32_t> rm, wm;
        CHECK(!trace_liveness(pre, trace, trace.empty() ? 100 : trace.size(), kOpM5, rm, wm, snaps));
        for (const SnapState &S : snaps) CHECK(S.live == 0xFFFFFFFEu);
        CHECK(rm.size() == trace.size() && wm.size() == trace.size());
    }
}

static std::vector<uint8_t> page(uint8_t fill) { return std::vector<uint8_t>(kPage, fill); }

struct Captured {   // pass 2's download, P pages per snapshot
    uint32_t P = 3;
    std::vector<SnapState> rs;
    std::vector<uint8_t> rp;
    std::vector<uint64_t> rv;
    void snap(std::initializer_list<std::pair<uint64_t, std::vector<uint8_t>>> pages) {
        SnapState S{};
        S.tab_n = (uint32_t)pages.size();
        S.ninst = 100 * rs.size();
        const size_t k = rs.size();
        rs.push_back(S);
        rp.resize((k + 1) * P * kPage, 0xEE);
        rv.resize((k + 1) * P, ~0ULL);
        size_t i = 0;
        for (const auto &pg : pages) {
            rv[k * P + i] = pg.first;
            memcpy(rp.data() + ((k * P + i) << 12), pg.second.data(), kPage);
            i++;
        }
    }
};

// Process start: the code page vpn 0x10 (frame 0, bytes 0xC0) and a data page
// vpn 0x20 (frame 1, bytes 0xD0); the executable bytes are [0x10100, 0x10200).
struct Start {
    std::vector<PageEnt> tab;
    std::vector<uint8_t> pool;
    std::map<uint64_t, std::vector<uint8_t>> org;
    uint64_t code_lo = 0x10100, code_hi = 0x10200;
    Start() {
        PageEnt a{}, b{};
        a.vpn = 0x10; a.frame = 0;
        b.vpn = 0x20; b.frame = 1;
        tab = {a, b};
        org[0x10] = page(0xC0);
        org[0x20] = page(0xD0);
        pool = org[0x10];
        pool.insert(pool.end(), org[0x20].begin(), org[0x20].end());
    }
};

static bool tab_is(const std::vector<PageEnt> &tab, const SnapState &S,
                   std::initializer_list<std::pair<uint64_t, uint32_t>> want) {
    if (S.tab_n != want.size() || (size_t)S.tab_off + S.tab_n > tab.size()) return false;
    size_t i = S.tab_off;
    for (const auto &w : want) {
        if (tab[i].vpn != w.first || tab[i].frame != w.second) return false;
        i++;
    }
    return true;
}

// Snapshot 0 captured nothing: the start table {0x10 -> 0, 0x20 -> 1}.
// Snapshot 1 captured a new page 0x30 (bytes 0x33) and then 0x20 changed
//   (bytes 0xD1): frames 2 and 3; its table {0x10 -> 0, 0x20 -> 3, 0x30 -> 2},
//   sorted by vpn although 0x30 was captured first.
// Snapshot 2 captured 0x30 and 0x20 again, unchanged -- they share frames 2
//   and 3 -- and the code page with byte 0x300 changed, outside the code
//   range: frame 4, pre_ok stays; its table {0x10 -> 4, 0x20 -> 3, 0x30 -> 2}.
// The pool ends with 5 frames.
static void check_dedupe() {
    Start s;
    Captured c;
    std::vector<uint8_t> code2 = page(0xC0);
    code2[0x300] = 1;
    c.snap({});
    c.snap({{0x30, page(0x33)}, {0x20, page(0xD1)}});
    c.snap({{0x30, page(0x33)}, {0x20, page(0xD1)}, {0x10, code2}});
    std::vector<SnapState> snaps;
    std::vector<PageEnt> tab;
    const bool pre_ok = dedupe_snapshot_pages(s.tab.data(), 2, s.pool, s.org, s.code_lo, s.code_hi, c.rs, c.rp, c.rv, c.P,
                                              snaps, tab);
    CHECK(pre_ok);
    CHECK(snaps.size() == 3 && tab.size() == 2 + 3 + 3);
    CHECK(s.pool.size() == 5 * kPage);
    CHECK(snaps[0].tab_off == 0 && snaps[1].tab_off == 2 && snaps[2].tab_off == 5);
    CHECK(tab_is(tab, snaps[0], {{0x10, 0}, {0x20, 1}}));
    CHECK(tab_is(tab, snaps[1], {{0x10, 0}, {0x20, 3}, {0x30, 2}}));
    CHECK(tab_is(tab, snaps[2], {{0x10, 4}, {0x20, 3}, {0x30, 2}}));
    CHECK(snaps[2].ninst == 200);   // (the rest of the state is carried over)
    CHECK(s.pool[2 * kPage] == 0x33 && s.pool[3 * kPage] == 0xD1 && s.pool[4 * kPage + 0x300] == 1 &&
          s.pool[4 * kPage] == 0xC0);
}

// The code page captured with one byte changed at `at`: pre_ok is lost exactly
// when 0x100 <= at < 0x200.  Without an original page to compare with it is
// lost too.
static void check_dedupe_code_range() {
    for (uint32_t at : {0x0u, 0xFFu, 0x100u, 0x180u, 0x1FFu, 0x200u, 0xFFFu}) {
        Start s;
        Captured c;
        std::vector<uint8_t> code2 = page(0xC0);
        code2[at] ^= 0xFF;
        c.snap({{0x10, code2}});
        std::vector<SnapState> snaps;
        std::vector<PageEnt> tab;
        const bool pre_ok = dedupe_snapshot_pages(s.tab.data(), 2, s.pool, s.org, s.code_lo, s.code_hi, c.rs, c.rp, c.rv,
                                                  c.P, snaps, tab);
        CHECK(pre_ok == !(at >= 0x100 && at < 0x200));
        CHECK(s.pool.size() == 3 * kPage && tab_is(tab, snaps[0], {{0x10, 2}, {0x20, 1}}));
    }
    Start s;
    Captured c;
    s.org.erase(0x10);
    std::vector<uint8_t> code2 = page(0xC0);
    code2[0] = 0;
    c.snap({{0x10, code2}});
    std::vector<SnapState> snaps;
    std::vector<PageEnt> tab;
    CHECK(!dedupe_snapshot_pages(s.tab.data(), 2, s.pool, s.org, s.code_lo, s.code_hi, c.rs, c.rp, c.rv, c.P, snaps, tab));
}

int main() {
    check_liveness_and_index();
    check_unusable_trace();
    check_dedupe();
    check_dedupe_code_range();
    if (!fails) printf("golden_host_check ok\n");
    return fails ? 1 : 0;
}
