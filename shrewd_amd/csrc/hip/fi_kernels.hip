// fi_kernels.hip -- CDNA4 (gfx950) kernels around the interpreter:
//
//   fi_sample_kernel    fault-site sampler: SplitMix64 keyed by (seed, trial)
//   fi_tick_map_kernel  tick-domain sites: the same draw over ticks, mapped to numInst sites
//   fi_predecode_kernel decodes every halfword of the golden text once
//   fi_hist_kernel      outcome histogram (structure x first-bit x class)
//   fi_exact_*_kernel   exact campaigns: sites by first-access class, the weighted histogram, the dead sites,
//                       the memory words' byte-liveness classes
//   fi_exact_tick_*     exact campaigns in the tick domain: sites by class record, the histogram with 64-bit
//                       weights, the ticks without a trial
//   hipcub radix sort   trials by inject time, so a wave's 64 lanes share the
//                       golden prefix and start at the same snapshot
//
// The interpreter itself (fi_trial_kernel) is in fi_trial.hip.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "fi_types.h"
#include "fi_site_draw.h"
#include "fi_tick_map.h"
#include "fi_exact.h"
#include "fi_exact_tick.h"
#include "fi_device.h"
#include "rv64_isa.h"
#include "fi_softfp.h"
#include "fi_crypto.h"

namespace fi {

// ------------------------------------------------------------------ sampler
__global__ void fi_sample_kernel(SampleCtx c, uint64_t n, fi_site *sites, uint64_t *keys, uint32_t *perm) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SiteDraw d = draw_site(c.d, i, c.golden_ninst);
    fi_site s;
    s.inst = d.when; s.mask = d.mask; s.target = d.target; s.trial = d.trial;
    s.addr = 0;
    if (s.target == FI_T_MEM) {
        const uint64_t w = mulhi64(d.r3, c.n_mem_pages * 512);
        s.addr = c.mem_pages[w / 512] + (w % 512) * 8;
    }
    sites[i] = s;
    keys[i] = s.inst;
    perm[i] = (uint32_t)i;
}

__global__ void fi_keys_kernel(const fi_site *sites, uint64_t n, uint64_t *keys, uint32_t *perm) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = sites[i].inst;
    perm[i] = (uint32_t)i;
}

// ------------------------------------------------------------------ tick-domain sites
// One trial per thread (DESIGN.md §4g "device map"): the tick site -- drawn
// with fi_sample_kernel's draw (fi_site_draw.h), golden_ticks in place of
// numInst, or read from c.in -- is mapped to the numInst site the trial kernels run
// (fi_tick_map.h).  Every trial keeps its slot: disp[i] != 0 (golden-equal,
// escape) is parked by fi_tick_park_kernel and, for an escape, given res[i]
// by fi_tick_fix_kernel.  tsites[i] is the tick site in fi_site layout
// (inst = tick): the histogram files the trial under it.  res[i] is the
// outcome of a disp 1 / 2 trial (zero for disp 0).
__global__ void __launch_bounds__(256) fi_tick_map_kernel(TickMapCtx c, uint64_t n, fi_site *sites, uint64_t *keys,
                                                          uint32_t *perm, fi_site *tsites, uint8_t *disp,
                                                          fi_outcome *res) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fi_site t;   // inst = the tick
    t.addr = 0;
    if (c.in) {
        const fi_tick_site x = c.in[i];
        t.inst = x.tick; t.mask = x.mask; t.target = x.target; t.trial = x.trial;
    } else {
        const SiteDraw d = draw_site(c.d, i, c.golden_ticks);
        t.inst = d.when; t.mask = d.mask; t.target = d.target; t.trial = d.trial;
    }
    const TickMap m = tick_map_site(c.done, c.rec, c.n_att, c.golden_ninst, t.inst, t.target, t.mask, t.trial,
                                    c.literal);
    sites[i] = m.site;
    keys[i] = m.site.inst;
    perm[i] = (uint32_t)i;
    tsites[i] = t;
    disp[i] = (uint8_t)m.disp;
    res[i] = tick_map_outcome(m, c.rec[m.attempt], c.gsub, c.gexit, c.gdetail, c.golden_ninst);
}

// After fi_forward_kernel (or in its place: fill = 1 writes the identity for
// the trials that run): a parked trial is dead at injection, so the trial
// kernels end it at once as the golden run, and it sorts first.
__global__ void fi_tick_park_kernel(const fi_site *sites, const uint8_t *disp, uint64_t n, uint32_t fill,
                                    uint64_t *keys, uint64_t *eff) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (disp[i]) {
        eff[i] = kFwDead;
        keys[i] = 0;
    } else if (fill) {
        eff[i] = sites[i].inst;
    }
}

// Before the histogram and the copy to the host: an escape's outcome.
__global__ void fi_tick_fix_kernel(const uint8_t *disp, const fi_outcome *res, uint64_t n, fi_outcome *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && disp[i] == 2) out[i] = res[i];
}

// First-access forwarding.  A register site (x1..x31) at
// time t is injected at the golden run's next access of that register
// instead: the golden run neither reads nor writes it in between, so the
// trial's machine is the same.  Next access a write (or none): dead, the
// trial is the golden run.  A memory site likewise moves to the next golden
// access of any of its flipped bytes, if its page is mapped at t (present
// in the page table of the snapshot at or before t; the golden run maps and
// unmaps nothing) and it lies outside the text (fetches are not accesses);
// its dead case stays with the kernel (mem_dead).  Sort key = the effective
// time (dead: 0, they end at once).
__device__ __forceinline__ bool fw_mapped(const FwdCtx &c, uint64_t vpn, uint64_t t) {
    const uint64_t k = t / c.snap_interval;
    const SnapState &S = c.snaps[k < c.n_snap ? k : c.n_snap - 1];
    uint32_t lo = S.tab_off, hi = S.tab_off + S.tab_n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (c.snap_tab[mid].vpn < vpn) lo = mid + 1; else hi = mid;
    }
    return lo < S.tab_off + S.tab_n && c.snap_tab[lo].vpn == vpn;
}
__global__ void fi_forward_kernel(const fi_site *sites, uint64_t n, FwdCtx c, uint64_t *keys, uint64_t *eff) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fi_site s = sites[i];
    uint64_t f = s.inst;
    // (a literal tick site, s.addr != 0, is applied where it lands: not forwarded)
    if (s.target >= 1 && s.target <= 31 && s.inst < (1ULL << 29) && !s.addr) {
        const uint32_t key = (uint32_t)(4 * s.inst);   // (2t) << 1: before both events of numInst t
        uint32_t lo = c.reg_off[s.target], hi = c.reg_off[s.target + 1];
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (c.reg_ev[mid] < key) lo = mid + 1; else hi = mid;
        }
        f = (lo == c.reg_off[s.target + 1] || !(c.reg_ev[lo] & 1u)) ? kFwDead : (uint64_t)(c.reg_ev[lo] >> 2);
    } else if (s.target == FI_T_MEM && c.mw_n && !(s.addr < c.text_hi && s.addr + 8 > c.text_lo) &&
               fw_mapped(c, s.addr >> 12, s.inst)) {
        uint32_t fb = 0;
        for (int b = 0; b < 8; b++) fb |= ((s.mask >> (8 * b)) & 0xFF) ? (1u << b) : 0u;
        uint32_t lo = 0, hi = c.mw_n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (c.mw_addr[mid] < s.addr) lo = mid + 1; else hi = mid;
        }
        if (lo < c.mw_n && c.mw_addr[lo] == s.addr) {
            uint32_t a = c.mw_off[lo], b = c.mw_off[lo + 1];
            const uint32_t e = b;
            while (a < b) {   // first event at numInst >= t
                const uint32_t mid = (a + b) >> 1;
                if ((c.mw_ev[mid] >> 16) < s.inst) a = mid + 1; else b = mid;
            }
            for (; a < e; a++) {
                const uint64_t ev = c.mw_ev[a];
                if (((ev >> 8) | ev) & fb & 0xFF) { f = ev >> 16; break; }
            }
        }
    }
    eff[i] = f;
    keys[i] = f == kFwDead ? 0 : f;
}

// ------------------------------------------------------------------ predecode
// One entry per halfword of [text_lo, text_hi).  Fetch follows
// Decoder::moreBytes (src/arch/riscv/decoder.cc:63-116): a 4-byte word at
// pc & ~3; pc % 4 != 0 takes its upper half; a 32-bit instruction starting in
// an upper half needs a second fetch tick (the "straddle").  Odd PCs behave
// like pc | 2 of the same word (handled by the caller's key computation).
__global__ void fi_predecode_kernel(const uint8_t *text, uint64_t code_off, uint64_t code_end, uint64_t nhalf,
                                    PreInst *pre) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nhalf) return;
    const uint64_t off = h * 2;
    const uint64_t bytes = nhalf * 2;
    PreInst p;
    p.flags = 0; p.aux = 0; p.raw = 0; p.op = OP_UNKNOWN; p.rd = p.rs1 = p.rs2 = 0; p.imm = 0; p.len = 2;
    uint32_t raw;
    bool straddle = false, ok = true;
    if ((off & 3) == 0) {
        raw = (uint32_t)text[off] | ((uint32_t)text[off + 1] << 8) | ((uint32_t)text[off + 2] << 16) |
              ((uint32_t)text[off + 3] << 24);
    } else {
        raw = (uint32_t)text[off] | ((uint32_t)text[off + 1] << 8);
        if ((raw & 3) == 3) {
            straddle = true;
            if (off + 4 > bytes) ok = false;   // second word outside the pre-decoded text
            else raw |= ((uint32_t)text[off + 2] << 16) | ((uint32_t)text[off + 3] << 24);
        }
    }
    // only instructions whose bytes lie inside the executable segments: a
    // lane's stores elsewhere in the text pages do not invalidate the table
    if (off < code_off || off + ((raw & 3) == 3 ? 4 : 2) > code_end) ok = false;
    if (ok) {
        Dec d = rv_decode(raw);
        const uint16_t u = uop_of(d);   // may normalise d.imm (c.zext.b/h, c.not)
        p.raw = d.raw; p.op = d.op; p.rd = d.rd; p.rs1 = d.rs1; p.rs2 = d.rs2; p.imm = d.imm; p.len = d.len;
        p.aux = u;
        p.flags = (uint8_t)(kPreValid | (straddle ? kPreStraddle : 0) | d.flags);
    }
    pre[h] = p;
}

// dispatch busy spans (DevCtx::span): every slot's min at ~0 (its max is zeroed by a memset)
__global__ void fi_span_init_kernel(unsigned long long *span, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) span[2 * i] = ~0ULL;
}
__global__ void fi_debug_decode_kernel(const uint32_t *raws, uint64_t n, PreInst *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Dec d = rv_decode(raws[i]);
    PreInst p;
    p.raw = d.raw; p.op = d.op; p.rd = d.rd; p.rs1 = d.rs1; p.rs2 = d.rs2; p.imm = d.imm; p.len = d.len;
    p.aux = d.aux; p.flags = d.flags;
    out[i] = p;
}

// ------------------------------------------------------------------ histogram
// One trial per lane.  The [structure][bit][class] bins are scattered, so each
// lane adds its own bin; everything else is reduced in the wave first: the
// crash / escape sub-codes by ballot + popcount (one wave-uniform count per
// code), the trial and instruction totals by a DPP/shuffle sum, then one
// atomic per wave and counter.
__global__ void __launch_bounds__(256) fi_hist_kernel(const fi_site *sites, const fi_outcome *out, uint64_t n,
                                                      fi_histogram *h) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool v = i < n;
    uint32_t cls = FI_N_CLASS, sub = 0;
    uint64_t ninst = 0;
    if (v) {
        const fi_site s = sites[i];
        const fi_outcome o = out[i];
        const uint32_t t = s.target < FI_N_STRUCT ? s.target : 0;
        const uint32_t bit = s.mask ? (uint32_t)__builtin_ctzll(s.mask) : 0;
        cls = o.cls < FI_N_CLASS ? o.cls : FI_ESCAPE;
        sub = o.sub;
        ninst = o.ninst;
        atomicAdd((unsigned long long *)&h->counts[t][bit][cls], 1ULL);
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t crash = __ballot(cls == FI_CRASH), esc = __ballot(cls == FI_ESCAPE);
    if (crash) {
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t c = (uint32_t)__popcll(crash & __ballot((sub & 15) == k));
            if (c && lane == 0) atomicAdd((unsigned long long *)&h->crash_sub[k], (unsigned long long)c);
        }
    }
    if (esc) {
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t c = (uint32_t)__popcll(esc & __ballot((sub & 7) == k));
            if (c && lane == 0) atomicAdd((unsigned long long *)&h->escape_sub[k], (unsigned long long)c);
        }
    }
    const uint64_t nt = (uint64_t)__popcll(__ballot(v)), ni = wave_sum64(ninst);
    if (lane == 0 && nt) {
        atomicAdd((unsigned long long *)&h->trials, (unsigned long long)nt);
        atomicAdd((unsigned long long *)&h->guest_insts, (unsigned long long)ni);
    }
}

// ------------------------------------------------------------------ exact campaigns
// The sampler's stand-in: thread i takes exact trial first + i (fi_exact.h
// exact_site: the structure's row, the class word -- shared by the nbits
// consecutive lanes of a class -- or the synthesised pc / result class, the
// slot's bit position).  weight[i] = the sites the trial stands for.
__global__ void __launch_bounds__(256) fi_exact_sites_kernel(ExactPlan p, uint64_t first, uint64_t n,
                                                             const uint64_t *classes, fi_site *sites, uint64_t *keys,
                                                             uint32_t *perm, uint32_t *weight) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ExactSite x = exact_site(p, classes, first + i);
    fi_site s;
    s.inst = x.inst; s.mask = x.mask; s.addr = x.addr; s.target = x.target; s.trial = (uint32_t)(first + i);
    sites[i] = s;
    keys[i] = s.inst;
    perm[i] = (uint32_t)i;
    weight[i] = x.weight;
}

// Memory classes (fi_exact.h "Memory words"), built once per golden run and
// (bits, burst) from the memory liveness index.  One thread per index word
// walks its events backwards and stores live_before, a byte per event.
__global__ void __launch_bounds__(256) fi_exact_mem_live_kernel(ExactMemCtx c, uint8_t *live) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= c.mw_n) return;
    const uint32_t a = c.mw_off[w];
    exact_mem_liveness(c.mw_ev + a, c.mw_off[w + 1] - a, live + a);
}
// One thread per (byte set = blockIdx.y, index word) walks the word's events
// forwards (exact_mem_walk).  emit = 0: cnt[set * mw_n + word] = its classes,
// their weights summed per byte set (in the wave first, then one atomic);
// emit = 1: the classes to cls at the scanned counts, each with its consumer
// row when the build is a profiled one (c.proxy != NULL).  A word outside the
// space (a page that is no candidate, an instruction word) has none.
__global__ void __launch_bounds__(256) fi_exact_mem_walk_kernel(ExactMemCtx c, const ExactMemRow *rows,
                                                                const uint8_t *live, uint64_t *cnt,
                                                                unsigned long long *wsum, ExactMemClass *cls,
                                                                uint32_t emit) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
    uint64_t sum = 0;
    if (w < c.mw_n) {
        const uint64_t id = (uint64_t)g * c.mw_n + w;
        uint64_t n = 0;
        if (exact_mem_in_space(c.pages, c.n_pages, c.text_lo, c.text_hi, c.mw_addr[w])) {
            const uint32_t a = c.mw_off[w];
            const uint64_t at = emit ? cnt[id] : 0;
            n = exact_mem_walk(c.mw_ev + a, live + a, c.mw_off[w + 1] - a, c.ninst, rows[g].fmask, w,
                               emit ? cls + at : nullptr, emit ? ~0ULL : 0, &sum, c.proxy ? &c.cons : nullptr, c.proxy, a);
        }
        if (!emit) cnt[id] = n;
    }
    if (emit) return;
    sum = wave_sum64(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&wsum[g], (unsigned long long)sum);
}

// fi_hist_kernel with weights: trial i counts weight[i] times in counts,
// crash_sub, escape_sub and trials, and adds weight[i] x its numInst to
// guest_insts.  An exact chunk's trials fall into the 64 x FI_N_CLASS bins of
// one structure (a few where the chunk crosses into the next), so the bins
// are privatised: the workgroup keeps the table of its first trial's
// structure in LDS (3 KiB: occupancy stays at the 8 waves/SIMD the registers
// allow), lanes of that structure add there, lanes of another one -- a block
// that straddles a segment boundary -- add to global memory directly, and the
// block flushes its non-zero bins with one global atomic each.  Sub-codes and
// totals are summed in the wave first.  Integer adds only: the result does
// not depend on arrival order.  W: uint32_t, a numInst campaign's weights, keyed
// by the run sites; uint64_t, a tick campaign's (tick counts pass 2^32), keyed
// by the tick sites (a pc flip that maps to a write of rd counts under the pc);
// every product and sum is modulo 2^64, so a wave's weights may sum to 0 while
// its instructions do not: the totals' guard tests both.
template <typename W>
__global__ void __launch_bounds__(256) fi_exact_hist_kernel(const fi_site *sites, const fi_outcome *out,
                                                            const W *weight, uint64_t n, fi_histogram *h) {
    __shared__ unsigned long long bins[64 * FI_N_CLASS];
    for (uint32_t b = threadIdx.x; b < 64 * FI_N_CLASS; b += blockDim.x) bins[b] = 0;
    // (the grid covers n: the block's first trial exists; every lane reads the same word)
    uint32_t t0 = sites[(uint64_t)blockIdx.x * blockDim.x].target;
    t0 = t0 < FI_N_STRUCT ? t0 : 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t cls = FI_N_CLASS, sub = 0;
    uint64_t w = 0, wi = 0;
    if (i < n) {
        const fi_site s = sites[i];
        const fi_outcome o = out[i];
        const uint32_t t = s.target < FI_N_STRUCT ? s.target : 0;
        const uint32_t bit = s.mask ? (uint32_t)__builtin_ctzll(s.mask) : 0;
        cls = o.cls < FI_N_CLASS ? o.cls : FI_ESCAPE;
        sub = o.sub;
        w = weight[i];
        wi = w * o.ninst;
        if (t == t0) atomicAdd(&bins[bit * FI_N_CLASS + cls], (unsigned long long)w);
        else atomicAdd((unsigned long long *)&h->counts[t][bit][cls], (unsigned long long)w);
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t crash = __ballot(cls == FI_CRASH), esc = __ballot(cls == FI_ESCAPE);
    if (crash) {
        for (uint32_t k = 0; k < 16; k++) {
            if (!(crash & __ballot((sub & 15) == k))) continue;   // (wave-uniform)
            const uint64_t c = wave_sum64(cls == FI_CRASH && (sub & 15) == k ? w : 0);
            if (c && lane == 0) atomicAdd((unsigned long long *)&h->crash_sub[k], (unsigned long long)c);
        }
    }
    if (esc) {
        for (uint32_t k = 0; k < 8; k++) {
            if (!(esc & __ballot((sub & 7) == k))) continue;
            const uint64_t c = wave_sum64(cls == FI_ESCAPE && (sub & 7) == k ? w : 0);
            if (c && lane == 0) atomicAdd((unsigned long long *)&h->escape_sub[k], (unsigned long long)c);
        }
    }
    const uint64_t nt = wave_sum64(w), ni = wave_sum64(wi);
    if (lane == 0 && (nt | ni)) {
        atomicAdd((unsigned long long *)&h->trials, (unsigned long long)nt);
        atomicAdd((unsigned long long *)&h->guest_insts, (unsigned long long)ni);
    }
    __syncthreads();
    unsigned long long *g = (unsigned long long *)&h->counts[t0][0][0];
    for (uint32_t b = threadIdx.x; b < 64 * FI_N_CLASS; b += blockDim.x)
        if (bins[b]) atomicAdd(&g[b], bins[b]);
}

// The profile (DESIGN.md §4j "Profile"): thread i recomputes exact trial
// first + i's class as fi_exact_sites_kernel does, takes the row the class is
// charged to (exact_trial_consumer) and adds weight[i] to prof[row][group][cls].
// A hot loop sends most of a campaign to a handful of rows, so the adds are
// combined before they reach global memory:
//  1. in the wave: equal (row, group, class) keys of consecutive lanes -- the
//     nbits lanes of a class share the row, a loop's classes repeat it -- are
//     summed by a segmented scan over the runs (a wave boundary cuts a run)
//     and only a run's last lane goes on;
//  2. in the workgroup: an LDS table of kProfSlots rows, kProfBins bins each
//     (6 KiB + the tags: eight workgroups a CU, the 32 waves the registers
//     allow, use 49 of its 160 KiB); a row claims a slot at row % kProfSlots
//     or one of the next kProfProbes - 1 by compare-and-swap on the tag; a
//     lane whose row finds none adds to global memory directly;
//  3. the block flushes its non-zero bins with one global atomic each.
// variant (fi_debug_set_profile_variant): 1 skips step 2, 2 skips 1 and 2.
// Integer adds only: the bins do not depend on arrival order or the variant.
__global__ void __launch_bounds__(256) fi_exact_profile_kernel(ExactPlan p, ExactProfCtx c, uint64_t first,
                                                               uint64_t n) {
    __shared__ unsigned long long bins[kProfSlots * kProfBins];
    __shared__ uint32_t tag[kProfSlots];
    for (uint32_t b = threadIdx.x; b < kProfSlots * kProfBins; b += blockDim.x) bins[b] = 0;
    if (threadIdx.x < kProfSlots) tag[threadIdx.x] = kExactNoConsumer;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t key = kExactNoConsumer;   // row * kProfBins + group * FI_N_CLASS + cls
    uint64_t w = 0;
    if (i < n) {
        uint32_t group;
        const uint32_t row = exact_trial_consumer(p, c.reg_cons, c.inst_row, first + i, &group);
        const uint32_t cls = c.out[i].cls < FI_N_CLASS ? c.out[i].cls : (uint32_t)FI_ESCAPE;
        if (row < c.n_rows) {   // (always: a class has a consumer)
            key = row * kProfBins + group * FI_N_CLASS + cls;
            w = c.weight[i];
        }
    }
    bool add = key != kExactNoConsumer;
    if (c.variant < 2) {
        const uint32_t lane = threadIdx.x & 63;
        const uint32_t up = __shfl_up(key, 1, 64);
        const uint64_t heads = __ballot(lane == 0 || up != key);   // the runs' first lanes (bit 0 is set)
        const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ULL >> (63u - lane)));
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t v = (uint64_t)__shfl_up((unsigned long long)w, d, 64);
            if (lane >= start + d) w += v;
        }
        add = add && (lane == 63 || ((heads >> (lane + 1)) & 1));   // the run's last lane has its sum
    }
    if (add) {
        const uint32_t row = key / kProfBins, bin = key - row * kProfBins;
        bool done = false;
        if (c.variant == 0) {
            uint32_t s = row & (kProfSlots - 1);
            for (uint32_t k = 0; k < kProfProbes && !done; k++, s = (s + 1) & (kProfSlots - 1)) {
                uint32_t old = ((volatile uint32_t *)tag)[s];   // (a tag, once set, stays)
                if (old == kExactNoConsumer) old = atomicCAS(&tag[s], kExactNoConsumer, row);
                if (old == kExactNoConsumer || old == row) {
                    atomicAdd(&bins[s * kProfBins + bin], (unsigned long long)w);
                    done = true;
                }
            }
        }
        if (!done) atomicAdd(&c.prof[key], (unsigned long long)w);
    }
    if (c.variant) return;   // (wave-uniform: the table is unused)
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kProfSlots * kProfBins; b += blockDim.x)
        if (bins[b]) atomicAdd(&c.prof[(uint64_t)tag[b / kProfBins] * kProfBins + b % kProfBins], bins[b]);
}
// fi_exact_consumers: the row of each of trials [first, first + n)
__global__ void __launch_bounds__(256) fi_exact_consumers_kernel(ExactPlan p, const uint32_t *reg_cons,
                                                                 const uint32_t *inst_row, uint64_t first, uint64_t n,
                                                                 uint32_t *row) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t group;
    row[i] = exact_trial_consumer(p, reg_cons, inst_row, first + i, &group);
}

// What an exact campaign counts without a trial (fi_exact.h ExactUntried):
// block r < 32, thread b adds register r's masked sites to
// counts[r][b][FI_MASKED] and its escaped ones to counts[r][b][FI_ESCAPE] for
// every eligible b, block 32 the dead (word, t) pairs of b's byte set to
// counts[FI_T_MEM][b][FI_MASKED]; the totals by one thread.
__global__ void __launch_bounds__(64) fi_exact_untried_kernel(ExactUntried d, fi_histogram *h) {
    const uint32_t r = blockIdx.x, b = threadIdx.x;
    const uint32_t t = r < 32 ? r : (uint32_t)FI_T_MEM;
    const uint64_t m = r < 32 ? d.masked[r] : d.mem_masked[b], x = r < 32 ? d.escaped[r] : 0;
    if ((d.bits >> b) & 1) {
        if (m) atomicAdd((unsigned long long *)&h->counts[t][b][FI_MASKED], (unsigned long long)m);
        if (x) atomicAdd((unsigned long long *)&h->counts[t][b][FI_ESCAPE], (unsigned long long)x);
    }
    if (r == 0 && b == 0 && d.total) {
        atomicAdd((unsigned long long *)&h->trials, (unsigned long long)d.total);
        atomicAdd((unsigned long long *)&h->guest_insts, (unsigned long long)d.insts);
        if (d.esc_total) atomicAdd((unsigned long long *)&h->escape_sub[FI_ESC_TIMING], (unsigned long long)d.esc_total);
    }
}

// ------------------------------------------------------------------ exact campaigns, tick domain
// fi_exact_sites_kernel's counterpart over the tick classes (fi_exact_tick.h
// exact_tick_site): thread i takes exact tick trial first + i -- the class
// record shared by the nbits consecutive lanes of a class; an interval class
// is a plain site, every other one goes through tick_map_site -- and writes
// what fi_tick_map_kernel writes (the site, the tick site in fi_site layout,
// disp, a disp 1 / 2 trial's outcome) plus the ticks the trial stands for.
__global__ void __launch_bounds__(256) fi_exact_tick_sites_kernel(ExactPlan p, TickMapCtx c, uint64_t first, uint64_t n,
                                                                  const ExactTickClass *cls, fi_site *sites,
                                                                  uint64_t *keys, uint32_t *perm, fi_site *tsites,
                                                                  uint8_t *disp, fi_outcome *res, uint64_t *weight) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ExactTickSite x = exact_tick_site(p, cls, c, first + i);
    fi_site t;   // inst = the tick
    t.inst = x.tsite.tick; t.mask = x.tsite.mask; t.addr = 0; t.target = x.tsite.target; t.trial = x.tsite.trial;
    sites[i] = x.site;
    keys[i] = x.site.inst;
    perm[i] = (uint32_t)i;
    tsites[i] = t;
    disp[i] = (uint8_t)x.disp;
    res[i] = x.res;
    weight[i] = x.weight;
}

// Epochs: sort keys of the suspended lanes (their pc: lanes of one loop end
// up in the same wave); entries past the survivor count sort last.
// Survivor sort key: pc offset from the text base (low 32 bits) above the
// low 32 bits of numInst, so that survivors standing at the same pc are
// adjacent and ordered by progress.  With n_odd (a solo-odd launch follows)
// the key is shifted down one bit under a top bit set for odd pcs, so that
// the odd-pc survivors sort last, and they are counted.
// solo != 0: the next epoch runs one trial per wave, where the order only
// decides when a trial starts: trials that rewrote their code (interpreted at
// ~20x the cost of translated code) start first, then the rest longest-first.
// The work-left estimate of a solo trial: the golden run's remaining length
// (the trial follows its path, the usual case: a wrong value carried to the
// end), or, when the trial stands in a counted loop of the golden text, that
// loop's remaining passes times its length if larger (a flipped bound, counter
// or pointer that stretches the loop: profiles/r05tl_solo_timeline_crc32.jsonl,
// the late starters); capped at the hang cap.
__device__ __forceinline__ uint64_t solo_work_left(const LaneSave &s, uint64_t text_lo, uint64_t golden_ninst,
                                                  const LoopEst *loops, uint32_t n_loops, uint64_t hang_cap) {
    uint64_t w = s.ninst < golden_ninst ? golden_ninst - s.ninst : 0;
    const uint64_t off = s.pc - text_lo;
    for (uint32_t i = 0; i < n_loops; i++) {
        const LoopEst L = loops[i];
        if (off < L.lo || off >= L.hi) continue;
        const uint64_t x = s.regs[L.reg] - (L.treg ? s.regs[L.treg] : 0ULL);
        const uint64_t d = L.step < 0 ? x : 0 - x;
        const uint32_t a = (uint32_t)(L.step < 0 ? -L.step : L.step);
        const uint64_t n = (d & (a - 1)) ? ~0ULL : (d / a ? d / a : ~0ULL);   // (fi_trial.hip loop_passes)
        const uint64_t e = n > (hang_cap / (L.m ? L.m : 1)) ? hang_cap : n * L.m;
        w = e > w ? e : w;
        break;
    }
    const uint64_t left = s.ninst < hang_cap ? hang_cap - s.ninst : 0;
    return w < left ? w : left;
}

__global__ void fi_surv_keys_kernel(const LaneSave *save, const uint32_t *list, const uint32_t *cnt, uint64_t cap,
                                    uint64_t text_lo, uint64_t *keys, uint32_t *vals, uint32_t *n_odd,
                                    uint32_t solo, uint64_t golden_ninst, uint32_t nb, const LoopEst *loops,
                                    uint32_t n_loops, uint64_t hang_cap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    if (i < *cnt) {
        const uint32_t sl = list[i];
        const uint64_t pc = save[sl].pc;
        uint64_t k = ((pc - text_lo) << 32) | (save[sl].ninst & 0xFFFFFFFFu);
        // solo epoch: code-rewriting survivors and those already past the
        // golden run's end first (the first are interpreted, the second went
        // somewhere the golden run did not -- a re-run of the program, a loop
        // to the hang cap: profiles/r04v_solo_timeline_crc32.jsonl), then
        // longest-first -- the fewest committed instructions have the most
        // left to run (golden suffix or hang cap); one survivor per wave, so
        // no pc grouping (profiles/r03k_ab_lpt.jsonl: crc32 +4 %, intmix +5 %)
        if (solo) {
            const bool first = ((save[sl].flags >> 3) & 1) || save[sl].ninst > golden_ninst;
            // (solo bit 1: survivors not yet injected -- their outcome still
            // unknown -- form a tier of their own after the first)
            const bool uninj = (solo & 2u) && ((save[sl].flags >> 1) & 3) == 0;
            // (nb: the bits of the hang cap, above every survivor's numInst --
            // the key then sorts in nb + 2 (+ 1 odd) bits: fewer radix passes)
            // (tier 2: the most work left first, by the estimate below the cap)
            const uint64_t low = (first || uninj || !n_loops)
                                     ? save[sl].ninst
                                     : ((1ULL << nb) - 1) - solo_work_left(save[sl], text_lo, golden_ninst, loops,
                                                                          n_loops, hang_cap);
            k = ((uint64_t)(first ? 0 : uninj ? 1 : 2) << nb) | low;
        }
        if (n_odd) {
            k = solo ? (((pc & 1) << (nb + 2)) | k) : (((pc & 1) << 63) | (k >> 1));
            if (pc & 1) atomicAdd(n_odd, 1u);
        }
        keys[i] = k;
        vals[i] = sl;
    } else {
        keys[i] = ~0ULL;
        vals[i] = 0;
    }
}

// The solo kernel's share of a sorted survivor list whose odd-pc survivors
// come last: all but the last min(n_odd, grid), which the solo-odd kernel's
// grid takes.
__global__ void fi_odd_split_kernel(const uint32_t *cnt, const uint32_t *n_odd, uint32_t *split, uint32_t grid) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const uint32_t o = *n_odd < grid ? *n_odd : grid;
        *split = *cnt - o;
    }
}

// Packed resume: a wave starts at every sorted survivor whose pc differs from
// its predecessor's, and at every 64th position; it ends at the next start.
// Waves are numbered in atomic order (any order is correct: waves are
// independent).
__global__ void fi_pack_runs_kernel(const uint64_t *keys, const uint32_t *cnt, uint64_t cap, uint32_t *wrange,
                                    uint32_t *n_waves) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = *cnt;
    if (i >= n) return;
    const uint32_t pc = (uint32_t)(keys[i] >> 32);
    if (i != 0 && (i & 63) != 0 && (uint32_t)(keys[i - 1] >> 32) == pc) return;
    uint32_t e = (uint32_t)i + 1;
    while (e < n && (e & 63) != 0 && (uint32_t)(keys[e] >> 32) == pc) e++;
    const uint32_t w = atomicAdd(n_waves, 1u);
    wrange[2 * w] = (uint32_t)i;
    wrange[2 * w + 1] = e;
}

// Second pass of the trials that ran out of private pages (fi_engine.cpp
// chunk_begin / chunk_end): list them, gather their sites densely, scatter the new outcomes.
// (A resource escape with exit code 1 hit a table bound -- the VMA list, the
// getrandom stream -- that more pages would not lift: fi_trial.hip kEscTable.)
__global__ void fi_redo_collect_kernel(const fi_outcome *out, uint64_t n, uint32_t *idx, uint32_t *cnt,
                                       unsigned long long *stats) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fi_outcome o = out[i];
    if (o.cls == FI_ESCAPE && o.sub == FI_ESC_RESOURCE && o.exit_code == 0) {
        idx[atomicAdd(cnt, 1u)] = (uint32_t)i;
        atomicAdd(&stats[ST_REDO_TRIALS], 1ull);
    }
}
__global__ void fi_redo_gather_kernel(const fi_site *sites, const uint32_t *idx, uint64_t n, fi_site *rsites,
                                      uint64_t *keys, uint32_t *perm) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const fi_site s = sites[idx[j]];
    rsites[j] = s;
    keys[j] = s.inst;
    perm[j] = (uint32_t)j;
}
__global__ void fi_redo_scatter_kernel(const uint32_t *idx, uint64_t n, const fi_outcome *rout, fi_outcome *out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[idx[j]] = rout[j];
}

// Output capture (fi_run_sites_capture).  Rows of `stride`
// bytes (a multiple of 16), one per trial of the chunk and stream; one thread
// per 16-byte piece of a row, so a wave stores 1 KiB contiguously.
// Before the pass: every row = the first cap bytes of the golden stream,
// zeros after -- a golden byte sits at the same offset in a trial's stream
// whether the trial started after it (snapshot start) or ended before it
// (the golden-suffix ends), so neither case copies a byte later.
__global__ void __launch_bounds__(256) fi_capture_init_kernel(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap,
                                                              const uint8_t *gold, uint64_t glen) {
    const uint32_t per = stride / 16;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const uint64_t o = (i % per) * 16;
    const uint64_t lim = glen < cap ? glen : cap;   // golden bytes a row holds
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o + 16 <= lim) {
        v = *(const uint4 *)(gold + o);   // (gold is the start of an allocation: 16-byte aligned)
    } else if (o < lim) {
        uint32_t wds[4] = {0, 0, 0, 0};
        for (uint64_t b = o; b < lim; b++) wds[(b - o) >> 2] |= (uint32_t)gold[b] << (8 * ((b - o) & 3));
        v = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    }
    *(uint4 *)(rows + i * 16) = v;
}
// After the pass and its second pass: zeros from min(len, cap) to the end of
// each row (the golden bytes a shorter trial never reached), so that the
// returned bytes are a function of the site alone.  err = 0: stdout rows.
__global__ void __launch_bounds__(256) fi_capture_finish_kernel(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap,
                                                                const fi_stream_len *lens, uint32_t err) {
    const uint32_t per = stride / 16;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const uint64_t o = (i % per) * 16;
    const fi_stream_len sl = lens[i / per];
    uint64_t len = err ? sl.err_len : sl.out_len;
    if (len > cap) len = cap;
    if (o + 16 <= len) return;
    uint4 *p = (uint4 *)(rows + i * 16);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o < len) {
        v = *p;
        uint32_t wds[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t b = (uint32_t)(len - o); b < 16; b++) wds[b >> 2] &= ~(0xFFu << (8 * (b & 3)));
        v = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    }
    *p = v;
}

__global__ void fi_hist_stats_kernel(const unsigned long long *stats, fi_histogram *h) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        h->fetch_bytes += stats[ST_FETCH_BYTES];
        h->data_bytes += stats[ST_DATA_BYTES];
        h->cow_pages += stats[ST_PAGES];
        h->device_insts += stats[ST_DEVICE_INSTS];
    }
}

// ------------------------------------------------------------------ launch wrappers (host side)
static inline unsigned nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

hipError_t launch_sample(const SampleCtx &c, uint64_t n, fi_site *sites, uint64_t *keys, uint32_t *perm,
                         hipStream_t st) {
    hipLaunchKernelGGL(fi_sample_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, c, n, sites, keys, perm);
    return hipGetLastError();
}
hipError_t launch_forward(const fi_site *sites, uint64_t n, const FwdCtx &c, uint64_t *keys, uint64_t *eff,
                          hipStream_t st) {
    hipLaunchKernelGGL(fi_forward_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, sites, n, c, keys, eff);
    return hipGetLastError();
}
hipError_t launch_keys(const fi_site *sites, uint64_t n, uint64_t *keys, uint32_t *perm, hipStream_t st) {
    hipLaunchKernelGGL(fi_keys_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, sites, n, keys, perm);
    return hipGetLastError();
}
hipError_t launch_tick_map(const TickMapCtx &c, uint64_t n, fi_site *sites, uint64_t *keys, uint32_t *perm,
                           fi_site *tsites, uint8_t *disp, fi_outcome *res, hipStream_t st) {
    hipLaunchKernelGGL(fi_tick_map_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, c, n, sites, keys, perm, tsites, disp,
                       res);
    return hipGetLastError();
}
hipError_t launch_tick_park(const fi_site *sites, const uint8_t *disp, uint64_t n, uint32_t fill, uint64_t *keys,
                            uint64_t *eff, hipStream_t st) {
    hipLaunchKernelGGL(fi_tick_park_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, sites, disp, n, fill, keys, eff);
    return hipGetLastError();
}
hipError_t launch_tick_fix(const uint8_t *disp, const fi_outcome *res, uint64_t n, fi_outcome *out, hipStream_t st) {
    hipLaunchKernelGGL(fi_tick_fix_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, disp, res, n, out);
    return hipGetLastError();
}
hipError_t launch_predecode(const uint8_t *text, uint64_t code_off, uint64_t code_end, uint64_t nhalf, PreInst *pre,
                           hipStream_t st) {
    hipLaunchKernelGGL(fi_predecode_kernel, dim3(nblk(nhalf, 256)), dim3(256), 0, st, text, code_off, code_end, nhalf,
                       pre);
    return hipGetLastError();
}
hipError_t launch_span_init(unsigned long long *span, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(fi_span_init_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, span, n);
    return hipGetLastError();
}
hipError_t launch_debug_decode(const uint32_t *raws, uint64_t n, PreInst *out, hipStream_t st) {
    hipLaunchKernelGGL(fi_debug_decode_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, raws, n, out);
    return hipGetLastError();
}
hipError_t launch_hist(const fi_site *sites, const fi_outcome *out, uint64_t n, fi_histogram *h,
                       const unsigned long long *stats, hipStream_t st) {
    hipLaunchKernelGGL(fi_hist_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, sites, out, n, h);
    if (stats) hipLaunchKernelGGL(fi_hist_stats_kernel, dim3(1), dim3(64), 0, st, stats, h);
    return hipGetLastError();
}
hipError_t launch_exact_sites(const ExactPlan &p, uint64_t first, uint64_t n, const uint64_t *classes, fi_site *sites,
                              uint64_t *keys, uint32_t *perm, uint32_t *weight, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_sites_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, p, first, n, classes, sites, keys,
                       perm, weight);
    return hipGetLastError();
}
template <typename W>
hipError_t launch_exact_hist(const fi_site *sites, const fi_outcome *out, const W *weight, uint64_t n, fi_histogram *h,
                             hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_hist_kernel<W>, dim3(nblk(n, 256)), dim3(256), 0, st, sites, out, weight, n, h);
    return hipGetLastError();
}
template hipError_t launch_exact_hist(const fi_site *, const fi_outcome *, const uint32_t *, uint64_t, fi_histogram *,
                                      hipStream_t);
template hipError_t launch_exact_hist(const fi_site *, const fi_outcome *, const uint64_t *, uint64_t, fi_histogram *,
                                      hipStream_t);
hipError_t launch_exact_profile(const ExactPlan &p, const ExactProfCtx &c, uint64_t first, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_profile_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, p, c, first, n);
    return hipGetLastError();
}
hipError_t launch_exact_consumers(const ExactPlan &p, const uint32_t *reg_cons, const uint32_t *inst_row,
                                  uint64_t first, uint64_t n, uint32_t *row, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_consumers_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, p, reg_cons, inst_row, first, n,
                       row);
    return hipGetLastError();
}
hipError_t launch_exact_untried(const ExactUntried &d, fi_histogram *h, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_untried_kernel, dim3(33), dim3(64), 0, st, d, h);
    return hipGetLastError();
}
hipError_t launch_exact_tick_sites(const ExactPlan &p, const TickMapCtx &c, uint64_t first, uint64_t n,
                                   const ExactTickClass *cls, fi_site *sites, uint64_t *keys, uint32_t *perm,
                                   fi_site *tsites, uint8_t *disp, fi_outcome *res, uint64_t *weight, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_tick_sites_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, p, c, first, n, cls, sites,
                       keys, perm, tsites, disp, res, weight);
    return hipGetLastError();
}
hipError_t launch_exact_mem_live(const ExactMemCtx &c, uint8_t *live, hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_mem_live_kernel, dim3(nblk(c.mw_n, 256)), dim3(256), 0, st, c, live);
    return hipGetLastError();
}
hipError_t launch_exact_mem_walk(const ExactMemCtx &c, const ExactMemRow *rows, uint32_t n_rows, const uint8_t *live,
                                 uint64_t *cnt, unsigned long long *wsum, ExactMemClass *cls, uint32_t emit,
                                 hipStream_t st) {
    hipLaunchKernelGGL(fi_exact_mem_walk_kernel, dim3(nblk(c.mw_n, 256), n_rows), dim3(256), 0, st, c, rows, live, cnt,
                       wsum, cls, emit);
    return hipGetLastError();
}
hipError_t scan_u64_bytes(uint64_t n, size_t &bytes) {
    bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n);
}
hipError_t scan_u64(void *tmp, size_t bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t st) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, st);
}
hipError_t launch_hist_stats(const unsigned long long *stats, fi_histogram *h, hipStream_t st) {
    hipLaunchKernelGGL(fi_hist_stats_kernel, dim3(1), dim3(64), 0, st, stats, h);
    return hipGetLastError();
}
hipError_t launch_redo_collect(const fi_outcome *out, uint64_t n, uint32_t *idx, uint32_t *cnt,
                               unsigned long long *stats, hipStream_t st) {
    hipLaunchKernelGGL(fi_redo_collect_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, out, n, idx, cnt, stats);
    return hipGetLastError();
}
hipError_t launch_redo_gather(const fi_site *sites, const uint32_t *idx, uint64_t n, fi_site *rsites, uint64_t *keys,
                              uint32_t *perm, hipStream_t st) {
    hipLaunchKernelGGL(fi_redo_gather_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, sites, idx, n, rsites, keys, perm);
    return hipGetLastError();
}
hipError_t launch_redo_scatter(const uint32_t *idx, uint64_t n, const fi_outcome *rout, fi_outcome *out,
                               hipStream_t st) {
    hipLaunchKernelGGL(fi_redo_scatter_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, idx, n, rout, out);
    return hipGetLastError();
}
hipError_t launch_capture_init(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap, const uint8_t *gold,
                               uint64_t glen, hipStream_t st) {
    hipLaunchKernelGGL(fi_capture_init_kernel, dim3(nblk(n * (stride / 16), 256)), dim3(256), 0, st, rows, n, stride,
                       cap, gold, glen);
    return hipGetLastError();
}
hipError_t launch_capture_finish(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap, const fi_stream_len *lens,
                                 uint32_t err, hipStream_t st) {
    hipLaunchKernelGGL(fi_capture_finish_kernel, dim3(nblk(n * (stride / 16), 256)), dim3(256), 0, st, rows, n, stride,
                       cap, lens, err);
    return hipGetLastError();
}
hipError_t launch_surv_keys(const LaneSave *save, const uint32_t *list, const uint32_t *cnt, uint64_t cap,
                            uint64_t text_lo, uint64_t *keys, uint32_t *vals, uint32_t *n_odd, uint32_t solo,
                            uint64_t golden_ninst, uint32_t nb, const LoopEst *loops, uint32_t n_loops,
                            uint64_t hang_cap, hipStream_t st) {
    hipLaunchKernelGGL(fi_surv_keys_kernel, dim3(nblk(cap, 256)), dim3(256), 0, st, save, list, cnt, cap, text_lo,
                       keys, vals, n_odd, solo, golden_ninst, nb, loops, n_loops, hang_cap);
    return hipGetLastError();
}
hipError_t launch_odd_split(const uint32_t *cnt, const uint32_t *n_odd, uint32_t *split, uint32_t grid,
                            hipStream_t st) {
    hipLaunchKernelGGL(fi_odd_split_kernel, dim3(1), dim3(64), 0, st, cnt, n_odd, split, grid);
    return hipGetLastError();
}
hipError_t launch_pack_runs(const uint64_t *keys, const uint32_t *cnt, uint64_t cap, uint32_t *wrange,
                            uint32_t *n_waves, hipStream_t st) {
    hipLaunchKernelGGL(fi_pack_runs_kernel, dim3(nblk(cap, 256)), dim3(256), 0, st, keys, cnt, cap, wrange, n_waves);
    return hipGetLastError();
}
hipError_t sort_pairs_bytes(uint64_t n, size_t &bytes) {
    bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                              (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n);
}
hipError_t sort_pairs(void *tmp, size_t bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                      uint32_t *vout, uint64_t n, int end_bit, hipStream_t st) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)n, 0, end_bit, st);
}

}  // namespace fi

// ------------------------------------------------------------------ FP port
// The engine's IEEE arithmetic (fi_softfp.h) run on vectors of operands, on
// the host or on the device, for the pinning tests against the reference's
// SoftFloat (tests/test_softfp.py).
namespace fi {
__global__ void softfp_kernel(int op, int fmt, int rm, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                              uint64_t n, uint64_t *out, uint32_t *fl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 0;
    out[i] = sf::op(op, fmt, rm, a[i], b[i], c[i], f);
    fl[i] = f;
}
}  // namespace fi

extern "C" fi_status fi_debug_softfp(int op, int fmt, int rm, const uint64_t *a, const uint64_t *b,
                                     const uint64_t *c, uint64_t n, uint64_t *out, uint32_t *fl, int on_device) {
    if (op < 0 || op >= fi::sf::OP_COUNT || fmt < 0 || fmt > 2 || rm < 0 || rm > 4 || !a || !b || !c || !out || !fl)
        return FI_E_ARG;
    if (!on_device) {
        for (uint64_t i = 0; i < n; i++) {
            uint32_t f = 0;
            out[i] = fi::sf::op(op, fmt, rm, a[i], b[i], c[i], f);
            fl[i] = f;
        }
        return FI_OK;
    }
    if (!n) return FI_OK;
    uint64_t *d = nullptr;
    if (hipMalloc(&d, n * 8 * 4 + n * 4) != hipSuccess) return FI_E_HIP;
    uint64_t *da = d, *db = d + n, *dc = d + 2 * n, *dout = d + 3 * n;
    uint32_t *dfl = (uint32_t *)(d + 4 * n);
    hipError_t err = hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dc, c, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(fi::softfp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, fmt, rm, da, db,
                           dc, n, dout, dfl);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(fl, dfl, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return err == hipSuccess ? FI_OK : FI_E_HIP;
}

// ------------------------------------------------------------- crypto port
// The engine's scalar-crypto port (fi_crypto.h) over operand vectors, on the
// host or on the device, for the pinning test against the reference's rvk.hh
// (tests/test_crypto.py).
namespace fi {
__global__ void crypto_kernel(int fn, const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rvk::exec(fn, a[i], b[i]);
}
}  // namespace fi

extern "C" fi_status fi_debug_crypto(int fn, const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *out,
                                     int on_device) {
    if ((fn & 0xFF) > 21 || !a || !b || !out) return FI_E_ARG;
    if (!on_device) {
        for (uint64_t i = 0; i < n; i++) out[i] = fi::rvk::exec(fn, a[i], b[i]);
        return FI_OK;
    }
    if (!n) return FI_OK;
    uint64_t *d = nullptr;
    if (hipMalloc(&d, n * 8 * 3) != hipSuccess) return FI_E_HIP;
    hipError_t err = hipMemcpy(d, a, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d + n, b, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(fi::crypto_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, d, d + n, n,
                           d + 2 * n);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(out, d + 2 * n, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return err == hipSuccess ? FI_OK : FI_E_HIP;
}
