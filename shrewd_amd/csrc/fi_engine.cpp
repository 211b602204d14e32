// fi_engine.cpp -- host side of the MI355X fault-injection engine (C ABI in
// include/fi_engine.h).
//
// Host responsibilities are the ones gem5 performs once per run before the
// tick loop starts: load the static ELF and build the SE process image
// (src/base/loader/elf_object.cc:374-404, src/sim/process.cc:289-306,
// src/arch/riscv/process.cc:71-261), then hand everything to the device.
// Every guest instruction -- golden run included -- executes in the HIP
// kernels (hip/fi_kernels.hip).  There is no CPU interpreter here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "fi_capture.h"
#include "fi_checkpoint.h"
#include "fi_debug.h"
#include "fi_exact.h"
#include "fi_exact_tick.h"
#include "fi_golden_host.h"
#include "fi_site_draw.h"
#include "fi_tick.h"
#include "fi_tick_map.h"
#include "fi_types.h"
#include "rv64_isa.h"

constexpr uint64_t kRndLen = 1ULL << 20;   // getrandom bytes precomputed per engine

namespace fi {
hipError_t launch_sample(const SampleCtx &c, uint64_t n, fi_site *sites, uint64_t *keys, uint32_t *perm,
                         hipStream_t st);
hipError_t launch_keys(const fi_site *sites, uint64_t n, uint64_t *keys, uint32_t *perm, hipStream_t st);
hipError_t launch_tick_map(const TickMapCtx &c, uint64_t n, fi_site *sites, uint64_t *keys, uint32_t *perm,
                           fi_site *tsites, uint8_t *disp, fi_outcome *res, hipStream_t st);
hipError_t launch_tick_park(const fi_site *sites, const uint8_t *disp, uint64_t n, uint32_t fill, uint64_t *keys,
                            uint64_t *eff, hipStream_t st);
hipError_t launch_tick_fix(const uint8_t *disp, const fi_outcome *res, uint64_t n, fi_outcome *out, hipStream_t st);
hipError_t launch_forward(const fi_site *sites, uint64_t n, const FwdCtx &c, uint64_t *keys, uint64_t *eff,
                          hipStream_t st);
hipError_t launch_predecode(const uint8_t *text, uint64_t code_off, uint64_t code_end, uint64_t nhalf, PreInst *pre,
                           hipStream_t st);
hipError_t launch_debug_decode(const uint32_t *raws, uint64_t n, PreInst *out, hipStream_t st);
hipError_t launch_trials(const DevCtx &c, hipStream_t st);
hipError_t launch_trials_solo(const DevCtx &c, hipStream_t st);
hipError_t launch_span_init(unsigned long long *span, uint64_t n, hipStream_t st);
hipError_t launch_debug_loop(const DevCtx &c, const fi_debug_loop *in, uint64_t n, fi_debug_loop_out *out,
                             hipStream_t st);
hipError_t launch_hist(const fi_site *sites, const fi_outcome *out, uint64_t n, fi_histogram *h,
                       const unsigned long long *stats, hipStream_t st);
hipError_t launch_hist_stats(const unsigned long long *stats, fi_histogram *h, hipStream_t st);
hipError_t launch_exact_sites(const ExactPlan &p, uint64_t first, uint64_t n, const uint64_t *classes, fi_site *sites,
                              uint64_t *keys, uint32_t *perm, uint32_t *weight, hipStream_t st);
template <typename W>   // uint32_t or uint64_t weights (instantiated in fi_kernels.hip)
hipError_t launch_exact_hist(const fi_site *sites, const fi_outcome *out, const W *weight, uint64_t n, fi_histogram *h,
                             hipStream_t st);
hipError_t launch_exact_profile(const ExactPlan &p, const ExactProfCtx &c, uint64_t first, uint64_t n, hipStream_t st);
hipError_t launch_exact_consumers(const ExactPlan &p, const uint32_t *reg_cons, const uint32_t *inst_row,
                                  uint64_t first, uint64_t n, uint32_t *row, hipStream_t st);
hipError_t launch_exact_untried(const ExactUntried &d, fi_histogram *h, hipStream_t st);
hipError_t launch_exact_tick_sites(const ExactPlan &p, const TickMapCtx &c, uint64_t first, uint64_t n,
                                   const ExactTickClass *cls, fi_site *sites, uint64_t *keys, uint32_t *perm,
                                   fi_site *tsites, uint8_t *disp, fi_outcome *res, uint64_t *weight, hipStream_t st);
hipError_t launch_exact_mem_live(const ExactMemCtx &c, uint8_t *live, hipStream_t st);
hipError_t launch_exact_mem_walk(const ExactMemCtx &c, const ExactMemRow *rows, uint32_t n_rows, const uint8_t *live,
                                 uint64_t *cnt, unsigned long long *wsum, ExactMemClass *cls, uint32_t emit,
                                 hipStream_t st);
hipError_t scan_u64_bytes(uint64_t n, size_t &bytes);
hipError_t scan_u64(void *tmp, size_t bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t st);
hipError_t sort_pairs_bytes(uint64_t n, size_t &bytes);
hipError_t launch_pack_runs(const uint64_t *keys, const uint32_t *cnt, uint64_t cap, uint32_t *wrange,
                            uint32_t *n_waves, hipStream_t st);
hipError_t launch_redo_collect(const fi_outcome *out, uint64_t n, uint32_t *idx, uint32_t *cnt,
                               unsigned long long *stats, hipStream_t st);
hipError_t launch_redo_gather(const fi_site *sites, const uint32_t *idx, uint64_t n, fi_site *rsites, uint64_t *keys,
                              uint32_t *perm, hipStream_t st);
hipError_t launch_redo_scatter(const uint32_t *idx, uint64_t n, const fi_outcome *rout, fi_outcome *out,
                               hipStream_t st);
hipError_t launch_capture_init(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap, const uint8_t *gold,
                               uint64_t glen, hipStream_t st);
hipError_t launch_capture_finish(uint8_t *rows, uint64_t n, uint32_t stride, uint32_t cap, const fi_stream_len *lens,
                                 uint32_t err, hipStream_t st);
hipError_t launch_surv_keys(const LaneSave *save, const uint32_t *list, const uint32_t *cnt, uint64_t cap,
                            uint64_t text_lo, uint64_t *keys, uint32_t *vals, uint32_t *n_odd, uint32_t solo,
                            uint64_t golden_ninst, uint32_t nb, const LoopEst *loops, uint32_t n_loops,
                            uint64_t hang_cap, hipStream_t st);
hipError_t launch_odd_split(const uint32_t *cnt, const uint32_t *n_odd, uint32_t *split, uint32_t grid,
                            hipStream_t st);
std::string translate_blocks(const std::vector<PreInst> &pre, uint64_t text_lo, const std::vector<uint32_t> &trace,
                             const std::vector<uint64_t> &extra_pcs, std::vector<uint32_t> &leaders_out,
                             uint32_t &n_insts, bool odd_streams, std::vector<LoopEst> *loops_out = nullptr,
                             bool load_ahead = true, bool loop_stretch = true);
std::vector<fi_issue_op> issue_ops_from_trace(const std::vector<PreInst> &pre, const std::vector<uint32_t> &trace);
std::string jit_compile(const std::string &body, const char *arch, std::vector<char> &code, bool &cached, int part,
                        bool use_cache);
bool jit_has_odd(const std::string &body);
bool jit_parallel_ok();
hipError_t sort_pairs(void *tmp, size_t bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                      uint32_t *vout, uint64_t n, int end_bit, hipStream_t st);
}  // namespace fi

using namespace fi;

// trials per wave when fi_config.lanes_per_wave is 0: 32 of
// a wave's 64 lanes -- twice the waves in the first epoch (3,125 for 100k
// trials: ~3 per SIMD instead of 1.5) and half the divergence per wave;
// profiles/r06w_sweep_lanes_*.jsonl: crc32 4.37 -> 4.13 ms, intmix 243 ->
// 225 ms, qsort even against 64; 16 loses on crc32
static constexpr uint32_t kDefaultLanes = 32;
static constexpr uint32_t kPreTail = 4;   // zero PreInst entries past the text (fi_trial.hip solo_pre_run)
static constexpr uint32_t kDefaultResumeLanes = 8;   // measured: profiles/README.md (r01b sweep)
// trials per launch while the translated kernels are still being built, so
// that a long campaign picks the build up at a chunk boundary.  Not smaller:
// a chunk lasts at least as long as its longest trial (the hang trials), so
// the static kernels' throughput grows with the chunk (crc32, 100k trials:
// 0.36 s in 16k chunks; profiles/r04e_bench.json)
static constexpr uint64_t kJitWindowChunk = 131072;

// The background build of the translated kernels (fi_golden_run starts it;
// run_chunks installs the result at a chunk boundary): the 64-lane, solo and,
// with odd-pc streams, solo-odd kernels as one code object each, compiled in
// parallel processes (fi_jit.cpp).  Until it lands the static kernels run
// every trial -- the same outcomes, bit for bit, more slowly.
struct JitJob {
    std::string body, arch;
    bool odd = false;
    bool use_cache = true;   // FI_CFG_JIT_NO_CACHE: always compile (cold-start measurements, tests)
    std::vector<char> code[3];
    std::string err;
    bool cached = true;
    uint64_t us = 0;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
};
static const char *const kTxKernel[3] = {"fi_trial_kernel_tx", "fi_trial_kernel_tx_solo",
                                         "fi_trial_kernel_tx_solo_odd"};

static void jit_job_run(std::shared_ptr<JitJob> j) {
    const auto t0 = std::chrono::steady_clock::now();
    const int np = j->odd ? 3 : 2;
    std::string err[3];
    bool cached[3] = {true, true, true};
    if (jit_parallel_ok()) {
        std::vector<std::thread> th;
        for (int k = 0; k < np; k++)
            th.emplace_back([&, k] { err[k] = jit_compile(j->body, j->arch.c_str(), j->code[k], cached[k], k + 1, j->use_cache); });
        for (auto &t : th) t.join();
    } else {   // in-process hipRTC: one build at a time
        for (int k = 0; k < np; k++) err[k] = jit_compile(j->body, j->arch.c_str(), j->code[k], cached[k], k + 1, j->use_cache);
    }
    std::lock_guard<std::mutex> lk(j->mu);
    for (int k = 0; k < np && j->err.empty(); k++) j->err = err[k];
    j->cached = cached[0] && cached[1] && cached[2];
    j->us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    j->done = true;
    j->cv.notify_all();
}

// An allocation of n elements that frees itself: device memory (hipMalloc),
// or with kPinned pinned host memory (hipHostMalloc).  Move-only; reads as the
// pointer it owns.  Every buffer the engine keeps is one of these, so a group
// of them (below) is released by assigning it a fresh value.
template <typename T, bool kPinned = false>
class DevBuf {
public:
    static constexpr uint64_t elem = sizeof(T);
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    hipError_t alloc(uint64_t n) {
        reset();
        return kPinned ? hipHostMalloc((void **)&p_, n * sizeof(T)) : hipMalloc((void **)&p_, n * sizeof(T));
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    void reset() {
        if (p_) (void)(kPinned ? hipHostFree((void *)p_) : hipFree((void *)p_));
        p_ = nullptr;
    }

private:
    T *p_ = nullptr;
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// A loaded code object, unloaded with its owner.
class Module {
public:
    Module() = default;
    Module(Module &&o) noexcept : m(o.m) { o.m = nullptr; }
    Module &operator=(Module &&o) noexcept {
        if (this != &o) { reset(); m = o.m; o.m = nullptr; }
        return *this;
    }
    ~Module() { reset(); }
    void reset() {
        if (m) (void)hipModuleUnload(m);
        m = nullptr;
    }
    hipModule_t m = nullptr;
};

// The engine's host state, grouped by what resets it: a reset
// is the assignment of a fresh value, after hipSetDevice(e->dev).

struct Seg { uint64_t lo, hi; bool w; };

// The loaded process image: fi_load_elf / fi_load_checkpoint build one and
// move it in; the next load replaces it.
struct Image {
    bool loaded = false;
    std::map<uint64_t, std::vector<uint8_t>> pages;   // vpn -> 4 KiB
    uint64_t entry = 0, sp0 = 0, stack_min0 = 0, svma_lo = 0, svma_hi = 0;
    uint64_t text_lo = 0, text_hi = 0, code_lo = 0, code_hi = 0;
    uint64_t brk0 = 0;                 // roundUp(maxAddr, page): the process-start brk point
    std::vector<uint64_t> mem_pages;   // memory fault candidates (sorted)
    std::vector<Seg> segs;             // PT_LOAD page ranges of the ELF (w = PF_W)
    std::vector<uint64_t> alloc_order; // process-start pages in allocation order (img_write)
    // checkpoint start state beyond registers, pages and the stack VMA
    bool fp0_on = false, vm0_on = false;
    uint64_t fp0[32] = {};
    uint32_t fcsr0 = 0;
    uint64_t tick0 = 0;
    VmState vm0{};
    DevBuf<uint64_t> d_fp0;
    DevBuf<VmState> d_vm0;
    DevBuf<PreInst> d_pre;
    DevBuf<uint8_t> d_zero, d_text, d_sink;
    DevBuf<uint64_t> d_mem_pages;
    // snapshot 0 = the process-start image, frames [0, n_start_frames); the
    // golden run appends snapshots 1..n-1 and golden_reset
    // truncates the tables back to the image's own
    std::vector<SnapState> snaps;
    std::vector<PageEnt> tab;
    std::vector<uint8_t> pool;            // host copy of the snapshot frames
    uint32_t n_start_frames = 0;
    DevBuf<SnapState> d_snaps;
    DevBuf<PageEnt> d_tab;
    DevBuf<uint8_t> d_pool;
};

// memory words of exact campaigns (fi_set_exact_memory): the classes of the golden run's memory index
// under one (bits, burst), built on the device at the first exact call that needs them (exact_mem_build)
struct ExMem {
    bool ok = false;
    bool cons = false;          // a profiled build: the class records carry their consumer rows

    uint64_t bits = 0;
    uint32_t burst = 0, n_rows = 0;
    ExactMemRow rows[kExactMaxMemRows] = {};
    uint64_t classes[kExactMaxMemRows] = {}, dead[kExactMaxMemRows] = {};   // per byte set; dead: (word, t) pairs
    uint64_t words = 0, text_words = 0, n_classes = 0;
    double build_ms = 0;
    DevBuf<ExactMemRow> d_rows;
    DevBuf<ExactMemClass> d_cls;
};

// the profile of exact campaigns (fi_run_exact_profile, DESIGN.md §4j "Profile"): the rows of the golden
// trace and the consumer tables, built at the first profiled call after a golden run (profile_build)
struct ExProf {
    bool ok = false;
    std::vector<fi_profile_row> rows;
    uint32_t n_ecall = 0;
    DevBuf<uint32_t> d_inst_row;            // [ninst]: the row of the instruction that commits as numInst t
    DevBuf<ExactEcall> d_ecall;             // (numInst, row) of the first ecall entry at a numInst, ascending
    DevBuf<uint32_t> d_reg_cons;            // a row per register class word, beside d_ex_classes
    DevBuf<uint32_t> d_mw_proxy;            // a bit per d_mw_ev entry (Golden::mw_proxy)
    DevBuf<unsigned long long> d_bins;      // [rows][kProfBins]: a call's profile
};

// exact campaigns in the tick domain (fi_exact_tick.h, DESIGN.md §4j "Tick domain"): the segments and
// every structure's classes under one tick contract, built at the first such call after a golden run
// or a change of contract (exact_tick_build)
struct ExTick {
    bool ok = false;
    int contract = 0;
    double build_ms = 0;
    ExactTickTable tab;
    DevBuf<ExactTickClass> d_cls;
};

// The translated kernels: the 64-lane, solo and solo-odd code objects.
struct Tx {
    Module mod[3];
    hipFunction_t fn = nullptr, fn_solo = nullptr;
    hipFunction_t fn_odd = nullptr;   // solo kernel with the odd-pc blocks (nullptr: none translated)
};

// Everything a golden run finds out: fi_golden_run starts from a fresh one,
// and so does a load.
struct Golden {
    bool have_golden = false;
    fi_golden_info info{};
    uint32_t gdetail = 0, gsub = 0;
    std::vector<uint8_t> gout, gerr;
    DevBuf<uint8_t> d_gout, d_gerr;
    bool golden_fp = false;          // the golden run wrote FP state: no snapshot start / early exit
    uint64_t clk_until = 0;          // 1 + numInst of the golden run's last curTick read (0: none; DevCtx::clk_until)
    bool golden_unmapped = false;    // the golden run freed frames (munmap / brk shrink)
    bool pre_ok = true;
    uint64_t snap_I = 1ULL << 62;
    // memory liveness index (build_mem_index)
    bool mem_live = false;
    uint32_t mw_n = 0;
    uint64_t mw_nev = 0;             // the index's events
    DevBuf<uint64_t> d_mw_addr, d_mw_ev;
    DevBuf<uint32_t> d_mw_off;
    std::vector<uint32_t> mw_proxy;  // a bit per event of the index: recorded as a syscall's access (kMemEvProxy)
    // first-access forwarding: per register x1..x31, the golden trace's
    // accesses in order, entry = (2 * numInst + !ecall) << 1 | reads
    DevBuf<uint32_t> d_fw_off, d_fw_ev;
    bool fw_ok = false;
    // exact campaigns (fi_exact.h): the host copy of the index and, built from it at
    // the first exact call after a golden run, every register's classes (register r's packed words
    // at ex_off[r] .. ex_off[r + 1]) and dead-site count
    std::vector<uint32_t> fw_off, fw_ev;
    bool ex_ok = false;
    uint32_t ex_off[33] = {};
    uint64_t ex_dead[32] = {};
    DevBuf<uint64_t> d_ex_classes;
    ExMem xm;
    ExProf xp;
    ExTick xt;
    // load-time build of the trial kernel with the translated golden blocks
    Tx tx;
    std::shared_ptr<JitJob> jit;     // the build in flight (nullptr: none); its thread holds the job too
    std::vector<PreInst> jit_pre;    // golden pre-decoded text with the leader flags, uploaded when it lands
    uint64_t jit_blocks = 0, jit_insts = 0;
    std::string tx_status = "no golden run";
    std::string tx_body;   // last generated translation (diagnostics)
    DevBuf<LoopEst> d_loops;         // counted loops of the golden text (the solo order's work-left estimate)
    uint32_t n_loops = 0;
    // SHREWD FU contention (fi_set_issue_model): shadow issued per golden numInst index
    fi_issue_stats issue_stats{};
    std::vector<uint8_t> shadow;
    DevBuf<uint32_t> d_shadow;       // the same as a bitmap, [ninst / 32 + 1]
    std::vector<PreInst> g_pre;      // golden pre-decoded text and trace (empty: unavailable)
    std::vector<uint32_t> g_trace;
    // tick-domain injection (fi_tick.cpp, fi_timing.cpp): the golden run's attempts as requests
    std::vector<fi_timing_op> t_ops;
    std::vector<fi_timing_ticks> t_ticks;
    fi_timing_stats t_stats{};
    std::string t_status = "no golden run";
    // the site map's table (fi_tick_map.h): the attempts and their ticks, packed with the tick model;
    // the device map's copy is made at its first use (ensure_tick_table)
    std::vector<uint64_t> tk_done;
    std::vector<TickRec> tk_rec;
    DevBuf<uint64_t> d_tk_done;
    DevBuf<TickRec> d_tk_rec;
};

// output capture (fi_run_sites_capture): on only while such a call runs (bytes != 0).
// Its rows live in the chunk slots (ChunkSlot::cap), grown on demand (ensure_capture).
struct Capture {
    uint32_t bytes = 0, stride = 0;   // bytes kept per stream; device row pitch (bytes rounded up to 16)
    uint64_t rows = 0;                // trials per chunk
    uint64_t held_b = 0, held_rows = 0;   // what is allocated: bytes per row buffer, entries per length buffer
    uint8_t *out = nullptr, *err = nullptr;   // the caller's arrays (err, lens may be NULL)
    fi_stream_len *lens = nullptr;
};

// a chunk's rows and lengths and their pinned mirror
struct CaptureRows {
    DevBuf<uint8_t> d_out, d_err;
    DevBuf<fi_stream_len> d_len;
    PinBuf<uint8_t> h_out, h_err;
    PinBuf<fi_stream_len> h_len;
};

// Everything that alternates between the two chunks in flight (run_chunks): chunk i uses slot i & 1,
// so that chunk i + 1 is filled and run while chunk i's second pass, tally and copies are still queued.
struct ChunkSlot {
    DevBuf<fi_site> d_sites;
    DevBuf<fi_outcome> d_out;
    DevBuf<uint32_t> d_weight;         // an exact chunk's weights: the sites each trial stands for
    // the device tick map's buffers, [cap] each, made on first use (ensure_tick_work; Work::tk_ok): the
    // tick sites in fi_site layout, the dispositions, the disp 1 / 2 outcomes, uploaded explicit sites
    DevBuf<fi_site> d_tk_sites;
    DevBuf<uint8_t> d_tk_disp;
    DevBuf<fi_outcome> d_tk_res;
    DevBuf<fi_tick_site> d_tk_in;
    DevBuf<uint64_t> d_xt_weight;      // an exact tick chunk's weights, made on first use (ensure_exact_tick_work)
    // the second pass (chunk_end): this slot's part of Work::d_redo_idx, d_redo_cnt and h_redo_cnt
    uint32_t *redo_idx = nullptr, *redo_cnt = nullptr, *h_redo_cnt = nullptr;
    // the redo count has reached h_redo_cnt / the outcomes have reached h_stage: fi_engine::ev_cnt,
    // ev_stage, which fi_create makes and fi_destroy releases (the slots come and go with the work buffers)
    hipEvent_t ev_cnt = nullptr, ev_stage = nullptr;
    // pinned staging of the outcomes on their way to the caller's (pageable) array, made on first
    // use (chunk_end): a copy straight into pageable memory would hold the host until the stream
    // reaches it
    PinBuf<fi_outcome> h_stage;
    CaptureRows cap;                   // a capture call's (ensure_capture)
};

// Work buffers, sized for `cap` trials per launch (work_buffers); a larger
// launch replaces them all.
struct Work {
    uint64_t cap = 0;
    ChunkSlot slot[2];
    DevBuf<uint64_t> d_keys, d_keys2;
    DevBuf<uint32_t> d_perm, d_perm2;
    DevBuf<uint8_t> d_tmp;
    size_t tmp_bytes = 0;
    DevBuf<uint64_t> d_eff;          // effective inject time per trial (kFwDead: dead at injection)
    DevBuf<fi_histogram> d_hist;
    DevBuf<unsigned long long> d_stats;
    DevBuf<uint64_t> d_wave_dbg;
    DevBuf<uint64_t> d_fregs;        // FP registers of the work slots
    DevBuf<uint64_t> d_inpos;        // per work slot: fd 0's file offset
    DevBuf<uint8_t> d_priv;
    DevBuf<uint64_t> d_priv_vpn;
    // overflow pages (DevCtx::ov_*): ov_blocks blocks of ov_pages
    DevBuf<uint8_t> d_ov;
    DevBuf<uint64_t> d_ov_vpn;
    DevBuf<uint32_t> d_ov_of, d_ov_next;
    uint32_t ov_blocks = 0, ov_pages = 0;
    DevBuf<VmState> d_vm;            // per-slot SE memory map (trials that made a VM syscall)
    // epochs: suspended lanes, survivor lists, counts, sort buffers
    DevBuf<LaneSave> d_save;
    DevBuf<uint32_t> d_surv[2], d_cnt;
    DevBuf<uint64_t> d_skeys, d_skeys2;
    DevBuf<uint32_t> d_svals, d_svals2;
    DevBuf<uint32_t> d_wrange, d_nwaves;   // packed resume (FI_CFG_PACK_RUNS)
    DevBuf<uint32_t> d_split;   // per epoch: odd-pc survivors, then the solo kernel's share of the list
    DevBuf<uint32_t> d_dmap;    // per slot: rewritten-code map (DevCtx::dmap, kDmapWords words)
    // second pass of the trials that ran out of private pages (chunk_end): the lists and counts of
    // both chunk slots (ChunkSlot::redo_*), one pass's sites and outcomes
    DevBuf<uint32_t> d_redo_idx, d_redo_cnt;
    PinBuf<uint32_t> h_redo_cnt;
    DevBuf<fi_site> d_redo_sites;
    DevBuf<fi_outcome> d_redo_out;
    bool tk_ok = false;         // both slots have the device tick map's buffers
    Capture cx;
};

struct fi_engine {
    fi_config cfg{};
    std::string err;
    int dev = 0;
    // streams and events: made by fi_create, released by fi_destroy.  The
    // solo-odd kernel runs beside the solo kernel on its own stream
    hipStream_t stream = nullptr, stream_odd = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_cnt[2] = {nullptr, nullptr}, ev_stage[2] = {nullptr, nullptr};   // the chunk slots' (ChunkSlot)
    double last_ms = 0;
    // per-launch timing of the interpreter kernel (bench roofline)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tpool;
    DevBuf<unsigned long long> d_span;   // per timer slot: [min wave start, max wave end] (kSpanSlots pairs)
    std::vector<uint32_t> tkind;
    size_t tused = 0;

    // campaign settings (fi_set_*)
    uint64_t seed = 0x5EED0001ULL, structures = 0;
    uint32_t burst = 1;
    uint64_t bits = ~0ULL;      // eligible lowest-bit positions (fi_set_bits)
    uint64_t clk_period = 500, rnd_seed = 5489;   // fi_set_clock
    DevBuf<uint8_t> d_rnd;      // getrandom's byte stream (kRndLen bytes)
    std::string exe_path;       // fi_set_exe_path
    DevBuf<uint8_t> d_exe;
    bool stdin_on = false;      // fi_set_stdin: Process.input is a file (else "cin")
    std::vector<uint8_t> stdin_data;
    DevBuf<uint8_t> d_stdin;
    uint64_t protect = 0;
    uint64_t protect_opc = 0;   // SHREWD replication by OpClass (fi_set_protect_opclasses)
    bool issue_on = false;      // fi_set_issue_model: every golden run recomputes its shadow
    fi_issue_params issue_p{};
    int cpu_model = FI_CPU_ATOMIC;   // fi_set_cpu_model FI_CPU_TIMING: tick-domain injection
    fi_timing_params tparams{};
    int tick_map = FI_TICK_MAP_HOST;                // fi_set_tick_map
    int tick_contract = FI_TICK_CONTRACT_NUMINST;   // fi_set_tick_contract
    bool exact_mem = false;     // fi_set_exact_memory
    uint32_t prof_variant = 0;  // fi_debug_set_profile_variant
    // builds this engine started: a finished one is joined when a build is
    // installed (jit_install), one still running by fi_destroy
    std::vector<std::pair<std::thread, std::shared_ptr<JitJob>>> jit_threads;

    Image img;
    Golden gold;
    Work w;
};

static fi_status fail(fi_engine *e, fi_status code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    return code;
}

// (what: the error text's prefix -- the call itself, or the step it belongs to)
#define HIPCHK_AS(what, call)                                                                \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess) return fail(e, FI_E_HIP, "%s: %s", what, hipGetErrorString(_e)); \
    } while (0)
#define HIPCHK(call) HIPCHK_AS(#call, call)

// Diagnostics (SHREWD_FI_TRACE): a native backtrace on SIGSEGV.
#include <execinfo.h>
#include <csignal>
#include <unistd.h>
static void segv_trace(int sig) {
    void *bt[64];
    const int n = backtrace(bt, 64);
    const char msg[] = "[fi] fatal signal, native backtrace:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(bt, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}

extern "C" {

// errors of calls that have no engine yet (fi_create), per host thread
static thread_local std::string g_create_err;

// getrandom's bytes: gem5's Random(globalSeed) generator (std::mt19937_64,
// base/random.hh:125) drawn once per byte, % 255 (Random::random<uint8_t>)
static fi_status upload_rnd(fi_engine *e) {
    std::vector<uint8_t> tab(kRndLen);
    std::mt19937_64 gen((uint32_t)e->rnd_seed);
    for (auto &b : tab) b = (uint8_t)(gen() % 255);
    if (!e->d_rnd) HIPCHK(e->d_rnd.alloc(kRndLen));
    HIPCHK(hipMemcpy(e->d_rnd, tab.data(), kRndLen, hipMemcpyHostToDevice));
    return FI_OK;
}

// private pages per slot of the second pass (and so the overflow blocks): 16 P, at least 256
static uint64_t redo_pages(uint64_t P) { return std::max<uint64_t>(P * 16ull, 256); }

// The work buffers of c trials per launch, described once: allocated into w,
// or (count) only added up -- fi_create's estimate of what a slot costs.
static fi_status work_buffers(fi_engine *e, Work &w, uint64_t c, uint64_t *count) {
    uint64_t total = 0;
    auto buf = [&](auto &b, uint64_t n) {
        total += n * b.elem;
        return count ? hipSuccess : b.alloc(n);
    };
    const uint64_t P = e->cfg.private_pages, P2 = redo_pages(P);
    for (ChunkSlot &s : w.slot) {
        HIPCHK(buf(s.d_sites, c));
        HIPCHK(buf(s.d_weight, c));
        HIPCHK(buf(s.d_out, c));
    }
    HIPCHK(buf(w.d_keys, c));
    HIPCHK(buf(w.d_keys2, c));
    HIPCHK(buf(w.d_perm, c));
    HIPCHK(buf(w.d_perm2, c));
    HIPCHK(sort_pairs_bytes(c, w.tmp_bytes));
    HIPCHK(buf(w.d_tmp, std::max<size_t>(w.tmp_bytes, 16)));
    HIPCHK(buf(w.d_eff, c));
    HIPCHK(buf(w.d_hist, 1));
    HIPCHK(buf(w.d_stats, kNStats));
    HIPCHK(buf(w.d_wave_dbg, c * kWaveDbgWords));
    HIPCHK(buf(w.d_priv, c * P * kPage));
    HIPCHK(buf(w.d_priv_vpn, c * P));
    HIPCHK(buf(w.d_save, c));
    HIPCHK(buf(w.d_vm, c));
    HIPCHK(buf(w.d_fregs, c * 32));
    HIPCHK(buf(w.d_inpos, c));
    HIPCHK(buf(w.d_surv[0], c));
    HIPCHK(buf(w.d_surv[1], c));
    HIPCHK(buf(w.d_cnt, 16));
    HIPCHK(buf(w.d_skeys, c));
    HIPCHK(buf(w.d_skeys2, c));
    HIPCHK(buf(w.d_svals, c));
    HIPCHK(buf(w.d_svals2, c));
    HIPCHK(buf(w.d_wrange, 2 * c));
    HIPCHK(buf(w.d_nwaves, 16));
    HIPCHK(buf(w.d_split, 64));
    HIPCHK(buf(w.d_dmap, c * kDmapWords));
    HIPCHK(buf(w.d_redo_idx, 2 * c));
    HIPCHK(buf(w.d_redo_cnt, 4));
    HIPCHK(buf(w.d_redo_sites, c));
    HIPCHK(buf(w.d_redo_out, c));
    // (the pinned staging of host-bound outcomes is made on first use:
    // chunk_end; device-resident runs never need it)
    if (!count) HIPCHK(w.h_redo_cnt.alloc(4));
    for (uint32_t i = 0; i < 2 && !count; i++) {
        ChunkSlot &s = w.slot[i];
        s.redo_idx = w.d_redo_idx + i * c; s.redo_cnt = w.d_redo_cnt + i; s.h_redo_cnt = w.h_redo_cnt + i;
        s.ev_cnt = e->ev_cnt[i]; s.ev_stage = e->ev_stage[i];
    }
    // overflow pool: a trial past P pages takes a block of P' - P more (P' the
    // redo pass's page count), one block per 2048 slots (at least 64)
    if (!(e->cfg.flags & FI_CFG_NO_OVERFLOW) && P2 > P) {
        w.ov_pages = (uint32_t)(P2 - P);
        w.ov_blocks = (uint32_t)std::max<uint64_t>(64, c / 2048);
        HIPCHK(buf(w.d_ov, (uint64_t)w.ov_blocks * w.ov_pages * kPage));
        HIPCHK(buf(w.d_ov_vpn, (uint64_t)w.ov_blocks * w.ov_pages));
        HIPCHK(buf(w.d_ov_of, c));
        HIPCHK(buf(w.d_ov_next, 4));
    }
    if (count) *count = total;
    else w.cap = c;
    return FI_OK;
}

fi_status fi_create(const fi_config *cfg, fi_engine **out) {
    if (!out) { g_create_err = "fi_create: out is NULL"; return FI_E_ARG; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        g_create_err = "fi_create: no HIP device visible (the engine has no CPU fallback)";
        return FI_E_NODEVICE;
    }
    if (getenv("SHREWD_FI_TRACE")) signal(SIGSEGV, segv_trace);
    fi_engine *e = new fi_engine();
    if (cfg) e->cfg = *cfg;
    // diagnostics (A/B runs of an unchanged caller): FI_CFG_* bits to add
    if (const char *x = getenv("SHREWD_FI_EXTRA_FLAGS")) e->cfg.flags |= (uint32_t)strtoul(x, nullptr, 0);
    if (e->cfg.private_pages == 0) e->cfg.private_pages = 16;
    if (e->cfg.hang_factor_x16 == 0) e->cfg.hang_factor_x16 = 32;
    if (e->cfg.lanes_per_wave == 0) e->cfg.lanes_per_wave = kDefaultLanes;
    if (e->cfg.resume_lanes == 0) e->cfg.resume_lanes = kDefaultResumeLanes;
    for (uint32_t l : {e->cfg.lanes_per_wave, e->cfg.resume_lanes}) {
        if (l > 64 || (l & (l - 1))) {
            g_create_err = "fi_create: lanes_per_wave / resume_lanes must be a power of two <= 64";
            delete e;
            return FI_E_ARG;
        }
    }
    e->dev = e->cfg.device;
    if (e->dev < 0 || e->dev >= n) {
        g_create_err = "fi_create: device " + std::to_string(e->dev) + " out of range (" + std::to_string(n) + " visible)";
        delete e;
        return FI_E_ARG;
    }
    if (hipSetDevice(e->dev) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->stream_odd, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_cnt[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_cnt[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_stage[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_stage[1], hipEventDisableTiming) != hipSuccess) {
        g_create_err = "fi_create: HIP stream/event creation failed on device " + std::to_string(e->dev);
        delete e;
        return FI_E_HIP;
    }
    if (upload_rnd(e) != FI_OK) {
        g_create_err = "fi_create: " + e->err;
        delete e;
        return FI_E_HIP;
    }
    if (e->cfg.max_trials_per_launch == 0) {
        // auto: a campaign's trials in as few launches as half the free HBM
        // holds (each launch ends in its own serial tail of long trials), at
        // what work_buffers takes per slot of the largest launch
        size_t free_b = 0, total_b = 0;
        const uint64_t c = 1u << 21;
        uint64_t bytes = 0;
        Work none;
        if (work_buffers(e, none, c, &bytes) != FI_OK) {
            g_create_err = "fi_create: " + e->err;
            delete e;
            return FI_E_HIP;
        }
        const uint64_t per = (bytes + c - 1) / c;
        if (getenv("SHREWD_FI_TRACE")) fprintf(stderr, "[fi] work buffers: %llu bytes per slot\n", (unsigned long long)per);
        uint64_t cap = 65536;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = (uint64_t)free_b / 2 / per;
        e->cfg.max_trials_per_launch = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(cap, 65536), 1u << 21);
    }
    *out = e;
    return FI_OK;
}

// Install a finished background build (at a chunk boundary, before anything
// of the chunk is queued on st): load the code objects and flag the block
// leaders in the pre-decoded text.  wait = block until the build is done.
static void jit_install(fi_engine *e, hipStream_t st, bool wait) {
    std::shared_ptr<JitJob> j = e->gold.jit;
    if (!j) return;
    {
        std::unique_lock<std::mutex> lk(j->mu);
        if (wait) j->cv.wait(lk, [&] { return j->done; });
        if (!j->done) return;
    }
    e->gold.jit.reset();
    // join the builds that have finished (this one, and any an earlier golden
    // run left behind): a long-lived engine keeps no finished threads
    for (size_t i = 0; i < e->jit_threads.size();) {
        bool fin;
        {
            std::lock_guard<std::mutex> lk(e->jit_threads[i].second->mu);
            fin = e->jit_threads[i].second->done;
        }
        if (fin) {
            if (e->jit_threads[i].first.joinable()) e->jit_threads[i].first.join();
            e->jit_threads.erase(e->jit_threads.begin() + (long)i);
        } else {
            i++;
        }
    }
    if (!j->err.empty()) {
        e->gold.tx_status = j->err;
        return;
    }
    Tx tx;   // (unloads itself unless it is moved in)
    hipFunction_t *fn[3] = {&tx.fn, &tx.fn_solo, &tx.fn_odd};
    for (int k = 0; k < (j->odd ? 3 : 2); k++) {
        if (hipModuleLoadData(&tx.mod[k].m, j->code[k].data()) != hipSuccess ||
            hipModuleGetFunction(fn[k], tx.mod[k].m, kTxKernel[k]) != hipSuccess) {
            e->gold.tx_status = "code object did not load";
            return;
        }
    }
    if (hipMemcpyAsync(e->img.d_pre, e->gold.jit_pre.data(), e->gold.jit_pre.size() * sizeof(PreInst), hipMemcpyHostToDevice, st) !=
        hipSuccess) {
        e->gold.tx_status = "pre-decoded text upload failed";
        return;
    }
    e->gold.tx = std::move(tx);
    e->gold.tx_status = "";
    e->gold.info.translated_blocks = e->gold.jit_blocks;
    e->gold.info.translated_insts = e->gold.jit_insts;
    e->gold.info.translate_us = j->cached ? 0 : j->us;
}

void fi_destroy(fi_engine *e) {
    if (!e) return;
    // a background build still running (a short campaign on a cold cache):
    // wait for it, so that no thread outlives the engine and no fi_jitc child
    // is left behind -- exiting under a running build races the static
    // destructors of the JIT cache and of hipRTC
    for (auto &t : e->jit_threads)
        if (t.first.joinable()) t.first.join();
    (void)hipSetDevice(e->dev);
    for (auto &tp : e->tpool) { (void)hipEventDestroy(tp.first); (void)hipEventDestroy(tp.second); }
    for (hipEvent_t ev : {e->ev0, e->ev1, e->ev_fork, e->ev_join, e->ev_cnt[0], e->ev_cnt[1], e->ev_stage[0], e->ev_stage[1]})
        if (ev) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->stream_odd) (void)hipStreamDestroy(e->stream_odd);
    delete e;
}

const char *fi_last_error(fi_engine *e) { return e ? e->err.c_str() : g_create_err.c_str(); }

// ------------------------------------------------------------------ image
static uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// SETranslatingPortProxy(Always) write: allocates pages on demand.
static void img_write(Image &img, uint64_t addr, const uint8_t *src, uint64_t n) {
    for (uint64_t i = 0; i < n;) {
        const uint64_t a = addr + i;
        auto &pg = img.pages[a >> 12];
        if (pg.empty()) {
            pg.assign(kPage, 0);
            // SETranslatingPortProxy (Always) allocates the frame on this first
            // write: frames go out in this order (sim/process.cc:318-343)
            img.alloc_order.push_back(a >> 12);
        }
        const uint64_t off = a & (kPage - 1);
        const uint64_t k = std::min<uint64_t>(n - i, kPage - off);
        if (src) memcpy(pg.data() + off, src + i, k);
        else memset(pg.data() + off, 0, k);
        i += k;
    }
}
static void img_push64(Image &img, uint64_t &sp, uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
    img_write(img, sp, b, 8);
    sp += 8;
}

// std::mt19937_64 with gem5's global seed 5489 (src/base/random.hh:211-217):
// AT_RANDOM byte i = gen() % 256 (RiscvProcess::argsInit, process.cc:171-175).
struct Mt64 {
    uint64_t mt[312];
    int idx;
    explicit Mt64(uint64_t seed) {
        mt[0] = seed;
        for (int i = 1; i < 312; i++) mt[i] = 6364136223846793005ULL * (mt[i - 1] ^ (mt[i - 1] >> 62)) + (uint64_t)i;
        idx = 312;
    }
    uint64_t operator()() {
        if (idx >= 312) {
            for (int i = 0; i < 312; i++) {
                const uint64_t x = (mt[i] & 0xFFFFFFFF80000000ULL) | (mt[(i + 1) % 312] & 0x7FFFFFFFULL);
                uint64_t xa = x >> 1;
                if (x & 1) xa ^= 0xB5026F5AA96619E9ULL;
                mt[i] = mt[(i + 156) % 312] ^ xa;
            }
            idx = 0;
        }
        uint64_t y = mt[idx++];
        y ^= (y >> 29) & 0x5555555555555555ULL;
        y ^= (y << 17) & 0x71D67FFFEDA60000ULL;
        y ^= (y << 37) & 0xFFF7EEE000000000ULL;
        y ^= y >> 43;
        return y;
    }
};

// The issue model over the golden trace (fi_issue.cpp), indexed by numInst
// (ecall events are replayed but numInst does not count them), uploaded as a
// bitmap for the result-fault commit (fi_trial.hip:replicated).
static fi_status compute_shadow(fi_engine *e) {
    if (e->gold.g_trace.empty() && e->gold.info.ninst)
        return fail(e, FI_E_STATE, "issue model: the golden trace is unavailable (trace overflow or rewritten text)");
    const std::vector<fi_issue_op> ops = issue_ops_from_trace(e->gold.g_pre, e->gold.g_trace);
    std::vector<uint8_t> all(ops.size());
    fi_issue_stats st{};
    const fi_status s = fi_issue_model_run(ops.data(), ops.size(), &e->issue_p, all.data(), &st);
    if (s) return fail(e, s, "issue model: invalid parameters");
    e->gold.shadow.clear();
    e->gold.shadow.reserve(e->gold.info.ninst);
    for (size_t i = 0; i < ops.size(); i++)
        if (!(e->gold.g_trace[i] & 0x80000000u)) e->gold.shadow.push_back(all[i]);
    if (e->gold.shadow.size() != e->gold.info.ninst)
        return fail(e, FI_E_STATE, "issue model: trace holds %zu instructions, golden run %llu", e->gold.shadow.size(),
                    (unsigned long long)e->gold.info.ninst);
    std::vector<uint32_t> bits(e->gold.shadow.size() / 32 + 1, 0);
    for (size_t k = 0; k < e->gold.shadow.size(); k++)
        if (e->gold.shadow[k]) bits[k >> 5] |= 1u << (k & 31);
    HIPCHK(e->gold.d_shadow.alloc(bits.size()));
    HIPCHK(hipMemcpy(e->gold.d_shadow, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
    e->gold.issue_stats = st;
    return FI_OK;
}

static fi_status upload_snaps(fi_engine *e, Image &img) {
    HIPCHK(img.d_snaps.alloc(img.snaps.size()));
    HIPCHK(img.d_tab.alloc(std::max<size_t>(1, img.tab.size())));
    // (+64: solo translated code reads shared frames with dword-granular scalar
    // loads that may run up to 11 bytes past an access at a frame's end)
    HIPCHK(img.d_pool.alloc(std::max<size_t>(kPage, img.pool.size()) + 64));
    HIPCHK(hipMemcpy(img.d_snaps, img.snaps.data(), img.snaps.size() * sizeof(SnapState), hipMemcpyHostToDevice));
    if (!img.tab.empty())
        HIPCHK(hipMemcpy(img.d_tab, img.tab.data(), img.tab.size() * sizeof(PageEnt), hipMemcpyHostToDevice));
    if (!img.pool.empty()) HIPCHK(hipMemcpy(img.d_pool, img.pool.data(), img.pool.size(), hipMemcpyHostToDevice));
    return FI_OK;
}

// The host side of an ELF's process-start image, and its start registers.
static fi_status elf_image(fi_engine *e, Image &img, const uint8_t *elf, size_t len, const char *const *argv,
                           const char *const *envp, uint64_t regs[32]) {
    if (len < 64 || memcmp(elf, "\x7f" "ELF", 4) || elf[4] != 2 || elf[5] != 1 || le16(elf + 18) != 243)
        return fail(e, FI_E_ELF, "not an ELF64 little-endian RISC-V executable");
    img.entry = le64(elf + 24);
    const uint64_t phoff = le64(elf + 32);
    const uint32_t phentsize = le16(elf + 54), phnum = le16(elf + 56);
    if (phoff + (uint64_t)phentsize * phnum > len) return fail(e, FI_E_ELF, "program headers out of file");
    uint64_t max_addr = 0, phdr_vaddr = 0;
    uint64_t xlo = ~0ULL, xhi = 0, clo = ~0ULL, chi = 0;
    std::vector<uint64_t> wpages;
    for (uint32_t i = 0; i < phnum; i++) {
        const uint8_t *ph = elf + phoff + (uint64_t)i * phentsize;
        if (le32(ph) != 1) continue;   // PT_LOAD
        const uint32_t flags = le32(ph + 4);
        const uint64_t off = le64(ph + 8), vaddr = le64(ph + 16), paddr = le64(ph + 24);
        const uint64_t filesz = le64(ph + 32), memsz = le64(ph + 40);
        if (memsz == 0) continue;                       // elf_object.cc:378-381
        if (off + filesz > len) return fail(e, FI_E_ELF, "segment %u beyond file", i);
        img_write(img, paddr, elf + off, filesz);          // loaded at p_paddr (elf_object.cc:383)
        if (memsz > filesz) img_write(img, paddr + filesz, nullptr, memsz - filesz);
        max_addr = std::max(max_addr, paddr + memsz);
        img.segs.push_back({paddr & ~(kPage - 1), (paddr + memsz + kPage - 1) & ~(kPage - 1), (flags & 2) != 0});
        if (off <= phoff && off + filesz > phoff) phdr_vaddr = vaddr + (phoff - off);
        if (flags & 1) {
            xlo = std::min(xlo, paddr & ~(kPage - 1));
            xhi = std::max(xhi, (paddr + memsz + kPage - 1) & ~(kPage - 1));
            clo = std::min(clo, paddr);
            chi = std::max(chi, paddr + memsz);
        }
        if (flags & 2)
            for (uint64_t pg = paddr & ~(kPage - 1); pg < paddr + memsz; pg += kPage) wpages.push_back(pg);
    }
    if (xlo == ~0ULL) return fail(e, FI_E_ELF, "no executable segment");
    if ((xlo >> 32) != ((xhi - 1) >> 32)) return fail(e, FI_E_ELF, "executable segments cross a 4 GiB boundary");
    img.text_lo = xlo;
    img.text_hi = xhi;
    img.code_lo = clo;
    img.code_hi = chi;

    // RiscvProcess::argsInit<uint64_t> (src/arch/riscv/process.cc:134-261)
    std::vector<std::string> av, ev;
    for (int i = 0; argv[i]; i++) av.emplace_back(argv[i]);
    for (int i = 0; envp && envp[i]; i++) ev.emplace_back(envp[i]);
    const int nauxv = 8;
    uint64_t stack_min = kStackBase;
    uint64_t stack_top = stack_min - 16;
    for (auto &s : av) stack_top -= s.size() + 1;
    for (auto &s : ev) stack_top -= s.size() + 1;
    stack_top &= ~7ULL;
    const uint64_t at_random = stack_top;   // AT_RANDOM points here (process.cc:156)
    const uint64_t arrays = (1 + av.size()) * 8 + (1 + ev.size()) * 8 + 8 + 2 * 8 * nauxv;
    stack_top -= arrays;
    stack_top &= ~15ULL;
    const uint64_t stack_size = kStackBase - stack_top;
    img.svma_lo = stack_top & ~(kPage - 1);
    img.svma_hi = img.svma_lo + ((stack_size + kPage - 1) & ~(kPage - 1));
    stack_min -= 16;
    Mt64 rng(5489);
    uint8_t rnd[16];
    for (int i = 0; i < 16; i++) rnd[i] = (uint8_t)(rng() % 256);
    img_write(img, stack_min, rnd, 16);
    std::vector<uint64_t> argp, envptr;
    for (auto &s : av) { stack_min -= s.size() + 1; img_write(img, stack_min, (const uint8_t *)s.c_str(), s.size() + 1); argp.push_back(stack_min); }
    for (auto &s : ev) { stack_min -= s.size() + 1; img_write(img, stack_min, (const uint8_t *)s.c_str(), s.size() + 1); envptr.push_back(stack_min); }
    stack_min &= ~7ULL;
    stack_min -= arrays;
    stack_min &= ~15ULL;
    uint64_t sp = stack_min;
    img_push64(img, sp, av.size());
    for (uint64_t p : argp) img_push64(img, sp, p);
    img_push64(img, sp, 0);
    for (uint64_t p : envptr) img_push64(img, sp, p);
    img_push64(img, sp, 0);
    const uint64_t aux[8][2] = {{9, img.entry}, {5, phnum}, {4, phentsize}, {3, phdr_vaddr},
                                {6, kPage}, {23, 0}, {25, at_random}, {0, 0}};
    for (auto &a : aux) { img_push64(img, sp, a[0]); img_push64(img, sp, a[1]); }
    img.sp0 = stack_min;
    img.stack_min0 = stack_min & ~(kPage - 1);
    for (uint64_t pg = img.stack_min0;; pg += kPage) {
        wpages.push_back(pg);
        if (pg == (kStackBase & ~(kPage - 1))) break;
    }
    std::sort(wpages.begin(), wpages.end());
    wpages.erase(std::unique(wpages.begin(), wpages.end()), wpages.end());
    img.mem_pages = wpages;
    img.brk0 = (max_addr + kPage - 1) & ~(kPage - 1);   // Process brk point (process.cc: roundUp(maxAddr))
    // RiscvProcess::argsInit leaves every register 0 but sp; pc = e_entry
    regs[2] = img.sp0;
    return FI_OK;
}

// ---- snapshot 0: the start image in img.pages (frames sorted by vpn) and the
// initial architectural state; the text pre-decoded on the device.  The
// common tail of fi_load_elf and fi_load_checkpoint.
static fi_status finish_load(fi_engine *e, Image &img, const uint64_t regs[32], uint64_t pc) {
    const std::vector<uint64_t> &wpages = img.mem_pages;
    img.pool.clear();
    img.tab.clear();
    img.snaps.clear();
    for (auto &kv : img.pages) {
        PageEnt pe{};
        pe.vpn = kv.first;
        pe.frame = (uint32_t)(img.pool.size() / kPage);
        img.tab.push_back(pe);
        img.pool.insert(img.pool.end(), kv.second.begin(), kv.second.end());
    }
    img.n_start_frames = (uint32_t)img.tab.size();
    SnapState s0{};
    for (int r = 1; r < 32; r++) s0.regs[r] = regs[r];
    s0.pc = pc;
    s0.stack_min = img.stack_min0;
    s0.tab_off = 0;
    s0.tab_n = (uint32_t)img.tab.size();
    img.snaps.push_back(s0);
    {
        fi_status st = upload_snaps(e, img);
        if (st) return st;
    }
    HIPCHK(img.d_zero.alloc(kPage + 64));   // (+64: as the frame pool)
    HIPCHK(img.d_sink.alloc(kPage));
    HIPCHK(img.d_mem_pages.alloc(std::max<size_t>(1, wpages.size())));
    HIPCHK(hipMemset(img.d_zero, 0, kPage + 64));
    if (!wpages.empty()) HIPCHK(hipMemcpy(img.d_mem_pages, wpages.data(), wpages.size() * 8, hipMemcpyHostToDevice));
    const uint64_t tbytes = img.text_hi - img.text_lo;
    std::vector<uint8_t> text(tbytes, 0);
    for (uint64_t a = img.text_lo; a < img.text_hi; a += kPage) {
        auto it = img.pages.find(a >> 12);
        if (it != img.pages.end()) memcpy(text.data() + (a - img.text_lo), it->second.data(), kPage);
    }
    HIPCHK(img.d_text.alloc(tbytes));
    HIPCHK(hipMemcpy(img.d_text, text.data(), tbytes, hipMemcpyHostToDevice));
    // + kPreTail zero entries (kind K_SLOW): the solo interpreter prefetches
    // the fall-through entry of the text's last instruction without a clamp
    HIPCHK(img.d_pre.alloc(tbytes / 2 + kPreTail));
    HIPCHK(hipMemset(img.d_pre + tbytes / 2, 0, kPreTail * sizeof(PreInst)));
    HIPCHK(launch_predecode(img.d_text, img.code_lo - img.text_lo, img.code_hi - img.text_lo, tbytes / 2, img.d_pre,
                            e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    img.loaded = true;
    return FI_OK;
}

// A load starts from an engine with no image and no golden run, and moves its
// own image in once it is whole: a failed load leaves the engine unloaded.
static fi_status unload(fi_engine *e) {
    HIPCHK(hipSetDevice(e->dev));
    e->gold = Golden{};
    e->img = Image{};
    return FI_OK;
}

fi_status fi_load_elf(fi_engine *e, const uint8_t *elf, size_t len, const char *const *argv, const char *const *envp) {
    if (!e || !elf || !argv || !argv[0]) return fail(e, FI_E_ARG, "fi_load_elf: elf and argv[0] required");
    fi_status st = unload(e);
    Image img;
    uint64_t regs[32] = {};
    if (!st) st = elf_image(e, img, elf, len, argv, envp, regs);
    if (!st) st = finish_load(e, img, regs, img.entry);
    if (!st) e->img = std::move(img);
    return st;
}

fi_status fi_load_checkpoint(fi_engine *e, const char *cpt_dir, const uint8_t *elf, size_t len) {
    if (!e || !cpt_dir || !elf) return fail(e, FI_E_ARG, "fi_load_checkpoint: checkpoint directory and ELF required");
    fi_status st = unload(e);
    if (st) return st;
    const char *argv[] = {"checkpoint", nullptr};
    Image img;
    uint64_t regs[32];
    st = elf_image(e, img, elf, len, argv, nullptr, regs);   // executable range, segments, entry checks
    if (st) return st;
    CptImage cpt;
    const std::string err = read_gem5_checkpoint(cpt_dir, cpt);
    if (!err.empty()) return fail(e, FI_E_ARG, "fi_load_checkpoint: %s", err.c_str());
    // the engine's SE model keeps RiscvProcess64's stack (process.cc:71-82)
    if (cpt.stack_base != kStackBase || cpt.max_stack != kMaxStack)
        return fail(e, FI_E_ARG, "fi_load_checkpoint: stack base / max stack differ from RiscvProcess64's");
    if (cpt.vmas.size() > kMaxVma)
        return fail(e, FI_E_ARG, "fi_load_checkpoint: %zu VMAs (at most %u)", cpt.vmas.size(), kMaxVma);
    // the checkpoint's pages in the ELF's place
    img.pages.clear();
    img.alloc_order.clear();   // a checkpoint's frames: not in process-start order (no tick model)
    for (auto &kv : cpt.pages) img.pages[kv.first] = kv.second;
    // memory-fault candidates, as at process start (the ELF's writable
    // segments and the stack): every mapped page no read-only PT_LOAD covers
    img.mem_pages.clear();
    for (auto &kv : cpt.pages) {
        const uint64_t a = kv.first << 12;
        bool ro = false, w = false;
        for (const Seg &g : img.segs)
            if (a >= g.lo && a < g.hi) (g.w ? w : ro) = true;
        if (w || !ro) img.mem_pages.push_back(a);
    }
    img.brk0 = cpt.brk;
    img.svma_lo = img.svma_hi = 0;
    for (size_t i = 0; i < cpt.vmas.size(); i++)
        if (cpt.vma_names[i] == "stack") { img.svma_lo = cpt.vmas[i].first; img.svma_hi = cpt.vmas[i].second; }
    // a VMA list other than argsInit's lone stack VMA, or another mmap end:
    // the trials start from it (DevCtx::vm0)
    const bool plain = cpt.vmas.size() == 1 && cpt.vma_names[0] == "stack" && cpt.mmap_end == 0x4000000000000000ULL;
    img.vm0_on = !plain;
    if (img.vm0_on) {
        img.vm0.brk = cpt.brk; img.vm0.mmap_end = cpt.mmap_end;
        img.vm0.nvma = (uint32_t)cpt.vmas.size();
        for (size_t i = 0; i < cpt.vmas.size(); i++) { img.vm0.vma[i][0] = cpt.vmas[i].first; img.vm0.vma[i][1] = cpt.vmas[i].second; }
        HIPCHK(img.d_vm0.alloc(1));
        HIPCHK(hipMemcpy(img.d_vm0, &img.vm0, sizeof(VmState), hipMemcpyHostToDevice));
    }
    img.fp0_on = cpt.fp_state;
    memcpy(img.fp0, cpt.fregs, sizeof img.fp0);
    img.fcsr0 = cpt.fflags | (cpt.frm << 5);
    if (img.fp0_on) {
        HIPCHK(img.d_fp0.alloc(32));
        HIPCHK(hipMemcpy(img.d_fp0, img.fp0, 32 * 8, hipMemcpyHostToDevice));
    }
    img.tick0 = cpt.tick0;
    img.sp0 = cpt.regs[2];
    img.stack_min0 = cpt.stack_min & ~(kPage - 1);
    st = finish_load(e, img, cpt.regs, cpt.pc);
    if (!st) e->img = std::move(img);
    return st;
}

// ------------------------------------------------------------------ work buffers
// Growth replaces every work buffer (the tick map's and the capture rows
// with them): the old ones go first, the new ones move in once all are made.
static fi_status ensure_work(fi_engine *e, uint64_t n) {
    if (n <= e->w.cap) return FI_OK;
    e->w = Work{};
    Work w;
    fi_status st = work_buffers(e, w, n, nullptr);
    if (!st) e->w = std::move(w);
    return st;
}
// ... for a call of n trials: one launch's worth, at least one slot
static fi_status ensure_work_for(fi_engine *e, uint64_t n) {
    return ensure_work(e, std::min<uint64_t>(std::max<uint64_t>(n, 1), e->cfg.max_trials_per_launch));
}

// n entries in pieces of at most e->w.cap: fn(done, k) enqueues a piece's launch and copies on
// e->stream, which is then waited for (the calls that borrow chunk slot 0 outside a run)
static fi_status for_chunks(fi_engine *e, uint64_t n, const std::function<fi_status(uint64_t, uint64_t)> &fn) {
    for (uint64_t done = 0; done < n;) {
        const uint64_t k = std::min<uint64_t>(n - done, e->w.cap);
        const fi_status s = fn(done, k);
        if (s) return s;
        HIPCHK(hipStreamSynchronize(e->stream));
        done += k;
    }
    return FI_OK;
}

// The rewritten-code map's granule: one byte, coarser for large code so that
// a slot's map stays within kDmapWords x 32 bits (the solo kernel's LDS
// copy, fi_trial.hip kDmapWords).  (Byte granules: a store next to a loop's
// instructions leaves the loop's translated blocks usable.)
static void dmap_params(const fi_engine *e, uint32_t &shift, uint32_t &words) {
    const uint64_t cb = e->img.code_hi > e->img.code_lo ? e->img.code_hi - e->img.code_lo : 1;
    shift = 0;
    while ((cb >> shift) >= kDmapWords * 32) shift++;
    words = (uint32_t)((((cb + (1ULL << shift) - 1) >> shift) + 31) / 32);
}

static DevCtx base_ctx(fi_engine *e) {
    DevCtx c{};
    c.pre = e->img.d_pre; c.text_lo = e->img.text_lo; c.text_hi = e->img.text_hi; c.pre_ok = e->gold.pre_ok ? 1 : 0;
    c.text_bytes = (uint32_t)(e->img.text_hi - e->img.text_lo);
    c.code_lo = e->img.code_lo; c.code_hi = e->img.code_hi;
    c.snaps = e->img.d_snaps; c.snap_tab = e->img.d_tab; c.pool = e->img.d_pool; c.zero_page = e->img.d_zero;
    const bool start = !(e->cfg.flags & FI_CFG_NO_SNAPSHOT_START);
    c.n_snap = (uint32_t)e->img.snaps.size();
    c.snap_start = (start && !e->gold.golden_fp) ? 1 : 0;
    c.snap_interval = e->gold.snap_I;
    c.early_exit = (!(e->cfg.flags & FI_CFG_NO_EARLY_EXIT) && e->img.snaps.size() > 1 && !e->gold.golden_fp) ? 1 : 0;
    if (c.early_exit && !(e->cfg.flags & FI_CFG_NO_SDC_EXIT)) c.early_exit = 3;   // bit 1: SDC early exit
    c.hang_proof = (e->cfg.flags & FI_CFG_NO_HANG_PROOF) ? 0 : 1;
    c.gout = e->gold.d_gout; c.gerr = e->gold.d_gerr; c.gout_len = e->gold.gout.size(); c.gerr_len = e->gold.gerr.size();
    c.gexit = e->gold.info.exit_code;
    c.gdetail = e->gold.gdetail;
    c.gsub = e->gold.gsub;
    c.gninst = e->gold.info.ninst;
    c.priv_pages = e->cfg.private_pages;
    c.hang_cap = e->gold.info.ninst * e->cfg.hang_factor_x16 / 16 + 1000;
    c.protect_mask = e->protect;
    c.protect_opc = e->protect_opc;
    c.shadow_bits = e->issue_on ? e->gold.d_shadow : nullptr;
    c.priv_frames = e->w.d_priv; c.priv_vpn = e->w.d_priv_vpn;
    c.ov_frames = e->w.d_ov; c.ov_vpn = e->w.d_ov_vpn; c.ov_of = e->w.d_ov_of; c.ov_next = e->w.d_ov_next;
    c.ov_blocks = e->w.ov_blocks; c.ov_pages = e->w.ov_pages;
    c.tx_sink = e->img.d_sink;
    c.fregs = e->w.d_fregs;
    c.wave_dbg = e->w.d_wave_dbg;
    c.stats = e->w.d_stats;
    c.brk0 = e->img.brk0; c.svma_lo = e->img.svma_lo; c.svma_hi = e->img.svma_hi; c.vm = e->w.d_vm;
    c.simt_min = (e->cfg.flags & FI_CFG_SIMT) ? 8u : 0u;
    c.rnd_tab = e->d_rnd; c.rnd_len = e->d_rnd ? kRndLen : 0; c.clk_period = e->clk_period;
    c.exe_path = e->d_exe; c.exe_len = e->d_exe ? e->exe_path.size() : 0;
    c.tick0 = e->img.tick0;
    c.clk_until = e->gold.clk_until;
    c.stdin_data = e->stdin_on ? e->d_stdin : nullptr;
    c.stdin_len = e->stdin_on ? e->stdin_data.size() : 0;
    c.in_pos = e->w.d_inpos;
    c.fp0 = e->img.fp0_on ? e->img.d_fp0 : nullptr;
    c.fcsr0 = e->img.fcsr0;
    c.vm0 = e->img.vm0_on ? e->img.d_vm0 : nullptr;
    c.dmap = e->w.d_dmap;
    dmap_params(e, c.dmap_shift, c.dmap_words);
    c.lanes = e->cfg.lanes_per_wave;
    c.mem_live = (e->gold.mem_live && !(e->cfg.flags & FI_CFG_NO_EARLY_EXIT)) ? 1 : 0;
    c.mw_n = e->gold.mw_n; c.mw_addr = e->gold.d_mw_addr; c.mw_off = e->gold.d_mw_off; c.mw_ev = e->gold.d_mw_ev;
    return c;
}

// What a golden launch records, each optional (NULL / 0: not recorded).
struct GoldenRec {
    uint8_t *out = nullptr, *err = nullptr;   // stdout / stderr, `cap` bytes each
    uint64_t cap = 0;
    uint64_t interval = 0;                    // a snapshot every `interval` instructions, at most max_snaps
    uint32_t max_snaps = 0;
    SnapState *snaps = nullptr;
    uint8_t *pages = nullptr;
    uint64_t *vpns = nullptr;
    uint32_t *trace = nullptr, trace_cap = 0;   // the committed instructions and ecalls
    MemEv *mem = nullptr;                       // the data accesses
    uint32_t mem_cap = 0;
};

// One golden (fault-free, record-mode) launch: a single lane from snapshot 0
// with P private pages.
static fi_status golden_launch(fi_engine *e, uint32_t P, const GoldenRec &r, fi_outcome &o,
                               unsigned long long *stats) {
    DevBuf<uint64_t> gvpn, gfregs;   // (declared so that they are freed in the order gpriv, gfregs, gvpn)
    DevBuf<uint8_t> gpriv;
    HIPCHK(gpriv.alloc((uint64_t)P * kPage));
    HIPCHK(gvpn.alloc(P));
    HIPCHK(gfregs.alloc(33));   // 32 FP registers + fd 0's offset
    DevCtx c = base_ctx(e);
    c.fregs = gfregs.get();
    c.in_pos = gfregs.get() + 32;
    c.dmap = nullptr;
    c.ov_blocks = 0;   // (the golden run has its own P pages, no overflow pool)
    c.record = 1;
    c.early_exit = 0;
    c.snap_start = 0;
    c.rec_out = r.out; c.rec_err = r.err; c.rec_cap = r.cap;
    c.hang_cap = 1ULL << 30;   // golden safety cap
    c.priv_pages = P; c.priv_frames = gpriv.get(); c.priv_vpn = gvpn.get();
    c.rec_snaps = r.snaps; c.rec_pages = r.pages; c.rec_vpns = r.vpns; c.rec_interval = r.interval; c.rec_max_snaps = r.max_snaps;
    c.rec_trace = r.trace; c.rec_trace_cap = r.trace ? r.trace_cap : 0;
    c.rec_mem = r.mem; c.rec_mem_cap = r.mem ? r.mem_cap : 0;
    c.mem_live = 0;
    c.out = e->w.slot[0].d_out;   // (borrowed: no run is in flight)
    c.n = 1;
    c.n_slots = 1;
    c.sites = nullptr; c.perm = nullptr;
#define GLCHK(call) HIPCHK_AS("golden launch", call)
    GLCHK(hipMemsetAsync(e->w.d_stats, 0, kNStats * sizeof(unsigned long long), e->stream));
    GLCHK(hipEventRecord(e->ev0, e->stream));
    GLCHK(launch_trials(c, e->stream));
    GLCHK(hipEventRecord(e->ev1, e->stream));
    GLCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    GLCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    GLCHK(hipMemcpy(&o, e->w.slot[0].d_out, sizeof o, hipMemcpyDeviceToHost));
    GLCHK(hipMemcpy(stats, e->w.d_stats, kNStats * sizeof(unsigned long long), hipMemcpyDeviceToHost));
#undef GLCHK
    e->last_ms = ms;
    if (o.cls != FI_MASKED)
        return fail(e, FI_E_GOLDEN, "golden run did not exit normally (class %u sub %u detail %#x after %llu insts)",
                    o.cls, o.sub, o.detail, (unsigned long long)o.ninst);
    return FI_OK;
}

// Memory liveness index (DevCtx::mw_*): the golden run's data accesses split
// into 8-byte words, per word in time order as numInst << 16 | bytes read << 8
// | bytes written.  A trial's memory fault looks its word up at injection
// (fi_trial.hip:mem_dead).  complete = the access trace did not overflow and
// every golden instruction came from the pre-decoded text.
static fi_status build_mem_index(fi_engine *e, const std::vector<MemEv> &mev, bool complete) {
    if (!complete) return FI_OK;
    std::vector<std::pair<uint64_t, uint64_t>> ent;   // (word, event)
    const uint64_t kMaxEnt = 1ULL << 26;
    for (const MemEv &ev : mev) {
        const uint64_t len = ev.len_kind & ((1u << 30) - 1), kind = ev.len_kind >> 30;
        const uint64_t end = ev.addr + len;
        if (end < ev.addr) return FI_OK;
        for (uint64_t a = ev.addr; a < end;) {
            const uint64_t wd = a & ~7ULL, we = std::min(end, wd + 8);
            uint64_t bm = 0;
            for (uint64_t b = a; b < we; b++) bm |= 1ULL << (b - wd);
            // (bit 63: the proxy flag, carried through the sort and kept out of the events)
            ent.emplace_back(wd, ((uint64_t)(ev.t & ~kMemEvProxy) << 16) | ((kind & 1) ? bm << 8 : 0) |
                                     ((kind & 2) ? bm : 0) | ((ev.t & kMemEvProxy) ? 1ULL << 63 : 0));
            if (ent.size() > kMaxEnt) return FI_OK;
            a = we;
        }
    }
    std::stable_sort(ent.begin(), ent.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    std::vector<uint64_t> addr, evs;
    std::vector<uint32_t> off, proxy(ent.size() / 32 + 1, 0);
    evs.reserve(ent.size());
    for (size_t i = 0; i < ent.size(); i++) {
        if (i == 0 || ent[i].first != ent[i - 1].first) {
            addr.push_back(ent[i].first);
            off.push_back((uint32_t)i);
        }
        evs.push_back(ent[i].second & ~(1ULL << 63));
        if (ent[i].second >> 63) proxy[i >> 5] |= 1u << (i & 31);
    }
    off.push_back((uint32_t)ent.size());
    DevBuf<uint64_t> d_addr, d_ev;   // (moved in once all three are up)
    DevBuf<uint32_t> d_off;
    HIPCHK(d_addr.alloc(std::max<size_t>(addr.size(), 1)));
    HIPCHK(d_off.alloc(off.size()));
    HIPCHK(d_ev.alloc(std::max<size_t>(evs.size(), 1)));
    if (!addr.empty()) HIPCHK(hipMemcpy(d_addr, addr.data(), addr.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!evs.empty()) HIPCHK(hipMemcpy(d_ev, evs.data(), evs.size() * 8, hipMemcpyHostToDevice));
    e->gold.d_mw_addr = std::move(d_addr);
    e->gold.d_mw_off = std::move(d_off);
    e->gold.d_mw_ev = std::move(d_ev);
    e->gold.mw_n = (uint32_t)addr.size();
    e->gold.mw_nev = evs.size();
    e->gold.mw_proxy = std::move(proxy);
    e->gold.mem_live = true;
    return FI_OK;
}

// The golden run under TimingSimpleCPU (fi_tick.cpp, fi_timing.cpp): its
// attempts as requests, then their ticks.  t_status says why not, if not.
static void tick_prepare(fi_engine *e, const std::vector<MemEv> &mev, bool mev_ok) {
    if (e->cpu_model != FI_CPU_TIMING) { e->gold.t_status = "the CPU model is AtomicSimpleCPU (fi_set_cpu_model)"; return; }
    if (e->img.alloc_order.empty()) { e->gold.t_status = "a checkpoint start: its frame order is not known"; return; }
    if (e->gold.clk_until) { e->gold.t_status = "the golden run reads curTick: its output depends on the CPU model"; return; }
    if (e->gold.golden_unmapped) { e->gold.t_status = "the golden run unmaps memory: freed frames are reused"; return; }
    if (!mev_ok || e->gold.g_trace.empty()) { e->gold.t_status = "the golden access record is incomplete"; return; }
    TickGoldenIn in{&e->gold.g_trace, &e->gold.g_pre, e->img.text_lo, &mev, &e->img.alloc_order, e->img.stack_min0, e->img.svma_lo,
                    e->img.svma_hi, kStackBase, kMaxStack, e->gold.info.ninst, e->gold.info.ncycles};
    std::vector<TickAttempt> att;
    std::string why = build_tick_attempts(in, e->gold.t_ops, att);
    if (why.empty()) {
        e->gold.t_ticks.resize(e->gold.t_ops.size());
        if (fi_timing_model_run(e->gold.t_ops.data(), e->gold.t_ops.size(), &e->tparams, e->gold.t_ticks.data(), &e->gold.t_stats))
            why = "the timing model rejected the golden requests (a state gem5 asserts on)";
    }
    if (!why.empty()) {
        e->gold.t_ops.clear(); e->gold.t_ticks.clear();
        e->gold.t_status = why;
        return;
    }
    pack_tick_table(att, e->gold.t_ticks, e->gold.tk_done, e->gold.tk_rec);
    e->gold.t_status = "";
}

// ---- fi_golden_run's steps, in the order it takes them

// Step 1: no golden run, and the snapshot tables back to the image's own
// frames (the golden run appends its snapshots to them).
static fi_status golden_reset(fi_engine *e) {
    e->gold = Golden{};
    e->img.snaps.resize(1);
    e->img.tab.resize(e->img.n_start_frames);
    e->img.pool.resize((uint64_t)e->img.n_start_frames * kPage);
    return upload_snaps(e, e->img);
}

constexpr uint64_t kGoldenRecCap = 1 << 24;   // bytes of stdout / stderr the golden launches record

// Step 2, pass 1: the golden run itself (output, instruction count,
// footprint) into e->gold.info and the golden streams.  rec_out / rec_err stay
// allocated for pass 2.
static fi_status golden_pass1(fi_engine *e, DevBuf<uint8_t> &rec_out, DevBuf<uint8_t> &rec_err, fi_outcome &o,
                              uint64_t &gpages) {
    const uint32_t kGoldenPages = 4096;   // 16 MiB of written pages
    HIPCHK(rec_out.alloc(kGoldenRecCap));
    HIPCHK(rec_err.alloc(kGoldenRecCap));
    unsigned long long stats[kNStats];
    GoldenRec rec;
    rec.out = rec_out; rec.err = rec_err; rec.cap = kGoldenRecCap;
    fi_status st = golden_launch(e, kGoldenPages, rec, o, stats);
    if (st) return st;
    const uint64_t ol = stats[ST_GOLDEN_OUT_LEN], el = stats[ST_GOLDEN_ERR_LEN];
    gpages = stats[ST_PAGES];
    if (ol > kGoldenRecCap || el > kGoldenRecCap)
        return fail(e, FI_E_GOLDEN, "golden output exceeds %llu bytes", (unsigned long long)kGoldenRecCap);
    if (gpages >= kGoldenPages) return fail(e, FI_E_GOLDEN, "golden run writes more than %u pages", kGoldenPages);
    e->gold.gout.assign(ol, 0);
    e->gold.gerr.assign(el, 0);
    if (ol) HIPCHK(hipMemcpy(e->gold.gout.data(), rec_out.get(), ol, hipMemcpyDeviceToHost));
    if (el) HIPCHK(hipMemcpy(e->gold.gerr.data(), rec_err.get(), el, hipMemcpyDeviceToHost));
    HIPCHK(e->gold.d_gout.alloc(std::max<uint64_t>(ol, 1)));
    HIPCHK(e->gold.d_gerr.alloc(std::max<uint64_t>(el, 1)));
    if (ol) HIPCHK(hipMemcpy(e->gold.d_gout, e->gold.gout.data(), ol, hipMemcpyHostToDevice));
    if (el) HIPCHK(hipMemcpy(e->gold.d_gerr, e->gold.gerr.data(), el, hipMemcpyHostToDevice));
    e->gold.info.ninst = o.ninst;
    e->gold.info.ncycles = stats[ST_GOLDEN_NCYCLES];
    e->gold.info.exit_code = o.exit_code;
    e->gold.info.stdout_len = ol;
    e->gold.info.stderr_len = el;
    e->gold.info.fetch_bytes = stats[ST_FETCH_BYTES];
    e->gold.info.data_bytes = stats[ST_DATA_BYTES];
    e->gold.gdetail = o.detail;
    e->gold.gsub = o.sub;
    e->gold.golden_fp = stats[ST_GOLDEN_EXTRA_STATE] != 0;
    e->gold.clk_until = stats[ST_CLK_UNTIL];
    return FI_OK;
}

// What pass 2 brings back to the host.
struct GoldenCapture {
    uint64_t I = 0;                  // snapshot interval
    uint32_t P = 0;                  // pages captured per snapshot (row pitch of pages / vpns)
    fi_outcome o{};                  // the capture run's outcome
    uint64_t n_snaps = 0;            // snapshots it took (ST_SNAPS_CAPTURED)
    uint64_t n_events = 0;           // its trace events (ST_TRACE_EVENTS; trace is empty if they overflowed)
    bool mem_ok = false;             // its access events fit their buffer: mev holds them all
    bool unmapped = false;           // ST_GOLDEN_UNMAPPED
    std::vector<SnapState> snaps;    // tab_n = pages captured with the snapshot
    std::vector<uint8_t> pages;
    std::vector<uint64_t> vpns;
    std::vector<uint32_t> trace;
    std::vector<PreInst> pre;        // the pre-decoded text, leader flags cleared
    std::vector<MemEv> mev;
};

// Step 3, pass 2: the same run again, capturing a snapshot every I committed
// instructions (state + every page written so far), within ~1 GiB; with it
// the golden trace and data accesses.  Releases rec_out / rec_err.
static fi_status golden_pass2(fi_engine *e, const fi_outcome &o, uint64_t gpages, DevBuf<uint8_t> &rec_out,
                              DevBuf<uint8_t> &rec_err, GoldenCapture &g) {
    uint64_t I = std::max<uint64_t>(e->cfg.snapshot_interval ? e->cfg.snapshot_interval : 256, 16);
    const uint32_t P = (uint32_t)std::max<uint64_t>(gpages, 1);
    while (o.ninst / I + 2 > 65536 || (o.ninst / I + 2) * P * kPage > (1ULL << 30)) I *= 2;
    const uint32_t rec_max = (uint32_t)(o.ninst / I + 2);
    DevBuf<uint64_t> d_rv;   // (declared so that they are freed in the order d_rs, d_rp, d_rv)
    DevBuf<uint8_t> d_rp;
    DevBuf<SnapState> d_rs;
    HIPCHK(d_rs.alloc(rec_max));
    HIPCHK(d_rp.alloc((uint64_t)rec_max * P * kPage));
    HIPCHK(d_rv.alloc((uint64_t)rec_max * P));
    // golden trace for the register liveness pass: one entry per committed
    // instruction and ecall (capped; without it every register counts as live)
    const uint32_t trace_cap = (uint32_t)std::min<uint64_t>(o.ninst + 4096, 1ULL << 26);
    DevBuf<uint32_t> d_trace;
    HIPCHK(d_trace.alloc(trace_cap));
    // and its data accesses for the memory liveness index
    const uint32_t mem_cap = (uint32_t)std::min<uint64_t>(2 * o.ninst + 4096, 1ULL << 24);
    DevBuf<MemEv> d_mem;
    HIPCHK(d_mem.alloc(mem_cap));
    unsigned long long stats[kNStats] = {};
    GoldenRec rec;
    rec.out = rec_out; rec.err = rec_err; rec.cap = kGoldenRecCap;
    rec.interval = I; rec.max_snaps = rec_max; rec.snaps = d_rs; rec.pages = d_rp; rec.vpns = d_rv;
    rec.trace = d_trace; rec.trace_cap = trace_cap;
    rec.mem = d_mem; rec.mem_cap = mem_cap;
    fi_status st = golden_launch(e, P, rec, g.o, stats);
    rec_out.reset();
    rec_err.reset();
    g.I = I;
    g.P = P;
    g.n_snaps = stats[ST_SNAPS_CAPTURED];
    g.n_events = stats[ST_TRACE_EVENTS];
    g.unmapped = stats[ST_GOLDEN_UNMAPPED] != 0;
    if (!st && g.n_events <= trace_cap) {
        g.trace.resize(g.n_events);
        g.pre.resize((e->img.text_hi - e->img.text_lo) / 2);
        hipError_t err = hipMemcpy(g.trace.data(), d_trace.get(), g.n_events * 4, hipMemcpyDeviceToHost);
        if (err == hipSuccess)
            err = hipMemcpy(g.pre.data(), e->img.d_pre, g.pre.size() * sizeof(PreInst), hipMemcpyDeviceToHost);
        for (auto &p : g.pre) p.flags &= (uint8_t)~(kPreLeader | kPreOddLeader);
        if (err != hipSuccess) st = fail(e, FI_E_HIP, "trace download: %s", hipGetErrorString(err));
    }
    d_trace.reset();
    const uint64_t n_mem = stats[ST_MEM_EVENTS];
    g.mem_ok = n_mem <= mem_cap;
    if (!st && g.mem_ok) {
        g.mev.resize(n_mem);
        hipError_t err =
            n_mem ? hipMemcpy(g.mev.data(), d_mem.get(), n_mem * sizeof(MemEv), hipMemcpyDeviceToHost) : hipSuccess;
        if (err != hipSuccess) st = fail(e, FI_E_HIP, "access trace download: %s", hipGetErrorString(err));
    }
    d_mem.reset();
    if (!st) {
        const uint32_t ns = (uint32_t)std::min<unsigned long long>(g.n_snaps, rec_max);
        g.snaps.resize(ns);
        g.pages.resize((uint64_t)ns * P * kPage);
        g.vpns.resize((uint64_t)ns * P);
        hipError_t err = hipMemcpy(g.snaps.data(), d_rs.get(), ns * sizeof(SnapState), hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(g.pages.data(), d_rp.get(), g.pages.size(), hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(g.vpns.data(), d_rv.get(), g.vpns.size() * 8, hipMemcpyDeviceToHost);
        if (err != hipSuccess) st = fail(e, FI_E_HIP, "snapshot download: %s", hipGetErrorString(err));
    }
    return st;   // (the snapshot capture buffers go here: before upload_snaps)
}

// Step 4: deduplicate the captured frames into e->img.pool and build one sorted
// page table per snapshot (fi_golden_host.h).
static void golden_snap_tables(fi_engine *e, const GoldenCapture &g) {
    std::vector<SnapState> snaps;
    std::vector<PageEnt> tab;
    e->gold.pre_ok = dedupe_snapshot_pages(e->img.tab.data(), e->img.n_start_frames, e->img.pool, e->img.pages, e->img.code_lo, e->img.code_hi,
                                      g.snaps, g.pages, g.vpns, g.P, snaps, tab);
    e->img.snaps = std::move(snaps);
    e->img.tab = std::move(tab);
    e->gold.snap_I = g.I;
}

// Step 5: register liveness at each snapshot (fi_golden_host.h); keeps the
// trace and the text it indexes when it is usable.  Returns live_ok.
static bool golden_liveness(fi_engine *e, const GoldenCapture &g, std::vector<uint32_t> &rmask,
                            std::vector<uint32_t> &wmask) {
    const bool live_ok = trace_liveness(g.pre, g.trace, g.n_events, OP_m5op, rmask, wmask, e->img.snaps);
    if (live_ok && !g.trace.empty()) { e->gold.g_pre = g.pre; e->gold.g_trace = g.trace; }
    return live_ok;
}

// Step 6: first-access index (DESIGN.md §4 "first-access forwarding"): a
// register flipped at numInst t is neither read nor written by the golden
// run before its next access, so flipping it at that access instead gives
// the same machine; written first (or never touched again) it is dead.
static fi_status golden_first_access(fi_engine *e, const GoldenCapture &g, bool live_ok,
                                     const std::vector<uint32_t> &rmask, const std::vector<uint32_t> &wmask) {
    if (!live_ok || g.trace.empty() || e->gold.info.ninst >= (1ULL << 29)) return FI_OK;
    std::vector<uint32_t> off, ev;
    first_access_index(g.trace, rmask, wmask, off, ev);
    HIPCHK(e->gold.d_fw_off.alloc(33));
    HIPCHK(e->gold.d_fw_ev.alloc(std::max<size_t>(ev.size(), 1)));
    HIPCHK(hipMemcpy(e->gold.d_fw_off, off.data(), 33 * 4, hipMemcpyHostToDevice));
    if (!ev.empty()) HIPCHK(hipMemcpy(e->gold.d_fw_ev, ev.data(), ev.size() * 4, hipMemcpyHostToDevice));
    e->gold.fw_off = std::move(off);
    e->gold.fw_ev = std::move(ev);
    e->gold.fw_ok = true;
    return FI_OK;
}

// Step 7: translate the golden basic blocks and build the trial kernel with
// them (hipRTC); the static kernel stays the fallback.  Takes g.pre.
static fi_status golden_translate(fi_engine *e, GoldenCapture &g, bool live_ok) {
    if (e->cfg.flags & FI_CFG_NO_TRANSLATE) e->gold.tx_status = "disabled (FI_CFG_NO_TRANSLATE)";
    else if (!e->gold.pre_ok) e->gold.tx_status = "golden run rewrites its text";
    else if (!live_ok || g.trace.empty()) e->gold.tx_status = "golden trace unavailable";
    else {
        // (snapshot pcs are not leaders: they fall all over the hot loops and
        // would cut the blocks into single instructions; a wave that starts
        // mid-block steps to the next leader in the interpreter)
        const std::vector<uint64_t> pcs;
        std::vector<uint32_t> leaders;
        std::vector<LoopEst> loops;
        uint32_t n_tx = 0;
        const bool ahead = !(e->cfg.flags & FI_CFG_NO_LOAD_AHEAD);   // (part of the text, which keys the code-object caches)
        const bool stretch = !(e->cfg.flags & FI_CFG_NO_LOOP_STRETCH);   // (likewise)
        std::string body = translate_blocks(g.pre, e->img.text_lo, g.trace, pcs, leaders, n_tx, true, &loops, ahead, stretch);
        if (n_tx > 24000) {   // the odd-pc streams make it too large: without them
            leaders.clear();
            loops.clear();
            body = translate_blocks(g.pre, e->img.text_lo, g.trace, pcs, leaders, n_tx, false, &loops, ahead, stretch);
        }
        if (!loops.empty() && !(e->cfg.flags & FI_CFG_NO_LOOP_ORDER)) {
            HIPCHK(e->gold.d_loops.alloc(loops.size()));
            HIPCHK(hipMemcpy(e->gold.d_loops, loops.data(), loops.size() * sizeof(LoopEst), hipMemcpyHostToDevice));
            e->gold.n_loops = (uint32_t)loops.size();
        }
        e->gold.tx_body = body;
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, e->dev));
        if (const char *dump = getenv("SHREWD_FI_DUMP_TX")) {   // diagnostics: the generated blocks
            if (FILE *f = fopen(dump, "w")) { fputs(body.c_str(), f); fclose(f); }
        }
        if (leaders.empty()) {   // nothing hot: the static kernels (pre-decoded + general interpreter) run everything
            e->gold.tx_status = "nothing to translate (no code run twice)";
        } else if (n_tx > 24000) {   // more than the load-time compiler handles in reasonable time
            e->gold.tx_status = "translation too large";
        } else {
            auto j = std::make_shared<JitJob>();
            j->body = body;
            j->arch = prop.gcnArchName;
            j->odd = jit_has_odd(body);
            j->use_cache = !(e->cfg.flags & FI_CFG_JIT_NO_CACHE);
            for (uint32_t h : leaders) g.pre[h & 0x7FFFFFFFu].flags |= (h >> 31) ? kPreOddLeader : kPreLeader;
            e->gold.jit_pre = std::move(g.pre);
            e->gold.jit_blocks = leaders.size();
            e->gold.jit_insts = n_tx;
            e->gold.jit = j;
            e->gold.tx_status = "compiling";
            e->jit_threads.emplace_back(std::thread(jit_job_run, j), j);
        }
    }
    return FI_OK;
}

fi_status fi_golden_run(fi_engine *e, fi_golden_info *out) {
    if (!e) return FI_E_ARG;
    if (!e->img.loaded) return fail(e, FI_E_STATE, "fi_golden_run: no workload loaded");
    HIPCHK(hipSetDevice(e->dev));
    fi_status st = ensure_work(e, 64);
    if (st) return st;
    st = golden_reset(e);
    if (st) return st;

    fi_outcome o;
    uint64_t gpages = 0;
    double golden_ms = 0;
    GoldenCapture g;
    {
        DevBuf<uint8_t> rec_out, rec_err;   // both passes record into them; pass 2 releases them
        st = golden_pass1(e, rec_out, rec_err, o, gpages);
        if (st) return st;
        golden_ms = e->last_ms;
        st = golden_pass2(e, o, gpages, rec_out, rec_err, g);
        if (st) return st;
    }
    if (g.o.ninst != o.ninst || g.o.detail != o.detail || g.n_snaps != o.ninst / g.I + 1)
        return fail(e, FI_E_GOLDEN, "golden capture pass diverged from the golden run");

    golden_snap_tables(e, g);
    std::vector<uint32_t> rmask, wmask;
    const bool live_ok = golden_liveness(e, g, rmask, wmask);
    st = golden_first_access(e, g, live_ok, rmask, wmask);
    if (st) return st;
    st = upload_snaps(e, e->img);
    if (st) return st;
    st = build_mem_index(e, g.mev, live_ok && g.mem_ok);
    if (st) return st;
    e->gold.golden_unmapped = g.unmapped;
    tick_prepare(e, g.mev, !g.trace.empty() && g.mem_ok);
    st = golden_translate(e, g, live_ok);
    if (st) return st;

    e->last_ms = golden_ms;
    e->gold.info.snapshots = e->img.snaps.size();
    e->gold.info.snapshot_interval = g.I;
    e->gold.info.snapshot_frames = e->img.pool.size() / kPage;
    e->gold.have_golden = true;
    if (e->issue_on) {   // the model follows the new golden run
        st = compute_shadow(e);
        if (st) return st;
    }
    if (out) *out = e->gold.info;
    return FI_OK;
}

fi_status fi_golden_stdout(fi_engine *e, uint8_t *buf, uint64_t cap, uint64_t *len) {
    if (!e || !e->gold.have_golden) return fail(e, FI_E_STATE, "no golden run");
    if (buf && cap) memcpy(buf, e->gold.gout.data(), std::min<uint64_t>(cap, e->gold.gout.size()));
    if (len) *len = e->gold.gout.size();
    return FI_OK;
}

fi_status fi_golden_stderr(fi_engine *e, uint8_t *buf, uint64_t cap, uint64_t *len) {
    if (!e || !e->gold.have_golden) return fail(e, FI_E_STATE, "no golden run");
    if (buf && cap) memcpy(buf, e->gold.gerr.data(), std::min<uint64_t>(cap, e->gold.gerr.size()));
    if (len) *len = e->gold.gerr.size();
    return FI_OK;
}

fi_status fi_set_campaign(fi_engine *e, uint64_t seed, uint64_t structures, uint32_t burst) {
    if (!e) return FI_E_ARG;
    structures &= ~1ULL;
    structures &= (1ULL << FI_N_STRUCT) - 1;
    if (!structures) return fail(e, FI_E_ARG, "no fault structures selected");
    if (burst < 1 || burst > 64) return fail(e, FI_E_ARG, "burst must be 1..64");
    e->seed = seed; e->structures = structures; e->burst = burst;
    e->bits = ~0ULL;
    return FI_OK;
}

fi_status fi_set_exe_path(fi_engine *e, const char *path) {
    if (!e) return FI_E_ARG;
    if (e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_exe_path: set before fi_golden_run (the golden run sees it)");
    HIPCHK(hipSetDevice(e->dev));
    e->exe_path = path ? path : "";
    if (e->exe_path.size() >= 4096) { e->exe_path.clear(); return FI_E_ARG; }   // PATH_MAX
    e->d_exe.reset();
    if (!e->exe_path.empty()) {
        HIPCHK(e->d_exe.alloc(e->exe_path.size()));
        HIPCHK(hipMemcpy(e->d_exe, e->exe_path.data(), e->exe_path.size(), hipMemcpyHostToDevice));
    }
    return FI_OK;
}

fi_status fi_set_stdin(fi_engine *e, const uint8_t *data, uint64_t len) {
    if (!e) return FI_E_ARG;
    if (e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_stdin: set before fi_golden_run (the golden run reads it)");
    if (data && len >= (1ULL << 40)) return fail(e, FI_E_ARG, "fi_set_stdin: input larger than 1 TiB");
    HIPCHK(hipSetDevice(e->dev));
    e->d_stdin.reset();
    e->stdin_data.clear();
    e->stdin_on = data != nullptr;
    if (!data) return FI_OK;
    e->stdin_data.assign(data, data + len);
    HIPCHK(e->d_stdin.alloc(std::max<uint64_t>(len, 1)));
    if (len) HIPCHK(hipMemcpy(e->d_stdin, data, len, hipMemcpyHostToDevice));
    return FI_OK;
}

fi_status fi_set_clock(fi_engine *e, uint64_t period_ticks, uint64_t random_seed) {
    if (!e || !period_ticks) return FI_E_ARG;
    if (e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_clock: set before fi_golden_run (the golden run sees it)");
    HIPCHK(hipSetDevice(e->dev));
    e->clk_period = period_ticks;
    e->rnd_seed = random_seed;
    return upload_rnd(e);
}

fi_status fi_set_bits(fi_engine *e, uint64_t bits_mask) {
    if (!e) return FI_E_ARG;
    if (!e->structures) return fail(e, FI_E_STATE, "fi_set_campaign first");
    const uint64_t valid = e->burst == 1 ? ~0ULL : ((2ULL << (64 - e->burst)) - 1);
    if (!(bits_mask & valid)) return fail(e, FI_E_ARG, "no eligible bit position for a %u-bit burst", e->burst);
    e->bits = bits_mask;
    return FI_OK;
}

fi_status fi_set_protect(fi_engine *e, uint64_t protect_mask) {
    if (!e) return FI_E_ARG;
    e->protect = protect_mask;
    return FI_OK;
}

fi_status fi_set_protect_opclasses(fi_engine *e, uint64_t opclass_mask) {
    if (!e) return FI_E_ARG;
    e->protect_opc = opclass_mask;
    return FI_OK;
}

fi_status fi_set_issue_model(fi_engine *e, const fi_issue_params *p) {
    if (!e) return FI_E_ARG;
    if (!p) {
        e->issue_on = false;
        return FI_OK;
    }
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_issue_model: no golden run");
    const fi_issue_params keep = e->issue_p;
    e->issue_p = *p;
    const fi_status st = compute_shadow(e);
    if (st) { e->issue_p = keep; return st; }
    e->issue_on = true;
    return FI_OK;
}

fi_status fi_shadow_map(fi_engine *e, uint8_t *shadow, uint64_t cap, uint64_t *n, fi_issue_stats *stats) {
    if (!e) return FI_E_ARG;
    if (!e->issue_on) return fail(e, FI_E_STATE, "fi_shadow_map: the issue model is off");
    if (shadow && cap) memcpy(shadow, e->gold.shadow.data(), std::min<uint64_t>(cap, e->gold.shadow.size()));
    if (n) *n = e->gold.shadow.size();
    if (stats) *stats = e->gold.issue_stats;
    return FI_OK;
}

// The campaign's draw from trial `first` on (fi_site_draw.h); memory words only where there are some
static DrawCtx campaign_draw(fi_engine *e, uint64_t first) {
    const uint64_t structures = e->img.mem_pages.empty() ? e->structures & ~(1ULL << FI_T_MEM) : e->structures;
    return draw_ctx(e->seed, structures, first, e->bits, e->burst);
}

static SampleCtx sample_ctx(fi_engine *e, uint64_t first) {
    SampleCtx s{};
    s.d = campaign_draw(e, first);
    s.golden_ninst = e->gold.info.ninst;
    s.mem_pages = e->img.d_mem_pages;
    s.n_mem_pages = e->img.mem_pages.size();
    return s;
}

fi_status fi_sample_sites(fi_engine *e, uint64_t first, uint64_t n, fi_site *out) {
    if (!e || !out) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "golden run required before sampling");
    if (!e->structures) return fail(e, FI_E_STATE, "fi_set_campaign first");
    HIPCHK(hipSetDevice(e->dev));
    const fi_status st = ensure_work_for(e, n);
    if (st) return st;
    return for_chunks(e, n, [&](uint64_t done, uint64_t k) -> fi_status {
        const ChunkSlot &s0 = e->w.slot[0];
        HIPCHK(launch_sample(sample_ctx(e, first + done), k, s0.d_sites, e->w.d_keys, e->w.d_perm, e->stream));
        HIPCHK(hipMemcpyAsync(out + done, s0.d_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        return FI_OK;
    });
}

// The trial kernel: the load-time build with translated blocks when there is
// one, else the static (interpreter-only) kernel.
// solo: the one-trial-per-wave build, one workgroup (kSoloLanes identical lanes) per slot.
static hipError_t launch_trial_kernel(fi_engine *e, DevCtx &c, hipStream_t st, bool solo) {
    void *args[] = {&c};
    if (solo) {
        if (!e->gold.tx.fn_solo) return launch_trials_solo(c, st);
        return hipModuleLaunchKernel(e->gold.tx.fn_solo, (unsigned)c.n, 1, 1, kSoloLanes, 1, 1, 0, st, args, nullptr);
    }
    if (!e->gold.tx.fn) return launch_trials(c, st);
    const uint32_t gl = (c.resume && c.resume_waves) ? 1u : c.lanes;   // grid for the fewest lanes per wave
    return hipModuleLaunchKernel(e->gold.tx.fn, (unsigned)((c.n + gl - 1) / gl), 1, 1, 64, 1, 1, 0, st, args,
                                 nullptr);
}

// The event pair of the next trial-kernel dispatch (kind: 0 the 64-lane
// kernel, 1 solo, 2 solo-odd; fi_debug_dispatch_ms).
static constexpr size_t kTimerSlots = 4096;   // dispatch timers kept between fi_kernel_timer_reset calls (a ring)
static std::pair<hipEvent_t, hipEvent_t> &timer_slot(fi_engine *e, uint32_t kind) {
    if (e->tused == kTimerSlots) e->tused = 0;
    if (e->tused == e->tpool.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        e->tpool.emplace_back(a, b);
        e->tkind.push_back(0);
    }
    e->tkind[e->tused] = kind;
    return e->tpool[e->tused++];
}

// One pass over sites[0..k) (keys/perm set) with P private pages per slot:
// forwarding, sort by inject time, the epochs.  Outcomes to d_out.
// tick: the sites are mapped tick sites -- this engine's clock is
// AtomicSimpleCPU's, so a curTick read escapes (DevCtx::clk_esc).
// disp (device-mapped chunks, else NULL): trials with disp[i] != 0 are parked --
// dead at injection, so the trial kernels end them at once as the golden run.
// cs (a capture call's chunks, else NULL): the trials' output goes to that
// slot's capture buffers, trial i of sites to row cidx[i] (NULL: row i).
static fi_status run_pass(fi_engine *e, fi_site *sites, uint64_t k, fi_outcome *d_out, uint32_t P, hipStream_t st,
                          bool tick, const uint8_t *disp = nullptr, const ChunkSlot *cs = nullptr,
                          const uint32_t *cidx = nullptr) {
    int end_bit = 64 - __builtin_clzll(std::max<uint64_t>(e->gold.info.ninst, 1));
    // (a dead site ends at injection: an early exit, so not with FI_CFG_NO_EARLY_EXIT)
    const bool fwd = e->gold.fw_ok && !(e->cfg.flags & (FI_CFG_NO_FORWARD | FI_CFG_NO_EARLY_EXIT));
    if (fwd) {
        FwdCtx fc{};
        fc.reg_off = e->gold.d_fw_off; fc.reg_ev = e->gold.d_fw_ev;
        // memory sites only when the golden run's mappings are static (no VM
        // syscalls: golden_fp covers them) and its access index is complete
        const bool memf = e->gold.mem_live && !e->gold.golden_fp && e->img.snaps.size() > 1;
        fc.mw_n = memf ? e->gold.mw_n : 0;
        fc.mw_addr = e->gold.d_mw_addr; fc.mw_off = e->gold.d_mw_off; fc.mw_ev = e->gold.d_mw_ev;
        fc.snaps = e->img.d_snaps; fc.snap_tab = e->img.d_tab; fc.n_snap = (uint32_t)e->img.snaps.size();
        fc.snap_interval = e->gold.snap_I; fc.text_lo = e->img.text_lo; fc.text_hi = e->img.text_hi;
        HIPCHK(launch_forward(sites, k, fc, e->w.d_keys, e->w.d_eff, st));
    }
    // (without forwarding the parked trials still need eff: the identity for the rest)
    if (disp) HIPCHK(launch_tick_park(sites, disp, k, fwd ? 0u : 1u, e->w.d_keys, e->w.d_eff, st));
    HIPCHK(sort_pairs(e->w.d_tmp, e->w.tmp_bytes, e->w.d_keys, e->w.d_keys2, e->w.d_perm, e->w.d_perm2, k, end_bit, st));
    DevCtx c = base_ctx(e);
    c.sites = sites;
    c.perm = e->w.d_perm2;
    c.eff = (fwd || disp) ? e->w.d_eff : nullptr;
    c.out = d_out;
    c.n = k;
    c.n_slots = (uint32_t)k;
    c.save = e->w.d_save;
    c.priv_pages = P;
    c.clk_esc = tick ? 1u : 0u;
    if (cs) {
        c.cap_out = cs->cap.d_out; c.cap_err = cs->cap.d_err; c.cap_len = cs->cap.d_len;
        c.cap_idx = cidx;
        c.cap_bytes = e->w.cx.bytes; c.cap_stride = e->w.cx.stride;
    }
    if (P != e->cfg.private_pages) c.ov_blocks = 0;   // the second pass has its own P' (chunk_end)
    if (c.ov_blocks) HIPCHK(hipMemsetAsync(e->w.d_ov_next, 0, 4, st));
    HIPCHK(hipMemsetAsync(e->w.d_cnt, 0, 16 * 4, st));
    HIPCHK(hipMemsetAsync(e->w.d_wave_dbg, 0, k * kWaveDbgWords * sizeof(uint64_t), st));
    const bool pack = (e->cfg.flags & FI_CFG_PACK_RUNS) != 0;
    int n_cu = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->dev));
    const uint32_t spread = (e->cfg.flags & FI_CFG_FIXED_RESUME) ? 0u : (uint32_t)std::max(1, n_cu) * 4u;   // SIMDs
    if (pack) HIPCHK(hipMemsetAsync(e->w.d_nwaves, 0, 16 * 4, st));
    // epochs: each wave runs a bounded number of loop
    // iterations, then its live lanes are suspended, sorted by pc and resumed
    // densely packed; the last epoch runs to completion.  All asynchronous:
    // resume grids are sized for every slot and surplus waves exit at once.
    std::vector<uint32_t> budgets;
    if (e->cfg.flags & FI_CFG_NO_EPOCHS) {
        budgets = {0};
    } else {
        const uint32_t b = e->cfg.epoch_iters ? e->cfg.epoch_iters : 384;
        // default: one 64-lane epoch, then every survivor to completion on the
        // solo kernel (profiles/r02c epoch_sweep: 2 epochs beat 3 and 4; with
        // first-access forwarding a 1024-iteration first epoch beat 4096:
        // crc32 12.7M vs 9.8M, qsort +3 %, intmix even, profiles/r02l_ab.txt;
        // with the round-5 solo kernel 384 beats 1024: crc32 4.77 vs 4.96 ms,
        // qsort 30.9 vs 32.2 ms, intmix 257 vs 253 ms, profiles/ep_sweep_r05*.jsonl)
        const uint32_t n_ep = e->cfg.epochs ? std::max(2u, std::min(e->cfg.epochs, 14u)) : 2u;
        for (uint32_t i = 0; i + 1 < n_ep; i++) budgets.push_back(b << (2 * std::min(i, 2u)));
        budgets.push_back(0);
    }
    // the odd-pc survivors of a resumed solo epoch run on the solo-odd kernel
    // (at most kOddGrid of them; the rest stay with the solo kernel), on its
    // own stream beside the solo kernel
    constexpr uint32_t kOddGrid = 2048;
    const bool odd_on = e->gold.tx.fn_odd && e->gold.tx.fn_solo && !(e->cfg.flags & FI_CFG_NO_ODD_KERNEL);
    if (odd_on) HIPCHK(hipMemsetAsync(e->w.d_split, 0, 64 * 4, st));
    for (size_t ep = 0; ep < budgets.size(); ep++) {
        const bool solo = (e->cfg.flags & FI_CFG_SOLO_ALL) || (ep > 0 && !(e->cfg.flags & FI_CFG_NO_SOLO));
        const bool odd = odd_on && solo && ep > 0 && ep < 16;
        c.wave_budget = budgets[ep];
        c.surv = e->w.d_surv[ep & 1];
        c.surv_n = e->w.d_cnt + ep;
        c.lanes = ep == 0 ? e->cfg.lanes_per_wave : e->cfg.resume_lanes;
        c.wrange = nullptr;
        c.n_waves = nullptr;
        c.resume_waves = ep == 0 ? 0u : spread;
        if (ep == 0) {
            c.resume = nullptr;
            c.resume_n = nullptr;
        } else {
            // survivors not yet injected form a tier right after the first
            // (fi_surv_keys_kernel; profiles/r04au: intmix -3 %, qsort -3 %
            // per step against the two-tier order)
            const uint32_t skey = (solo && !pack) ? 3u : 0u;
            // solo keys: tier above numInst, which stays below the hang cap -- a
            // key of nb + 2 bits (+ 1 for the odd-pc flag) sorts in fewer passes
            const uint32_t nb = 64u - (uint32_t)__builtin_clzll(std::max<uint64_t>(c.hang_cap, 1));
            HIPCHK(launch_surv_keys(e->w.d_save, e->w.d_surv[(ep - 1) & 1], e->w.d_cnt + ep - 1, k, c.text_lo, e->w.d_skeys,
                                    e->w.d_svals, odd ? e->w.d_split + 4 * ep : nullptr, skey, e->gold.info.ninst, nb,
                                    e->gold.d_loops, e->gold.n_loops, c.hang_cap, st));
            HIPCHK(sort_pairs(e->w.d_tmp, e->w.tmp_bytes, e->w.d_skeys, e->w.d_skeys2, e->w.d_svals, e->w.d_svals2, k,
                              skey ? (int)std::min(64u, nb + 3u) : 64, st));
            c.resume = e->w.d_svals2;
            c.resume_n = e->w.d_cnt + ep - 1;
            if (odd) {   // odd survivors sort last: the solo kernel takes [0, split), the solo-odd kernel the rest
                const uint32_t grid = (uint32_t)std::min<uint64_t>(k, kOddGrid);
                HIPCHK(launch_odd_split(c.resume_n, e->w.d_split + 4 * ep, e->w.d_split + 4 * ep + 1, grid, st));
                DevCtx co = c;
                co.lanes = 1; co.resume_waves = 0; co.wrange = nullptr; co.n_waves = nullptr;
                co.resume_lo = e->w.d_split + 4 * ep + 1;
                c.resume_n = e->w.d_split + 4 * ep + 1;
                HIPCHK(hipEventRecord(e->ev_fork, st));
                HIPCHK(hipStreamWaitEvent(e->stream_odd, e->ev_fork, 0));
                auto &tq = timer_slot(e, 2);
                co.span = e->d_span ? e->d_span + 2 * (e->tused - 1) : nullptr;
                HIPCHK(hipEventRecord(tq.first, e->stream_odd));
                void *args[] = {&co};
                HIPCHK(hipModuleLaunchKernel(e->gold.tx.fn_odd, grid, 1, 1, kSoloLanes, 1, 1, 0, e->stream_odd, args, nullptr));
                HIPCHK(hipEventRecord(tq.second, e->stream_odd));
                HIPCHK(hipEventRecord(e->ev_join, e->stream_odd));
            }
            if (pack && !solo) {
                // one wave per same-pc run of survivors (<= 64 lanes); the grid
                // covers the worst case (every survivor alone), surplus waves exit
                HIPCHK(launch_pack_runs(e->w.d_skeys2, c.resume_n, k, e->w.d_wrange + 0, e->w.d_nwaves + ep, st));
                c.wrange = e->w.d_wrange;
                c.n_waves = e->w.d_nwaves + ep;
                c.lanes = 1;
                c.resume_waves = 0;
            }
        }
        // every dispatch of the trial kernel is bracketed by its own event
        // pair on the launch stream (the bench's per-dispatch kernel time)
        auto &tp = timer_slot(e, solo ? 1 : 0);
        c.span = e->d_span ? e->d_span + 2 * (e->tused - 1) : nullptr;
        HIPCHK(hipEventRecord(tp.first, st));
        if (solo) { c.lanes = 1; c.resume_waves = 0; c.wrange = nullptr; c.n_waves = nullptr; }
        HIPCHK(launch_trial_kernel(e, c, st, solo));
        HIPCHK(hipEventRecord(tp.second, st));
        if (odd) HIPCHK(hipStreamWaitEvent(st, e->ev_join, 0));
    }
    return FI_OK;
}

// Chunks are pipelined on the launch stream with no host wait between them
// (DESIGN.md §4e): chunk i runs its pass and lists its resource escapes
// (FI_ESC_RESOURCE: an engine capacity limit -- the overflow pool ran dry --
// not gem5 behaviour) and copies their count to pinned memory; the host then
// enqueues chunk i+1 and only after that reads chunk i's count, while the GPU
// is busy with chunk i+1.  Chunk i's second pass (redo_pages-fold pages, in
// batches that reuse the same frames: batch x P' <= k x P), its histogram and
// its host copy follow chunk i+1 on the stream; their outcomes replace the
// escapes.  The two chunks in flight alternate between the two ChunkSlots.
// FI_CFG_NO_REDO keeps the escapes.

// How chunk_end tallies a chunk; chunk_fill records it.
struct Tally {
    // the site array that keys the histogram: the run sites, or -- a chunk mapped on the device, whose
    // disp != 0 trials are parked (run_pass) and fixed (chunk_end) -- the tick sites
    enum Key { kRunSites, kTickSites } key = kRunSites;
    enum Weight { kNone, kW32, kW64 } weight = kNone;   // unweighted, ChunkSlot::d_weight, ChunkSlot::d_xt_weight
    const ExactPlan *prof = nullptr;   // the profile kernel follows (else NULL): the plan, the chunk's first trial
    uint64_t prof_first = 0;
};

struct Chunk {
    uint64_t k = 0;
    ChunkSlot *s = nullptr;
    uint64_t off = 0;                 // its first entry in the call's arrays
    fi_outcome *out_dev = nullptr;    // its part of the caller's device array (NULL: the outcomes stay in the slot)
    fi_outcome *host_out = nullptr;   // where the outcomes go on the host (NULL: nowhere)
    bool tick = false;                // its sites are mapped tick sites (run_pass)
    bool capture = false;             // a capture call's: its output goes to the slot's capture buffers
    Tally tally;
    fi_outcome *out() const { return out_dev ? out_dev : s->d_out.get(); }
    const uint8_t *disp() const { return tally.key == Tally::kTickSites ? s->d_tk_disp.get() : nullptr; }
};

// The device map's arguments: the packed table, the campaign's draw, the
// golden outcome.  in = uploaded explicit sites (NULL: sample from `first`).
static TickMapCtx tick_map_ctx(fi_engine *e, uint64_t first, const fi_tick_site *in) {
    TickMapCtx c{};
    c.done = e->gold.d_tk_done; c.rec = e->gold.d_tk_rec; c.n_att = e->gold.tk_done.size();
    c.golden_ninst = e->gold.info.ninst; c.golden_ticks = e->gold.t_stats.ticks;
    c.in = in;
    c.d = campaign_draw(e, first);
    c.gsub = e->gold.gsub; c.gexit = e->gold.info.exit_code; c.gdetail = e->gold.gdetail;
    c.literal = e->tick_contract == FI_TICK_CONTRACT_LITERAL ? 1u : 0u;
    return c;
}

// Where a run's sites come from: one kind and the payload that kind needs.
struct SiteSource {
    enum Kind {
        kSampled,        // trials first, first + 1, ... drawn on the device
        kGiven,          // sites: the caller's, a host array of n
        kMapped,         // sites: the host map's, made of tick sites (fi_run_tick_sites)
        kSampledTicks,   // tick sites drawn and mapped on the device, the mapper in the sampler's place
        kGivenTicks,     // ticks: the caller's tick sites, a host array of n, mapped on the device
        kExact,          // trials first, first + 1, ... of plan, enumerated on the device (fi_run_exact)
        kExactProfile,   // ... with the profile (fi_run_exact_profile)
        kExactTicks,     // ... of a tick campaign's plan and class records cls (fi_run_exact_ticks)
    };
    Kind kind;
    const fi_site *sites;
    const fi_tick_site *ticks;
    const ExactPlan *plan;
    const ExactTickClass *cls;

    static SiteSource sampled() { return {kSampled, nullptr, nullptr, nullptr, nullptr}; }
    static SiteSource given(const fi_site *sites) { return {kGiven, sites, nullptr, nullptr, nullptr}; }
    static SiteSource mapped(const fi_site *sites) { return {kMapped, sites, nullptr, nullptr, nullptr}; }
    static SiteSource sampled_ticks() { return {kSampledTicks, nullptr, nullptr, nullptr, nullptr}; }
    static SiteSource given_ticks(const fi_tick_site *ticks) { return {kGivenTicks, nullptr, ticks, nullptr, nullptr}; }
    static SiteSource exact(const ExactPlan *plan, bool profile) {
        return {profile ? kExactProfile : kExact, nullptr, nullptr, plan, nullptr};
    }
    static SiteSource exact_ticks(const ExactPlan *plan, const ExactTickClass *cls) {
        return {kExactTicks, nullptr, nullptr, plan, cls};
    }
    // its sites are mapped tick sites: this engine's clock is AtomicSimpleCPU's (run_pass)
    bool tick() const { return kind == kMapped || kind == kSampledTicks || kind == kGivenTicks || kind == kExactTicks; }
};

// The chunk's sites, keys and perm into its slot and the work buffers -- trial
// `first` on, or entries ch.off on of the source's array -- and how it is to be
// tallied into ch.tally.
static fi_status chunk_fill(fi_engine *e, const SiteSource &src, uint64_t first, Chunk &ch, hipStream_t st) {
    ChunkSlot &s = *ch.s;
    Work &w = e->w;
    ch.tick = src.tick();
    switch (src.kind) {
    case SiteSource::kSampled:
        HIPCHK(launch_sample(sample_ctx(e, first), ch.k, s.d_sites, w.d_keys, w.d_perm, st));
        break;
    case SiteSource::kGiven:
    case SiteSource::kMapped:
        HIPCHK(hipMemcpyAsync(s.d_sites, src.sites + ch.off, ch.k * sizeof(fi_site), hipMemcpyHostToDevice, st));
        HIPCHK(launch_keys(s.d_sites, ch.k, w.d_keys, w.d_perm, st));
        break;
    case SiteSource::kGivenTicks:
        HIPCHK(hipMemcpyAsync(s.d_tk_in, src.ticks + ch.off, ch.k * sizeof(fi_tick_site), hipMemcpyHostToDevice, st));
        [[fallthrough]];
    case SiteSource::kSampledTicks:   // tick sites: the mapper takes the sampler's place
        ch.tally.key = Tally::kTickSites;
        HIPCHK(launch_tick_map(tick_map_ctx(e, first, src.ticks ? s.d_tk_in.get() : nullptr), ch.k, s.d_sites, w.d_keys,
                               w.d_perm, s.d_tk_sites, s.d_tk_disp, s.d_tk_res, st));
        break;
    case SiteSource::kExactProfile:
        ch.tally.prof = src.plan; ch.tally.prof_first = first;
        [[fallthrough]];
    case SiteSource::kExact:
        ch.tally.weight = Tally::kW32;
        HIPCHK(launch_exact_sites(*src.plan, first, ch.k, e->gold.d_ex_classes, s.d_sites, w.d_keys, w.d_perm, s.d_weight, st));
        break;
    case SiteSource::kExactTicks:   // parked and fixed as mapped tick sites are
        ch.tally.key = Tally::kTickSites;
        ch.tally.weight = Tally::kW64;
        HIPCHK(launch_exact_tick_sites(*src.plan, tick_map_ctx(e, 0, nullptr), first, ch.k, src.cls, s.d_sites, w.d_keys,
                                       w.d_perm, s.d_tk_sites, s.d_tk_disp, s.d_tk_res, s.d_xt_weight, st));
        break;
    }
    return FI_OK;
}

static fi_status chunk_begin(fi_engine *e, const Chunk &ch, hipStream_t st) {
    const ChunkSlot &s = *ch.s;
    if (ch.capture) {   // every row = the golden stream (the prefix and golden-suffix rules)
        const Capture &x = e->w.cx;
        HIPCHK(launch_capture_init(s.cap.d_out, ch.k, x.stride, x.bytes, e->gold.d_gout, e->gold.gout.size(), st));
        HIPCHK(launch_capture_init(s.cap.d_err, ch.k, x.stride, x.bytes, e->gold.d_gerr, e->gold.gerr.size(), st));
    }
    fi_status st2 = run_pass(e, s.d_sites, ch.k, ch.out(), e->cfg.private_pages, st, ch.tick, ch.disp(),
                             ch.capture ? &s : nullptr);
    if (st2) return st2;
    if (!(e->cfg.flags & FI_CFG_NO_REDO)) {
        HIPCHK(hipMemsetAsync(s.redo_cnt, 0, 4, st));
        HIPCHK(launch_redo_collect(ch.out(), ch.k, s.redo_idx, s.redo_cnt, e->w.d_stats, st));
        HIPCHK(hipMemcpyAsync(s.h_redo_cnt, s.redo_cnt, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev_cnt, st));
    }
    return FI_OK;
}

static fi_status chunk_end(fi_engine *e, const Chunk &ch, fi_histogram *d_hist, hipStream_t st) {
    ChunkSlot &s = *ch.s;
    fi_outcome *out = ch.out();
    if (!(e->cfg.flags & FI_CFG_NO_REDO)) {
        HIPCHK(hipEventSynchronize(s.ev_cnt));   // (normally long done: a chunk later was enqueued first)
        const uint64_t nr = *s.h_redo_cnt;
        const uint32_t *idx = s.redo_idx;
        if (nr) {
            const uint64_t P = e->cfg.private_pages;
            const uint64_t pool = e->w.cap * P;   // page frames a pass has
            const uint64_t P2 = std::min<uint64_t>(pool, redo_pages(P));
            const uint64_t B = std::max<uint64_t>(1, pool / P2);
            for (uint64_t d = 0; d < nr; d += B) {
                const uint64_t b = std::min(B, nr - d);
                HIPCHK(launch_redo_gather(s.d_sites, idx + d, b, e->w.d_redo_sites, e->w.d_keys, e->w.d_perm, st));
                // (capture: the same deterministic run, only longer, into the trial's own row again)
                fi_status st2 = run_pass(e, e->w.d_redo_sites, b, e->w.d_redo_out, (uint32_t)P2, st, ch.tick, nullptr,
                                         ch.capture ? &s : nullptr, idx + d);
                if (st2) return st2;
                HIPCHK(launch_redo_scatter(idx + d, b, e->w.d_redo_out, out, st));
            }
        }
    }
    // (a redo trial is never a parked one: those end masked, not as resource escapes)
    if (ch.disp()) HIPCHK(launch_tick_fix(ch.disp(), s.d_tk_res, ch.k, out, st));
    const fi_site *key = ch.tally.key == Tally::kTickSites ? s.d_tk_sites : s.d_sites;
    switch (ch.tally.weight) {
    case Tally::kNone: HIPCHK(launch_hist(key, out, ch.k, d_hist, nullptr, st)); break;
    case Tally::kW32: HIPCHK(launch_exact_hist(key, out, s.d_weight.get(), ch.k, d_hist, st)); break;
    case Tally::kW64: HIPCHK(launch_exact_hist(key, out, s.d_xt_weight.get(), ch.k, d_hist, st)); break;
    }
    if (ch.tally.prof) {   // (an exact chunk: after its histogram)
        const ExProf &x = e->gold.xp;
        const ExactProfCtx c{x.d_reg_cons, x.d_inst_row, out, s.d_weight, x.d_bins, (uint32_t)x.rows.size(), e->prof_variant};
        HIPCHK(launch_exact_profile(*ch.tally.prof, c, ch.tally.prof_first, ch.k, st));
    }
    if (ch.host_out) {
        if (!s.h_stage) HIPCHK(s.h_stage.alloc(e->w.cap));
        HIPCHK(hipMemcpyAsync(s.h_stage, out, ch.k * sizeof(fi_outcome), hipMemcpyDeviceToHost, st));
        if (ch.capture) {   // zeros past each stream's end, then rows and lengths to their staging
            const Capture &x = e->w.cx;
            HIPCHK(launch_capture_finish(s.cap.d_out, ch.k, x.stride, x.bytes, s.cap.d_len, 0u, st));
            HIPCHK(hipMemcpyAsync(s.cap.h_out, s.cap.d_out, ch.k * x.stride, hipMemcpyDeviceToHost, st));
            if (x.err) {
                HIPCHK(launch_capture_finish(s.cap.d_err, ch.k, x.stride, x.bytes, s.cap.d_len, 1u, st));
                HIPCHK(hipMemcpyAsync(s.cap.h_err, s.cap.d_err, ch.k * x.stride, hipMemcpyDeviceToHost, st));
            }
            if (x.lens)
                HIPCHK(hipMemcpyAsync(s.cap.h_len, s.cap.d_len, ch.k * sizeof(fi_stream_len), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipEventRecord(s.ev_stage, st));
    }
    return FI_OK;
}

// A chunk's staged outcomes to the caller's array, once their copy has landed.
static fi_status chunk_deliver(fi_engine *e, Chunk &ch) {
    if (!ch.host_out || !ch.k) return FI_OK;
    const ChunkSlot &s = *ch.s;
    HIPCHK(hipEventSynchronize(s.ev_stage));
    memcpy(ch.host_out, s.h_stage, ch.k * sizeof(fi_outcome));
    if (ch.capture) {
        const Capture &x = e->w.cx;
        capture_rows(x.out + ch.off * x.bytes, s.cap.h_out, ch.k, x.bytes, x.stride);
        if (x.err) capture_rows(x.err + ch.off * x.bytes, s.cap.h_err, ch.k, x.bytes, x.stride);
        if (x.lens) memcpy(x.lens + ch.off, s.cap.h_len, ch.k * sizeof(fi_stream_len));
    }
    ch.k = 0;
    return FI_OK;
}

static void hist_add(fi_histogram *dst, const fi_histogram *src) {
    const uint64_t *s = (const uint64_t *)src;
    uint64_t *d = (uint64_t *)dst;
    for (size_t i = 0; i < sizeof(fi_histogram) / 8; i++) d[i] += s[i];
}

// Trials [first, first + n) or the given sites (src), in chunks of at most
// e->w.cap; outcomes to out_dev (device, n entries) or out_host (through the
// slots' device buffers), histogram added to d_hist.  The event pair
// ev0 / ev1 spans the whole call.
static fi_status run_chunks(fi_engine *e, uint64_t first, const SiteSource &src, uint64_t n, fi_outcome *out_dev,
                            fi_outcome *out_host, fi_histogram *d_hist, hipStream_t st) {
    HIPCHK(hipMemsetAsync(e->w.d_stats, 0, kNStats * sizeof(unsigned long long), st));
    HIPCHK(hipEventRecord(e->ev0, st));
    Chunk prev, staged[2];   // (staged: per slot, the chunk whose outcomes still sit in h_stage)
    bool have_prev = false;
    uint32_t i = 0;
    for (uint64_t done = 0; done < n; i++) {
        jit_install(e, st, false);   // the translated kernels, once their build has landed
        Chunk ch;
        ch.k = std::min<uint64_t>({n - done, e->w.cap, e->gold.jit ? kJitWindowChunk : e->w.cap});
        if (e->w.cx.bytes) { ch.k = std::min(ch.k, e->w.cx.rows); ch.capture = true; }
        ch.s = &e->w.slot[i & 1];
        ch.off = done;
        ch.out_dev = out_dev ? out_dev + done : nullptr;
        ch.host_out = out_host ? out_host + done : nullptr;
        fi_status s = chunk_fill(e, src, first + done, ch, st);
        if (!s) s = chunk_begin(e, ch, st);
        if (s) return s;
        if (have_prev) {
            Chunk &held = staged[prev.s - e->w.slot];
            if ((s = chunk_deliver(e, held))) return s;   // (two chunks ago: long landed)
            if ((s = chunk_end(e, prev, d_hist, st))) return s;
            held = prev;
        }
        prev = ch;
        have_prev = true;
        done += ch.k;
    }
    if (have_prev) {
        Chunk &held = staged[prev.s - e->w.slot];
        fi_status s = chunk_deliver(e, held);
        if (!s) s = chunk_end(e, prev, d_hist, st);
        if (s) return s;
        held = prev;
    }
    HIPCHK(hipEventRecord(e->ev1, st));
    HIPCHK(launch_hist_stats(e->w.d_stats, d_hist, st));
    for (auto &c : staged) {
        fi_status s = chunk_deliver(e, c);
        if (s) return s;
    }
    return FI_OK;
}

// The end of a blocking run on e->stream into e->w.d_hist: wait for it, its
// device time (ev0 .. ev1) to last_ms, its histogram added to hist.
static fi_status run_finish(fi_engine *e, fi_histogram *hist) {
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->last_ms = ms;
    if (hist) {
        fi_histogram h;
        HIPCHK(hipMemcpy(&h, e->w.d_hist, sizeof h, hipMemcpyDeviceToHost));
        hist_add(hist, &h);
    }
    return FI_OK;
}

// A blocking run on e->stream (the work buffers are there): e->w.d_hist from
// zero, what the caller enqueues ahead of the chunks (before, may be empty: the
// sites that need no trial, the profile bins' memset), the chunks, run_finish.
static fi_status run_blocking(fi_engine *e, uint64_t first, const SiteSource &src, uint64_t n, fi_outcome *out,
                              fi_histogram *hist, const std::function<fi_status()> &before = nullptr) {
    HIPCHK(hipMemsetAsync(e->w.d_hist, 0, sizeof(fi_histogram), e->stream));
    fi_status s = before ? before() : FI_OK;
    if (!s) s = run_chunks(e, first, src, n, nullptr, out, e->w.d_hist, e->stream);
    return s ? s : run_finish(e, hist);
}

static fi_status run_common(fi_engine *e, uint64_t first, const SiteSource &src, uint64_t n, fi_outcome *out,
                            fi_histogram *hist) {
    if (!e) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "golden run required");
    if (src.kind == SiteSource::kSampled && !e->structures) return fail(e, FI_E_STATE, "fi_set_campaign first");
    HIPCHK(hipSetDevice(e->dev));
    const fi_status s = ensure_work_for(e, n);
    return s ? s : run_blocking(e, first, src, n, out, hist);
}

fi_status fi_wait_translation(fi_engine *e, fi_golden_info *out) {
    if (!e) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "no golden run");
    HIPCHK(hipSetDevice(e->dev));
    jit_install(e, e->stream, true);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (out) *out = e->gold.info;
    return FI_OK;
}

fi_status fi_run_trials(fi_engine *e, uint64_t first, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    return run_common(e, first, SiteSource::sampled(), n, out, hist);
}

fi_status fi_run_sites(fi_engine *e, const fi_site *sites, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    if (!sites && n) return FI_E_ARG;
    // (no sites: an empty sampled run)
    return run_common(e, 0, sites ? SiteSource::given(sites) : SiteSource::sampled(), n, out, hist);
}

// ---- Exact campaigns (the classes and the trial ids: fi_exact.h)
fi_status fi_exact_classes(const uint32_t *off33, const uint32_t *ev, uint64_t ninst, uint32_t reg,
                           fi_exact_class *out, uint64_t cap, uint64_t *n, uint64_t *dead) {
    if (!off33 || (!ev && off33[32]) || reg < 1 || reg > 31 || ninst >= (1ULL << kExactInstBits)) return FI_E_ARG;
    std::vector<uint64_t> w(out ? (size_t)std::min<uint64_t>(cap, off33[reg + 1] - off33[reg]) : 0);
    uint64_t d = 0;
    const uint64_t cnt = exact_reg_classes(off33, ev, ninst, reg, w.data(), w.size(), &d);
    for (size_t i = 0; i < w.size() && i < cnt; i++) {
        out[i].inst = (uint32_t)exact_word_inst(w[i]);
        out[i].weight = exact_word_weight(w[i]);
    }
    if (n) *n = cnt;
    if (dead) *dead = d;
    return FI_OK;
}

// Every register's classes, once per golden run: packed, uploaded beside d_fw_ev.
static fi_status exact_build(fi_engine *e) {
    if (e->gold.ex_ok) return FI_OK;
    std::vector<uint64_t> words;
    for (uint32_t r = 1; r < 32; r++) {
        e->gold.ex_off[r] = (uint32_t)words.size();
        const uint64_t cnt = exact_reg_classes(e->gold.fw_off.data(), e->gold.fw_ev.data(), e->gold.info.ninst, r, nullptr, 0,
                                               &e->gold.ex_dead[r]);
        words.resize(words.size() + cnt);
        exact_reg_classes(e->gold.fw_off.data(), e->gold.fw_ev.data(), e->gold.info.ninst, r, words.data() + e->gold.ex_off[r], cnt,
                          nullptr);
    }
    e->gold.ex_off[0] = 0;
    e->gold.ex_off[32] = (uint32_t)words.size();
    DevBuf<uint64_t> d_classes;
    HIPCHK(d_classes.alloc(std::max<size_t>(words.size(), 1)));
    if (!words.empty()) HIPCHK(hipMemcpy(d_classes, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    e->gold.d_ex_classes = std::move(d_classes);
    e->gold.ex_ok = true;
    return FI_OK;
}

fi_status fi_exact_class_consumers(const uint32_t *trace, uint64_t n_trace, const uint32_t *off33, const uint32_t *ev,
                                   uint64_t ninst, uint32_t reg, uint32_t *out, uint64_t cap, uint64_t *n) {
    if ((!trace && n_trace) || !off33 || (!ev && off33[32]) || reg < 1 || reg > 31 || ninst >= (1ULL << kExactInstBits))
        return FI_E_ARG;
    std::vector<uint32_t> inst_val;
    std::vector<ExactEcall> ecall;
    if (!exact_consumer_tables(trace, n_trace, nullptr, ninst, inst_val, ecall)) return FI_E_ARG;
    const ExactConsumers c{inst_val.data(), ecall.data(), ninst, (uint32_t)ecall.size(), 0};
    const uint64_t cnt = exact_reg_consumers(off33, ev, ninst, reg, c, out, out ? cap : 0);
    if (n) *n = cnt;
    return FI_OK;
}

// The process-start text's instruction word at pc (len 2 or 4), 0 where the image has no such bytes
static uint32_t image_inst_word(const Image &img, uint64_t pc, uint32_t len) {
    uint32_t raw = 0;
    for (uint32_t i = 0; i < len; i++) {
        auto it = img.pages.find((pc + i) >> 12);
        if (it == img.pages.end()) return 0;
        raw |= (uint32_t)it->second[(pc + i) & 4095] << (8 * i);
    }
    return raw;
}

// The profile's rows and consumer tables (fi_exact.h "Profile"), once per golden run, after
// exact_build: rows and inst_row / the ecall list from the golden trace, a row per register class.
static fi_status profile_build(fi_engine *e) {
    Golden &g = e->gold;
    if (g.xp.ok) return FI_OK;
    ExProf x;
    std::vector<uint32_t> half, row_of, inst_row;
    std::vector<uint64_t> execs;
    std::vector<uint8_t> is_ecall;
    std::vector<ExactEcall> ecall;
    exact_profile_rows(g.g_trace.data(), g.g_trace.size(), half, execs, is_ecall, row_of);
    if (!exact_consumer_tables(g.g_trace.data(), g.g_trace.size(), row_of.data(), g.info.ninst, inst_row, ecall))
        return fail(e, FI_E_STATE, "exact profile: the golden trace does not hold the golden run's %llu instructions",
                    (unsigned long long)g.info.ninst);
    if ((uint64_t)half.size() * kProfBins >= kExactNoConsumer) return fail(e, FI_E_ARG, "exact profile: too many rows");
    x.rows.resize(half.size());
    for (size_t r = 0; r < half.size(); r++) {
        fi_profile_row &o = x.rows[r];
        o = fi_profile_row{};
        o.pc = e->img.text_lo + 2ULL * half[r];
        o.execs = execs[r];
        o.len = half[r] < g.g_pre.size() ? g.g_pre[half[r]].len : 0;
        o.raw = image_inst_word(e->img, o.pc, o.len);
        o.ecall = is_ecall[r];
    }
    std::vector<uint32_t> cons(g.ex_off[32]);
    const ExactConsumers c{inst_row.data(), ecall.data(), g.info.ninst, (uint32_t)ecall.size(), 0};
    for (uint32_t r = 1; r < 32; r++)
        exact_reg_consumers(g.fw_off.data(), g.fw_ev.data(), g.info.ninst, r, c, cons.data() + g.ex_off[r],
                            g.ex_off[r + 1] - g.ex_off[r]);
    x.n_ecall = (uint32_t)ecall.size();
    HIPCHK(x.d_inst_row.alloc(std::max<size_t>(inst_row.size(), 1)));
    HIPCHK(x.d_ecall.alloc(std::max<size_t>(ecall.size(), 1)));
    HIPCHK(x.d_reg_cons.alloc(std::max<size_t>(cons.size(), 1)));
    HIPCHK(x.d_bins.alloc(std::max<size_t>(x.rows.size(), 1) * kProfBins));
    if (!inst_row.empty()) HIPCHK(hipMemcpy(x.d_inst_row, inst_row.data(), inst_row.size() * 4, hipMemcpyHostToDevice));
    if (!ecall.empty()) HIPCHK(hipMemcpy(x.d_ecall, ecall.data(), ecall.size() * sizeof(ExactEcall), hipMemcpyHostToDevice));
    if (!cons.empty()) HIPCHK(hipMemcpy(x.d_reg_cons, cons.data(), cons.size() * 4, hipMemcpyHostToDevice));
    if (g.mem_live) {
        HIPCHK(x.d_mw_proxy.alloc(g.mw_proxy.size()));
        HIPCHK(hipMemcpy(x.d_mw_proxy, g.mw_proxy.data(), g.mw_proxy.size() * 4, hipMemcpyHostToDevice));
    }
    x.ok = true;
    g.xp = std::move(x);
    return FI_OK;
}

// Why exact campaigns cannot cover memory words here, or NULL.  The classes
// rest on what forwarding a memory site rests on (run_pass): a complete access
// index and a word that stays mapped from the site's t to its next access.  The
// candidate pages are mapped at process start and leave only through
// vm_unmap, so "the golden run unmapped nothing" stands for the second --
// golden_fp, which run_pass uses, would also refuse every golden run that
// merely writes FP or LR/SC state, which changes nothing about its memory.
static const char *exact_mem_refusal(const fi_engine *e) {
    if (e->cpu_model != FI_CPU_ATOMIC) return "the CPU model is TimingSimpleCPU (exact campaigns enumerate numInst sites)";
    if (!e->gold.mem_live) return "the golden run's memory index is incomplete (the access trace overflowed, or an "
                             "instruction came from outside the pre-decoded text)";
    if (e->gold.golden_unmapped) return "the golden run unmapped memory (munmap, a shrinking brk): a word need not stay "
                                   "mapped up to its next access";
    return nullptr;
}

// The memory classes under the campaign's (bits, burst), once per golden run
// and pair: liveness, count, scan, emit (fi_kernels.hip), then the rows.
// profiled (after profile_build): the emit pass also writes each class's
// consumer row; classes built without them are built again, id for id.
static fi_status exact_mem_build(fi_engine *e, bool profiled = false) {
#define XMCHK(call) HIPCHK_AS("exact memory classes", call)
    ExMem &m = e->gold.xm;
    const uint64_t bits = e->bits & burst_positions(e->burst);
    if (m.ok && m.bits == bits && m.burst == e->burst && (m.cons || !profiled)) return FI_OK;
    profiled = profiled || (m.ok && m.cons);
    m = ExMem{};   // (not ok until the end)
    m.n_rows = exact_mem_sets(bits, e->burst, m.rows);
    m.text_words = exact_mem_text_words(e->img.mem_pages.data(), e->img.mem_pages.size(), e->img.text_lo, e->img.text_hi);
    m.words = e->img.mem_pages.size() * 512 - m.text_words;
    const uint64_t ninst = e->gold.info.ninst, pairs = m.words * ninst;
    if (m.words && pairs / m.words != ninst) return fail(e, FI_E_ARG, "exact memory: words x ninst overflows");
    std::vector<uint64_t> offs(m.n_rows + 1, 0), wsum(kExactMaxMemRows, 0);
    const uint64_t n_cnt = (uint64_t)m.n_rows * e->gold.mw_n + 1;
    auto t0 = std::chrono::steady_clock::now();
    if (e->gold.mw_n && m.n_rows) {
        if (n_cnt >= (1ULL << 31)) return fail(e, FI_E_ARG, "exact memory: 2^31 (byte set, word) pairs or more");
        ExactMemCtx c{};
        c.mw_addr = e->gold.d_mw_addr; c.mw_ev = e->gold.d_mw_ev; c.mw_off = e->gold.d_mw_off; c.mw_n = e->gold.mw_n;
        c.pages = e->img.d_mem_pages; c.n_pages = e->img.mem_pages.size();
        c.text_lo = e->img.text_lo; c.text_hi = e->img.text_hi; c.ninst = ninst;
        if (profiled) {
            const ExProf &x = e->gold.xp;
            c.cons = ExactConsumers{x.d_inst_row, x.d_ecall, ninst, x.n_ecall, 0};
            c.proxy = x.d_mw_proxy;
        }
        DevBuf<uint8_t> d_live, d_tmp;
        DevBuf<uint64_t> d_cnt, d_offs;
        DevBuf<unsigned long long> d_wsum;
        size_t tmp_bytes = 0;
        XMCHK(scan_u64_bytes(n_cnt, tmp_bytes));
        XMCHK(d_live.alloc(std::max<uint64_t>(e->gold.mw_nev, 1)));
        XMCHK(d_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
        XMCHK(d_cnt.alloc(n_cnt));
        XMCHK(d_offs.alloc(n_cnt));
        XMCHK(d_wsum.alloc(kExactMaxMemRows));
        XMCHK(m.d_rows.alloc(kExactMaxMemRows));
        hipStream_t st = e->stream;
        XMCHK(hipMemsetAsync(d_cnt + (n_cnt - 1), 0, 8, st));
        XMCHK(hipMemsetAsync(d_wsum, 0, kExactMaxMemRows * 8, st));
        XMCHK(hipMemcpyAsync(m.d_rows, m.rows, m.n_rows * sizeof(ExactMemRow), hipMemcpyHostToDevice, st));
        XMCHK(launch_exact_mem_live(c, d_live, st));
        XMCHK(launch_exact_mem_walk(c, m.d_rows, m.n_rows, d_live, d_cnt, d_wsum, nullptr, 0, st));
        XMCHK(scan_u64(d_tmp, tmp_bytes, d_cnt, d_offs, n_cnt, st));
        // the offsets at the rows' starts and the total: every mw_n-th entry
        XMCHK(hipStreamSynchronize(st));
        XMCHK(hipMemcpy2D(offs.data(), 8, d_offs, (size_t)e->gold.mw_n * 8, 8, m.n_rows + 1, hipMemcpyDeviceToHost));
        XMCHK(hipMemcpy(wsum.data(), d_wsum, kExactMaxMemRows * 8, hipMemcpyDeviceToHost));
        const uint64_t total = offs[m.n_rows];
        if (total >= (1ULL << 32)) return fail(e, FI_E_ARG, "exact memory: 2^32 classes or more");
        XMCHK(m.d_cls.alloc(std::max<uint64_t>(total, 1)));
        if (total) XMCHK(launch_exact_mem_walk(c, m.d_rows, m.n_rows, d_live, d_offs, nullptr, m.d_cls, 1, st));
        XMCHK(hipStreamSynchronize(st));
    } else {
        HIPCHK(m.d_rows.alloc(kExactMaxMemRows));
        HIPCHK(m.d_cls.alloc(1));
    }
#undef XMCHK
    for (uint32_t g = 0; g < m.n_rows; g++) {
        m.classes[g] = offs[g + 1] - offs[g];
        m.dead[g] = pairs - wsum[g];
        m.n_classes += m.classes[g];
    }
    // the rows' first trials and class offsets, as every plan will have them
    ExactPlan scratch{};
    exact_plan_mem(scratch, m.rows, m.n_rows, m.classes, nullptr, nullptr, nullptr);
    HIPCHK(hipMemcpy(m.d_rows, m.rows, sizeof m.rows, hipMemcpyHostToDevice));
    m.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    m.bits = bits; m.burst = e->burst;
    m.cons = profiled;
    m.ok = true;
    return FI_OK;
}

// "who: trials [first, first + n) outside the campaign's ..." unless the range lies within `trials`
static fi_status trial_range_check(fi_engine *e, const char *who, uint64_t first, uint64_t n, uint64_t trials) {
    if (first > trials || n > trials - first)
        return fail(e, FI_E_ARG, "%s: trials [%llu, %llu) outside the campaign's %llu", who, (unsigned long long)first,
                    (unsigned long long)(first + n), (unsigned long long)trials);
    return FI_OK;
}

// The checks every exact entry point shares, then the campaign's plan, its
// dead sites and (info, may be NULL) its sizes.  profiled: the profile's tables too.
static fi_status exact_prepare(fi_engine *e, const char *who, ExactPlan &p, ExactUntried &dd, fi_exact_info *info,
                               bool profiled = false) {
    if (!e) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "%s: golden run required", who);
    if (!e->structures) return fail(e, FI_E_STATE, "%s: fi_set_campaign first", who);
    const bool mem = (e->structures >> FI_T_MEM) & 1;
    if (mem && !e->exact_mem)
        return fail(e, FI_E_ARG, "%s: memory words (structure %d) have no exact classes unless fi_set_exact_memory "
                    "is on; select registers, the pc and instruction results", who, FI_T_MEM);
    if (mem) {
        const char *why = exact_mem_refusal(e);
        if (why) return fail(e, FI_E_STATE, "%s: exact memory: %s", who, why);
    }
    if (e->cpu_model != FI_CPU_ATOMIC)
        return fail(e, FI_E_STATE, "%s: exact campaigns enumerate numInst sites (the CPU model is TimingSimpleCPU)", who);
    if (!e->gold.fw_ok)
        return fail(e, FI_E_STATE, "%s: the golden run has no first-access index (a golden trace that is incomplete "
                    "or 2^29 instructions or more)", who);
    HIPCHK(hipSetDevice(e->dev));
    fi_status s = exact_build(e);
    if (!s && profiled) s = profile_build(e);
    if (!s && mem) s = exact_mem_build(e, profiled);
    if (s) return s;
    dd = ExactUntried{};
    fi_exact_info x{};
    const uint64_t ninst = e->gold.info.ninst;
    p = exact_plan(e->structures, e->gold.ex_off, ninst, e->bits, e->burst, x.classes);
    for (uint32_t t = 1; t < FI_N_STRUCT; t++) {
        if (!((e->structures >> t) & 1)) continue;
        if (t == FI_T_MEM) continue;
        x.space += ninst * p.nbits;
        if (t < 32) {
            dd.masked[t] = e->gold.ex_dead[t];
            x.dead_sites += e->gold.ex_dead[t] * p.nbits;
        }
    }
    if (mem) {
        ExMem &m = e->gold.xm;
        exact_plan_mem(p, m.rows, m.n_rows, m.classes, m.d_rows, m.d_cls, e->gold.d_mw_addr);
        x.classes[FI_T_MEM] = m.n_classes;
        x.space += m.words * ninst * p.nbits;
        for (uint32_t g = 0; g < m.n_rows; g++) {
            x.dead_sites += m.dead[g] * m.rows[g].npos;
            for (uint64_t b = m.rows[g].pos; b; b &= b - 1) dd.mem_masked[__builtin_ctzll(b)] = m.dead[g];
        }
        uint64_t nc = m.n_classes;
        for (uint32_t t = 1; t < FI_N_STRUCT; t++) nc += t == FI_T_MEM ? 0 : x.classes[t];
        if (nc >= (1ULL << 32)) return fail(e, FI_E_ARG, "%s: 2^32 exact classes or more", who);
    }
    x.trials = p.trials;
    x.nbits = p.nbits;
    dd.bits = p.bits; dd.total = x.dead_sites; dd.insts = x.dead_sites * ninst;
    if (p.trials >= kExactMaxTrials) return fail(e, FI_E_ARG, "%s: 2^40 exact trials or more", who);
    if (info) *info = x;
    return FI_OK;
}

fi_status fi_exact_get_info(fi_engine *e, fi_exact_info *out) {
    if (!e || !out) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    return exact_prepare(e, "fi_exact_get_info", p, dd, out);
}

fi_status fi_set_exact_memory(fi_engine *e, int on) {
    if (!e) return FI_E_ARG;
    if (on) {
        if (!e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_exact_memory: golden run required");
        const char *why = exact_mem_refusal(e);
        if (why) return fail(e, FI_E_STATE, "fi_set_exact_memory: %s", why);
    }
    e->exact_mem = on != 0;
    return FI_OK;
}

fi_status fi_exact_mem_get_info(fi_engine *e, fi_exact_mem_info *out) {
    if (!e || !out) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "fi_exact_mem_get_info: golden run required");
    if (!e->structures) return fail(e, FI_E_STATE, "fi_exact_mem_get_info: fi_set_campaign first");
    if (!e->exact_mem) return fail(e, FI_E_STATE, "fi_exact_mem_get_info: fi_set_exact_memory is off");
    const char *why = exact_mem_refusal(e);
    if (why) return fail(e, FI_E_STATE, "fi_exact_mem_get_info: %s", why);
    HIPCHK(hipSetDevice(e->dev));
    fi_status s = exact_mem_build(e);
    if (s) return s;
    const ExMem &m = e->gold.xm;
    *out = fi_exact_mem_info{};
    out->words = m.words; out->text_words = m.text_words; out->index_words = e->gold.mw_n;
    out->byte_sets = m.n_rows;
    out->build_ms = m.build_ms;
    for (uint32_t g = 0; g < m.n_rows; g++) {
        out->set[g].bytes = m.rows[g].fmask;
        out->set[g].positions = m.rows[g].pos;
        out->set[g].classes = m.classes[g];
        out->set[g].dead_sites = m.dead[g] * m.rows[g].npos;
    }
    return FI_OK;
}

fi_status fi_exact_mem_classes(const uint64_t *ev, uint64_t n_ev, uint64_t ninst, uint32_t byte_mask,
                               fi_exact_class *out, uint64_t cap, uint64_t *n, uint64_t *dead) {
    if ((!ev && n_ev) || n_ev >= (1ULL << 32) || ninst >= (1ULL << kExactInstBits) || !byte_mask || byte_mask > 0xFF)
        return FI_E_ARG;
    std::vector<uint8_t> live(n_ev);
    exact_mem_liveness(ev, (uint32_t)n_ev, live.data());
    uint64_t sum = 0;
    const uint64_t cnt = exact_mem_walk(ev, live.data(), (uint32_t)n_ev, ninst, byte_mask, 0, nullptr, 0, &sum);
    std::vector<ExactMemClass> c(out ? (size_t)std::min(cap, cnt) : 0);
    exact_mem_walk(ev, live.data(), (uint32_t)n_ev, ninst, byte_mask, 0, c.data(), c.size(), nullptr);
    for (size_t i = 0; i < c.size(); i++) {
        out[i].inst = c[i].inst;
        out[i].weight = c[i].weight;
    }
    if (n) *n = cnt;
    if (dead) *dead = ninst - sum;
    return FI_OK;
}

fi_status fi_golden_mem_index(fi_engine *e, uint64_t *addr, uint64_t addr_cap, uint32_t *off, uint64_t off_cap,
                              uint64_t *ev, uint64_t ev_cap, uint64_t counts[2]) {
    if (!e) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "fi_golden_mem_index: golden run required");
    if (!e->gold.mem_live) return fail(e, FI_E_STATE, "fi_golden_mem_index: the golden run's memory index is incomplete");
    HIPCHK(hipSetDevice(e->dev));
    if (counts) { counts[0] = e->gold.mw_n; counts[1] = e->gold.mw_nev; }
    if (addr) HIPCHK(hipMemcpy(addr, e->gold.d_mw_addr, std::min<uint64_t>(addr_cap, e->gold.mw_n) * 8, hipMemcpyDeviceToHost));
    if (off) HIPCHK(hipMemcpy(off, e->gold.d_mw_off, std::min<uint64_t>(off_cap, (uint64_t)e->gold.mw_n + 1) * 4, hipMemcpyDeviceToHost));
    if (ev) HIPCHK(hipMemcpy(ev, e->gold.d_mw_ev, std::min<uint64_t>(ev_cap, e->gold.mw_nev) * 8, hipMemcpyDeviceToHost));
    return FI_OK;
}

fi_status fi_exact_sites(fi_engine *e, uint64_t first, uint64_t n, fi_site *sites, uint32_t *weights) {
    if (!e || (n && !sites)) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_prepare(e, "fi_exact_sites", p, dd, nullptr);
    if (!s) s = trial_range_check(e, "fi_exact_sites", first, n, p.trials);
    if (!s) s = ensure_work_for(e, n);
    if (s) return s;
    return for_chunks(e, n, [&](uint64_t done, uint64_t k) -> fi_status {
        const ChunkSlot &s0 = e->w.slot[0];
        HIPCHK(launch_exact_sites(p, first + done, k, e->gold.d_ex_classes, s0.d_sites, e->w.d_keys, e->w.d_perm, s0.d_weight,
                                  e->stream));
        HIPCHK(hipMemcpyAsync(sites + done, s0.d_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        if (weights) HIPCHK(hipMemcpyAsync(weights + done, s0.d_weight, k * 4, hipMemcpyDeviceToHost, e->stream));
        return FI_OK;
    });
}

// fi_run_exact (prof == NULL: nothing of the profile is built, launched or copied) and
// fi_run_exact_profile
static fi_status run_exact(fi_engine *e, const char *who, uint64_t first, uint64_t n, fi_outcome *out,
                           fi_histogram *hist, fi_profile_bins *prof, uint64_t prof_rows) {
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_prepare(e, who, p, dd, nullptr, prof != nullptr);
    if (!s) s = trial_range_check(e, who, first, n, p.trials);
    if (s) return s;
    if (prof && prof_rows != e->gold.xp.rows.size())
        return fail(e, FI_E_ARG, "%s: prof_rows %llu, the profile has %llu rows (fi_profile_rows)", who,
                    (unsigned long long)prof_rows, (unsigned long long)e->gold.xp.rows.size());
    if ((s = ensure_work_for(e, n))) return s;
    const size_t prof_bytes = prof ? prof_rows * sizeof(fi_profile_bins) : 0;
    s = run_blocking(e, first, SiteSource::exact(&p, prof != nullptr), n, out, hist, [&]() -> fi_status {
        if (first == 0) HIPCHK(launch_exact_untried(dd, e->w.d_hist, e->stream));   // the sites that need no trial
        if (prof_bytes) HIPCHK(hipMemsetAsync(e->gold.xp.d_bins, 0, prof_bytes, e->stream));
        return FI_OK;
    });
    if (s || !prof_bytes) return s;
    std::vector<fi_profile_bins> got(prof_rows);
    HIPCHK(hipMemcpy(got.data(), e->gold.xp.d_bins, prof_bytes, hipMemcpyDeviceToHost));
    const uint64_t *src64 = (const uint64_t *)got.data();
    uint64_t *dst64 = (uint64_t *)prof;
    for (size_t i = 0; i < prof_bytes / 8; i++) dst64[i] += src64[i];
    return FI_OK;
}

fi_status fi_run_exact(fi_engine *e, uint64_t first, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    return run_exact(e, "fi_run_exact", first, n, out, hist, nullptr, 0);
}

fi_status fi_run_exact_profile(fi_engine *e, uint64_t first, uint64_t n, fi_outcome *out, fi_histogram *hist,
                               fi_profile_bins *prof, uint64_t prof_rows) {
    if (!prof) return e ? fail(e, FI_E_ARG, "fi_run_exact_profile: prof is NULL") : FI_E_ARG;
    return run_exact(e, "fi_run_exact_profile", first, n, out, hist, prof, prof_rows);
}

fi_status fi_profile_rows(fi_engine *e, fi_profile_row *rows, uint64_t cap, uint64_t *n) {
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_prepare(e, "fi_profile_rows", p, dd, nullptr, true);
    if (s) return s;
    const std::vector<fi_profile_row> &r = e->gold.xp.rows;
    if (rows) memcpy(rows, r.data(), std::min<uint64_t>(cap, r.size()) * sizeof(fi_profile_row));
    if (n) *n = r.size();
    return FI_OK;
}

fi_status fi_exact_consumers(fi_engine *e, uint64_t first, uint64_t n, uint32_t *row) {
    if (!e || (n && !row)) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_prepare(e, "fi_exact_consumers", p, dd, nullptr, true);
    if (!s) s = trial_range_check(e, "fi_exact_consumers", first, n, p.trials);
    if (!s) s = ensure_work_for(e, n);
    if (s) return s;
    return for_chunks(e, n, [&](uint64_t done, uint64_t k) -> fi_status {   // (d_perm: a uint32 per trial, free between runs)
        HIPCHK(launch_exact_consumers(p, e->gold.xp.d_reg_cons, e->gold.xp.d_inst_row, first + done, k, e->w.d_perm, e->stream));
        HIPCHK(hipMemcpyAsync(row + done, e->w.d_perm, k * 4, hipMemcpyDeviceToHost, e->stream));
        return FI_OK;
    });
}

uint32_t fi_debug_profile_slots(void) { return kProfSlots; }

fi_status fi_debug_set_profile_variant(fi_engine *e, uint32_t variant) {
    if (!e || variant > 2) return FI_E_ARG;
    e->prof_variant = variant;
    return FI_OK;
}

// Output capture (the sizing and the staging copy: fi_capture.h).
// The rows and their pinned mirror are grown on demand like the other work
// buffers and replaced with them.
static fi_status ensure_capture(fi_engine *e, uint64_t rows, uint32_t stride) {
    Capture &x = e->w.cx;
    if (rows * stride <= x.held_b && rows <= x.held_rows) return FI_OK;
    const uint64_t b = std::max(x.held_b, rows * stride), r = std::max(x.held_rows, rows);
    x = Capture{};   // (holds nothing until every buffer is made)
    for (ChunkSlot &s : e->w.slot) s.cap = CaptureRows{};
    for (ChunkSlot &s : e->w.slot) {
        HIPCHK(s.cap.d_out.alloc(b));
        HIPCHK(s.cap.d_err.alloc(b));
        HIPCHK(s.cap.d_len.alloc(r));
        HIPCHK(s.cap.h_out.alloc(b));
        HIPCHK(s.cap.h_err.alloc(b));
        HIPCHK(s.cap.h_len.alloc(r));
    }
    x.held_b = b; x.held_rows = r;
    return FI_OK;
}

fi_status fi_run_sites_capture(fi_engine *e, const fi_site *sites, uint64_t n, uint32_t cap_bytes, fi_outcome *out,
                               fi_histogram *hist, uint8_t *out_buf, uint8_t *err_buf, fi_stream_len *lens) {
    if (!e) return FI_E_ARG;
    if (const char *why = capture_args_error(sites, n, cap_bytes, out_buf))
        return fail(e, FI_E_ARG, "fi_run_sites_capture: %s", why);
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "golden run required");
    if (n == 0) return FI_OK;
    HIPCHK(hipSetDevice(e->dev));
    const uint32_t stride = capture_stride(cap_bytes);
    // the work buffers first, at run_common's own size (growing them frees and reallocates everything, so
    // not once the rows exist), then the rows within a quarter of what is free
    const uint64_t want = std::min<uint64_t>(n, e->cfg.max_trials_per_launch);
    fi_status s = ensure_work(e, want);
    if (s) return s;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // (what an earlier call left is counted as free: it is reused or replaced)
    const uint64_t held = 4 * e->w.cx.held_b + 2 * e->w.cx.held_rows * sizeof(fi_stream_len);
    const uint64_t rows = capture_rows_for(want, ((uint64_t)free_b + held) / 4, stride);
    std::vector<fi_outcome> own;   // the rows travel with the outcomes' staging: the run has a host array
    if (!out) { own.resize(n); out = own.data(); }
    s = ensure_capture(e, rows, stride);
    if (!s) {
        Capture &x = e->w.cx;
        x.rows = rows; x.stride = stride;
        x.out = out_buf; x.err = err_buf; x.lens = lens;
        x.bytes = cap_bytes;   // capture is on
        s = run_common(e, 0, SiteSource::given(sites), n, out, hist);
        if (s) (void)hipStreamSynchronize(e->stream);   // nothing in flight still writes the caller's arrays
        x.bytes = 0;           // ... and off again for every other entry point
        x.out = x.err = nullptr; x.lens = nullptr;
    }
    return s;
}

// ---------------------------------------------------- tick-domain injection
fi_status fi_set_cpu_model(fi_engine *e, int model, const fi_timing_params *p) {
    if (!e) return FI_E_ARG;
    if (model != FI_CPU_ATOMIC && model != FI_CPU_TIMING) return fail(e, FI_E_ARG, "unknown CPU model %d", model);
    if (e->gold.have_golden) return fail(e, FI_E_STATE, "fi_set_cpu_model: set before fi_golden_run");
    e->cpu_model = model;
    if (p) e->tparams = *p; else fi_timing_default_params(&e->tparams);
    return FI_OK;
}

fi_status fi_tick_golden(fi_engine *e, fi_tick_info *out) {
    if (!e || !out) return FI_E_ARG;
    *out = fi_tick_info{};
    snprintf(out->status, sizeof out->status, "%s", e->gold.t_status.c_str());
    out->attempts = e->gold.t_ops.size();
    out->golden_ticks = e->gold.t_stats.ticks;
    out->stats = e->gold.t_stats;
    return FI_OK;
}

fi_status fi_tick_trace(fi_engine *e, fi_timing_op *ops, fi_timing_ticks *ticks, uint64_t cap, uint64_t *n) {
    if (!e) return FI_E_ARG;
    if (!e->gold.t_status.empty()) return fail(e, FI_E_STATE, "tick model: %s", e->gold.t_status.c_str());
    const uint64_t k = std::min<uint64_t>(cap, e->gold.t_ops.size());
    if (ops && k) memcpy(ops, e->gold.t_ops.data(), k * sizeof *ops);
    if (ticks && k) memcpy(ticks, e->gold.t_ticks.data(), k * sizeof *ticks);
    if (n) *n = e->gold.t_ops.size();
    return FI_OK;
}

static fi_status tick_ready(fi_engine *e) {
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "golden run required");
    if (!e->gold.t_status.empty()) return fail(e, FI_E_STATE, "tick model: %s", e->gold.t_status.c_str());
    return FI_OK;
}

// What every tick entry point refuses, host map or device map, in one order
// and one wording: the campaign's draw (sampled), a run's restrictions (run),
// then each explicit site (ts; NULL: none).
static fi_status tick_check(fi_engine *e, const fi_tick_site *ts, uint64_t n, bool sampled, bool run) {
    fi_status st = tick_ready(e);
    if (st) return st;
    if (sampled) {
        if (!e->structures) return fail(e, FI_E_STATE, "fi_set_campaign first");
        if (e->structures & (1ULL << FI_T_MEM)) return fail(e, FI_E_ARG, "tick sites: memory words are not supported");
    }
    if (run && (e->protect || e->protect_opc))
        return fail(e, FI_E_ARG, "tick sites: selective replication (fi_set_protect*) is not supported");
    for (uint64_t i = 0; ts && i < n; i++) {
        const fi_tick_site &t = ts[i];
        const bool target_ok = (t.target >= 1 && t.target <= FI_T_PC) || t.target == FI_T_RESULT;
        if (!t.mask || !target_ok || t.tick >= e->gold.t_stats.ticks)
            return fail(e, FI_E_ARG, "tick site %llu: target %u, tick %llu (golden run %llu ticks)",
                        (unsigned long long)i, t.target, (unsigned long long)t.tick,
                        (unsigned long long)e->gold.t_stats.ticks);
    }
    return FI_OK;
}

fi_status fi_sample_tick_sites(fi_engine *e, uint64_t first, uint64_t n, fi_tick_site *out) {
    if (!e || (!out && n)) return FI_E_ARG;
    fi_status st = tick_check(e, nullptr, n, true, false);
    if (st) return st;
    const DrawCtx d = campaign_draw(e, first);   // the sampler's draw with the golden run's ticks for numInst
    for (uint64_t i = 0; i < n; i++) {
        const SiteDraw s = draw_site(d, i, e->gold.t_stats.ticks);
        out[i] = fi_tick_site{s.when, s.mask, s.target, s.trial};
    }
    return FI_OK;
}

// The host map over checked sites (tick_check)
static void map_tick_sites(fi_engine *e, const fi_tick_site *ts, uint64_t n, fi_site *sites, uint8_t *disp,
                           fi_outcome *host_out) {
    const uint32_t literal = e->tick_contract == FI_TICK_CONTRACT_LITERAL ? 1u : 0u;
    for (uint64_t i = 0; i < n; i++) {
        const fi_tick_site &t = ts[i];
        const TickMap m = tick_map_site(e->gold.tk_done.data(), e->gold.tk_rec.data(), e->gold.tk_done.size(), e->gold.info.ninst,
                                        t.tick, t.target, t.mask, t.trial, literal);
        disp[i] = (uint8_t)m.disp;
        sites[i] = m.site;
        if (host_out)
            host_out[i] = tick_map_outcome(m, e->gold.tk_rec[m.attempt], e->gold.gsub, e->gold.info.exit_code, e->gold.gdetail,
                                           e->gold.info.ninst);
    }
}

fi_status fi_map_tick_sites(fi_engine *e, const fi_tick_site *ts, uint64_t n, fi_site *sites, uint8_t *disp,
                            fi_outcome *host_out) {
    if (!e || (n && (!ts || !sites || !disp))) return FI_E_ARG;
    fi_status st = tick_check(e, ts, n, false, false);
    if (st) return st;
    map_tick_sites(e, ts, n, sites, disp, host_out);
    return FI_OK;
}

// ---- the device map (fi_set_tick_map FI_TICK_MAP_DEVICE)
// A tick site as the device keeps it -- fi_site layout, inst = the tick -- back as a fi_tick_site
static fi_tick_site tick_site_of(const fi_site &t) { return fi_tick_site{t.inst, t.mask, t.target, t.trial}; }

fi_status fi_set_tick_map(fi_engine *e, int where) {
    if (!e) return FI_E_ARG;
    if (where != FI_TICK_MAP_HOST && where != FI_TICK_MAP_DEVICE) return fail(e, FI_E_ARG, "unknown tick map %d", where);
    e->tick_map = where;
    return FI_OK;
}

fi_status fi_set_tick_contract(fi_engine *e, int contract) {
    if (!e) return FI_E_ARG;
    if (contract != FI_TICK_CONTRACT_NUMINST && contract != FI_TICK_CONTRACT_LITERAL)
        return fail(e, FI_E_ARG, "unknown tick contract %d", contract);
    e->tick_contract = contract;
    return FI_OK;
}

// The packed attempt table on the device: the host map's own, uploaded at the
// first device map after a golden run (fi_golden_run drops the copy).
static fi_status ensure_tick_table(fi_engine *e) {
    Golden &g = e->gold;
    if (g.d_tk_done) return FI_OK;
    if (g.tk_done.empty()) return fail(e, FI_E_STATE, "tick model: no attempts");
    DevBuf<uint64_t> d_done;
    DevBuf<TickRec> d_rec;
    HIPCHK(d_done.alloc(g.tk_done.size()));
    HIPCHK(d_rec.alloc(g.tk_rec.size()));
    HIPCHK(hipMemcpy(d_done, g.tk_done.data(), g.tk_done.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_rec, g.tk_rec.data(), g.tk_rec.size() * sizeof(TickRec), hipMemcpyHostToDevice));
    g.d_tk_rec = std::move(d_rec);
    g.d_tk_done = std::move(d_done);
    return FI_OK;
}

// The device map's work buffers in both chunk slots (growth of the work
// buffers drops them with the slots): made once a device tick run or map is
// first asked for; tk_ok once all are.
static fi_status ensure_tick_work(fi_engine *e) {
    Work &w = e->w;
    if (w.tk_ok) return FI_OK;
    for (ChunkSlot &s : w.slot) {
        HIPCHK(s.d_tk_sites.alloc(w.cap));
        HIPCHK(s.d_tk_disp.alloc(w.cap));
        HIPCHK(s.d_tk_res.alloc(w.cap));
        HIPCHK(s.d_tk_in.alloc(w.cap));
    }
    w.tk_ok = true;
    return FI_OK;
}

static fi_status tick_device_prepare(fi_engine *e, uint64_t n) {
    HIPCHK(hipSetDevice(e->dev));
    fi_status s = ensure_work_for(e, n);
    if (!s) s = ensure_tick_work(e);
    if (!s) s = ensure_tick_table(e);
    return s;
}

// fi_run_tick_sites / fi_run_tick_trials with the device map (ts NULL:
// sampled): run_chunks with the mapper in the sampler's place; only outcomes
// and the histogram come back.
static fi_status tick_run_device(fi_engine *e, uint64_t first, const fi_tick_site *ts, uint64_t n, fi_outcome *out,
                                 fi_histogram *hist) {
    fi_status s = tick_check(e, ts, n, !ts, true);
    if (s || !n) return s;
    if ((s = tick_device_prepare(e, n))) return s;
    return run_blocking(e, first, ts ? SiteSource::given_ticks(ts) : SiteSource::sampled_ticks(), n, out, hist);
}

fi_status fi_run_tick_trials_device(fi_engine *e, uint64_t first, uint64_t n, void *d_out, void *d_hist, void *stream) {
    if (!e || !d_out || !d_hist) return FI_E_ARG;
    fi_status s = tick_check(e, nullptr, n, true, true);
    if (s || !n) return s;
    if ((s = tick_device_prepare(e, n))) return s;
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    return run_chunks(e, first, SiteSource::sampled_ticks(), n, (fi_outcome *)d_out, nullptr, (fi_histogram *)d_hist, st);
}

fi_status fi_map_tick_sites_device(fi_engine *e, const fi_tick_site *ts, uint64_t first, uint64_t n,
                                   fi_tick_site *ts_out, fi_site *sites, uint8_t *disp, fi_outcome *host_out) {
    if (!e || (n && (!sites || !disp))) return FI_E_ARG;
    fi_status s = tick_check(e, ts, n, !ts, false);
    if (s || !n) return s;
    if ((s = tick_device_prepare(e, n))) return s;
    std::vector<fi_site> tsv(ts_out ? n : 0);
    s = for_chunks(e, n, [&](uint64_t done, uint64_t k) -> fi_status {
        const ChunkSlot &s0 = e->w.slot[0];
        if (ts) HIPCHK(hipMemcpyAsync(s0.d_tk_in, ts + done, k * sizeof(fi_tick_site), hipMemcpyHostToDevice, e->stream));
        HIPCHK(launch_tick_map(tick_map_ctx(e, first + done, ts ? s0.d_tk_in.get() : nullptr), k, s0.d_sites, e->w.d_keys,
                               e->w.d_perm, s0.d_tk_sites, s0.d_tk_disp, s0.d_tk_res, e->stream));
        HIPCHK(hipMemcpyAsync(sites + done, s0.d_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(disp + done, s0.d_tk_disp, k, hipMemcpyDeviceToHost, e->stream));
        if (host_out)
            HIPCHK(hipMemcpyAsync(host_out + done, s0.d_tk_res, k * sizeof(fi_outcome), hipMemcpyDeviceToHost, e->stream));
        if (ts_out)
            HIPCHK(hipMemcpyAsync(tsv.data() + done, s0.d_tk_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        return FI_OK;
    });
    for (uint64_t i = 0; !s && ts_out && i < n; i++) ts_out[i] = tick_site_of(tsv[i]);
    return s;
}

fi_status fi_run_tick_sites(fi_engine *e, const fi_tick_site *ts, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    if (!e || (n && !ts)) return FI_E_ARG;
    if (e->tick_map == FI_TICK_MAP_DEVICE && n) return tick_run_device(e, 0, ts, n, out, hist);
    fi_status st = tick_check(e, ts, n, false, true);
    if (st) return st;
    std::vector<fi_site> sites(n);
    std::vector<uint8_t> disp(n);
    std::vector<fi_outcome> res(n);
    map_tick_sites(e, ts, n, sites.data(), disp.data(), res.data());
    std::vector<fi_site> run;
    std::vector<uint64_t> idx;
    for (uint64_t i = 0; i < n; i++)
        if (disp[i] == 0) { run.push_back(sites[i]); idx.push_back(i); }
    fi_histogram dh{};
    if (!run.empty()) {
        std::vector<fi_outcome> ro(run.size());
        st = run_common(e, 0, SiteSource::mapped(run.data()), run.size(), ro.data(), &dh);
        if (st) return st;
        for (size_t q = 0; q < idx.size(); q++) res[idx[q]] = ro[q];
    }
    if (out) memcpy(out, res.data(), n * sizeof *out);
    if (hist) {   // by the tick site's own structure and bit (fi_hist_kernel's layout)
        for (uint64_t i = 0; i < n; i++) {
            const fi_outcome &o = res[i];
            const uint32_t cls = o.cls < FI_N_CLASS ? o.cls : FI_ESCAPE;
            hist->counts[ts[i].target][__builtin_ctzll(ts[i].mask)][cls]++;
            if (cls == FI_CRASH) hist->crash_sub[o.sub & 15]++;
            if (cls == FI_ESCAPE) hist->escape_sub[o.sub & 7]++;
            hist->trials++;
            hist->guest_insts += o.ninst;
        }
        hist->fetch_bytes += dh.fetch_bytes; hist->data_bytes += dh.data_bytes;
        hist->cow_pages += dh.cow_pages; hist->device_insts += dh.device_insts;
    }
    return FI_OK;
}

fi_status fi_run_tick_trials(fi_engine *e, uint64_t first, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    if (!e) return FI_E_ARG;
    if (e->tick_map == FI_TICK_MAP_DEVICE) return tick_run_device(e, first, nullptr, n, out, hist);
    std::vector<fi_tick_site> ts(n);
    fi_status st = fi_sample_tick_sites(e, first, n, ts.data());
    if (st) return st;
    return fi_run_tick_sites(e, ts.data(), n, out, hist);
}

// ---- Exact campaigns in the tick domain (DESIGN.md §4j "Tick domain"; the segments, the classes and the
// trial ids: fi_exact_tick.h)
static std::vector<TickRec> tick_recs(const fi_tick_attempt *att, uint64_t n, std::vector<uint64_t> &done) {
    std::vector<TickRec> rec(n);
    done.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        const fi_tick_attempt &a = att[i];
        done[i] = a.done;
        TickRec r{};
        r.pc = a.pc; r.n = a.n; r.fetch_done0 = a.fetch_done0; r.exec = a.exec; r.imm = a.imm; r.g = a.g;
        r.len = a.len; r.nfetch = a.nfetch; r.ctl = a.ctl; r.rd = a.rd; r.rs1 = a.rs1; r.rs2 = a.rs2;
        r.done_rd = a.done_rd; r.flags = a.flags;
        rec[i] = r;
    }
    return rec;
}
static_assert(FI_TA_COMMITS == kTrCommits && FI_TA_ECALL == kTrEcall && FI_TA_PGFAULT == kTrPgfault &&
              FI_TA_END == kTrEnd && FI_TA_MACRO == kTrMacro && FI_TA_TAKEN == kTrTaken, "fi_tick_attempt.flags");
static_assert(FI_XT_MAPPED == kExactTickMapped && FI_XT_TRIAL == kXtTrial && FI_XT_DEAD == kXtDeadTick &&
              FI_XT_GOLDEN == kXtGoldenTick && FI_XT_ESCAPE == kXtEscapeTick, "fi_exact_tick_* constants");

fi_status fi_exact_tick_classes(const fi_tick_attempt *att, uint64_t n_att, uint64_t golden_ticks, uint64_t ninst,
                                int contract, const uint32_t *off33, const uint32_t *ev, uint32_t reg,
                                fi_exact_tick_class *out, uint64_t cap, uint64_t *n, fi_exact_tick_totals *totals) {
    if (!att || !n_att || !golden_ticks || !off33 || (!ev && off33[32]) || reg < 1 || reg > 31 ||
        ninst >= (1ULL << kExactInstBits) || n_att >= (1ULL << 30) ||
        (contract != FI_TICK_CONTRACT_NUMINST && contract != FI_TICK_CONTRACT_LITERAL))
        return FI_E_ARG;
    for (uint64_t i = 0; i < n_att; i++)
        if (att[i].g > i || (i && att[i].done < att[i - 1].done)) return FI_E_ARG;
    std::vector<uint64_t> done;
    const std::vector<TickRec> rec = tick_recs(att, n_att, done);
    std::vector<TickSeg> segs;
    std::vector<uint32_t> seg_off;
    exact_tick_segments(done.data(), rec.data(), n_att, golden_ticks, segs, seg_off);
    std::vector<ExactTickClass> cls;
    ExactTickTotals t{};
    exact_tick_reg_classes(done.data(), rec.data(), n_att, ninst, contract == FI_TICK_CONTRACT_LITERAL ? 1u : 0u,
                           segs.data(), segs.size(), off33, ev, reg, cls, nullptr, nullptr, &t);
    for (size_t i = 0; out && i < cls.size() && i < cap; i++) out[i] = fi_exact_tick_class{cls[i].weight, cls[i].tick, cls[i].inst, 0};
    if (n) *n = cls.size();
    if (totals) *totals = fi_exact_tick_totals{t.dead, t.golden, t.escaped, t.esc_insts};
    return FI_OK;
}

fi_status fi_exact_tick_attempts(fi_engine *e, fi_tick_attempt *out, uint64_t cap, uint64_t *n) {
    if (!e) return FI_E_ARG;
    fi_status s = tick_ready(e);
    if (s) return s;
    const Golden &g = e->gold;
    for (uint64_t i = 0; out && i < cap && i < g.tk_rec.size(); i++) {
        const TickRec &r = g.tk_rec[i];
        out[i] = fi_tick_attempt{g.tk_done[i], r.pc, r.n, r.fetch_done0, r.exec, r.imm, r.g, r.len, r.nfetch, r.ctl,
                                 r.rd, r.rs1, r.rs2, r.done_rd, r.flags};
    }
    if (n) *n = g.tk_rec.size();
    return FI_OK;
}

// The segments and classes of the golden run under the engine's tick contract, on the host; the
// class records uploaded for fi_exact_tick_sites_kernel.
static fi_status exact_tick_build(fi_engine *e) {
    Golden &g = e->gold;
    if (g.xt.ok && g.xt.contract == e->tick_contract) return FI_OK;
    g.xt = ExTick{};
    const auto t0 = std::chrono::steady_clock::now();
    exact_tick_table(g.tk_done.data(), g.tk_rec.data(), g.tk_done.size(), g.info.ninst, g.t_stats.ticks,
                     e->tick_contract == FI_TICK_CONTRACT_LITERAL ? 1u : 0u, g.fw_off.data(), g.fw_ev.data(), g.xt.tab);
    DevBuf<ExactTickClass> d_cls;
    const std::vector<ExactTickClass> &cls = g.xt.tab.cls;
    HIPCHK(d_cls.alloc(std::max<size_t>(cls.size(), 1)));
    if (!cls.empty()) HIPCHK(hipMemcpy(d_cls, cls.data(), cls.size() * sizeof(ExactTickClass), hipMemcpyHostToDevice));
    g.xt.d_cls = std::move(d_cls);
    g.xt.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g.xt.contract = e->tick_contract;
    g.xt.ok = true;
    return FI_OK;
}

// The checks every exact tick entry point shares, then the plan, the ticks without a trial and
// (info, may be NULL) the sizes.  run: a call that runs trials (fi_set_protect* must be off).
static fi_status exact_tick_prepare(fi_engine *e, const char *who, bool run, ExactPlan &p, ExactUntried &dd,
                                    fi_exact_tick_info *info) {
    if (!e) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "%s: golden run required", who);
    if (e->cpu_model != FI_CPU_TIMING)
        return fail(e, FI_E_STATE, "%s: exact tick campaigns need the TimingSimpleCPU model (fi_set_cpu_model)", who);
    if (!e->gold.t_status.empty()) return fail(e, FI_E_STATE, "%s: tick model: %s", who, e->gold.t_status.c_str());
    if (!e->gold.fw_ok)
        return fail(e, FI_E_STATE, "%s: the golden run has no first-access index (a golden trace that is incomplete "
                    "or 2^29 instructions or more)", who);
    if (!e->structures) return fail(e, FI_E_STATE, "%s: fi_set_campaign first", who);
    if (e->structures & (1ULL << FI_T_MEM)) return fail(e, FI_E_ARG, "%s: memory words are not in the tick domain", who);
    if (run && (e->protect || e->protect_opc))
        return fail(e, FI_E_ARG, "%s: selective replication (fi_set_protect*) is not supported", who);
    if (e->gold.tk_done.empty() || !e->gold.t_stats.ticks) return fail(e, FI_E_STATE, "%s: tick model: no attempts", who);
    HIPCHK(hipSetDevice(e->dev));
    fi_status s = exact_tick_build(e);
    if (s) return s;
    const ExTick &x = e->gold.xt;
    fi_exact_tick_info o{};
    p = exact_tick_plan(e->structures, x.tab.off, e->bits, e->burst, o.classes);
    dd = ExactUntried{};
    dd.bits = p.bits;
    const uint64_t T = e->gold.t_stats.ticks;
    for (uint32_t t = 1; t < FI_N_STRUCT; t++) {
        if (!((e->structures >> t) & 1)) continue;
        o.space += T * p.nbits;
        if (t >= 32) continue;
        const ExactTickTotals &r = x.tab.tot[t];
        dd.masked[t] = r.dead + r.golden;
        dd.escaped[t] = r.escaped;
        o.dead_ticks += r.dead + r.golden;
        o.escaped_ticks += r.escaped;
        dd.insts += ((r.dead + r.golden) * e->gold.info.ninst + r.esc_insts) * p.nbits;
    }
    dd.total = (o.dead_ticks + o.escaped_ticks) * p.nbits;
    dd.esc_total = o.escaped_ticks * p.nbits;
    o.trials = p.trials;
    o.segments = x.tab.segs.size();
    o.nbits = p.nbits;
    o.build_ms = x.build_ms;
    if (p.trials >= kExactMaxTrials) return fail(e, FI_E_ARG, "%s: 2^40 exact trials or more", who);
    if (info) *info = o;
    return FI_OK;
}

static fi_status ensure_exact_tick_work(fi_engine *e, uint64_t n) {
    fi_status s = tick_device_prepare(e, n);
    if (s) return s;
    for (ChunkSlot &sl : e->w.slot)
        if (!sl.d_xt_weight) HIPCHK(sl.d_xt_weight.alloc(e->w.cap));
    return FI_OK;
}

fi_status fi_exact_tick_get_info(fi_engine *e, fi_exact_tick_info *out) {
    if (!e || !out) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    return exact_tick_prepare(e, "fi_exact_tick_get_info", false, p, dd, out);
}

fi_status fi_exact_tick_sites(fi_engine *e, uint64_t first, uint64_t n, fi_site *sites, fi_tick_site *representative,
                              uint64_t *weights) {
    if (!e || (n && !sites)) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_tick_prepare(e, "fi_exact_tick_sites", false, p, dd, nullptr);
    if (!s) s = trial_range_check(e, "fi_exact_tick_sites", first, n, p.trials);
    if (s || !n) return s;
    if ((s = ensure_exact_tick_work(e, n))) return s;
    std::vector<fi_site> tsv(representative ? n : 0);
    s = for_chunks(e, n, [&](uint64_t done, uint64_t k) -> fi_status {
        const ChunkSlot &s0 = e->w.slot[0];
        HIPCHK(launch_exact_tick_sites(p, tick_map_ctx(e, 0, nullptr), first + done, k, e->gold.xt.d_cls, s0.d_sites,
                                       e->w.d_keys, e->w.d_perm, s0.d_tk_sites, s0.d_tk_disp, s0.d_tk_res, s0.d_xt_weight,
                                       e->stream));
        HIPCHK(hipMemcpyAsync(sites + done, s0.d_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        if (weights) HIPCHK(hipMemcpyAsync(weights + done, s0.d_xt_weight, k * 8, hipMemcpyDeviceToHost, e->stream));
        if (representative)
            HIPCHK(hipMemcpyAsync(tsv.data() + done, s0.d_tk_sites, k * sizeof(fi_site), hipMemcpyDeviceToHost, e->stream));
        return FI_OK;
    });
    for (uint64_t i = 0; !s && representative && i < n; i++) representative[i] = tick_site_of(tsv[i]);
    return s;
}

fi_status fi_run_exact_ticks(fi_engine *e, uint64_t first, uint64_t n, fi_outcome *out, fi_histogram *hist) {
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_tick_prepare(e, "fi_run_exact_ticks", true, p, dd, nullptr);
    if (!s) s = trial_range_check(e, "fi_run_exact_ticks", first, n, p.trials);
    if (!s) s = ensure_exact_tick_work(e, n);
    if (s) return s;
    return run_blocking(e, first, SiteSource::exact_ticks(&p, e->gold.xt.d_cls), n, out, hist, [&]() -> fi_status {
        if (first == 0) HIPCHK(launch_exact_untried(dd, e->w.d_hist, e->stream));   // the ticks that need no trial
        return FI_OK;
    });
}

fi_status fi_exact_tick_locate(fi_engine *e, const fi_tick_site *ts, uint64_t n, uint64_t *trial, uint8_t *kind) {
    if (!e || (n && (!ts || !trial || !kind))) return FI_E_ARG;
    ExactPlan p;
    ExactUntried dd;
    fi_status s = exact_tick_prepare(e, "fi_exact_tick_locate", false, p, dd, nullptr);
    if (s) return s;
    const Golden &g = e->gold;
    const ExactTickTable &x = g.xt.tab;
    uint64_t row_first[FI_N_STRUCT] = {};   // per selected structure: its first trial
    for (uint32_t t = 1, r = 0; t < FI_N_STRUCT; t++)
        if (((e->structures >> t) & 1)) row_first[t] = p.row[r++].first;
    const uint32_t literal = e->tick_contract == FI_TICK_CONTRACT_LITERAL ? 1u : 0u;
    for (uint64_t i = 0; i < n; i++) {
        const fi_tick_site &t = ts[i];
        const bool target_ok = t.target >= 1 && t.target < FI_N_STRUCT && ((e->structures >> t.target) & 1);
        const uint32_t b = t.mask ? (uint32_t)__builtin_ctzll(t.mask) : 0;
        if (!target_ok || !t.mask || !((p.bits >> b) & 1) || t.mask != exact_burst_mask(p.burst) << b ||
            t.tick >= g.t_stats.ticks)
            return fail(e, FI_E_ARG, "fi_exact_tick_locate: site %llu (target %u, mask %llx, tick %llu) is outside the "
                        "campaign's space", (unsigned long long)i, t.target, (unsigned long long)t.mask,
                        (unsigned long long)t.tick);
        uint32_t c = 0;
        kind[i] = exact_tick_locate(x, g.tk_done.data(), g.tk_rec.data(), g.tk_done.size(), g.info.ninst, g.t_stats.ticks,
                                    literal, g.fw_off.data(), g.fw_ev.data(), t.tick, t.target, t.mask, &c);
        const uint64_t slot = (uint64_t)__builtin_popcountll(p.bits & ((1ULL << b) - 1));
        trial[i] = kind[i] == kXtTrial ? row_first[t.target] + (uint64_t)c * p.nbits + slot : 0;
    }
    return FI_OK;
}

fi_status fi_run_trials_device(fi_engine *e, uint64_t first, uint64_t n, void *d_out, void *d_hist, void *stream) {
    if (!e || !d_out || !d_hist) return FI_E_ARG;
    if (!e->gold.have_golden) return fail(e, FI_E_STATE, "golden run required");
    if (!e->structures) return fail(e, FI_E_STATE, "fi_set_campaign first");
    HIPCHK(hipSetDevice(e->dev));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    const fi_status s = ensure_work_for(e, n);
    if (s) return s;
    return run_chunks(e, first, SiteSource::sampled(), n, (fi_outcome *)d_out, nullptr, (fi_histogram *)d_hist, st);
}

fi_status fi_sync(fi_engine *e) {
    if (!e) return FI_E_ARG;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->ev0, e->ev1) == hipSuccess) e->last_ms = ms;
    return FI_OK;
}

double fi_last_kernel_ms(fi_engine *e) { return e ? e->last_ms : 0.0; }

const char *fi_translate_status(fi_engine *e) { return e ? e->gold.tx_status.c_str() : "no engine"; }

// hipRTC build of the trial kernel with `body` as translated blocks, no
// device needed (tests; inspecting generated code offline).
fi_status fi_debug_jit_compile(const char *body, const char *arch, void *code, uint64_t cap, uint64_t *len,
                               char *err, uint64_t err_cap) {
    std::vector<char> co;
    bool cached = false;
    const std::string msg = jit_compile(body ? body : "", arch ? arch : "gfx950", co, cached, 0, true);
    if (err && err_cap) {
        const uint64_t n = std::min<uint64_t>(err_cap - 1, msg.size());
        memcpy(err, msg.data(), n);
        err[n] = 0;
    }
    if (!msg.empty()) return FI_E_HIP;
    if (code && cap) memcpy(code, co.data(), std::min<uint64_t>(cap, co.size()));
    if (len) *len = co.size();
    return FI_OK;
}

// One part of the load-time build as an engine runs it (part 1..3, the disk
// cache on or off, FI_CFG_JIT_NO_CACHE), no device needed: *cached = 1 when
// the code object came from the cache.  Tests of the per-node build lock.
fi_status fi_debug_jit_build(const char *body, const char *arch, int part, int use_cache, uint64_t *len,
                             int *cached, char *err, uint64_t err_cap) {
    std::vector<char> co;
    bool c = false;
    const std::string msg = jit_compile(body ? body : "", arch ? arch : "gfx950", co, c, part, use_cache != 0);
    if (err && err_cap) {
        const uint64_t n = std::min<uint64_t>(err_cap - 1, msg.size());
        memcpy(err, msg.data(), n);
        err[n] = 0;
    }
    if (len) *len = co.size();
    if (cached) *cached = c ? 1 : 0;
    return msg.empty() ? FI_OK : FI_E_HIP;
}

fi_status fi_debug_waves(fi_engine *e, uint64_t *out, uint64_t n_waves) {
    if (!e || !out) return FI_E_ARG;
    if (n_waves > e->w.cap) return fail(e, FI_E_ARG, "more waves than the work buffers hold");
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->w.d_wave_dbg, n_waves * kWaveDbgWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FI_OK;
}

fi_status fi_debug_epochs(fi_engine *e, uint32_t *out16) {
    if (!e || !out16 || !e->w.d_cnt) return FI_E_ARG;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out16, e->w.d_cnt, 16 * 4, hipMemcpyDeviceToHost));
    return FI_OK;
}

fi_status fi_debug_golden_trace(fi_engine *e, void *pre_out, uint64_t pre_cap, uint64_t *n_pre, uint32_t *trace_out,
                                uint64_t trace_cap, uint64_t *n_trace, uint64_t *text_lo) {
    if (!e) return FI_E_ARG;
    if (pre_out) memcpy(pre_out, e->gold.g_pre.data(), std::min<uint64_t>(pre_cap, e->gold.g_pre.size()) * sizeof(PreInst));
    if (trace_out) memcpy(trace_out, e->gold.g_trace.data(), std::min<uint64_t>(trace_cap, e->gold.g_trace.size()) * 4);
    if (n_pre) *n_pre = e->gold.g_pre.size();
    if (n_trace) *n_trace = e->gold.g_trace.size();
    if (text_lo) *text_lo = e->img.text_lo;
    return FI_OK;
}

fi_status fi_debug_loop_est(const void *pre, uint64_t n_pre, uint64_t text_lo, const uint32_t *trace,
                            uint64_t n_trace, void *out, uint64_t cap, uint64_t *n) {
    if (!pre || !trace) return FI_E_ARG;
    std::vector<PreInst> p((const PreInst *)pre, (const PreInst *)pre + n_pre);
    std::vector<uint32_t> t(trace, trace + n_trace), leaders;
    std::vector<LoopEst> loops;
    uint32_t n_tx = 0;
    (void)translate_blocks(p, text_lo, t, {}, leaders, n_tx, true, &loops);
    static_assert(sizeof(LoopEst) == 16, "LoopEst is 16 bytes (fi_debug.h)");
    if (out) memcpy(out, loops.data(), std::min<uint64_t>(cap, loops.size()) * sizeof(LoopEst));
    if (n) *n = loops.size();
    return FI_OK;
}

fi_status fi_debug_translate(const void *pre, uint64_t n_pre, uint64_t text_lo, const uint32_t *trace,
                             uint64_t n_trace, char *out, uint64_t cap, uint64_t *len) {
    return fi_debug_translate_flags(pre, n_pre, text_lo, trace, n_trace, 0, out, cap, len);
}

fi_status fi_debug_translate_flags(const void *pre, uint64_t n_pre, uint64_t text_lo, const uint32_t *trace,
                                   uint64_t n_trace, uint32_t flags, char *out, uint64_t cap, uint64_t *len) {
    if (!pre || !trace) return FI_E_ARG;
    std::vector<PreInst> p((const PreInst *)pre, (const PreInst *)pre + n_pre);
    std::vector<uint32_t> t(trace, trace + n_trace);
    std::vector<uint32_t> leaders;
    uint32_t n_tx = 0;
    const std::string body = translate_blocks(p, text_lo, t, {}, leaders, n_tx, true, nullptr,
                                              !(flags & FI_CFG_NO_LOAD_AHEAD), !(flags & FI_CFG_NO_LOOP_STRETCH));
    if (out && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, body.size());
        memcpy(out, body.data(), n);
        out[n] = 0;
    }
    if (len) *len = body.size();
    return FI_OK;
}

fi_status fi_debug_translation(fi_engine *e, char *buf, uint64_t cap, uint64_t *len) {
    if (!e) return FI_E_ARG;
    if (buf && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, e->gold.tx_body.size());
        memcpy(buf, e->gold.tx_body.data(), n);
        buf[n] = 0;
    }
    if (len) *len = e->gold.tx_body.size();
    return FI_OK;
}

const char *fi_debug_stat_name(uint32_t slot) {
    switch (slot) {
#define FI_STAT_NAME(name, idx, what) \
    case idx: return #name;
        FI_STAT_SLOTS(FI_STAT_NAME)
#undef FI_STAT_NAME
    }
    return nullptr;
}

fi_status fi_debug_stats(fi_engine *e, uint64_t *out64) {
    if (!e || !out64) return FI_E_ARG;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out64, e->w.d_stats, kNStats * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FI_OK;
}

fi_status fi_get_config(fi_engine *e, fi_config *out) {
    if (!e || !out) return FI_E_ARG;
    *out = e->cfg;
    return FI_OK;
}

fi_status fi_kernel_timer_reset(fi_engine *e) {
    if (!e) return FI_E_ARG;
    e->tused = 0;
    if (!e->d_span) {
        HIPCHK(hipSetDevice(e->dev));
        HIPCHK(e->d_span.alloc(kTimerSlots * 2));
    }
    // every slot's min starts at ~0, its max at 0 (layout: slot i at [2i, 2i + 1])
    HIPCHK(hipMemsetAsync(e->d_span, 0, kTimerSlots * 2 * sizeof(unsigned long long), e->stream));
    HIPCHK(launch_span_init(e->d_span, kTimerSlots, e->stream));
    return FI_OK;
}

fi_status fi_kernel_timer_read(fi_engine *e, double *total_ms, uint32_t *launches) {
    if (!e) return FI_E_ARG;
    double t = 0;
    for (size_t i = 0; i < e->tused; i++) {
        HIPCHK(hipEventSynchronize(e->tpool[i].second));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e->tpool[i].first, e->tpool[i].second));
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = (uint32_t)e->tused;
    return FI_OK;
}

// ------------------------------------------------------------------ debug hooks (tests)
fi_status fi_debug_dispatch_ms(fi_engine *e, float *ms, uint32_t cap, uint32_t *n) {
    if (!e || (!ms && cap)) return FI_E_ARG;
    for (size_t i = 0; i < e->tused && i < cap; i++) {
        HIPCHK(hipEventSynchronize(e->tpool[i].second));
        HIPCHK(hipEventElapsedTime(&ms[i], e->tpool[i].first, e->tpool[i].second));
    }
    if (n) *n = (uint32_t)e->tused;
    return FI_OK;
}

fi_status fi_debug_dispatch_span_ms(fi_engine *e, float *ms, uint32_t cap, uint32_t *n) {
    if (!e || (!ms && cap)) return FI_E_ARG;
    const size_t k = std::min<size_t>(e->tused, cap);
    if (k) {
        if (!e->d_span) return fail(e, FI_E_STATE, "fi_debug_dispatch_span_ms: fi_kernel_timer_reset first");
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipStreamSynchronize(e->stream_odd));
        std::vector<unsigned long long> h(2 * k);
        HIPCHK(hipMemcpy(h.data(), e->d_span, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < k; i++)   // (s_memrealtime runs at 100 MHz; no trial ran: 0)
            ms[i] = h[2 * i + 1] > h[2 * i] ? (float)((h[2 * i + 1] - h[2 * i]) * 1e-5) : 0.0f;
    }
    if (n) *n = (uint32_t)e->tused;
    return FI_OK;
}
fi_status fi_debug_dispatch_kinds(fi_engine *e, uint32_t *kinds, uint32_t cap, uint32_t *n) {
    if (!e || (!kinds && cap)) return FI_E_ARG;
    for (size_t i = 0; i < e->tused && i < cap; i++) kinds[i] = e->tkind[i];
    if (n) *n = (uint32_t)e->tused;
    return FI_OK;
}

fi_status fi_debug_decode(fi_engine *e, const uint32_t *raws, uint64_t n, void *out16) {
    if (!e || !raws || !out16) return FI_E_ARG;
    HIPCHK(hipSetDevice(e->dev));
    DevBuf<uint32_t> d_raw;
    DevBuf<PreInst> d_o;
    HIPCHK(d_raw.alloc(n));
    HIPCHK(d_o.alloc(n));
    HIPCHK(hipMemcpy(d_raw.get(), raws, n * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_debug_decode(d_raw.get(), n, d_o.get(), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out16, d_o.get(), n * sizeof(PreInst), hipMemcpyDeviceToHost));
    return FI_OK;
}

fi_status fi_debug_loop_outcome(fi_engine *e, const fi_debug_loop *in, uint64_t n, fi_debug_loop_out *out) {
    if (!e || (n && (!in || !out))) return FI_E_ARG;
    if (e->img.snaps.empty()) return fail(e, FI_E_STATE, "fi_debug_loop_outcome: fi_golden_run first");
    if (!n) return FI_OK;
    HIPCHK(hipSetDevice(e->dev));
    DevBuf<fi_debug_loop> d_in;
    DevBuf<fi_debug_loop_out> d_out;
    HIPCHK(d_in.alloc(n));
    HIPCHK(d_out.alloc(n));
    HIPCHK(hipMemcpy(d_in.get(), in, n * sizeof *in, hipMemcpyHostToDevice));
    DevCtx c = base_ctx(e);
    HIPCHK(launch_debug_loop(c, d_in.get(), n, d_out.get(), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, d_out.get(), n * sizeof *out, hipMemcpyDeviceToHost));
    return FI_OK;
}

}  // extern "C"
