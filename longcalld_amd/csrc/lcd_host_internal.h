// lcd_host_internal.h -- what the host files of liblcd_hotpath.so share: the runtime core (error string, device selection, the device-memory budget and its
// buffers, host thread teams), the interval helpers and the definitions of the two opaque handles.  Not part of the C ABI, not installed; every name lives in
// lcd_internal, whose visibility is hidden, so nothing here becomes an exported symbol of the library.  State is defined in lcd_runtime.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/lcd_hotpath.h"
#include "lcd_kernels.h"
#include "lcd_types.h"
#include "lcd_io_internal.h"
#include "lcd_plan.h" // the planner of lcd_plan.cpp (ChainRec, PlanHints, chain_caps, wfa_plan, ...) and, through it, lcd_switches.h (HostSwitches)

namespace lcd_internal __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;   // what lcd_last_error returns on this thread
inline int set_err(int code, const std::string &m) { g_err = m; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { return set_err(-10, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)

#define LCD_MAX_DEV 16
extern int g_n_devices;
extern int g_n_cus; // compute units of the device (MI355X: 256)
// (device selection: lcd_runtime.cpp)
int init_default_device();
int use_device(int dev); // dev < 0: the calling thread's device (lcd_set_thread_device), else the process default
inline int ensure_init() { return use_device(-1); }
inline int cur_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; } return d < LCD_MAX_DEV ? d : 0; }

// the device-memory ledger of the grow-only buffers and its budget (lcd_runtime.cpp)
extern std::atomic<long long> g_dev_bytes[LCD_MAX_DEV];
extern std::atomic<unsigned long long> g_copy_bytes[4]; // [0] digars device -> host, [1] digars host -> device, [2] read bases host -> device (packed or unpacked), [3] read bases device -> host
extern std::atomic<long long> g_alloc_events; // hipMalloc calls of the grow-only buffers (bench.py reports how many fell into its timed region)
long long dev_budget(int d);
// grow-only PINNED host block (hipHostMalloc): the destination of a batch's result download -- a pageable destination is staged by the runtime at a few GB/s
struct PinnedBuf {
    uint8_t *p = nullptr; size_t n = 0, cap = 0;
    void resize(size_t want) {
        if (want > cap) {
            if (p) hipHostFree(p);
            p = nullptr; cap = 0;
            const size_t c = want + (want >> 2) + 4096;
            void *q = nullptr;
            if (hipHostMalloc(&q, c, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); q = malloc(c); pageable = true; }
            p = (uint8_t *)q; cap = c;
        }
        n = want;
    }
    bool pageable = false;
    uint8_t *data() { return p; } const uint8_t *data() const { return p; } size_t size() const { return n; }
    ~PinnedBuf() { if (p) { if (pageable) free(p); else hipHostFree(p); } }
    PinnedBuf() = default; PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
};
struct DevBuf {
    void *p = nullptr; size_t cap = 0; int dev = 0;
    int ensure(size_t n, int headroom_shift = 2);
    void release() { if (p) { hipFree(p); g_dev_bytes[dev] -= (long long)cap; p = nullptr; cap = 0; } }
    uint64_t addr() const { return (uint64_t)(uintptr_t)p; }
    ~DevBuf() { release(); }
    DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
};
// an ad-hoc stream of a per-call entry point: destroyed on every return path
struct StreamGuard {
    hipStream_t s = nullptr;
    int create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? 0 : set_err(-10, "hipStreamCreate failed"); }
    ~StreamGuard() { if (s) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
// one host staging block whose offsets become device addresses: put(p, bytes) appends `bytes` at the next 16-byte boundary (copied from p; left zero where p is
// NULL) and returns their offset
struct StagePut {
    std::vector<uint8_t> &hb;
    uint64_t operator()(const void *p, size_t bytes) const { size_t o = lcd_align_up(hb.size(), 16); hb.resize(o + bytes); if (p && bytes) memcpy(hb.data() + o, p, bytes); return (uint64_t)o; }
};

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// host threads per team of the submission's short parallel loops (capacities, job tables, records, plans).  LCD_HOST_TEAM (HostSwitches.host_team): a caller whose own
// threads are busy beside the submission -- bench.py's PCIe-inclusive pipeline on a box whose cgroup allows 16 CPUs -- asks for fewer; a team that overruns the
// quota freezes every thread of the process, the submitter included, until the next period
// CPUs this process may use: its affinity mask, cut by the cgroup's CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us) -- a container with 128 visible
// cores and a 16-CPU quota is a 16-CPU box for thread teams
inline int host_cpus() {
    static const int n = [] {
        int k = 0;
        cpu_set_t set; CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) k = CPU_COUNT(&set);
        if (k <= 0) k = (int)std::max(1u, std::thread::hardware_concurrency());
        double quota = 0;
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { char a[64] = {0}; long long per = 0; if (fscanf(f, "%63s %lld", a, &per) == 2 && strcmp(a, "max") != 0 && per > 0) quota = atof(a) / (double)per; fclose(f); }
        else {
            long long q = -1, per = 0;
            if (FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%lld", &q) != 1) q = -1; fclose(fq); }
            if (FILE *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%lld", &per) != 1) per = 0; fclose(fp); }
            if (q > 0 && per > 0) quota = (double)q / (double)per;
        }
        if (quota > 0) k = std::max(1, std::min(k, (int)(quota + 0.5)));
        return k;
    }();
    return n;
}
// processes of this job on this host: one per GPU under torch.distributed.run (LOCAL_WORLD_SIZE; WORLD_SIZE on a single node)
inline int host_local_world() {
    const char *e = getenv("LOCAL_WORLD_SIZE"); if (!e || atoi(e) < 1) e = getenv("WORLD_SIZE");
    const int w = e ? atoi(e) : 1;
    return w < 1 ? 1 : w;
}
// With N ranks on one host every rank runs these teams at the same moments (the ranks step together): the default is the host's CPUs divided by the ranks, at most 8.
inline int host_team(const HostSwitches &sw) {
    const int v = sw.host_team != kSwitchUnset ? sw.host_team : std::min(8, std::max(1, host_cpus() / host_local_world()));
    return v < 1 ? 1 : v > 32 ? 32 : v;
}
// (threads that lay results out on the host, lcd_batch_results_arena: LCD_ARENA_THREADS, default 16 -- or the rank's share of the host's CPUs)
inline int host_arena_threads(const HostSwitches &sw) {
    return sw.arena_threads != kSwitchUnset ? std::max(1, sw.arena_threads) : std::min(16, std::max(1, host_cpus() / host_local_world()));
}
// a loop over [0, n) cut into chunks taken by up to `max_threads` host threads (the calling thread is one of them); f(lo, hi, thread index)
template <class F> static void par_chunks(const size_t n, const int max_threads, const size_t chunk, F f) {
    const int nth = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, max_threads), (n + chunk - 1) / std::max<size_t>(1, chunk)));
    if (nth <= 1) { if (n) f((size_t)0, n, 0); return; }
    std::atomic<size_t> next{0};
    auto work = [&](const int t) { for (size_t lo; (lo = next.fetch_add(chunk)) < n;) f(lo, std::min(n, lo + chunk), t); };
    std::vector<std::thread> ths;
    for (int t = 1; t < nth; ++t) ths.emplace_back(work, t);
    work(0);
    for (auto &t : ths) t.join();
}
inline LcdScoring scoring_of(const lcd_opt_t &o, const HostSwitches &sw) { LcdScoring s; s.match = o.match; s.mismatch = o.mismatch; s.o1 = o.gap_open1; s.e1 = o.gap_ext1; s.o2 = o.gap_open2; s.e2 = o.gap_ext2; s.dbg = sw.dbg; s.wd_s = sw.watchdog_s; return s; }
struct NIv { uint64_t x; long long en; int label; }; // x: the interval index's sort key (contig 0: the start)

// ---- the records of a region batch (lcd_host.cpp) ----
struct RegRead { // one read of a region, in sorted order after add
    int id, len, cover, hap; int64_t ps; uint64_t off; double err;
    int rb = -1, re = -2; // read_reg_beg / read_reg_end of collect_noisy_read_info (chunk-view entry only)
};
struct AnchorRec {
    int pread;                    // index into preads
    int ext;                      // 1 L->R, 2 R->L ; 0: sampling-mode full-read K4 filter only
    int tlen_full, qlen_full;     // _tlen, _qlen
    int ed_job, wfa_job;
    int min_len;
};
struct RegionRec {
    int64_t reg_len; int n_reads;
    std::vector<RegRead> reads;   // sorted (src/align.c:1774)
    uint64_t ref_off; int ref_len;
    int branch;                   // 0 skipped, 1 with-PS (K1 x2), 2 no-PS (K2)
    int sampling;
    int chain[2];                 // chain indices (-1 none)
    // results
    int n_cons = 0;
};

// pre_process_noisy_regs' host part in front of the read support (lcd_noisy_regs.cpp): cr_index, low-complexity extension, cr_merge twice
void pre_regs_merge(std::vector<NIv> &v, const int64_t *low_comp, int n_low);

// lcd_call_files' links of a window of chunks to what lies outside it (lcd_call.cpp: chunks_call_core)
struct CallLinks { const char *const *chroms; const int *tids; const lcd_stitch_carry_t *carry_in; lcd_stitch_carry_t *carry_out; int next_tid; int64_t next_beg, next_end; };
// the VCF options of one driver call (lcd_vcf_fields_t), resolved once: the TE library and its names, the names mode; and what the call gives back
// (lcd_vcf_fields_out_t).  The library is read-only after open(); n_mei / rnames are written by the one thread that runs chunks_call_core
struct FieldsRun {
    lcd_te_lib_t *lib = nullptr; char **te_names = nullptr; int n_te = 0, rnames_mode = 0;
    bool collect_rnames = false; int64_t n_mei = 0; std::vector<char *> rnames;
    int open(const lcd_vcf_fields_t *f, const std::string &W);       // before any output file is created
    void give(lcd_vcf_fields_out_t *out);                            // moves the names and the collected values into *out (NULL: nothing)
    bool active() const { return lib || rnames_mode; }
    ~FieldsRun();
    FieldsRun() = default; FieldsRun(const FieldsRun &) = delete; FieldsRun &operator=(const FieldsRun &) = delete;
};
int chunks_call_core(int n, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, const CallLinks *links, FieldsRun *fields, lcd_var1_t **records, int *n_records,
                     char **vcf_body);
// a driver's entry: every output the caller named is zeroed, refusal paths included (n_reads_per_file has the driver's own length and is zeroed there)
inline void zero_run_out(const lcd_run_out_t *out) {
    if (!out) return;
    if (out->idx_stats) memset(out->idx_stats, 0, sizeof(*out->idx_stats));
    if (out->fields_out) memset(out->fields_out, 0, sizeof(*out->fields_out));
    if (out->refine_stats) memset(out->refine_stats, 0, sizeof(*out->refine_stats));
    if (out->sam_stats) memset(out->sam_stats, 0, sizeof(*out->sam_stats));
}
// what the two drivers refuse of lcd_run_opt_t.aln before anything else
inline int check_aln_opt(const std::string &W, const lcd_run_opt_t *opt) {
    if (!opt || !opt->aln) return 0;
    if (opt->aln->format != LCD_ALN_BAM && opt->aln->format != LCD_ALN_SAM) return set_err(-4, W + ": format must be LCD_ALN_BAM or LCD_ALN_SAM");
    if (opt->aln->refine && opt->fields) return set_err(-2, W + ": refined alignments together with the VCF fields are not supported");
    return 0;
}

// the device buffers of lcd_chunk_mod_pileup: a call of its own makes and frees them, a driver run keeps one set for all its chunks (grow-only, as every DevBuf)
struct ModsScratch { DevBuf d_jobs, d_cls, d_ref, d_idx, d_small, d_tab, d_rows; };
lcd_mods_t *mod_pileup_core(const lcd_chunk_t *c, const int *haps, const lcd_mods_opt_t *opt, lcd_mods_stats_t *stats, ModsScratch &S);
// the methylation table of a driver run (lcd_run_ext2_t.mods_path; lcd_mods.cpp): the refusals, the file, every chunk's pile-up in plan order, the sums of the
// statistics and -- with combine_strands -- the last row of the chunk before, held back until the next chunk's first row is known.  One thread at a time.
struct ModsSink {
    FILE *f = nullptr; std::string path; lcd_mods_opt_t opt; lcd_mods_stats_t sum; lcd_mods_stats_t *stats_out = nullptr;
    bool head = false, held = false; std::string held_chrom; int64_t held_pos = 0; uint32_t held_cnt[9];
    ModsScratch scratch;     // (freed with the sink)
    // ext2 as the caller's struct of any size -> *x2 (what lies behind its `size` reads as zero) and the pile-up's options; -4 before anything is created
    static int parse(const std::string &W, const lcd_run_ext2_t *ext2, lcd_run_ext2_t *x2, lcd_mods_opt_t *mo);
    int open(const std::string &W, const lcd_run_ext2_t &x2, const lcd_mods_opt_t &mo);     // creates the file
    int chunk(const lcd_chunk_t *handle, const lcd_first_chunk_t &x, const char *chrom);    // the chunk's pile-up with its final haplotypes, its rows written
    int finish(bool ok);     // ok: the held row, the header of an empty table, close, *stats_out; else (or when that fails): close and remove.  0 or -30
    bool active() const { return f != nullptr; }
    ~ModsSink() { if (f) { fclose(f); remove(path.c_str()); } }
    ModsSink() = default; ModsSink(const ModsSink &) = delete; ModsSink &operator=(const ModsSink &) = delete;
private:
    int put(int n, const int64_t *pos, const char *strand, const uint32_t *cnt, const char *chrom);
    int flush_held();
};
// the device buffers of lcd_chunk_depth (the difference array, the tile partials, the rows): kept by the sink of a driver run, as ModsScratch is
struct DepthScratch { DevBuf d_jobs, d_diff, d_parts, d_small, d_rows; };
lcd_depth_t *depth_core(const lcd_chunk_t *c, const int *haps, const lcd_depth_opt_t *opt, lcd_depth_stats_t *stats, DepthScratch &S);
// the depth track of a driver run (lcd_run_ext2_t.depth_path; lcd_depth.cpp): the refusals, the file, every chunk's rows in plan order (through the window rule
// with depth_window), the sums of the statistics and the last row of the chunk before, ALWAYS held back until the next chunk's first row is known: the two join
// by the seam rule of include/lcd_hotpath.h, or the held row is written as it is.  One thread at a time.
struct DepthSink {
    FILE *f = nullptr; std::string path; lcd_depth_opt_t opt; lcd_depth_stats_t sum; lcd_depth_stats_t *stats_out = nullptr;
    bool head = false, held = false; std::string held_chrom; int64_t held_beg = 0, held_end = 0; uint64_t held_val[3];
    DepthScratch scratch;    // (freed with the sink)
    static int parse(const std::string &W, const lcd_run_ext2_t &x2);          // x2 as ModsSink::parse left it; -4 before anything is created
    int open(const std::string &W, const lcd_run_ext2_t &x2);                  // creates the file
    int chunk(const lcd_chunk_t *handle, const lcd_first_chunk_t &x, const char *chrom);
    int finish(bool ok);     // ok: the held row, the header of an empty track, close, *stats_out; else (or when that fails): close and remove.  0 or -30
    bool active() const { return f != nullptr; }
    ~DepthSink() { if (f) { fclose(f); remove(path.c_str()); } }
    DepthSink() = default; DepthSink(const DepthSink &) = delete; DepthSink &operator=(const DepthSink &) = delete;
private:
    int put(int n, const int64_t *beg, const int64_t *end, const uint64_t *val, const char *chrom);      // val: depths, or the windows' sums
    int flush_held();
};
// the per-haplotype read sets of a driver run (lcd_run_ext2_split_t; lcd_split.cpp): the refusals, the three FASTQ files and the haplotag list, every chunk's
// lcd_chunk_split_reads in plan order with the plan the alignment writer makes for that chunk (rules 4 and 5), the sums of the statistics.  With gz every append
// of a FASTQ file is compressed in HBM and close adds the EOF member.  One thread at a time.
struct SplitSink {
    FILE *f[4] = {nullptr, nullptr, nullptr, nullptr}; std::string path[4];      // streams 0 none, 1, 2; 3: the list
    bool gz = false; int sort_output = 0; lcd_split_opt_t opt; lcd_split_stats_t sum; lcd_split_stats_t *stats_out = nullptr; lcd_sam_names_t *names = nullptr;
    // ext2 as the caller's struct of any size -> *xs (what lies behind its `size` reads as zero); other: the run's further output paths (NULL entries: none).
    // -4 before anything is created
    static int parse(const std::string &W, const lcd_run_ext2_t *ext2, lcd_run_ext2_split_t *xs, int n_other, const char *const *other);
    int open(const std::string &W, const lcd_run_ext2_split_t &xs, int n_ref, const char *const *ref_names, int sort_output);     // creates the files
    // the chunks of a window, as lcd_bam_writer_append takes them (tids NULL: one contig; prev: the chunk in front of the window or NULL)
    int window(int n, const lcd_call_chunk_t *chunks, const int *tids, const lcd_stitch_carry_t *prev);
    int finish(bool ok);     // ok: the EOF members, close, *stats_out; else (or when that fails): close and remove.  0 or -30
    bool active() const { return f[0] || f[3]; }
    ~SplitSink() { drop(); }
    SplitSink() = default; SplitSink(const SplitSink &) = delete; SplitSink &operator=(const SplitSink &) = delete;
private:
    int put(int s, const lcd_split_t *h);
    void drop();             // closes and removes what is open
};
struct VarRegionRec { int region, n_cons, rows[2], cap, n_vars, alt_bytes; uint64_t rec_off, alt_off, prof_off, se_off; };

} // namespace lcd_internal

// lcd_vcf_index.cpp: what a VCF index builder has counted so far (lines, contigs, chunks, the bytes and times of finish), for the VCF writer and the whole-file driver
void lcd_vcf_index_builder_counts(const lcd_vcf_index_builder_t *b, lcd_vcf_index_stats_t *S) __attribute__((visibility("hidden")));
extern "C" void lcd_account_device_bytes(int device, long long delta); // the ledger's entry for buffers allocated outside DevBuf (lcd_io.cpp's inflated streams); exported, not in the public header
// the planner's probes (lcd_host.cpp; exported, not in the public header): the decisions of lcd_plan.cpp for one chain / one WFA job, without a device.
// out[12]: threads, wmax, lds_bytes, ring_k, ring16, solo, cert, node_cap, edge_cap, cell_cap, spill_x, min_w.  cert_level / solo: -1 automatic; hints: cell K1, cell K2, node (NULL: the learned ones)
extern "C" int lcd_plan_chain_probe(const lcd_opt_t *opt, int mode, int n_reads, const int *read_len, int scale, int cert_level, int solo, long long n_chains, const int *hints, int64_t *out);
// out[6]: lds, s_cap, blk_rows, n_ckpt, ws_bytes, class
extern "C" int lcd_plan_wfa_probe(int plen, int tlen, long long s_want, int anchor, int wfa_hint, const int *scoring, int64_t *out);

// lcd_batch_s and lcd_chunk_s are the global types behind the public handles: their members name the types above
using lcd_internal::RegRead; using lcd_internal::ChainRec; using lcd_internal::AnchorRec; using lcd_internal::RegionRec; using lcd_internal::VarRegionRec;
using lcd_internal::DevBuf; using lcd_internal::PinnedBuf;
#define LCD_NSIDE 12
static_assert(lcd_internal::kMaxStreams == LCD_NSIDE + 1, "LCD_STREAMS is clamped to the caller's stream plus the side streams of a batch");
struct lcd_batch_s {
    lcd_opt_t opt;
    int device = 0;                      // every entry point on this batch selects it (HIP's current device is per host thread)
    hipStream_t stream = nullptr;
    hipStream_t side[LCD_NSIDE] = {};
    hipEvent_t ev[10];
    hipEvent_t sev[LCD_NSIDE + 1];
    std::vector<uint8_t> h_pool;
    std::vector<UnpackJob> unpack_abs; DevBuf d_unpack_abs; uint64_t pool_read_bytes = 0; // slices whose packed bases are ALREADY in HBM (lcd_chunk_t): src = device address; read bases inside h_pool (the copy counter)
    std::vector<uint8_t> h_packed; std::vector<UnpackJob> unpack_jobs; // read slices handed over 4-bit packed: unpacked into d_in after the upload
    std::vector<RegionRec> regs;
    std::vector<ChainRec> chains;
    std::vector<PoaRead> preads;         // seq_off relative to h_pool until run()
    std::vector<AnchorRec> anchors;
    std::vector<EdJob> ed_jobs;          // offsets relative to h_pool until run()
    std::vector<WfaJob> wfa_jobs;
    // device
    // (d_poa_arena: the ONE transient workspace of a submission led by this batch -- chain arenas, WFA wavefronts and edlib blocks in turn)
    DevBuf d_read_patches, d_aends_jobs, d_aends_outs, d_in, d_chains, d_preads, d_poa_arena, d_poa_out, d_poa_outs, d_ed_jobs, d_ed_outs, d_wfa_jobs,
        d_wfa_out, d_wfa_outs, d_str_jobs, d_str_outs, d_final, d_gate, d_cmp_jobs, d_cmp_outs, d_cmp_seg, d_cmp_segres, d_seg_out, d_rr,
        d_var_jobs, d_var_outs, d_var_work, d_vreg_jobs, d_vreg_outs, d_var_out, d_slot_flags, d_spare, d_packed, d_unpack,
        d_early_arena, d_chains_early, d_poa_outs_early,   // the long K2 chains that start before the anchor stage (lcd_host.cpp launch_early)
        d_ed_arena;                                                         // K4's stored columns when it runs beside K3 in the anchor stage
    bool uploaded = false, ran = false, downloaded = false;
    // results (host)
    std::vector<PoaChainOut> couts;
    std::vector<PoaChain> pchains;
    std::vector<WfaJob> rc_jobs; std::vector<WfaOut> rc_outs; // ref<->cons
    std::vector<int> rc_region, rc_clu;
    std::vector<uint32_t> reg_rc0, reg_str0;   // [n_regions + 1]: the ref<->cons / string jobs of region r are [reg_rc0[r], reg_rc0[r + 1]) and [reg_str0[r], reg_str0[r + 1]) (jobs are made region by region)
    std::vector<StrJob> str_jobs; std::vector<StrOut> str_outs;
    std::vector<int> str_region, str_clu, str_k;
    PinnedBuf h_final; std::vector<uint8_t> h_poa_out; std::vector<uint8_t> h_cig;
    PinnedBuf h_sub_pin, h_tmp_pin; // leader: the chain table of a round and the chains' output records (page-locked and kept: 7 + 9 MB per 20-batch round were allocated, zeroed and faulted in every time)
    std::vector<std::pair<int, uint32_t>> clu_gather_index;
    bool gathered = false; uint64_t g_extra = 0, g_clu_base = 0; std::vector<uint64_t> g_rc_off; // the scattered result pieces are already in d_gather (stage_gather at the end of the run): the download is copies only
    DevBuf d_gather, d_gather_jobs; std::vector<std::pair<int, uint32_t>> clu_index;   // download: staging block of the scattered pieces; (chain, offset into h_poa_out) of the K2 cluster lists
    std::vector<WfaJob> h_rc_all; std::vector<StrJob> h_str_all; std::vector<StrOut> h_str_outs; // leader: the joint job tables of a submission (kept between submissions: no reallocation, no first-touch page faults in the steady state)
    // ref<->read strings (opt.collect_ref_read_aln_str): per string job, rows in d_rr at rr_off (target row, query row at +rr_stride)
    std::vector<uint64_t> rr_off; std::vector<int> rr_len, rr_stride; std::vector<uint8_t> h_rr; uint64_t rr_bytes = 0;
    // candidate variants (opt.collect_noisy_vars): per resolved region, offsets into d_var_out / h_var
    std::vector<VarRegionRec> vregs; std::vector<int> vreg_of; std::vector<uint8_t> h_var; uint64_t var_bytes = 0;
    std::vector<std::unique_ptr<DevBuf>> retry_out; // output blocks of chains re-run with a larger graph capacity (live until the next run; the buffers
    size_t retry_out_used = 0;                      // themselves are kept and re-used: freeing ~60 of them per noisy-read submission synchronised the device each time)
    // the chains' work arenas live in d_poa_arena and, when a later submission needs more, in additional chunks: growing by a chunk costs the difference,
    // re-allocating tens of GB costs seconds (and the pools' slot sizes make the total jump by a third from one set of chunks to the next)
    std::vector<std::unique_ptr<DevBuf>> arena_extra;
    uint64_t final_bytes = 0;
    lcd_batch_stats_t st;
};

// what lcd_chunk_open_from_bam leaves for lcd_chunk_resolve (lcd_chunk.cpp): the loader's per-read tables, the CIGAR words gathered in HBM, the aux jobs
struct ChunkPending {
    int64_t reg_beg = 0, reg_end = 0, tlen = 0;
    std::vector<int64_t> pos0, rl_true; std::vector<int> ncig, qlen, nindel; std::vector<uint64_t> coff, soff, qoff; std::vector<RefCmpOut> counts;
    std::vector<BamAuxJob> auxj; lcd_internal::DevBuf d_cig;
};
// a device-resident chunk (lcd_chunk.cpp)
struct lcd_chunk_s {
    int device = 0, n_reads = 0; lcd_digar_opt_t opt;
    DevBuf d_dig, d_seq;                                   // digars (DigarRec, per read at slot[r], n_digar[r] of them); the records' 4-bit packed bases
    lcd_inflated_t *stream = nullptr;                      // lcd_chunk_create_from_bam: the inflated BGZF blocks; bases and qualities are read where they lie in it
    uint64_t seq_base = 0, qual_base = 0;                  // device address seq_off / qual_off are relative to (qual_base 0: the qualities are in h_qual)
    std::vector<uint64_t> slot, seq_off; std::vector<int> n_digar, qlen;
    std::vector<uint8_t> h_qual; std::vector<uint64_t> qual_off;   // host copy: the sampling rule of >= 10 kb regions reads qualities on the host (src/seq.c:429)
    std::vector<int> status, n_cand; std::vector<int64_t> beg, end;
    std::vector<uint8_t> source, pal; uint64_t tag_bytes = 0;   // lcd_chunk_create_from_bam_src: LCD_SRC_* and is_ont_palindrome per read; cs / MD bytes brought to the host
    double stage_ms[4] = {0, 0, 0, 0};                          // ... and its wall-clock split: aux fields, reference comparison, tag download + host parse, digars
    bool from_bam = false; std::vector<uint64_t> aux_off, rec_end;   // lcd_chunk_create_from_bam*: per read its auxiliary fields [aux_off, rec_end) as offsets of the inflated stream (lcd_chunk_read_nm)
    // lcd_chunk_create_from_bam*: EVERY record the region's iterator yields, in file order (lcd_chunk_tag_records, lcd_write_phased): [rec_beg, rec_stop) of the
    // inflated stream from its block_size word on, the chunk read id of a kept record or -1 for one the loader's flag / MAPQ filter dropped, pos0 and bam_endpos
    std::vector<uint64_t> rec_beg, rec_stop; std::vector<int> rec_read; std::vector<int64_t> rec_pos0, rec_endpos;
    // lcd_chunk_open_from_bams: the number of input files (1 otherwise), and per record / per kept read the file it came from; both tables are file-major
    int n_files = 1; std::vector<int> rec_file, read_file;
    int64_t reg_beg = 0, reg_end = -1;                          // lcd_chunk_open_from_bam*: the region the chunk was made for (lcd_chunk_mod_pileup counts the sites inside it)
    uint64_t *iv_off = nullptr; lcd_noisy_iv_t *ivs = nullptr; uint8_t *iv_in_chunk = nullptr;
    DevBuf d_qual; std::mutex qual_mu;                     // lcd_chunk_clean_vars: a host-array chunk's qualities, uploaded on first use
    std::unique_ptr<ChunkPending> pending;                 // lcd_chunk_open_from_bam: set until lcd_chunk_resolve (a handle with it has no digars yet)
    DevBuf d_plan; bool plan_ready = false; std::mutex plan_mu;   // lcd_chunk_plan_pass: PlanRead per read (beg / end / status / digar slot), uploaded on first use
    lcd_refine_log_t *refine_log = nullptr;                // lcd_chunk_set_refine: the sink of the chunk's rounds; with it the writer refines the chunk's records
    ~lcd_chunk_s() { free(iv_off); free(ivs); free(iv_in_chunk); if (stream) lcd_inflated_free(stream); lcd_refine_log_free(refine_log); }
};

// the contigs' names in HBM (lcd_sam_names_create, lcd_bam_out.cpp): back to back in `pool`, name r = [offs[r], offs[r + 1]); read by the SAM text and the haplotag list
struct lcd_sam_names_s { DevBuf pool, offs; size_t pool_bytes = 0; int n_ref = 0, device = 0; };

namespace lcd_internal __attribute__((visibility("hidden"))) {
// the records with skip[i] == 0 (NULL: all) in the order `order` names them (NULL: table order)
inline int pick_selected(const std::string &W, const lcd_chunk_t *c, const uint8_t *skip, const int *order, std::vector<int> &pick) {
    const int n_rec = (int)c->rec_beg.size();
    int m = 0;
    for (int i = 0; i < n_rec; ++i) if (!skip || !skip[i]) ++m;
    pick.assign(m, 0); std::vector<uint8_t> seen(n_rec + 1, 0);
    for (int k = 0, i = 0; k < m; ++k) {
        if (order) i = order[k]; else { while (skip && skip[i]) ++i; }
        if (i < 0 || i >= n_rec || (skip && skip[i]) || seen[i]) return set_err(-4, W + ": `order` must name every record that is not skipped exactly once");
        seen[i] = 1; pick[k] = i;
        if (!order) ++i;
    }
    return 0;
}
} // namespace lcd_internal

// ---- noisy-region intervals with cgranges' index order and merge rule (lcd_noisy_regs.cpp).  These names have C linkage and default visibility: written inside
// an extern "C" block they have been dynamic symbols of the library from the start, and the export surface stays as it is ----
using lcd_internal::NIv;
extern "C" {
void niv_index(std::vector<NIv> &v);
void niv_add(std::vector<NIv> &v, long long st, long long en, int label);
void niv_merge(std::vector<NIv> &v, const int fixed_win = -1);
} // extern "C"
