// lcd_host.cpp -- the region-batch pipeline of liblcd_hotpath.so: host orchestration of a submission + its C ABI (compiled with hipcc, HIP runtime only).
// The runtime core, the per-call entry points, the interval code, the chunk and the collect_var_main port are in the files beside it (DESIGN "Source map").
//
// Host glue kept in C++ because the reference's glue is compiled C (src/align.c): read ordering
// (sort_noisy_region_reads :955), phase-set choice (:1225), homopolymer test (:1000), anchor windows
// (:667-707) and the final malloc()'d aln_str_t materialisation.  Everything with a DP in it runs on the
// GPU: K4 edlib_kernel.hip, K3 wfa_kernel.hip, K1/K2 poa_kernel.hip, MSA->strings strings_kernel.hip.
// There is no CPU fallback: if HIP reports no device every entry point fails with an error string.
//
// All *_off fields handed to kernels are absolute device addresses (kernels get nullptr bases), so every
// stage can live in its own grow-only hipMalloc buffer.
#include <sys/mman.h>
#include <array>
#include <cfloat>
#include <cmath>
#include <functional>
#include <numeric>
#include <map>
#include "lcd_host_internal.h"

using namespace lcd_internal;

namespace {

// ---------------- host glue (restating src/align.c; see cited lines) ----------------
int full_cover_cmp(int c1, int c2) { // src/align.c:945-952
    if (c1 == c2) return 0;
    if (LCD_IS_BOTH_COVER(c1)) return 1;
    else if (LCD_IS_BOTH_COVER(c2)) return -1;
    if (LCD_IS_LEFT_COVER(c1) && LCD_IS_LEFT_COVER(c2)) return 0;
    if (LCD_IS_RIGHT_COVER(c1) && LCD_IS_RIGHT_COVER(c2)) return 0;
    return c1 - c2;
}
double calc_read_error_rate(int len, const uint8_t *qual) { // src/seq.c:429-436
    if (len <= 0 || qual == nullptr) return 0.0;
    double e = 0.0;
    for (int i = 0; i < len; ++i) e += pow(10.0, -((double)qual[i]) / 10.0);
    return e / len;
}
bool is_homopolymer(const uint8_t *seq, int seq_len, int flank) { // src/align.c:1000-1026
    if (seq_len < 2 * flank || seq_len > 2 * flank + 50) return false;
    int hp_len = 0;
    for (int i = flank - 1; i < seq_len - flank + 1; ++i) {
        if (seq[i] == seq[i - 1]) hp_len++;
        else { if (hp_len >= 5) return true; hp_len = 0; }
    }
    return hp_len >= 5;
}

// The learned levels of the planner (lcd_plan.cpp), 0..2 each.  They belong to the code that learns them -- the POA rounds of a submission and the anchor WFA
// stage -- and reach the planner as a PlanHints value loaded by whoever calls it.
std::atomic<int> g_wfa_hint{0};                // learned from the overflow retries of earlier ANCHOR stages (read vs read windows of noisy reads)
std::atomic<int> g_cell_hint[2] = {{0}, {0}};  // per mode (K1, K2), see chain_caps
std::atomic<int> g_node_hint{0};               // graph capacity estimate, see chain_caps
PlanHints learned_hints() { PlanHints h; h.cell[0] = g_cell_hint[0].load(); h.cell[1] = g_cell_hint[1].load(); h.node = g_node_hint.load(); h.wfa = g_wfa_hint.load(); return h; }

// ---- generic stage runners (absolute device addresses in job structs) ----
// (defer_copy: the statuses stay on the device -- a copy into pageable host memory holds the calling thread until the kernel has ended; the caller fetches them later)
int run_edlib_stage(hipStream_t st, std::vector<EdJob> &jobs, DevBuf &d_jobs, DevBuf &d_arena, DevBuf &d_outs, std::vector<EdOut> &outs, bool defer_copy = false) {
    const int n = (int)jobs.size();
    outs.resize(n);
    if (n == 0) return 0;
    uint64_t tot = 0;
    // Longest pairs first: the kernel is one wavefront per pair and lasts as long as the pair that ends last -- in submission order a 4 kb x 4 kb pair near the end of
    // 17 000 was the stage's tail.  pad_ carries the pair's index in the caller's order: that is where its result goes.
    for (int i = 0; i < n; ++i) jobs[i].pad_ = i;
    std::stable_sort(jobs.begin(), jobs.end(), [](const EdJob &a, const EdJob &b) { return (long long)a.qlen * a.tlen > (long long)b.qlen * b.tlen; });
    for (auto &j : jobs) { j.ws_bytes = lcd_align_up(ed_arena_bytes(j.qlen, j.tlen), 256); j.ws_off = tot; tot += j.ws_bytes; }
    if (d_arena.ensure(tot)) return -11;
    for (auto &j : jobs) j.ws_off += d_arena.addr();
    if (d_jobs.ensure(n * sizeof(EdJob)) || d_outs.ensure(n * sizeof(EdOut))) return -11;
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(EdJob), hipMemcpyHostToDevice, st));
    lcd_launch_edlib((const EdJob *)d_jobs.p, nullptr, nullptr, (EdOut *)d_outs.p, n, st);
    HIPCHK(hipGetLastError());
    if (!defer_copy) HIPCHK(hipMemcpyAsync(outs.data(), d_outs.p, n * sizeof(EdOut), hipMemcpyDeviceToHost, st));
    return 0;
}

// WFA stage with the overflow retry ladder (score bound x4 + 64).  jobs[i].s_cap holds the wanted score bound on entry (wfa_default_scap);
// every round plans the pending jobs (class, block, snapshots), launches the LDS buckets and the HBM-ring class and waits for the statuses.
int run_wfa_stage(hipStream_t st, std::vector<WfaJob> &jobs, DevBuf &d_jobs, DevBuf &d_arena, DevBuf &d_out, DevBuf &d_outs,
                  std::vector<WfaOut> &outs, LcdScoring sc, const HostSwitches &sw, int *retries, bool learn = false, hipStream_t *side = nullptr, hipEvent_t *sev = nullptr, int n_side = 0) {
    // side / sev / n_side: the classes' launches are dealt to st and these streams (one kernel per class: six for a HiFi-shape stage, each as long as its longest job)
    const int n = (int)jobs.size();
    outs.assign(n, WfaOut());
    if (n == 0) return 0;
    if (sc.e1 < 1 || sc.e2 < 1) return set_err(-2, "WFA: gap extension penalties must be >= 1");
    uint64_t otot = 0;
    std::vector<uint64_t> ooff(n);
    for (int i = 0; i < n; ++i) { ooff[i] = otot; otot += lcd_align_up(wfa_out_bytes(jobs[i]), 256); }
    if (d_out.ensure(otot)) return -11;
    for (int i = 0; i < n; ++i) jobs[i].out_off = d_out.addr() + ooff[i];
    std::vector<long long> want(n);
    for (int i = 0; i < n; ++i) want[i] = jobs[i].s_cap;
    std::vector<int> first_want;
    if (learn) { first_want.resize(n); for (int i = 0; i < n; ++i) first_want[i] = jobs[i].s_cap; }
    std::vector<int> which(n);
    for (int i = 0; i < n; ++i) which[i] = i;
    std::vector<WfaJob> sub; std::vector<WfaOut> tmp;
    for (int round = 0; round < 10 && !which.empty(); ++round) {
        const size_t m = which.size();
        const double tw0 = now_ms();
        // (plans and classes of the jobs are independent: a few host threads -- 50 000 ref<->cons jobs of a 20-batch submission were 3.5 ms of one thread with the GPU idle)
        std::vector<int> cls(n, 0);
        par_chunks(m, host_team(sw), 4096, [&](const size_t lo, const size_t hi, int) { for (size_t q = lo; q < hi; ++q) { const int i = which[q]; wfa_plan(jobs[i], sc, want[i], sw); cls[i] = wfa_class(jobs[i], sc, sw); } });
        const double tw1 = now_ms();
        // equal classes contiguous (one launch each); inside a class the larger arenas first (they last longest): a stable counting sort on class | size class (the
        // arena size's exponent and four mantissa bits, descending) -- the order inside a launch is about its tail, nothing else depends on it
        {
            auto key_of = [&](const int i) { const uint64_t w = std::max<uint64_t>(jobs[i].ws_bytes, 16); const int e = 63 - __builtin_clzll(w); return (unsigned)cls[i] * 1024u + (1023u - (unsigned)(e * 16 + (int)((w >> (e - 4)) & 15))); };
            std::vector<uint32_t> cnt((sw.wfa_buckets_kb.size() + 1) * 1024 + 1, 0);
            std::vector<unsigned> kq(m);
            for (size_t q = 0; q < m; ++q) { kq[q] = key_of(which[q]); cnt[kq[q] + 1]++; }
            for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
            std::vector<int> w2(m);
            for (size_t q = 0; q < m; ++q) w2[cnt[kq[q]]++] = which[q];
            which.swap(w2);
        }
        uint64_t tot = 0;
        for (int i : which) { jobs[i].ws_off = tot; tot += jobs[i].ws_bytes; }
        if (sw.mem_debug) {
            size_t nl = 0, nck = 0; uint64_t big = 0; for (int i : which) { nl += jobs[i].lds; nck += jobs[i].n_ckpt > 0; big = std::max(big, jobs[i].ws_bytes); }
            fprintf(stderr, "[mem] WFA stage round %d: %zu jobs (%zu in LDS, %zu checkpointed), arena %.3f GB, largest job %.1f MB (hint %d)\n", round, m, nl, nck, tot / 1e9, big / 1e6, g_wfa_hint.load());
        }
        if (d_arena.ensure(tot) || d_jobs.ensure(m * sizeof(WfaJob)) || d_outs.ensure(m * sizeof(WfaOut))) return -11;
        sub.resize(m); tmp.resize(m);
        for (size_t q = 0; q < m; ++q) { jobs[which[q]].ws_off += d_arena.addr(); sub[q] = jobs[which[q]]; }
        HIPCHK(hipMemcpyAsync(d_jobs.p, sub.data(), m * sizeof(WfaJob), hipMemcpyHostToDevice, st));
        if (sw.time_host) fprintf(stderr, "[host]   WFA stage round %d: %zu jobs planned (%.1f ms), ordered and laid out in %.1f ms\n", round, m, tw1 - tw0, now_ms() - tw0);
        const int ns = (side && sev && n_side > 0) ? n_side + 1 : 1;
        if (ns > 1) HIPCHK(hipEventRecord(sev[0], st)); // the job table is there
        std::vector<char> used(ns, 0);
        int turn = 0;
        // (the HBM-ring class's jobs with workspaces of a megabyte and more -- fronts of thousands of diagonals: SV-size gaps -- are a launch of their own, on the
        //  instantiation that keeps several diagonals per thread in flight; the class is sorted by workspace size, largest first, so they are its head)
        const uint64_t wide_from = (uint64_t)sw.wfa_wide_kb << 10; // LCD_WFA_WIDE_KB
        // (only when there are enough of them to be a workload of their own -- 64, LCD_WFA_WIDE_MIN: a handful of such jobs in a clean-read submission as one more launch
        //  took a stream's turn from the LDS classes, which then queued behind the longest jobs: 156 k against 172 k regions/s at the default flags, two lanes of 32 batches)
        const size_t wide_min = (size_t)sw.wfa_wide_min;
        size_t n_wide = 0;
        if (wide_from > 0) for (size_t q = 0; q < m; ++q) n_wide += cls[which[q]] == 0 && jobs[which[q]].ws_bytes >= wide_from;
        const bool wide_on = wide_from > 0 && n_wide >= wide_min;
        auto is_wide = [&](const size_t q) { return wide_on && cls[which[q]] == 0 && jobs[which[q]].ws_bytes >= wide_from; };
        for (size_t a = 0; a < m;) {
            size_t b = a; const int c = cls[which[a]]; const bool wide = is_wide(a);
            while (b < m && cls[which[b]] == c && is_wide(b) == wide) ++b;
            const int t = turn++ % ns;
            hipStream_t s2 = t == 0 ? st : side[t - 1];
            if (t != 0 && !used[t]) { HIPCHK(hipStreamWaitEvent(s2, sev[0], 0)); used[t] = 1; }
            lcd_launch_wfa((const WfaJob *)d_jobs.p + a, nullptr, nullptr, nullptr, (WfaOut *)d_outs.p + a, sc, (int)(b - a), c ? sw.wfa_buckets_kb[c - 1] << 10 : 0, s2, wide ? 1 : 0);
            HIPCHK(hipGetLastError());
            a = b;
        }
        for (int t = 1; t < ns; ++t) if (used[t]) { HIPCHK(hipEventRecord(sev[t], side[t - 1])); HIPCHK(hipStreamWaitEvent(st, sev[t], 0)); }
        HIPCHK(hipMemcpyAsync(tmp.data(), d_outs.p, m * sizeof(WfaOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st)); // (`sub` and `tmp` outlive the copies: they are only touched again after this)
        std::vector<int> again;
        for (size_t q = 0; q < m; ++q) {
            const int i = which[q];
            const unsigned long long prev = outs[i].offsets;
            outs[i] = tmp[q]; outs[i].offsets += prev;
            if (tmp[q].status == LCD_ERR_WF) { want[i] = std::min<long long>((long long)jobs[i].s_cap * 4 + 64, 4000000); again.push_back(i); }
            else if (tmp[q].status != LCD_OK) return set_err(-20, "WFA kernel status " + std::to_string(tmp[q].status));
        }
        if (learn && round == 0 && again.size() * 20 > m && g_wfa_hint.load() < 2) g_wfa_hint++;
        if (!again.empty() && retries) (*retries)++;
        which.swap(again);
    }
    if (!which.empty()) return set_err(-21, "WFA score bound exhausted after retries");
    if (learn && sw.mem_debug) { // anchor stage: how the optimal scores compare with the first score bound
        double r_sum = 0; int cnt = 0, over = 0; double worst = 0;
        for (int i = 0; i < n; ++i) { const int mm = std::min(jobs[i].plen, jobs[i].tlen); if (mm < 50) continue; const double r = (double)outs[i].score / mm; r_sum += r; ++cnt; worst = std::max(worst, r); over += outs[i].score > first_want[i]; }
        fprintf(stderr, "[mem] anchor WFA: %d jobs >= 50 bp, score / min(len) mean %.3f max %.3f; %d above their first bound\n", cnt, cnt ? r_sum / cnt : 0.0, worst, over);
    }
    return 0;
}

} // namespace

// =====================================================================================================
extern "C" {

void lcd_opt_default(lcd_opt_t *o) {
    o->match = 2; o->mismatch = 6; o->gap_open1 = 6; o->gap_ext1 = 2; o->gap_open2 = 24; o->gap_ext2 = 1;
    o->gap_aln = 1; o->min_af = 0.20; o->min_dp = 5; o->partial_aln_ratio = 1.1;
    o->min_noisy_reg_size_to_sample_reads = 10000; o->max_noisy_reg_len = 50000; o->noisy_reg_flank_len = 10;
    o->min_hap_full_reads = 1; o->min_hap_reads = 2; o->collect_ref_read_aln_str = 0; o->is_ont = 0; o->collect_noisy_vars = 0; o->min_sv_len = 30; // LONGCALLD_MIN_SV_LEN, src/call_var_main.h:54
}

// ---------------------------------------------------------------------------------------------------
lcd_batch_t *lcd_batch_create(const lcd_opt_t *opt) { return lcd_batch_create_on(opt, -1); }
// streams and events of a batch live on its device: created when the batch is bound to one
static int bind_batch(lcd_batch_t *b, int device) {
    if (use_device(device)) return -1;
    b->device = cur_device();
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { b->stream = nullptr; b->device = -1; return set_err(-10, "hipStreamCreate failed"); }
    for (auto &e : b->ev) hipEventCreate(&e);
    for (auto &e : b->sev) hipEventCreateWithFlags(&e, hipEventDisableTiming);
    for (auto &s : b->side) hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    return 0;
}
lcd_batch_t *lcd_batch_create_on(const lcd_opt_t *opt, int device) {
    if (init_default_device()) return nullptr;
    lcd_batch_t *b = new lcd_batch_s();
    b->opt = *opt; b->device = -1;
    memset(&b->st, 0, sizeof(b->st));
    // LCD_DEVICE_ANY: a host-only job buffer; the device is chosen when it is uploaded (lcd_batch_upload: the calling thread's; lcd_dispatch_run: the
    // device whose queue takes it)
    if (device != LCD_DEVICE_ANY && bind_batch(b, device)) { delete b; return nullptr; }
    return b;
}
void lcd_batch_destroy(lcd_batch_t *b) {
    if (!b) return;
    if (b->device >= 0) {
        hipSetDevice(b->device);
        for (auto &e : b->ev) hipEventDestroy(e);
        for (auto &e : b->sev) hipEventDestroy(e);
        for (auto &s : b->side) if (s) hipStreamDestroy(s);
        if (b->stream) hipStreamDestroy(b->stream);
    }
    delete b;
}
void lcd_batch_clear(lcd_batch_t *b) {
    b->h_pool.clear(); b->h_packed.clear(); b->unpack_jobs.clear(); b->unpack_abs.clear(); b->pool_read_bytes = 0; b->regs.clear(); b->chains.clear(); b->preads.clear(); b->anchors.clear(); b->ed_jobs.clear(); b->wfa_jobs.clear();
    b->uploaded = b->ran = b->downloaded = false;
    memset(&b->st, 0, sizeof(b->st));
}

static uint64_t pool_push(std::vector<uint8_t> &pool, const uint8_t *p, int n) {
    uint64_t off = pool.size();
    if (p) pool.insert(pool.end(), p, p + n);
    else pool.resize(pool.size() + n, (uint8_t)4); // a hole: filled on the device (lcd_batch_add_region_from_chunk_packed)
    size_t pad = (16 - (pool.size() & 15)) & 15;
    pool.insert(pool.end(), pad, (uint8_t)4);
    return off;
}

static int add_region_impl(lcd_batch_t *b, int64_t reg_len, int n_reads, const int *read_ids, const int *lens, const uint8_t *const *seqs,
                           const uint8_t *const *quals, const int *fully_covers, const int *haps, const int64_t *phase_sets,
                           const uint8_t *ref_seq, int ref_seq_len, const double *errs);
int lcd_batch_add_region(lcd_batch_t *b, int64_t reg_len, int n_reads, const int *read_ids, const int *lens, const uint8_t *const *seqs,
                         const uint8_t *const *quals, const int *fully_covers, const int *haps, const int64_t *phase_sets,
                         const uint8_t *ref_seq, int ref_seq_len) {
    return add_region_impl(b, reg_len, n_reads, read_ids, lens, seqs, quals, fully_covers, haps, phase_sets, ref_seq, ref_seq_len, nullptr);
}
// errs: the reads' error rates where the qualities live on the device (lcd_chunk_create_from_bam), else computed here from `quals`
static int add_region_impl(lcd_batch_t *b, int64_t reg_len, int n_reads, const int *read_ids, const int *lens, const uint8_t *const *seqs,
                           const uint8_t *const *quals, const int *fully_covers, const int *haps, const int64_t *phase_sets,
                           const uint8_t *ref_seq, int ref_seq_len, const double *errs) {
    const lcd_opt_t &opt = b->opt;
    b->uploaded = b->ran = b->downloaded = false;
    RegionRec R;
    R.reg_len = reg_len; R.n_reads = n_reads; R.branch = 0; R.chain[0] = R.chain[1] = -1;
    R.sampling = reg_len >= opt.min_noisy_reg_size_to_sample_reads;
    R.ref_off = pool_push(b->h_pool, ref_seq, ref_seq_len); R.ref_len = ref_seq_len;
    R.reads.resize(n_reads > 0 ? n_reads : 0);
    for (int i = 0; i < n_reads; ++i) {
        RegRead &r = R.reads[i];
        r.id = read_ids[i]; r.len = lens[i]; r.cover = fully_covers[i]; r.hap = haps[i]; r.ps = phase_sets[i];
        r.off = lens[i] > 0 ? pool_push(b->h_pool, seqs[i], lens[i]) : b->h_pool.size();
        if (lens[i] > 0 && seqs[i]) b->pool_read_bytes += (uint64_t)lens[i]; // (read bases that cross PCIe inside the pool: lcd_copy_counters)
        r.err = !R.sampling ? 0.0 : errs ? errs[i] : calc_read_error_rate(lens[i], quals ? quals[i] : nullptr);
    }
    if (n_reads <= 0) { b->regs.push_back(R); return (int)b->regs.size() - 1; }
    // sort_noisy_region_reads, src/align.c:963-985 (exchange sort, exact swap sequence)
    const bool use_err = R.sampling;
    for (int i = 0; i < n_reads - 1; ++i)
        for (int j = i + 1; j < n_reads; ++j) {
            int cc = full_cover_cmp(R.reads[i].cover, R.reads[j].cover);
            if (cc < 0 || (cc == 0 && use_err && R.reads[i].err > R.reads[j].err) ||
                (cc == 0 && ((use_err && R.reads[i].err == R.reads[j].err) || !use_err) && R.reads[i].len < R.reads[j].len))
                std::swap(R.reads[i], R.reads[j]);
        }
    // collect_phase_set_with_both_haps, src/align.c:1225-1279
    int64_t ps_sel = -1;
    {
        std::vector<int64_t> uniq; std::vector<std::array<int, 2>> full, all, minlen;
        for (int i = 0; i < n_reads; ++i) {
            const RegRead &r = R.reads[i];
            if (r.hap == 0) continue;
            size_t k = 0;
            for (; k < uniq.size(); ++k) if (uniq[k] == r.ps) break;
            if (k == uniq.size()) { uniq.push_back(r.ps); full.push_back({0, 0}); all.push_back({0, 0}); minlen.push_back({INT32_MAX, INT32_MAX}); }
            const int h = r.hap - 1;
            if (LCD_IS_BOTH_COVER(r.cover)) { full[k][h]++; all[k][h]++; if (minlen[k][h] > r.len) minlen[k][h] = r.len; }
            else if (LCD_IS_LEFT_COVER(r.cover) || LCD_IS_RIGHT_COVER(r.cover)) { if (r.len >= minlen[k][h]) all[k][h]++; }
        }
        int max_i = -1, m1 = -1, m2 = -1;
        for (size_t i = 0; i < uniq.size(); ++i) {
            int c1 = std::min(full[i][0], full[i][1]), c2 = std::max(full[i][0], full[i][1]);
            if (c1 > m1) { m1 = c1; m2 = c2; ps_sel = uniq[i]; max_i = (int)i; }
            else if (c1 == m1 && c2 > m2) { m2 = c2; ps_sel = uniq[i]; max_i = (int)i; }
        }
        if (m1 < opt.min_hap_full_reads) ps_sel = -1;
        if (ps_sel != -1 && max_i != -1)
            if (all[max_i][0] < opt.min_hap_reads || all[max_i][1] < opt.min_hap_reads) ps_sel = -1;
    }
    int n_full = 0;
    for (auto &r : R.reads) if (LCD_IS_BOTH_COVER(r.cover)) n_full++;
    const int region_idx = (int)b->regs.size();
    auto add_chain = [&](int mode, int clu, const std::vector<int> &members) {
        ChainRec C; C.region = region_idx; C.clu = clu; C.mode = mode; C.members = members; C.read0 = (int)b->preads.size();
        const RegRead &r0 = R.reads[members[0]];
        for (size_t k = 0; k < members.size(); ++k) {
            const RegRead &r = R.reads[members[k]];
            PoaRead pr; pr.seq_off = r.off; pr.len = r.len; pr.skip = 0; pr.ref_beg = 1; pr.ref_end = r0.len; pr.read_beg = 1; pr.read_end = r.len;
            const int pidx = (int)b->preads.size();
            b->preads.push_back(pr);
            if (mode != 0 || k == 0) continue;
            // collect_partial_aln_beg_end, src/align.c:709-745 (target = read 0, always both-cover)
            const int qfc = r.cover;
            if (LCD_IS_BOTH_COVER(qfc) || (LCD_IS_LEFT_COVER(qfc) && LCD_IS_RIGHT_GAP(qfc)) || (LCD_IS_RIGHT_COVER(qfc) && LCD_IS_LEFT_GAP(qfc))) {
                if (R.sampling) {
                    AnchorRec A; A.pread = pidx; A.ext = 0; A.tlen_full = r0.len; A.qlen_full = r.len; A.wfa_job = -1; A.min_len = std::min(r0.len, r.len);
                    EdJob ej; ej.t_off = r0.off; ej.tlen = r0.len; ej.q_off = r.off; ej.qlen = r.len; ej.ws_off = 0; ej.ws_bytes = 0; ej.mode = 0; ej.pad_ = 0;
                    A.ed_job = (int)b->ed_jobs.size(); b->ed_jobs.push_back(ej); b->anchors.push_back(A);
                }
            } else if (LCD_IS_LEFT_COVER(qfc) || LCD_IS_RIGHT_COVER(qfc)) {
                // cal_wfa_partial_aln_beg_end, src/align.c:667-707
                const int ext = LCD_IS_LEFT_COVER(qfc) ? 1 : 2;
                const int _tlen = r0.len, _qlen = r.len; const double ratio = opt.partial_aln_ratio;
                int tlen = _tlen, qlen = _qlen; uint64_t toff = r0.off, qoff = r.off;
                if (ext == 1) {
                    if (_tlen > _qlen * ratio) tlen = (int)(_qlen * ratio);
                    else if (_qlen > _tlen * ratio) qlen = (int)(_tlen * ratio);
                } else {
                    if (_tlen > _qlen * ratio) { toff = r0.off + _tlen - (int)(_qlen * ratio); tlen = (int)(_qlen * ratio); }
                    else if (_qlen > _tlen * ratio) { qoff = r.off + _qlen - (int)(_tlen * ratio); qlen = (int)(_tlen * ratio); }
                }
                int gap_aln = opt.gap_aln;
                if (ext == 1) gap_aln = (gap_aln == 2) ? 1 : 2;
                const int min_len = std::min(tlen, qlen);
                AnchorRec A; A.pread = pidx; A.ext = ext; A.tlen_full = _tlen; A.qlen_full = _qlen; A.min_len = min_len;
                EdJob ej; ej.qlen = min_len; ej.tlen = min_len; ej.ws_off = 0; ej.ws_bytes = 0; ej.mode = 0; ej.pad_ = 0;
                if (ext == 1) { ej.t_off = toff; ej.q_off = qoff; } else { ej.t_off = toff + tlen - min_len; ej.q_off = qoff + qlen - min_len; }
                A.ed_job = (int)b->ed_jobs.size(); b->ed_jobs.push_back(ej);
                WfaJob wj; wj.p_off = toff; wj.plen = tlen; wj.t_off = qoff; wj.tlen = qlen; wj.gap_aln = gap_aln; wj.want = 1;
                wj.s_cap = wfa_default_scap(tlen, qlen, g_wfa_hint.load()); wj.ws_off = 0; wj.ws_bytes = 0; wj.out_off = 0;
                A.wfa_job = (int)b->wfa_jobs.size(); b->wfa_jobs.push_back(wj);
                b->anchors.push_back(A);
            }
        }
        b->chains.push_back(C);
        return (int)b->chains.size() - 1;
    };
    if (ps_sel > 0) { // src/align.c:1789 with wfa_collect_noisy_aln_str_with_ps_hap :1286-1375
        const bool use_non_full = !is_homopolymer(ref_seq, ref_seq_len, opt.noisy_reg_flank_len);
        int stale_len0 = 0, n_ch = 0; bool broke = false;
        std::vector<int> mem[2];
        for (int hap = 1; hap <= 2; ++hap) {
            std::vector<int> &m = mem[hap - 1];
            for (int i = 0; i < n_reads; ++i) {
                const RegRead &r = R.reads[i];
                if (r.len <= 0 || r.ps != ps_sel || r.hap != hap) continue;
                if (!use_non_full && !LCD_IS_BOTH_COVER(r.cover)) continue;
                m.push_back(i);
            }
            if (!m.empty()) stale_len0 = R.reads[m[0]].len;
            if (stale_len0 >= opt.max_noisy_reg_len) { broke = true; break; }
            if (m.empty()) continue;
            n_ch++;
        }
        if (!broke && n_ch == 2) {
            R.branch = 1;
            R.chain[0] = add_chain(0, 0, mem[0]);
            R.chain[1] = add_chain(0, 1, mem[1]);
        }
    } else if (n_full >= opt.min_dp) { // src/align.c:1794 with wfa_collect_noisy_aln_str_no_ps_hap :1148-1211
        std::vector<int> m;
        for (int i = 0; i < n_reads; ++i) { const RegRead &r = R.reads[i]; if (r.len > 0 && LCD_IS_BOTH_COVER(r.cover)) m.push_back(i); }
        if (!m.empty() && R.reads[m[0]].len < opt.max_noisy_reg_len) { R.branch = 2; R.chain[0] = add_chain(1, 0, m); }
    }
    b->regs.push_back(R);
    return region_idx;
}

static int add_region_from_chunk(lcd_batch_t *b, const lcd_read_view_t *cr, int64_t reg_beg, int64_t reg_end, int n, const int *noisy_reads,
                                 const uint8_t *ref_seq, int ref_seq_len, const bool packed) {
    // collect_noisy_read_info, src/align.c:1377-1461
    static const uint8_t nt16_int[16] = {4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4}; // htslib seq_nt16_int
    std::vector<int> ids(n), lens(n), covers(n), haps(n), rbs(n), res(n); std::vector<int64_t> pss(n);
    std::vector<std::vector<uint8_t>> seqs(n), quals(n);
    std::vector<const uint8_t *> sp(n), qp(n);
    for (int i = 0; i < n; ++i) {
        const lcd_read_view_t &rv = cr[noisy_reads[i]];
        const lcd_digar1_t *d = rv.digars; const int nd = rv.n_digar;
        int64_t rdb = -1, rde = -1;
        int rb = 0, re = rv.qlen - 1;
        if (d[0].type == 5) rb = d[0].len;
        if (d[nd - 1].type == 5) re = d[nd - 1].qi - 1;
        int beg_is_del = 0, end_is_del = 0, cover = 0;
        for (int k = 0; k < nd; ++k) {
            int64_t db = d[k].pos, de; const int op = d[k].type, len = d[k].len, qi = d[k].qi;
            if (op == 4 || op == 5) continue;
            if (op == 8 || op == 7 || op == 2) de = db + len - 1; else de = db;
            if (db > reg_end) break;
            if (de < reg_beg) continue;
            if (db <= reg_beg && de >= reg_beg) {
                if (op == 2) { rdb = reg_beg; rb = qi; if (len > b->opt.noisy_reg_flank_len) beg_is_del = 1; }
                else { rdb = reg_beg; rb = qi + (int)(reg_beg - db); }
            }
            if (db <= reg_end && de >= reg_end) {
                if (op == 2) { rde = reg_end; re = qi - 1; if (len > b->opt.noisy_reg_flank_len) end_is_del = 1; }
                else { rde = reg_end; re = qi + (int)(reg_end - db); }
            }
        }
        if (rdb == reg_beg && rde == reg_end) {
            if (!beg_is_del && !end_is_del) cover = LCD_LEFT_COVER | LCD_RIGHT_COVER;
            else if (!beg_is_del && end_is_del) cover = LCD_LEFT_COVER | LCD_RIGHT_GAP;
            else if (beg_is_del && !end_is_del) cover = LCD_LEFT_GAP | LCD_RIGHT_COVER;
            else cover = LCD_LEFT_GAP | LCD_RIGHT_GAP;
        } else if (rdb == reg_beg) cover = beg_is_del ? LCD_LEFT_GAP : LCD_LEFT_COVER;
        else if (rde == reg_end) cover = end_is_del ? LCD_RIGHT_GAP : LCD_RIGHT_COVER;
        const int L = re - rb + 1;
        rbs[i] = rb; res[i] = re;
        ids[i] = noisy_reads[i]; lens[i] = L; covers[i] = cover; haps[i] = rv.hap; pss[i] = rv.phase_set;
        if (L > 0 && !packed) {
            seqs[i].resize(L); quals[i].resize(L);
            for (int j = rb; j <= re; ++j) {
                seqs[i][j - rb] = nt16_int[(rv.bseq[j >> 1] >> ((~j & 1) << 2)) & 0xf]; // bam_seqi
                quals[i][j - rb] = rv.qual ? rv.qual[j] : 0;
            }
        }
        if (!packed) { sp[i] = seqs[i].data(); qp[i] = quals[i].data(); }
        else { sp[i] = nullptr; qp[i] = rv.qual && L > 0 ? rv.qual + rb : nullptr; } // (the qualities are only read on the host: the sampling rule of long regions)
    }
    const int ri = lcd_batch_add_region(b, reg_end - reg_beg + 1, n, ids.data(), lens.data(), sp.data(), qp.data(), covers.data(), haps.data(),
                                        pss.data(), ref_seq, ref_seq_len);
    if (ri >= 0) // remember each read's slice (the caller of update_digars_from_aln_str needs read_reg_beg / read_reg_end, src/align.c:1748)
        for (RegRead &r : b->regs[ri].reads)
            for (int i = 0; i < n; ++i) if (noisy_reads[i] == r.id) {
                r.rb = rbs[i]; r.re = res[i];
                if (packed && r.len > 0) { // the slice's bytes as they are in the record; its place in the pool is a hole until lcd_batch_upload has run lcd_unpack_kernel
                    const lcd_read_view_t &rv = cr[r.id];
                    UnpackJob j; j.src = b->h_packed.size(); j.dst = r.off; j.first = rbs[i] & 1; j.len = r.len;
                    b->h_packed.insert(b->h_packed.end(), rv.bseq + (rbs[i] >> 1), rv.bseq + (res[i] >> 1) + 1);
                    b->h_packed.push_back(0); // (the kernel's four-base steps read one byte past an odd start)
                    b->unpack_jobs.push_back(j);
                }
                break;
            }
    return ri;
}
int lcd_batch_add_region_from_chunk(lcd_batch_t *b, const lcd_read_view_t *cr, int64_t reg_beg, int64_t reg_end, int n, const int *noisy_reads,
                                    const uint8_t *ref_seq, int ref_seq_len) {
    return add_region_from_chunk(b, cr, reg_beg, reg_end, n, noisy_reads, ref_seq, ref_seq_len, false);
}
// the same region, with the reads' bases left 4-bit packed: the host copies each slice's bytes as they are in the BAM record (half a byte per base, no per-base
// loop) and lcd_batch_upload unpacks them on the device into the places add_region reserved.  Results are those of lcd_batch_add_region_from_chunk.
int lcd_batch_add_region_from_chunk_packed(lcd_batch_t *b, const lcd_read_view_t *cr, int64_t reg_beg, int64_t reg_end, int n, const int *noisy_reads,
                                           const uint8_t *ref_seq, int ref_seq_len) {
    return add_region_from_chunk(b, cr, reg_beg, reg_end, n, noisy_reads, ref_seq, ref_seq_len, true);
}
// per read of a region in its sorted order: chunk read id, cover flag, read_reg_beg / read_reg_end (-1 / -2 unless the region came from chunk views)
int lcd_batch_region_read_slices(lcd_batch_t *b, int region, int *read_ids, int *covers, int *read_beg, int *read_end) {
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    const RegionRec &R = b->regs[region];
    for (size_t i = 0; i < R.reads.size(); ++i) { read_ids[i] = R.reads[i].id; covers[i] = R.reads[i].cover; read_beg[i] = R.reads[i].rb; read_end[i] = R.reads[i].re; }
    return (int)R.reads.size();
}

int lcd_batch_upload(lcd_batch_t *b) {
    if (b->device < 0 && bind_batch(b, -1)) return -1; // a job buffer created with LCD_DEVICE_ANY: the calling thread's device
    if (use_device(b->device)) return -1;
    const double t0 = now_ms();
    if (b->d_in.ensure(b->h_pool.size() + 64)) return -11;
    HIPCHK(hipMemcpyAsync(b->d_in.p, b->h_pool.data(), b->h_pool.size(), hipMemcpyHostToDevice, b->stream));
    g_copy_bytes[2] += b->pool_read_bytes + b->h_packed.size();
    if (!b->unpack_abs.empty()) { // slices of a device-resident chunk: the packed bases never left HBM
        if (b->d_unpack_abs.ensure(b->unpack_abs.size() * sizeof(UnpackJob))) return -11;
        HIPCHK(hipMemcpyAsync(b->d_unpack_abs.p, b->unpack_abs.data(), b->unpack_abs.size() * sizeof(UnpackJob), hipMemcpyHostToDevice, b->stream));
        lcd_launch_unpack((const UnpackJob *)b->d_unpack_abs.p, (int)b->unpack_abs.size(), nullptr, (uint8_t *)b->d_in.p, b->stream);
        HIPCHK(hipGetLastError());
    }
    if (!b->unpack_jobs.empty()) { // slices that came 4-bit packed: unpacked here, into their holes in the pool
        if (b->d_packed.ensure(b->h_packed.size() + 64) || b->d_unpack.ensure(b->unpack_jobs.size() * sizeof(UnpackJob))) return -11;
        HIPCHK(hipMemcpyAsync(b->d_packed.p, b->h_packed.data(), b->h_packed.size(), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->d_unpack.p, b->unpack_jobs.data(), b->unpack_jobs.size() * sizeof(UnpackJob), hipMemcpyHostToDevice, b->stream));
        lcd_launch_unpack((const UnpackJob *)b->d_unpack.p, (int)b->unpack_jobs.size(), (const uint8_t *)b->d_packed.p, (uint8_t *)b->d_in.p, b->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->uploaded = true; b->ran = false; b->downloaded = false;
    b->st.ms_upload = now_ms() - t0;
    return 0;
}

static int stage_gather(lcd_batch_t *b, hipStream_t st);
static int stage_gather_many(lcd_batch_t **bs, int nb, hipStream_t st);
// uploads `sub` (already ordered so that equal classes are contiguous) and launches one kernel per class
// (different classes go to side streams so a long wide chain does not hold back the narrow ones)
static int launch_poa_grouped(hipStream_t st, const PoaChain *sub_p, const size_t sub_n, DevBuf &d_chains, const PoaRead *d_reads, DevBuf &d_outs, LcdScoring sc, const HostSwitches &sw,
                              hipStream_t *side = nullptr, hipEvent_t *sev = nullptr, DevBuf *d_gate = nullptr, PoaSpare *spare = nullptr, int busy_idx = -1, double busy_load = 0, bool noisy = false) {
    struct View { const PoaChain *p; size_t n; size_t size() const { return n; } const PoaChain &operator[](size_t i) const { return p[i]; } const PoaChain *begin() const { return p; } const PoaChain *end() const { return p + n; } } sub{sub_p, sub_n};
    HIPCHK(hipMemcpyAsync(d_chains.p, sub_p, sub_n * sizeof(PoaChain), hipMemcpyHostToDevice, st));
    // The wide classes start first, widest first: a 1 024-thread chain needs ALL the vector registers of a CU and a 512-thread chain half of
    // them, so once narrower workgroups are spread over the chip they wait for a CU to drain completely -- and they are the longest
    // chains.  gate[0] / gate[1] count the 1 024- / 512-thread workgroups that have started; the 512-thread launch is held
    // (lcd_gate_kernel) until target0 of the former are resident, the narrow launches until target1 of the latter are as well.
    const int n_streams = sw.streams; // LCD_STREAMS
    int n1024 = 0, n512 = 0; bool any_narrow = false;
    for (const PoaChain &pc : sub) { if (pc.threads >= 1024) ++n1024; else if (pc.threads >= 512) ++n512; else any_narrow = true; }
    const int cap = (int)(sw.gate_frac * g_n_cus); // leave a share of the CUs to the narrow classes from the start
    // the narrow launches are also held until all but `keep` of the 512-thread workgroups have started: chains of that class beyond one round
    // of residency (2 per CU) otherwise become the tail of the submission, two per CU on half-empty CUs (+3.5 % at 32 batches per submission)
    const int keep512 = sw.gate512_keep != kSwitchUnset ? sw.gate512_keep : 2 * g_n_cus; // one round of residency
    const int target0 = std::min(n1024, cap), target1 = std::min(n512, std::max(n512 - keep512, std::max(0, 2 * (cap - target0))));
    int *gate = nullptr;
    if (side && d_gate && n_streams > 1 && (n1024 + n512) > 0 && (any_narrow || (n1024 && n512))) {
        if (d_gate->ensure(256)) return -11;
        gate = (int *)d_gate->p;
        HIPCHK(hipMemsetAsync(gate, 0, 128, st));
    }
    if (side) HIPCHK(hipEventRecord(sev[0], st));
    // groups of equal (threads, LDS bucket) -> a small pool of streams (LCD_STREAMS, default 4 with the caller's): every stream is a
    // hardware queue, and with many queues holding runnable kernels the queue scheduler time-slices them -- measured on MI355X: the
    // same 48 wide chains take 1.09 s next to 8 other active queues and 0.42 s with 4 queues in total.  Groups are dealt to the
    // streams longest-first by their DP work (LPT); a stream runs its groups back to back.
    struct Grp { size_t i, j; double cost, tail; };
    std::vector<Grp> grps;
    for (size_t i = 0; i < sub.size();) {
        const long long key = chain_group_key(sub[i]);
        size_t j = i; double cost = 0;
        // a group's demand in CU-time: a chain runs ~ reads x rows (a row costs about the same few thousand cycles in every class), and
        // `per_cu` chains of this (threads, LDS) shape share a CU (160 KB LDS, 16 wavefronts at 128 VGPRs)
        double tail = 0;
        // (time per read-base by kind, measured with LCD_PROFILE_CHAINS on the SV shape: K1 chains of noisy reads 11 - 12 us -- general rows, a re-sort after every read --
        //  K2 chains of noisy reads 6 - 7 us in every wide class; clean reads 1.6 us.  Tried: weighting the noisy K1 chains 1.8x here -- the eight launch groups of an
        //  SV-shape submission are already packed onto the four queues within 5 % of each other (LCD_GROUP_DEBUG=1 prints the table), 1 676 regions/s either way;
        //  eight hardware queues (GPU_MAX_HW_QUEUES=8 LCD_STREAMS=8) make it worse, 1 398: the queues time-slice)
        // (noisy reads: a K1 chain's read-base costs 11 - 12 us -- general rows, a re-sort after every read -- against 6 - 7 us in the K2 classes (LCD_PROFILE_CHAINS, SV
        //  shape); unweighted, the two groups whose single longest K1 chain runs 4 s looked like the lightest streams and the last small groups queued behind them:
        //  342 + 170 ms at the end of a 6.2 s submission while another stream had been idle for 2.5 s -- tools/timeline.py)
        const double k1w = sw.noisy_k1_weight, k1w_from = sw.noisy_k1_from; // LCD_NOISY_K1_WEIGHT; LCD_NOISY_K1_FROM: read-bases (reads x longest read)
        while (j < sub.size() && chain_group_key(sub[j]) == key) { const double t = (double)sub[j].n_reads * (sub[j].max_len + 64); cost += t; tail = std::max(tail, t * (noisy && sub[j].mode == 0 && t >= k1w_from ? k1w : 1.0)); ++j; } // (the weight on a group's LONGEST chain only, and only on chains of SV-shape size: weighting the ONT shape's K1 groups -- many short chains -- as well moved that shape from 18.5 to 16.9 - 17.5 k regions/s)
        cost /= chains_per_cu(sub[i].lds_words * 4, sub[i].threads, kSchedOverhead);
        grps.push_back({i, j, cost, tail});
        i = j;
    }
    const int ns = side ? n_streams : 1;
    std::vector<size_t> order(grps.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    // launch order: 1 024-thread groups, then 512-thread groups, then the rest (a gate only ever waits for kernels enqueued before it, so it
    // cannot deadlock whatever the stream -> hardware-queue mapping is); longest first inside a class
    auto rank = [&](size_t k) { const int t = chain_threads(sub[grps[k].i]); return t >= 1024 ? 0 : t >= 512 ? 1 : 2; };
    // inside a class rank: the group with the longest single chain first (its duration is that chain whatever else runs); the groups of
    // many short chains come last and fill the machine while the long ones finish
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t c) { return rank(a) != rank(c) ? rank(a) < rank(c) : grps[a].tail > grps[c].tail; });
    std::vector<double> load(ns, 0.0);
    if (busy_idx >= 0 && busy_idx < ns) load[busy_idx] = busy_load; // (a stream that already runs the long chains launched before the anchor stage: run_many_once)
    std::vector<bool> used(ns, false);
    for (size_t k : order) {
        int best = 0;
        for (int t = 1; t < ns; ++t) if (load[t] < load[best]) best = t;
        // a stream runs its kernels one after the other, and a kernel lasts at least as long as its longest chain whatever else shares the chip: what adds up on a
        // stream is tail + share of the chip's work, not the work alone (two groups of a few long chains each on one stream were the whole tail of an
        // SV-shape submission: 7.8 s before the last group could start, with 0.9 s of work for 256 CUs)
        if (sw.group_debug) fprintf(stderr, "[groups] thr %4d lds %3dK: %6zu chains, tail %.3g, cost / CUs %.3g -> stream %d (load %.3g before)\n", chain_threads(sub[grps[k].i]), sub[grps[k].i].lds_words * 4 >> 10,
                                               grps[k].j - grps[k].i, grps[k].tail, grps[k].cost / std::max(1, g_n_cus), best, load[best]);
        load[best] += grps[k].tail + grps[k].cost / std::max(1, g_n_cus);
        // stream 0 is the caller's; the others are side streams that first wait for the chain table to be uploaded
        hipStream_t s = best == 0 ? st : side[best - 1];
        if (best != 0 && !used[best]) HIPCHK(hipStreamWaitEvent(s, sev[0], 0));
        used[best] = true;
        const int cls = chain_threads(sub[grps[k].i]);
        if (gate && cls < 1024 && (target0 > 0 || (cls < 512 && target1 > 0))) lcd_launch_gate(gate, target0, cls < 512 ? target1 : 0, s);
        lcd_launch_poa((const PoaChain *)d_chains.p + grps[k].i, d_reads, nullptr, nullptr, nullptr, (PoaChainOut *)d_outs.p + grps[k].i, sc, (int)(grps[k].j - grps[k].i), cls,
                       sub[grps[k].i].lds_words * 4, s, !gate ? nullptr : cls >= 1024 ? gate : cls >= 512 ? gate + 1 : nullptr, spare);
        HIPCHK(hipGetLastError());
    }
    for (int t = 1; t < ns; ++t) if (used[t]) { HIPCHK(hipEventRecord(sev[t], side[t - 1])); HIPCHK(hipStreamWaitEvent(st, sev[t], 0)); }
    if (gate && sw.gate_debug) { int h[8]; hipStreamSynchronize(st); hipMemcpy(h, gate, 32, hipMemcpyDeviceToHost); fprintf(stderr, "[gate] started: %d x 1024-thread, %d x 512-thread workgroups; longest gate wait %d polls (targets %d, %d)\n", h[0], h[1], h[4], target0, target1); }
    return 0;
}
static int launch_poa_grouped(hipStream_t st, const std::vector<PoaChain> &sub, DevBuf &d_chains, const PoaRead *d_reads, DevBuf &d_outs, LcdScoring sc, const HostSwitches &sw,
                              hipStream_t *side = nullptr, hipEvent_t *sev = nullptr, DevBuf *d_gate = nullptr, PoaSpare *spare = nullptr, int busy_idx = -1, double busy_load = 0, bool noisy = false) {
    return launch_poa_grouped(st, sub.data(), sub.size(), d_chains, d_reads, d_outs, sc, sw, side, sev, d_gate, spare, busy_idx, busy_load, noisy);
}

// ================= one submission: the hot path of n batches run JOINTLY =================
// Every stage is one set of launches over the jobs / chains of all batches, so the GPU's
// own workgroup dispatcher packs the chains of several batches onto the CUs (a chain is a sequential object that can use at most
// one CU; one batch of configs[1] size cannot fill 256 CUs, and separate streams per batch serialise on shared hardware queues).
// The leader (batches[0]) lends its stream and its job / arena buffers; inputs, chain outputs and final strings stay per batch.
// Results of batch k must be downloaded before the same leader runs again (the ref<->cons rows live in the leader's WFA buffer).
//
// A submission is a Submission object (below): its members are the state that crosses stage boundaries, its member functions are the stages, and
// run_many_once is the list of the stages with the two helper threads started and joined in it.  Every stage says what it reads, what it writes and
// which host thread runs it: the CALLING thread, the PREPARATION thread, the STRINGS thread, or a TEAM (host threads of one parallel loop, joined before
// the stage that started them returns).

// compact CU index of the arena slots: one probe launch per device records which (XCC, SE, SH, CU) ids exist (poa_kernel.hip lcd_cu_probe_kernel)
static DevBuf *g_cu_rank[LCD_MAX_DEV]; static int g_cu_n[LCD_MAX_DEV]; static std::mutex g_cu_mu;
static int cu_rank_table(hipStream_t st, uint64_t *addr, int *n_cu, const bool mem_debug) {
    const int dev = cur_device();
    std::lock_guard<std::mutex> lk(g_cu_mu);
    if (!g_cu_rank[dev]) {
        std::unique_ptr<DevBuf> seen(new DevBuf()), rank(new DevBuf());
        if (seen->ensure(4096 * 4) || rank->ensure(4096 * 4)) return -11;
        HIPCHK(hipMemsetAsync(seen->p, 0, 4096 * 4, st));
        lcd_launch_cu_probe((int *)seen->p, st);
        HIPCHK(hipGetLastError());
        std::vector<int> h(4096);
        HIPCHK(hipMemcpyAsync(h.data(), seen->p, 4096 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int n = 0;
        for (int &x : h) x = x ? n++ : -1;
        HIPCHK(hipMemcpyAsync(rank->p, h.data(), 4096 * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        if (mem_debug) fprintf(stderr, "[mem] device %d: %d compute units seen by the probe (%d reported)\n", dev, n, g_n_cus);
        g_cu_n[dev] = std::max(n, 1); g_cu_rank[dev] = rank.release();
    }
    *addr = g_cu_rank[dev]->addr(); *n_cu = std::max(g_cu_n[dev], g_n_cus); // (a CU the probe missed hashes into the table: never fewer slots than CUs)
    return 0;
}
static int run_many_once(lcd_batch_t **bs, int nb);
int lcd_batch_run_many(lcd_batch_t **bs, int nb) {
    // a joint submission whose arenas do not fit the device (the estimates of noisy reads are 4x those of clean ones) is split in halves,
    // each led by its own first batch; results are the same either way
    const int rc = run_many_once(bs, nb);
    if (rc != -11 || nb <= 1) return rc;
    // the work arenas (DP cells, wavefronts, edlib columns) are transient: dropped around each half so that the halves do not add up;
    // the outputs of a half stay in its leader's buffers until they are downloaded
    auto drop = [](lcd_batch_t *b) { b->d_poa_arena.release(); b->arena_extra.clear(); b->d_var_work.release(); b->d_spare.release(); };
    const int h = nb / 2;
    drop(bs[0]);
    const int r1 = lcd_batch_run_many(bs, h);
    drop(bs[0]);
    if (r1) return r1;
    const int r2 = lcd_batch_run_many(bs + h, nb - h);
    drop(bs[h]);
    return r2;
}
// submissions in flight per device (host lanes: several threads inside lcd_batch_run_many at once)
static std::atomic<int> g_inflight[LCD_MAX_DEV];
struct InflightGuard { int dev; int n; InflightGuard(int d) : dev(d) { n = g_inflight[d].fetch_add(1) + 1; } ~InflightGuard() { g_inflight[dev].fetch_sub(1); } };

namespace { // everything of a submission but its driver is local to this file


// the arena layout of a round (pure host work: slot pools and private arenas per launch group); round 0's is made on the preparation thread
struct ArenaItem { uint64_t start, bytes, phys; };
struct ArenaPlan { uint64_t tot = 0, flag_ints = 0; size_t n_pooled = 0, n_pools = 0; uint64_t private_bytes = 0, pool_bytes = 0; std::vector<ArenaItem> items; std::vector<uint32_t> item_of; std::vector<uint64_t> need; bool valid = false; };
// one POA round: what its steps hand each other (calling thread; the blocks the round's asynchronous copies read and write live here until the round ends)
struct PoaRound {
    int round = 0; ArenaPlan P;
    PoaChain *sub = nullptr; size_t sub_n = 0;     // the round's chain table (leader's pinned block), in the order of `which`
    PoaSpare *d_spare = nullptr; PoaSpare spare_hdr, spare_seen;
    PoaChainOut *tmp = nullptr;                    // the chains' output records (leader's pinned block), in the order of `which`
    std::vector<size_t> again; size_t n_node_ovf = 0, n_cert_fail = 0;
};
struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } };
struct Submission;
// diagnostics of a submission (behind the stages, below): they read the submission and print
static void report_round_memory(const Submission &S, const PoaRound &R);
static void report_round_retries(const Submission &S, const PoaRound &R);
static void dump_failed_chain(const Submission &S, size_t g, int status);
static std::string failed_chain_text(const Submission &S, size_t g, const PoaChainOut &o);
static void report_placement(const Submission &S);
static void report_chain_times(const Submission &S);
static void report_profile_chains(const Submission &S);

struct Submission {
    // ---- set by the constructor, constant afterwards: read by every stage on every thread ----
    lcd_batch_t **const bs; const int nb;
    lcd_batch_t *const L;                 // the leader: lends its stream, events, job tables and arenas
    const hipStream_t st; const HostSwitches env; const LcdScoring sc; const double t_begin; // env: the switches, read once at the start of the submission (lcd_switches.h)
    InflightGuard inflight;               // (alive for the whole submission)
    // The long K2 chains ahead of the anchor stage (launch_early) take a stream -- one of the runtime's four hardware queues -- for the length of the submission.  That pays
    // when this submission has the device to itself; with other submissions in flight (host lanes) the queues are what is scarce and the lanes overlap each other's
    // stages anyway: measured with two lanes of 32 batches 82.8 k instead of 100 k regions/s.  LCD_EARLY=0: never.
    const bool early_k2;
    // chain g of the submission is chain g - chain_base[k] of batch k = chain_batch[g]; the device read table is the concatenation of the batches' tables
    std::vector<size_t> chain_base, pread_base; std::vector<int> chain_batch; size_t nC_all = 0;
    // (streams share the runtime's four hardware queues in creation order: the leader's stream and its first three side streams have one each -- a later side
    //  stream would share the leader's queue and hold the anchor stage and the first launch group behind the long chains: measured, 272 instead of 220 ms of POA)
    const hipStream_t es;                 // the long chains' stream
    uint64_t cu_rank_addr = 0; int n_cu;  // the arena slots' CU table (begin)
    // ---- written by prep_chains (preparation thread) and its teams ----
    // the reads of every chain with their device addresses (the anchor stage narrows the partial reads of K1 chains; lengths never change)
    // (filled per batch by the host threads of size_chains: 24 MB for a 20-batch submission, 3 ms when one thread copied them)
    std::vector<std::vector<PoaRead>> preads;
    std::vector<std::vector<uint64_t>> out_rel; std::vector<uint64_t> out_tots; // the chains' first output blocks: offsets into their batch's d_poa_out
    std::vector<size_t> early;            // the long K2 chains that run on `es` since before the anchor stage
    double early_load = 0; bool reads_up = false; // (reads_up: the read table is in d_preads already, as of before the anchor stage)
    std::vector<size_t> which;            // the chains of the round at hand, in launch order (prepare_round0; then the POA rounds)
    ArenaPlan plan0;                      // round 0's arena layout (prepare_round0)
    // ---- THE HAND-OVER.  Written on the preparation thread, read by the calling thread only after join_prep() has returned: early, reads_up, early_load,
    // preads, which, plan0 and pchains[*] of every batch (with them out_rel, out_tots, couts and the chains' solo / cert fields).  Until then the calling
    // thread touches none of them: begin and anchor_stage run beside the preparation thread ----
    bool order_async = false; int prep_rc = 0;
    std::string prep_err;                 // (g_err is per thread: a helper's message is carried over to the calling thread at the join)
    // ---- the POA rounds (calling thread) ----
    double tp0 = 0, th0 = 0;              // host clock at the start of the POA stage / of the stages behind it
    int scale = 1;
    std::map<size_t, uint64_t> retry_out_off; // chains whose output block moved to a retry buffer
    // ---- S3 / S4: the joint job tables live in the leader (kept between submissions: no reallocation, no first-touch page faults in the steady state) ----
    std::vector<WfaJob> &rc_all; std::vector<StrJob> &str_all; std::vector<StrOut> &str_outs;
    std::vector<size_t> rc_base, str_base; std::vector<uint64_t> str_tots;
    bool strings_beside = false; int strings_rc = 0; std::string strings_err;
    float ms_vars = 0;
    // ---- the helper threads.  Declared LAST: members are destroyed in reverse order, so on every way out of run_many_once the two threads are joined before
    // anything they touch dies ----
    Joiner prep_thread, strings_thread;

    Submission(lcd_batch_t **bs_, int nb_)
        : bs(bs_), nb(nb_), L(bs_[0]), st(L->stream), env(HostSwitches::from_env()), sc(scoring_of(L->opt, env)), t_begin(now_ms()), inflight(L->device >= 0 && L->device < LCD_MAX_DEV ? L->device : 0),
          early_k2(inflight.n == 1 && env.early), chain_base(nb_ + 1, 0), pread_base(nb_ + 1, 0), es(L->side[2]), n_cu(g_n_cus), preads(nb_), out_rel(nb_), out_tots(nb_, 0),
          rc_all(L->h_rc_all), str_all(L->h_str_all), str_outs(L->h_str_outs), rc_base(nb_ + 1, 0), str_base(nb_ + 1, 0), str_tots(nb_, 0) {
        for (int k = 0; k < nb; ++k) { chain_base[k + 1] = chain_base[k] + bs[k]->chains.size(); pread_base[k + 1] = pread_base[k] + bs[k]->preads.size(); }
        nC_all = chain_base[nb];
        chain_batch.resize(nC_all);
        for (int k = 0; k < nb; ++k) for (size_t g = chain_base[k]; g < chain_base[k + 1]; ++g) chain_batch[g] = k;
        which.reserve(nC_all);
    }
    // chain g of the submission: its descriptor, its output record, its record in its batch
    PoaChain &chain(size_t g) const { const int k = chain_batch[g]; return bs[k]->pchains[g - chain_base[k]]; }
    PoaChainOut &out(size_t g) const { const int k = chain_batch[g]; return bs[k]->couts[g - chain_base[k]]; }
    ChainRec &rec(size_t g) const { const int k = chain_batch[g]; return bs[k]->chains[g - chain_base[k]]; }
    // f(k) for every batch, on a team of up to `team` host threads (the calling thread is one of them)
    void over_batches(const int team, const std::function<void(int)> &f) const {
        par_chunks((size_t)nb, std::min(nb, team), 1, [&](const size_t lo, const size_t hi, int) { for (size_t k = lo; k < hi; ++k) f((int)k); });
    }

    // ---- validation.  Reads: the batches' flags, options, devices.  Writes: nothing; selects the device.  Calling thread, before the submission exists ----
    static int validate(lcd_batch_t **bs, int nb) {
        for (int k = 0; k < nb; ++k) {
            if (!bs[k]->uploaded) return set_err(-3, "lcd_batch_run before lcd_batch_upload");
            if (memcmp(&bs[k]->opt, &bs[0]->opt, sizeof(lcd_opt_t)) != 0) return set_err(-4, "lcd_batch_run_many: batches with different options");
            if (bs[k]->device != bs[0]->device) return set_err(-4, "lcd_batch_run_many: batches on different devices");
        }
        if (use_device(bs[0]->device)) return -1;
        return 0;
    }
    // ---- statistics reset, the submission's first event, the arena slots' CU table.  Reads: env.  Writes: every batch's st, cu_rank_addr, n_cu; ev[0] on st
    // (the probe of a device's first submission runs and synchronises on st).  Calling thread, before the preparation thread starts ----
    int begin() {
        for (int k = 0; k < nb; ++k) {
            lcd_batch_stats_t &S = bs[k]->st;
            const double keep_up = S.ms_upload;
            memset(&S, 0, sizeof(S)); S.ms_upload = keep_up;
            S.n_chains = (int)bs[k]->chains.size(); S.n_anchor_jobs = (int)bs[k]->anchors.size();
        }
        HIPCHK(hipEventRecord(L->ev[0], st));
        if (env.arena_slots) { const int rc3 = cu_rank_table(st, &cu_rank_addr, &n_cu, env.mem_debug); if (rc3) return rc3; }
        if (env.arena_slot_cus) n_cu = env.arena_slot_cus;
        return 0;
    }

    // Everything between here and the round-0 arena layout needs nothing from the anchor stage and the anchor stage nothing from it (the reads' narrowed ends are applied
    // after the join): capacities (3 ms of a 20-batch submission), the early launch of the long K2 chains (2 ms) and classes / order / arenas (1 ms) run on a helper
    // thread while the calling thread builds the anchor job tables and runs the anchor kernels -- the anchor kernels start ~5 ms earlier.  LCD_NO_PREP_THREAD=1: in line, as before
    //
    // ---- prep_chains: long-chain cut, capacities, output blocks, early launch.  Reads: the batches' chains / preads, env, the learned levels, early_k2.  Writes: the hand-over state
    // but which / plan0 (ChainRec.solo, preads, pchains, couts, out_rel, out_tots, d_poa_out, early, early_load, reads_up); the read table, ev[8] and the long
    // chains' launches on es.  Preparation thread (LCD_NO_PREP_THREAD: calling thread), with one team ----
    int prep_chains() {
        choose_long_chains();
        over_batches(host_team(env), [&](const int k) { size_chains(k); });
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k];
            const int nC = (int)b->chains.size();
            if (nC && b->d_poa_out.ensure(out_tots[k])) return -11;
            for (int c = 0; c < nC; ++c) b->pchains[c].out_off = b->d_poa_out.addr() + out_rel[k][c];
        }
        if (env.time_host) fprintf(stderr, "[host]   POA prep: capacities after %.1f ms\n", now_ms() - t_begin);
        return launch_early();
    }
    // Which chains are LONG (256-thread workgroup: rows on wavefront 0, per-read phases on four) is decided for the submission at hand: at most LCD_SOLO_N
    // (default: one per two CUs) of the longest chains in flight, and none below LCD_SOLO_MIN read-bases.  A lone batch leaves most of the chip idle and its
    // longest chain IS its latency, so there the cut is low; twenty batches keep the wide workgroups for their top hundred.  LCD_SOLO_RL fixes the cut instead.
    // Reads: the batches' chains / preads, early_k2.  Writes: ChainRec.solo.  Preparation thread
    void choose_long_chains() {
        if (env.solo_rl_set) { for (int k = 0; k < nb; ++k) for (ChainRec &C : bs[k]->chains) C.solo = -1; return; }
        const long long solo_min = env.solo_min;
        const size_t solo_n = (size_t)(env.solo_n >= 0 ? env.solo_n : std::max(1, g_n_cus / 2));
        std::vector<long long> rls;
        for (int k = 0; k < nb; ++k) for (ChainRec &C : bs[k]->chains) {
            int maxl = 0; for (size_t q = 0; q < C.members.size(); ++q) maxl = std::max(maxl, bs[k]->preads[C.read0 + q].len);
            rls.push_back((long long)C.members.size() * maxl);
        }
        long long cut = solo_min;
        if (solo_n == 0) cut = 1ll << 62;
        else if (rls.size() > solo_n) { std::vector<long long> t = rls; std::nth_element(t.begin(), t.begin() + (solo_n - 1), t.end(), std::greater<long long>()); cut = std::max(cut, t[solo_n - 1]); }
        size_t q = 0;
        // (with the long K2 chains launched ahead of the anchor stage -- launch_early -- one of the four hardware queues is theirs for the length of the submission: K1 chains,
        //  which wait for their anchors, then stay in the single-wavefront class instead of forming a fourth launch group that would queue behind another)
        for (int k = 0; k < nb; ++k) for (ChainRec &C : bs[k]->chains) C.solo = rls[q++] >= cut && (C.mode == 1 || !early_k2) ? 1 : 0; // (noisy reads have no certified-band K2 chains, but their long K1 chains are no faster in the wide workgroup: SV shape 1 608 with them there, 1 680 without)
    }
    // capacities, class and output offsets of a batch's chains (independent of the other batches).  Reads: batch k, env, the learned levels.  Writes: preads[k], out_rel[k], out_tots[k],
    // batch k's couts / pchains / cert fields.  Team of prep_chains
    void size_chains(const int k) {
        lcd_batch_t *b = bs[k];
        { preads[k] = b->preads; const uint64_t in_base = b->d_in.addr(); for (auto &r : preads[k]) r.seq_off += in_base; }
        const int nC = (int)b->chains.size();
        b->couts.assign(nC, PoaChainOut());
        b->pchains.assign(nC, PoaChain());
        out_rel[k].resize(nC);
        uint64_t out_tot = 0;
        const PlanHints hints = learned_hints();
        for (int c = 0; c < nC; ++c) {
            b->chains[c].cert_level = -1; b->chains[c].cert_fail_round = -1; // (nothing about the certified band is remembered from an earlier run of the same batch)
            chain_caps(b->opt, b->chains[c], preads[k], 1, (long long)nC_all, env, hints, b->pchains[c]);
            out_rel[k][c] = out_tot; out_tot += lcd_align_up(poa_out_bytes(b->pchains[c].node_cap, b->pchains[c].n_reads), 256);
        }
        out_tots[k] = out_tot;
    }
    // ---- the long K2 chains start NOW: they are the latency of the submission (the longest chain lasts as long as the whole POA stage) and need nothing from
    // the anchor stage -- their reads are aligned whole.  Own stream, own chain table / read table / arenas (the anchor stage's workspace is the leader's arena);
    // their results join the others' after the first round's launches.  LCD_EARLY=0: off (they start with everybody else, as before).
    // Reads: preads, pchains, early_k2.  Writes: early, early_load, reads_up, the early chains' ws_off / slot fields; d_preads, ev[8] and the launches on es.  Preparation thread
    int launch_early() {
        // the read table goes up ONCE, here, on the long chains' stream (24 MB for 20 batches: 1.5 - 1.8 ms of this helper thread instead of the calling thread's, which
        // used to send it a second time between the anchor stage and the main launches); the reads the anchor stage narrows are patched afterwards (lcd_patch_reads_kernel)
        if (early_k2 && es && nC_all && !L->d_preads.ensure(pread_base[nb] * sizeof(PoaRead))) {
            HIPCHK(hipStreamWaitEvent(es, L->ev[0], 0)); // (behind whatever the leader's stream held before this submission)
            for (int k = 0; k < nb; ++k) if (!preads[k].empty())
                HIPCHK(hipMemcpyAsync((PoaRead *)L->d_preads.p + pread_base[k], preads[k].data(), preads[k].size() * sizeof(PoaRead), hipMemcpyHostToDevice, es));
            HIPCHK(hipEventRecord(L->ev[8], es));
            reads_up = true;
        } else (void)hipGetLastError();
        if (early_k2 && es) for (size_t g = 0; g < nC_all; ++g) { const PoaChain &pc = chain(g); if (pc.solo && pc.mode == 1 && pc.threads == 256 && pc.n_reads > 0) early.push_back(g); }
        if (early.size() == nC_all) early.clear(); // (the first round is built around the launches of the others)
        if (early.empty()) return 0;
        std::vector<PoaChain> sub_e(early.size());
        uint64_t tot_e = 0;
        for (size_t i = 0; i < early.size(); ++i) {
            PoaChain &pc = chain(early[i]);
            early_load = std::max(early_load, (double)pc.n_reads * (pc.max_len + 64));
            pc.ws_off = tot_e; pc.slot_flags = 0; pc.slot_bytes = 0; pc.n_slots = 0; pc.per_cu = 0; pc.cu_rank = 0;
            tot_e += lcd_align_up(poa_layout(pc.node_cap, pc.edge_cap, pc.rid_words, pc.max_len, pc.cell_cap, pc.n_reads, pc.spill_x, pc.cert).total, 256);
        }
        if (!reads_up || L->d_early_arena.ensure(tot_e, 3) || L->d_chains_early.ensure(early.size() * sizeof(PoaChain)) ||
            L->d_poa_outs_early.ensure(early.size() * sizeof(PoaChainOut))) { (void)hipGetLastError(); early.clear(); return 0; } // (no memory for it: they start with the others)
        for (size_t i = 0; i < early.size(); ++i) { PoaChain &pc = chain(early[i]); pc.ws_off += L->d_early_arena.addr(); sub_e[i] = pc; sub_e[i].read0 += (int)pread_base[chain_batch[early[i]]]; }
        { const int rc2 = launch_poa_grouped(es, sub_e, L->d_chains_early, (const PoaRead *)L->d_preads.p, L->d_poa_outs_early, sc, env); if (rc2) return rc2; }
        if (env.time_host) fprintf(stderr, "[host]   %zu long K2 chains launched %.1f ms after the start (%.2f GB of arenas)\n", early.size(), now_ms() - t_begin, tot_e / 1e9);
        return 0;
    }

    // ---- prepare_round0: classes and order of the chains that start after the anchor stage, and their arena layout: host work that needs nothing from the anchor
    // stage -- made on the preparation thread while the anchor kernels run (4 ms of a 260 ms submission with the main launches waiting for it, before).
    // Reads: early, pchains, n_cu, cu_rank_addr.  Writes: which, plan0, the chains' lds_words / ws_off / slot fields.  Preparation thread when order_async, else calling
    // thread after the join ----
    void prepare_round0() {
        order_chains();
        plan0.need.resize(which.size());
        for (size_t i = 0; i < which.size(); ++i) { const PoaChain &pc = chain(which[i]); plan0.need[i] = poa_layout(pc.node_cap, pc.edge_cap, pc.rid_words, pc.max_len, pc.cell_cap, pc.n_reads, pc.spill_x, pc.cert).total; }
        segment_arenas(plan0);
        plan0.valid = true;
    }
    void order_chains() {
        { std::vector<char> is_early(nC_all, 0); for (size_t g : early) is_early[g] = 1; for (size_t g = 0; g < nC_all; ++g) if (!is_early[g]) which.push_back(g); }
        // No more launch groups than streams: a stream runs its kernels one after the other, so a fifth group starts only when some other group's LAST chain has
        // ended -- with the bulk of the work (40 000 short chains in the smallest LDS bucket) queued behind a group of a few hundred long chains the chip idled for a
        // third of the stage.  The single-wavefront group with the fewest chains moves up into the next larger LDS bucket in use (a bigger pool is always valid).
        for (const int n_streams = env.streams;;) {
            // (only SMALL groups move -- less than 8 % of the submission's CU-time: a bigger pool means fewer chains per CU, and the bulk of the work must keep the
            //  occupancy of its own bucket; noisy-read submissions have five wide classes besides, there is no getting down to four groups)
            std::map<long long, std::pair<size_t, double>> cnt;
            double tot_w = 0;
            for (size_t g = 0; g < nC_all; ++g) {
                const PoaChain &pc = chain(g);
                const double w = (double)pc.n_reads * (pc.max_len + 64) / chains_per_cu(pc.lds_words * 4, pc.threads, kSchedOverhead);
                auto &e = cnt[chain_group_key(pc)]; e.first++; e.second += w; tot_w += w;
            }
            if ((int)cnt.size() <= n_streams) break;
            long long from = -1, to = -1; double least = 0.08 * tot_w;
            for (auto it = cnt.begin(); it != cnt.end(); ++it) {
                if ((it->first >> 20) != 64) continue;
                auto nx = std::next(it);
                if (nx == cnt.end() || (nx->first >> 20) != 64) continue;
                if (it->second.second < least) { least = it->second.second; from = it->first; to = nx->first; }
            }
            if (from < 0) break;
            const int lw = (int)(to & ((1 << 20) - 1));
            for (size_t g = 0; g < nC_all; ++g) if (chain_group_key(chain(g)) == from) chain(g).lds_words = lw;
        }
        // widest / largest-LDS group first, then biggest first so the long chains start early (LPT)
        // (keys taken once: the comparator used to look both chains up through their batch for each of the ~600 000 comparisons of a 20-batch submission)
        std::vector<std::pair<long long, uint64_t>> sk(nC_all);
        for (size_t g = 0; g < nC_all; ++g) { const PoaChain &pc = chain(g); sk[g] = {chain_group_key(pc), pc.cell_cap}; }
        std::sort(which.begin(), which.end(), [&](size_t a, size_t c2) {
            if (sk[a].first != sk[c2].first) return sk[a].first > sk[c2].first;
            if (sk[a].second != sk[c2].second) return sk[a].second > sk[c2].second;
            return a < c2; });
    }
    // Work arenas.  A chain's arena is live only while its workgroup is resident, and a CU holds at most per_cu workgroups of a launch group:
    // runs of chains of one launch group and one size class (half octaves of the arena size) that outnumber the chip's capacity share a pool of
    // n_cu x per_cu SLOTS claimed at workgroup start (poa_kernel.hip); the others keep private arenas.  Memory then scales with resident
    // workgroups, not with the number of chains in flight.
    // Reads: which (ordered), P.need[i] for which[i], n_cu, cu_rank_addr.  Writes: P, the chains' ws_off (relative to P) and slot fields.  The thread of its caller
    void segment_arenas(ArenaPlan &P) {
        const bool use_slots = env.arena_slots;
        P.tot = 0; P.flag_ints = 0; P.n_pooled = P.n_pools = 0; P.private_bytes = P.pool_bytes = 0; P.items.clear(); P.item_of.assign(which.size(), 0);
        for (size_t i = 0; i < which.size();) {
            const long long key = chain_group_key(chain(which[i]));
            size_t j = i;
            while (j < which.size() && chain_group_key(chain(which[j])) == key) ++j;
            const PoaChain &p0 = chain(which[i]);
            const int per_cu = chains_per_cu(p0.lds_words * 4, p0.threads, kSlotOverhead);
            const uint64_t R = (uint64_t)n_cu * per_cu;
            // the group's chains by arena size, largest first, cut into segments at breakpoints where the size has dropped by >= 1.3x; a segment
            // either keeps private arenas (cost: the sum of its sizes) or, if it has more than R chains, shares R slots of its largest size
            // (cost R x size).  The cheapest segmentation is a shortest path over the <= ~40 breakpoints (sizes of a group span two orders of magnitude).
            std::vector<size_t> ord(j - i);
            for (size_t q = 0; q < ord.size(); ++q) ord[q] = i + q;
            std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b2) { return P.need[a] > P.need[b2]; });
            const size_t n = ord.size();
            std::vector<size_t> bp(1, 0);
            for (size_t q = 1; q < n; ++q) if ((double)P.need[ord[q]] * 1.3 <= (double)P.need[ord[bp.back()]]) bp.push_back(q);
            bp.push_back(n);
            std::vector<uint64_t> pre(n + 1, 0);
            for (size_t q = 0; q < n; ++q) pre[q + 1] = pre[q] + P.need[ord[q]];
            const size_t nbp = bp.size();
            std::vector<uint64_t> cost(nbp, ~0ull); std::vector<size_t> nxt(nbp, nbp - 1);
            cost[nbp - 1] = 0;
            auto seg_pooled = [&](size_t a, size_t b2) { return use_slots && bp[b2] - bp[a] > R && R * lcd_align_up(P.need[ord[bp[a]]], 256) < pre[bp[b2]] - pre[bp[a]]; };
            for (size_t a = nbp - 1; a-- > 0;)
                for (size_t b2 = a + 1; b2 < nbp; ++b2) {
                    const uint64_t c = (seg_pooled(a, b2) ? R * lcd_align_up(P.need[ord[bp[a]]], 256) : pre[bp[b2]] - pre[bp[a]]) + cost[b2];
                    if (c < cost[a]) { cost[a] = c; nxt[a] = b2; }
                }
            for (size_t a = 0; a + 1 < nbp; a = nxt[a]) {
                const size_t b2 = nxt[a];
                if (seg_pooled(a, b2)) {
                    const uint64_t slot = lcd_align_up(P.need[ord[bp[a]]], 256);
                    for (size_t q = bp[a]; q < bp[b2]; ++q) { PoaChain &pc = chain(which[ord[q]]); pc.ws_off = P.tot; pc.slot_flags = 1 + P.flag_ints; pc.slot_bytes = slot; pc.n_slots = (int)R; pc.per_cu = per_cu; pc.cu_rank = cu_rank_addr; P.item_of[ord[q]] = (uint32_t)P.items.size(); }
                    P.items.push_back({P.tot, R * slot, 0});
                    P.tot += R * slot; P.flag_ints += R; P.n_pooled += bp[b2] - bp[a]; ++P.n_pools; P.pool_bytes += R * slot;
                } else
                    for (size_t q = bp[a]; q < bp[b2]; ++q) { PoaChain &pc = chain(which[ord[q]]); pc.ws_off = P.tot; pc.slot_flags = 0; pc.slot_bytes = 0; pc.n_slots = 0; pc.per_cu = 0; pc.cu_rank = 0; P.item_of[ord[q]] = (uint32_t)P.items.size(); P.items.push_back({P.tot, P.need[ord[q]], 0}); P.tot += P.need[ord[q]]; P.private_bytes += P.need[ord[q]]; }
            }
            i = j;
        }
    }
    // ---- the preparation thread: prep_chains, then prepare_round0 when the submission is large enough to pay for it.  start_prep returns prep_chains' own code
    // when it ran in line (LCD_NO_PREP_THREAD).  A helper thread selects the device first and hands its error text over at the join.  Calling thread ----
    int start_prep() {
        order_async = nC_all >= 2048 && !env.no_prep_thread;
        if (env.no_prep_thread) return prep_chains();
        const int dev_here = cur_device();
        prep_thread.t = std::thread([this, dev_here]() {
            if (hipSetDevice(dev_here) != hipSuccess) { prep_rc = -1; prep_err = "hipSetDevice failed on the preparation thread"; return; }
            prep_rc = prep_chains();
            if (!prep_rc && order_async) prepare_round0();
            if (prep_rc) prep_err = g_err;
        });
        return 0;
    }
    // from here on the hand-over state (above) is the calling thread's
    int join_prep() { if (prep_thread.t.joinable()) prep_thread.t.join(); if (prep_rc && !prep_err.empty()) g_err = prep_err; return prep_rc; }

    // ---------------- S1: anchors (K4 prefilter + K3b) ----------------
    // Reads: the batches' anchors / ed_jobs / wfa_jobs, env.  Writes: the leader's anchor buffers; K4 on side[0] (or st), K3 on st and side[1], the ends kernel on st;
    // synchronises st (and side[0]).  Joins the preparation thread before it touches preads (apply_anchor_ends); without anchor jobs it returns without joining.
    // Calling thread, beside the preparation thread ----
    int anchor_stage() {
        std::vector<EdJob> ej; std::vector<WfaJob> wj;
        std::vector<size_t> ej_base(nb + 1, 0), wj_base(nb + 1, 0);
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k];
            const uint64_t in_base = b->d_in.addr();
            ej_base[k] = ej.size(); wj_base[k] = wj.size();
            if (b->anchors.empty()) continue;
            for (EdJob j : b->ed_jobs) { j.q_off += in_base; j.t_off += in_base; ej.push_back(j); }
            for (WfaJob j : b->wfa_jobs) { j.p_off += in_base; j.t_off += in_base; j.s_cap = wfa_default_scap(j.plen, j.tlen, g_wfa_hint.load()); wj.push_back(j); } // (the hint may have risen since the region was added)
        }
        ej_base[nb] = ej.size(); wj_base[nb] = wj.size();
        if (ej.empty() && wj.empty()) return 0;
        std::vector<EdOut> eo; std::vector<WfaOut> wo;
        // (ONE transient arena per leader for every stage's workspace -- edlib blocks, WFA wavefronts, the chains' DP regions: the stages of a
        // submission follow each other on the leader's stream and none of them reads another's workspace, so the arena is their maximum, not their sum)
        const bool th = env.time_host;
        if (th) fprintf(stderr, "[host]   anchors: job tables (%zu edlib, %zu WFA) after %.1f ms\n", ej.size(), wj.size(), now_ms() - t_begin);
        // K4 and K3 of the anchor stage are independent and both latency-bound (one wavefront per pair, 60 % of its cycles waiting): side by side on two
        // streams when K4's stored columns (1 MiB per pair, edlib's own rule) fit a workspace of their own of up to 20 GB -- 17 000 pairs; larger submissions and the noisy shapes keep the one shared arena and the old order
        uint64_t ed_tot = 0; for (const EdJob &j : ej) ed_tot += lcd_align_up(ed_arena_bytes(j.qlen, j.tlen), 256);
        const bool side_by_side = !ej.empty() && !wj.empty() && L->side[0] && ed_tot <= (20ull << 30) && !env.anchor_seq;
        hipStream_t ks = side_by_side ? L->side[0] : st;
        if (side_by_side) HIPCHK(hipStreamWaitEvent(ks, L->ev[0], 0));
        int rc = run_edlib_stage(ks, ej, L->d_ed_jobs, side_by_side ? L->d_ed_arena : L->d_poa_arena, L->d_ed_outs, eo, side_by_side);
        if (rc) return rc;
        if (th && !side_by_side) { hipStreamSynchronize(st); fprintf(stderr, "[host]   anchors: edlib stage done after %.1f ms\n", now_ms() - t_begin); }
        // (K3's class launches -- each as long as its longest job -- on the leader's stream and the second side stream: the first has K4, the third the long chains;
        //  LCD_ANCHOR_WFA_SEQ=1: one after the other on the leader's stream, as before)
        const bool k3_two = !env.anchor_wfa_seq;
        rc = run_wfa_stage(st, wj, L->d_wfa_jobs, L->d_poa_arena, L->d_wfa_out, L->d_wfa_outs, wo, sc, env, nullptr, true, k3_two && side_by_side && L->side[1] ? L->side + 1 : nullptr, L->sev, k3_two && side_by_side && L->side[1] ? 1 : 0);
        if (rc) return rc;
        if (side_by_side) { HIPCHK(hipMemcpyAsync(eo.data(), L->d_ed_outs.p, eo.size() * sizeof(EdOut), hipMemcpyDeviceToHost, ks)); HIPCHK(hipStreamSynchronize(ks)); }
        HIPCHK(hipStreamSynchronize(st));
        if (th) fprintf(stderr, "[host]   anchors: WFA stage done after %.1f ms\n", now_ms() - t_begin);
        // cigars of the anchor jobs: ONE device->host copy of the output span of all of them (a copy per job costs more in
        // launch overhead than in bytes)
        // the alignments' ends (collect_aln_beg_end) are computed where the CIGARs are: 20 bytes per job come back (strings_kernel.hip lcd_anchor_ends_kernel)
        std::vector<AnchorEndsOut> aends(wj.size());
        if (!wj.empty()) {
            std::vector<AnchorEndsJob> aj(wj.size());
            for (size_t i = 0; i < wj.size(); ++i) { aj[i].cigar = wj[i].out_off; aj[i].n_cigar = wo[i].n_cigar; aj[i].pad_ = 0; }
            if (L->d_aends_jobs.ensure(aj.size() * sizeof(AnchorEndsJob)) || L->d_aends_outs.ensure(aj.size() * sizeof(AnchorEndsOut))) return -11;
            HIPCHK(hipMemcpyAsync(L->d_aends_jobs.p, aj.data(), aj.size() * sizeof(AnchorEndsJob), hipMemcpyHostToDevice, st));
            lcd_launch_anchor_ends((const AnchorEndsJob *)L->d_aends_jobs.p, (AnchorEndsOut *)L->d_aends_outs.p, (int)aj.size(), st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(aends.data(), L->d_aends_outs.p, aends.size() * sizeof(AnchorEndsOut), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        if (th) fprintf(stderr, "[host]   anchors: alignment ends (%.2f MB) on the host after %.1f ms\n", aends.size() * sizeof(AnchorEndsOut) / 1e6, now_ms() - t_begin);
        for (auto &e : eo) if (e.status != LCD_OK) return set_err(-20, "edlib kernel status " + std::to_string(e.status));
        { const int rcp = join_prep(); if (rcp) return rcp; } // (the read tables below are the helper thread's)
        apply_anchor_ends(ej_base, wj_base, eo, wo, aends);
        return 0;
    }
    // the anchor stage's verdicts and narrowed ends, into the read tables.  Reads: the anchor stage's results, the batches' anchors.  Writes: preads (skip, the four
    // ends), the batches' anchor statistics.  Calling thread, after join_prep
    void apply_anchor_ends(const std::vector<size_t> &ej_base, const std::vector<size_t> &wj_base, const std::vector<EdOut> &eo, const std::vector<WfaOut> &wo, const std::vector<AnchorEndsOut> &aends) {
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k]; lcd_batch_stats_t &S = b->st;
            for (size_t i = ej_base[k]; i < ej_base[k + 1]; ++i) S.edlib_blocks += eo[i].blocks;
            for (size_t i = wj_base[k]; i < wj_base[k + 1]; ++i) S.wfa_offsets += wo[i].offsets;
            S.n_edlib_jobs = (int)(ej_base[k + 1] - ej_base[k]); S.n_wfa_jobs += (int)(wj_base[k + 1] - wj_base[k]);
            for (const AnchorRec &A : b->anchors) {
                PoaRead &pr = preads[k][A.pread];
                const int x = eo[ej_base[k] + A.ed_job].xgaps;
                if (x > A.min_len * 0.10) { pr.skip = 1; continue; }
                if (A.ext == 0) continue;
                const size_t wi = wj_base[k] + A.wfa_job;
                const int ncg = wo[wi].n_cigar;
                if (ncg == 0) { pr.skip = 1; continue; }
                // collect_aln_beg_end, src/align.c:630-663: left to right the end of the last '=' run, right to left the start of the first one (counted back from
                // tlen + 1 / qlen + 1); an alignment without a '=' run keeps the whole sequences
                const AnchorEndsOut &ae = aends[wi];
                int rb = 1, qb = 1, re = A.tlen_full, qe = A.qlen_full;
                if (ae.has_eq) {
                    if (A.ext == 1) { re = ae.pre_r; qe = ae.pre_q; }
                    else { rb = A.tlen_full + 1 - ae.suf_r; qb = A.qlen_full + 1 - ae.suf_q; }
                }
                pr.ref_beg = rb; pr.ref_end = re; pr.read_beg = qb; pr.read_end = qe;
            }
        }
    }

    // ---------------- S2: POA chains ----------------
    // the read table: only what the anchor stage changed when it went up with the long chains (reads_up), else all of it.  Reads: preads, reads_up, the batches'
    // anchors.  Writes: d_preads (st; waits for ev[8]), sizes d_chains / d_poa_outs.  Calling thread, after join_prep
    int upload_reads() {
        if (L->d_preads.ensure(pread_base[nb] * sizeof(PoaRead)) || L->d_chains.ensure(nC_all * sizeof(PoaChain)) || L->d_poa_outs.ensure(nC_all * sizeof(PoaChainOut))) return -11;
        if (reads_up) { // only what the anchor stage changed
            std::vector<ReadPatch> pt;
            for (int k = 0; k < nb; ++k) for (const AnchorRec &A : bs[k]->anchors) { ReadPatch p; p.idx = (uint32_t)(pread_base[k] + A.pread); p.pad_ = 0; p.r = preads[k][A.pread]; pt.push_back(p); }
            HIPCHK(hipStreamWaitEvent(st, L->ev[8], 0));
            if (!pt.empty()) {
                if (L->d_read_patches.ensure(pt.size() * sizeof(ReadPatch))) return -11;
                HIPCHK(hipMemcpyAsync(L->d_read_patches.p, pt.data(), pt.size() * sizeof(ReadPatch), hipMemcpyHostToDevice, st));
                lcd_launch_patch_reads((PoaRead *)L->d_preads.p, (const ReadPatch *)L->d_read_patches.p, (int)pt.size(), st);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st)); // (pt is a local)
            }
        } else
            for (int k = 0; k < nb; ++k)
                if (!preads[k].empty())
                    HIPCHK(hipMemcpyAsync((PoaRead *)L->d_preads.p + pread_base[k], preads[k].data(), preads[k].size() * sizeof(PoaRead), hipMemcpyHostToDevice, st));
        return 0;
    }
    // up to 12 rounds: the chains of `which`, then those that came back.  Reads / writes: everything the rounds' steps do (below).  Calling thread, after join_prep
    int poa_stage() {
        if (!nC_all) return 0;
        if (const int rc = upload_reads()) return rc;
        if (!order_async) prepare_round0();
        if (env.time_host) fprintf(stderr, "[host]   POA prep: classes + order after %.1f ms\n", now_ms() - tp0);
        for (int k = 0; k < nb; ++k) bs[k]->retry_out_used = 0;
        for (int round = 0; round < 12 && !which.empty(); ++round) {
            PoaRound R; R.round = round;
            int rc = plan_round(R);
            if (!rc) rc = place_arenas(R);
            if (!rc) rc = spare_pool(R);
            if (!rc) rc = launch_round(R);
            if (!rc) rc = judge_round(R);
            if (rc) return rc;
        }
        if (!which.empty()) return set_err(-21, "POA DP arena exhausted after retries");
        return 0;
    }
    // a round's chain table and arena layout: round 0 takes plan0 when the preparation thread made it; a later round re-sizes its chains (retry_scale), gives a chain whose
    // graph capacity grew a fresh output block of its batch, and lays the arenas out again.  Reads: which, plan0, scale, ChainRec, preads.  Writes: R.P, R.sub / R.sub_n,
    // pchains (capacities, out_off, ws_off, slot fields), retry_out_off, the batches' retry_out.  Calling thread
    int plan_round(PoaRound &R) {
        ArenaPlan &P = R.P;
        if (R.round == 0 && plan0.valid) P = std::move(plan0);
        else P.need.assign(which.size(), 0);
        const bool planned = P.valid;
        L->h_sub_pin.resize(which.size() * sizeof(PoaChain));
        R.sub = (PoaChain *)L->h_sub_pin.data(); R.sub_n = which.size();
        if (!planned) {
            const PlanHints hints = learned_hints(); // (as the round before left them)
            for (size_t i = 0; i < which.size(); ++i) {
                const int k = chain_batch[which[i]]; const size_t c = which[i] - chain_base[k];
                PoaChain &pc = chain(which[i]);
                if (R.round) {
                    const int old_cap = pc.node_cap;
                    chain_caps(bs[k]->opt, rec(which[i]), preads[k], retry_scale(rec(which[i]), scale), (long long)nC_all, env, hints, pc);
                    if (pc.node_cap > old_cap) { // the chain's output block (cons + MSA rows of node_cap columns) grows with it: a fresh block
                        lcd_batch_t *b = bs[k];
                        if (b->retry_out_used == b->retry_out.size()) b->retry_out.emplace_back(new DevBuf());
                        DevBuf *ro2 = b->retry_out[b->retry_out_used++].get();
                        if (ro2->ensure(poa_out_bytes(pc.node_cap, pc.n_reads) + 256)) return -11;
                        pc.out_off = ro2->addr(); retry_out_off[which[i]] = pc.out_off;
                    } else pc.out_off = retry_out_off.count(which[i]) ? retry_out_off[which[i]] : bs[k]->d_poa_out.addr() + out_rel[k][c];
                }
                P.need[i] = poa_layout(pc.node_cap, pc.edge_cap, pc.rid_words, pc.max_len, pc.cell_cap, pc.n_reads, pc.spill_x, pc.cert).total;
            }
            segment_arenas(P);
        }
        if (env.time_host) fprintf(stderr, "[host]   POA prep: arenas laid out after %.1f ms\n", now_ms() - tp0);
        if (env.mem_debug) report_round_memory(*this, R);
        return 0;
    }
    // device memory for the layout.  placement: first fit over [d_poa_arena, extra chunks...] in item order; one more chunk (what is left of this submission) when
    // they are full.  Reads: R.P, which.  Writes: the slot flags (memset on st), the leader's arena chunks, the chains' final ws_off / slot_flags, R.sub.  Calling
    // thread, with one team
    int place_arenas(PoaRound &R) {
        ArenaPlan &P = R.P;
        if (P.flag_ints) {
            if (L->d_slot_flags.ensure(P.flag_ints * 4 + 64)) return -11;
            HIPCHK(hipMemsetAsync(L->d_slot_flags.p, 0, P.flag_ints * 4, st));
        }
        {
            if (L->d_poa_arena.cap == 0 && L->d_poa_arena.ensure(P.tot, 3)) return -11;
            std::vector<DevBuf *> ch(1, &L->d_poa_arena);
            for (auto &c : L->arena_extra) ch.push_back(c.get());
            size_t k = 0; uint64_t off = 0, left = P.tot;
            for (ArenaItem &it : P.items) {
                while (k < ch.size() && off + it.bytes > ch[k]->cap) { ++k; off = 0; }
                if (k == ch.size()) {
                    L->arena_extra.emplace_back(new DevBuf());
                    if (L->arena_extra.back()->ensure(left, 3)) { L->arena_extra.pop_back(); return -11; }
                    ch.push_back(L->arena_extra.back().get());
                    if (env.mem_debug) fprintf(stderr, "[mem] arena chunk %zu: %.2f GB\n", ch.size() - 1, ch.back()->cap / 1e9);
                }
                it.phys = ch[k]->addr() + off; off += it.bytes; left -= it.bytes;
            }
        }
        par_chunks(which.size(), host_team(env), 4096, [&](const size_t lo, const size_t hi, int) { for (size_t i = lo; i < hi; ++i) {
            PoaChain &pc = chain(which[i]);
            pc.ws_off = P.items[P.item_of[i]].phys + (pc.ws_off - P.items[P.item_of[i]].start);
            if (pc.slot_flags) pc.slot_flags = L->d_slot_flags.addr() + (pc.slot_flags - 1) * 4;
            R.sub[i] = pc; R.sub[i].read0 += (int)pread_base[chain_batch[which[i]]]; // the device read table is the concatenation of the batches' tables
        } });
        return 0;
    }
    // Spare DP memory (PoaSpare, poa_kernel.hip grow_dp_region): what a chain whose estimate was too small for one of its reads continues in.  Taken
    // after the arenas have their memory, from what the budget leaves (LCD_SPARE_GB caps it, 0 switches it off); without it -- or once it is used
    // up -- such a chain comes back with LCD_ERR_CELLS and is re-run from its first read in the next round, as before.
    // Reads: env, the device's budget.  Writes: the leader's d_spare (header copy on st), R.d_spare, R.spare_hdr.  Calling thread
    int spare_pool(PoaRound &R) {
        // (noisy reads: 16 GB were used up by ~200 regions of an SV-shape submission and the chains refused after that -- a 36-read x 8 kb chain among them --
        //  started over in a second round of 3 s)
        const double spare_gb = env.spare_set ? env.spare_gb : L->opt.is_ont ? 32.0 : 16.0; // (read per call: tests switch it)
        if (spare_gb <= 0) L->d_spare.release();
        else if (L->d_spare.cap == 0) {
            const long long room = (dev_budget(L->device) - g_dev_bytes[L->device].load() - (4ll << 30)) / 2;
            const long long want = std::min<long long>((long long)(spare_gb * (double)(1ll << 30)), room);
            if (want >= (64ll << 20) && L->d_spare.ensure((size_t)want, 40)) { /* no spare pool this time */ }
        }
        if (L->d_spare.cap > 4096) { // (R.spare_hdr lives until the round's stream synchronisation: the source of an asynchronous copy)
            R.spare_hdr.used = 0; R.spare_hdr.cap = L->d_spare.cap - 256; R.spare_hdr.base = L->d_spare.addr() + 256; R.spare_hdr.n_grown = R.spare_hdr.n_refused = 0;
            HIPCHK(hipMemcpyAsync(L->d_spare.p, &R.spare_hdr, sizeof(R.spare_hdr), hipMemcpyHostToDevice, st));
            R.d_spare = (PoaSpare *)L->d_spare.p;
        }
        return 0;
    }
    // the round's launches, and its records back on the host; after round 0 the early chains join `which`.  Reads: R.sub, R.d_spare, early, early_load.  Writes: ev[6],
    // ev[7], the launch groups on st and side[] (launch_poa_grouped), R.tmp, R.spare_seen, which (+= early), the batches' kernel-time statistics; synchronises st (round 0
    // with early chains: es too).  Calling thread
    int launch_round(PoaRound &R) {
        const int round = R.round; const size_t sub_n = R.sub_n;
        if (env.time_host) fprintf(stderr, "[host] POA stage: %.1f ms of host work before the launches of round %d\n", now_ms() - tp0, round);
        HIPCHK(hipEventRecord(L->ev[6], st));
        { int rc2 = launch_poa_grouped(st, R.sub, sub_n, L->d_chains, (const PoaRead *)L->d_preads.p, L->d_poa_outs, sc, env, L->side, L->sev, &L->d_gate, R.d_spare, round == 0 && !early.empty() ? 3 : -1, early_load, L->opt.is_ont != 0); if (rc2) return rc2; }
        HIPCHK(hipEventRecord(L->ev[7], st));
        L->h_tmp_pin.resize((sub_n + (round == 0 ? early.size() : 0)) * sizeof(PoaChainOut)); // (with room for the early chains' records: appending them to a vector re-allocated 9 MB with the GPU idle)
        R.tmp = (PoaChainOut *)L->h_tmp_pin.data();
        HIPCHK(hipMemcpyAsync(R.tmp, L->d_poa_outs.p, sub_n * sizeof(PoaChainOut), hipMemcpyDeviceToHost, st));
        R.spare_seen.used = 0; R.spare_seen.n_grown = R.spare_seen.n_refused = 0;
        if (R.d_spare) HIPCHK(hipMemcpyAsync(&R.spare_seen, R.d_spare, sizeof(PoaSpare), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (env.time_host) fprintf(stderr, "[host]   round %d: kernels and statuses back %.1f ms after the stage's start\n", round, now_ms() - tp0);
        if (round == 0 && !early.empty()) { // the long chains that started before the anchor stage: from here on they are chains of this round like the others
            HIPCHK(hipMemcpyAsync(R.tmp + sub_n, L->d_poa_outs_early.p, early.size() * sizeof(PoaChainOut), hipMemcpyDeviceToHost, es));
            HIPCHK(hipStreamSynchronize(es));
            which.insert(which.end(), early.begin(), early.end());
        }
        if (R.d_spare) {
            bs[0]->st.poa_grown += (int)R.spare_seen.n_grown; // (a count of the launch set: kept on the leader, so that the batches' statistics add up)
            if (env.mem_debug) fprintf(stderr, "[mem] round %d: spare DP memory %.2f GB: %u regions grown in place (%.2f GB), %u refused\n", round, L->d_spare.cap / 1e9, R.spare_seen.n_grown, R.spare_seen.used / 1e9, R.spare_seen.n_refused);
        }
        float kms = 0; hipEventElapsedTime(&kms, L->ev[6], L->ev[7]);
        for (int k = 0; k < nb; ++k) { bs[k]->st.ms_poa_kernel += kms; bs[k]->st.n_poa_launches++; }
        if (env.mem_debug) fprintf(stderr, "[mem] round %d: %zu chains, POA kernels %.1f ms\n", round, which.size(), kms);
        return 0;
    }
    // the records to their batches, then the verdict on every chain that did not end with LCD_OK: back into the next round (chain_goes_back), or the submission's
    // error.  Reads: R.tmp, which.  Writes: the batches' couts, ChainRec's cert fields, R.again, the learned hints, poa_retries, scale, which (= the chains that
    // go back).  Calling thread, with one team
    int judge_round(PoaRound &R) {
        const int round = R.round; const PoaChainOut *const tmp = R.tmp;
        // (the chains' output records -- 200 B each, 46 000 of them in a 20-batch submission -- go to their batches on a few threads: serial this was 3.4 ms
        //  with the GPU idle; the chains that did not end with LCD_OK are few and are looked at one by one below)
        std::vector<size_t> flagged;
        {
            constexpr int NTH = 32; const int nth_r = host_team(env);
            std::vector<size_t> fl[NTH];
            par_chunks(which.size(), nth_r, 2048, [&](const size_t lo, const size_t hi, const int t) {
                for (size_t i = lo; i < hi; ++i) {
                    out(which[i]) = tmp[i];
                    if (tmp[i].status != LCD_OK) fl[t].push_back(i);
                }
            });
            for (int t = 0; t < NTH; ++t) flagged.insert(flagged.end(), fl[t].begin(), fl[t].end());
            std::sort(flagged.begin(), flagged.end());
        }
        if (env.time_host) fprintf(stderr, "[host]   round %d: records in their batches %.1f ms after the stage's start (%zu not LCD_OK)\n", round, now_ms() - tp0, flagged.size());
        for (const size_t i : flagged) {
            const size_t g = which[i]; const int status = tmp[i].status;
            if (chain_goes_back(status, chain(g), rec(g), round)) { R.again.push_back(g); R.n_node_ovf += status == LCD_ERR_NODES || status == LCD_ERR_EDGES; R.n_cert_fail += status == LCD_ERR_CERT; }
            else { // the failing chain's reads, for a replay in isolation (tools/replay_chain.py)
                if (env.dump_chain) dump_failed_chain(*this, g, status);
                return set_err(-20, failed_chain_text(*this, g, tmp[i]));
            }
        }
        if (env.mem_debug) report_round_retries(*this, R);
        if (round == 0 && R.n_node_ovf * 20 > nC_all && g_node_hint.load() < 2) g_node_hint++;
        if (round == 0) { // learn: more than 1 % of a mode's chains overflowed their DP region -> start from the next estimate next time
            int tot[2] = {0, 0}, ovf[2] = {0, 0};
            for (size_t g = 0; g < nC_all; ++g) tot[chain(g).mode ? 1 : 0]++;
            for (size_t g : R.again) if (out(g).status != LCD_ERR_CERT) ovf[chain(g).mode ? 1 : 0]++;
            for (int m = 0; m < 2; ++m) if (tot[m] && ovf[m] * 100 > tot[m] && g_cell_hint[m].load() < 2) g_cell_hint[m]++;
        }
        if (!R.again.empty()) { for (int k = 0; k < nb; ++k) bs[k]->st.poa_retries++; scale *= 2; }
        which.swap(R.again);
        return 0;
    }

    // ---------------- S3: ref<->cons WFA, S4: MSA rows -> strings ----------------
    // the job tables of the batches are independent: built on a few host threads (37 000 string jobs per configs[1] batch; serial, this was 30 ms of a 20-batch
    // submission), concatenated and given their device blocks afterwards
    // (two passes over a batch's regions: `what` 1 = consensus counts, statistics and the ref<->cons jobs -- what the WFA stage waits for; 2 = the string jobs, twelve
    //  times as many, built on the strings stage's own thread while the WFA kernels run)
    // Reads: batch k's regs, couts, pchains.  Writes: what 1: batch k's rc_* tables, reg_rc0, the regions' n_cons, n_regions / n_regions_resolved; what 2: its str_*
    // tables, reg_str0, str_tots[k].  A team of refcons_jobs (what 1) / of build_string_tables (what 2)
    void build_jobs(const int k, const int what) {
        lcd_batch_t *b = bs[k]; lcd_batch_stats_t &S = b->st;
        const uint64_t in_base = b->d_in.addr();
        if (what == 1) { b->rc_jobs.clear(); b->rc_region.clear(); b->rc_clu.clear(); b->reg_rc0.assign(b->regs.size() + 1, 0); }
        else { b->str_jobs.clear(); b->str_region.clear(); b->str_clu.clear(); b->str_k.clear(); b->reg_str0.assign(b->regs.size() + 1, 0); }
        uint64_t str_tot = 0;
        for (size_t ri = 0; ri < b->regs.size(); ++ri) {
            RegionRec &R = b->regs[ri];
            if (what == 1) {
                b->reg_rc0[ri] = (uint32_t)b->rc_jobs.size();
                R.n_cons = 0;
                if (R.branch == 0) continue;
                S.n_regions++;
                if (R.branch == 1) {
                    const PoaChainOut &o0 = b->couts[R.chain[0]], &o1 = b->couts[R.chain[1]];
                    if (o0.n_cons + o1.n_cons != 2) continue; // src/align.c:1339
                    R.n_cons = 2;
                } else R.n_cons = b->couts[R.chain[0]].n_cons;
                if (R.n_cons > 0) S.n_regions_resolved++;
            } else {
                b->reg_str0[ri] = (uint32_t)b->str_jobs.size();
                if (R.branch == 0) continue;
            }
            for (int c = 0; c < R.n_cons; ++c) {
                const int ch = R.branch == 1 ? R.chain[c] : R.chain[0];
                const int cc = R.branch == 1 ? 0 : c; // consensus index inside the chain
                const PoaChain &pc = b->pchains[ch]; const PoaChainOut &co = b->couts[ch];
                if (what == 1) {
                    WfaJob wj; wj.p_off = in_base + R.ref_off; wj.plen = R.ref_len; wj.t_off = pc.out_off + (uint64_t)cc * pc.node_cap; wj.tlen = co.cons_len[cc];
                    wj.gap_aln = b->opt.gap_aln; wj.want = 2; wj.s_cap = wfa_default_scap(wj.plen, wj.tlen); wj.ws_off = wj.ws_bytes = wj.out_off = 0;
                    b->rc_jobs.push_back(wj); b->rc_region.push_back((int)ri); b->rc_clu.push_back(c);
                    continue;
                }
                const uint64_t msa0 = pc.out_off + 2ull * pc.node_cap;
                const uint64_t cons_row = msa0 + (uint64_t)(pc.n_reads + cc) * pc.node_cap;
                const int nk = R.branch == 1 ? pc.n_reads : co.clu_n[cc];
                for (int kk = 0; kk < nk; ++kk) {
                    StrJob sj; sj.member_addr = 0; sj.row0 = 0; sj.row_stride = 0; sj.cons_off = cons_row; sj.msa_len = co.msa_len; sj.out_off = str_tot; str_tot += lcd_align_up((uint64_t)2 * co.msa_len + 16, 16);
                    if (R.branch == 1) { sj.read_off = msa0 + (uint64_t)kk * pc.node_cap; sj.full_cover = R.reads[b->chains[ch].members[kk]].cover; }
                    else { // K2: row of the kk-th member of cluster cc, resolved on the device from the chain's cluster list (the host copy
                           // of the lists is fetched by lcd_batch_download)
                        const uint64_t clu_addr = pc.out_off + lcd_align_up((uint64_t)(pc.n_reads + 4) * pc.node_cap, 16);
                        sj.read_off = 0; sj.member_addr = clu_addr + ((uint64_t)cc * pc.n_reads + kk) * 4; sj.row0 = msa0; sj.row_stride = pc.node_cap;
                        sj.full_cover = R.reads[c].cover; /* fully_covers[cluster] quirk, src/align.c:1194 */
                    }
                    b->str_jobs.push_back(sj); b->str_region.push_back((int)ri); b->str_clu.push_back(c); b->str_k.push_back(kk);
                }
            }
        }
        if (what == 1) b->reg_rc0[b->regs.size()] = (uint32_t)b->rc_jobs.size();
        else { b->reg_str0[b->regs.size()] = (uint32_t)b->str_jobs.size(); str_tots[k] = str_tot; }
    }
    // the joint ref<->cons job table.  Reads: the batches' couts / pchains.  Writes: the batches' rc tables and region statistics (teams), rc_base, rc_all; ev[3] on st.
    // Calling thread, with one team
    int refcons_jobs() {
        over_batches(2 * host_team(env), [&](const int k) { build_jobs(k, 1); });
        for (int k = 0; k < nb; ++k) rc_base[k + 1] = rc_base[k] + bs[k]->rc_jobs.size();
        if (rc_all.capacity() < rc_base[nb]) rc_all.reserve(rc_base[nb] + rc_base[nb] / 4 + 64); // (headroom: the next submission's tables are a few per cent larger or smaller)
        rc_all.resize(rc_base[nb]);
        for (int k = 0; k < nb; ++k) if (!bs[k]->rc_jobs.empty()) memcpy(rc_all.data() + rc_base[k], bs[k]->rc_jobs.data(), bs[k]->rc_jobs.size() * sizeof(WfaJob));
        if (env.time_host) fprintf(stderr, "[host] job table of the WFA stage: %.1f ms (%zu jobs)\n", now_ms() - th0, rc_all.size());
        HIPCHK(hipEventRecord(L->ev[3], st));
        return 0;
    }
    // the string jobs (670 000 per 20 batches; appended serially into fresh vectors their tables were 15 - 25 ms of a 300 ms submission with the GPU idle): per batch on
    // host threads, the joint table sized once and filled by the same threads, the batches' output blocks given their device memory in between.
    // Reads: the batches' couts / pchains / regs.  Writes: the batches' str tables, d_final, final_bytes, str_tots, str_base, str_all.  The thread of strings_stage, with two teams
    int build_string_tables() {
        over_batches(2 * host_team(env), [&](const int k) { build_jobs(k, 2); });
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k]; const uint64_t str_tot = str_tots[k];
            if (!b->str_jobs.empty() && b->d_final.ensure(str_tot)) return -11;
            b->final_bytes = str_tot;
            str_base[k + 1] = str_base[k] + b->str_jobs.size();
        }
        if (str_all.capacity() < str_base[nb]) str_all.reserve(str_base[nb] + str_base[nb] / 4 + 64);
        str_all.resize(str_base[nb]);
        over_batches(2 * host_team(env), [&](const int k) {
            lcd_batch_t *b = bs[k];
            const uint64_t fin = b->d_final.addr();
            for (auto &j : b->str_jobs) j.out_off += fin;
            if (!b->str_jobs.empty()) memcpy(str_all.data() + str_base[k], b->str_jobs.data(), b->str_jobs.size() * sizeof(StrJob));
        });
        return 0;
    }
    // S4 (MSA rows -> strings) needs the chains' outputs only, not the ref<->cons alignments: it runs BESIDE S3 -- its 37 MB job table (670 000 jobs of a 20-batch
    // submission) goes up from a helper thread on a side stream while the calling thread plans and launches the WFA classes (one after the other they were 8 + 4 ms, the
    // table's pageable upload alone 2 ms of the calling thread).  LCD_STRINGS_SEQ=1: after S3 on the leader's stream, as before.
    // Reads: what build_string_tables reads.  Writes: what it writes, str_outs, the leader's d_str_jobs / d_str_outs; table, kernel and download on s2 (not synchronised
    // here).  Strings thread with s2 = side[3]; LCD_STRINGS_SEQ: calling thread with s2 = st
    int strings_stage(hipStream_t s2) {
        if (const int rcb = build_string_tables()) return rcb;
        if (str_outs.capacity() < str_all.size()) str_outs.reserve(str_all.size() + str_all.size() / 4 + 64);
        str_outs.resize(str_all.size());
        if (str_all.empty()) return 0;
        if (L->d_str_jobs.ensure(str_all.size() * sizeof(StrJob)) || L->d_str_outs.ensure(str_all.size() * sizeof(StrOut))) return -11;
        HIPCHK(hipMemcpyAsync(L->d_str_jobs.p, str_all.data(), str_all.size() * sizeof(StrJob), hipMemcpyHostToDevice, s2));
        lcd_launch_strings((const StrJob *)L->d_str_jobs.p, nullptr, (StrOut *)L->d_str_outs.p, (int)str_all.size(), s2);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(str_outs.data(), L->d_str_outs.p, str_all.size() * sizeof(StrOut), hipMemcpyDeviceToHost, s2));
        return 0;
    }
    // starts the strings thread (side[3] waits for ev[3]); it synchronises side[3] itself.  Until join_strings the calling thread touches none of what strings_stage
    // writes.  Writes: strings_beside; the thread writes strings_rc / strings_err.  Calling thread
    int start_strings() {
        strings_beside = L->side[3] && !env.strings_seq;
        if (!strings_beside) return 0;
        HIPCHK(hipStreamWaitEvent(L->side[3], L->ev[3], 0));
        const int dev_here = cur_device();
        strings_thread.t = std::thread([this, dev_here]() {
            if (hipSetDevice(dev_here) != hipSuccess) { strings_rc = -1; return; }
            strings_rc = strings_stage(L->side[3]);
            if (strings_rc) strings_err = g_err;
            if (!strings_rc && hipStreamSynchronize(L->side[3]) != hipSuccess) strings_rc = -1;
        });
        return 0;
    }
    // the ref<->cons WFA stage.  Reads: rc_all, rc_base.  Writes: rc_all (planned jobs), the batches' rc_jobs / rc_outs and WFA statistics; the WFA classes on st
    // and side[0..2] (LCD_WFA_SEQ: st alone), ev[4] on st; synchronises st per WFA round.  Calling thread, beside the strings thread
    int wfa_stage() {
        int wret = 0;
        std::vector<WfaOut> rc_outs;
        int rc = run_wfa_stage(st, rc_all, L->d_wfa_jobs, L->d_poa_arena, L->d_wfa_out, L->d_wfa_outs, rc_outs, sc, env, &wret, false, env.wfa_seq ? nullptr : L->side, L->sev, 3); // (the POA streams are idle by now)
        if (rc) return rc;
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k];
            b->rc_jobs.assign(rc_all.begin() + rc_base[k], rc_all.begin() + rc_base[k + 1]);
            b->rc_outs.assign(rc_outs.begin() + rc_base[k], rc_outs.begin() + rc_base[k + 1]);
            b->st.n_wfa_jobs += (int)b->rc_jobs.size();
            for (auto &w : b->rc_outs) b->st.wfa_offsets += w.offsets;
        }
        HIPCHK(hipEventRecord(L->ev[4], st));
        return 0;
    }
    // the strings stage's end: the join of its thread (its error text comes over with it), or the stage itself in line.  Writes: ev[5] on st; synchronises st.  Calling thread
    int join_strings() {
        if (strings_beside) { if (strings_thread.t.joinable()) strings_thread.t.join(); if (strings_rc) return strings_rc == -11 ? set_err(-11, strings_err.empty() ? "device memory budget (strings stage)" : strings_err) : set_err(-20, "strings stage failed on its side stream" + (strings_err.empty() ? std::string() : ": " + strings_err)); }
        else { const int rcs = strings_stage(st); if (rcs) return rcs; }
        HIPCHK(hipEventRecord(L->ev[5], st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }

    // ---------------- S5 (only with opt.collect_ref_read_aln_str): ref<->read strings, src/align.c:1056-1146 ----------------
    // Reads: the batches' rc / str tables, str_outs, str_base.  Writes: the batches' rr_* tables and d_rr, the leader's compose buffers; compose kernels and one WFA stage
    // on st, synchronised.  Calling thread
    int compose_ref_read() {
        for (int k = 0; k < nb; ++k) { bs[k]->rr_off.clear(); bs[k]->rr_len.clear(); bs[k]->rr_stride.clear(); bs[k]->rr_bytes = 0; }
        if (!(L->opt.collect_ref_read_aln_str && !str_all.empty())) return 0;
        std::vector<CmpJob> cj(str_all.size());
        uint64_t seg_tot = 0;
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k];
            std::map<std::pair<int, int>, size_t> rc_of;
            for (size_t i = 0; i < b->rc_jobs.size(); ++i) rc_of[{b->rc_region[i], b->rc_clu[i]}] = i;
            uint64_t rr_tot = 0;
            b->rr_off.resize(b->str_jobs.size()); b->rr_len.assign(b->str_jobs.size(), 0); b->rr_stride.resize(b->str_jobs.size());
            for (size_t j = 0; j < b->str_jobs.size(); ++j) {
                const size_t r = rc_of.at({b->str_region[j], b->str_clu[j]});
                const WfaJob &wj = b->rc_jobs[r]; const StrJob &sj = b->str_jobs[j]; const StrOut &so = str_outs[str_base[k] + j];
                CmpJob &c = cj[str_base[k] + j];
                c.rc_t = wj.out_off; c.rc_q = wj.out_off + (uint64_t)(wj.plen + wj.tlen + 1); c.rc_len = b->rc_outs[r].aln_len;
                c.cr_t = sj.out_off + so.shift; c.cr_q = sj.out_off + sj.msa_len + so.shift; c.cr_len = so.aln_len > 0 ? so.aln_len : 0;
                c.seg_cap = (std::min(c.rc_len, c.cr_len) + 1) / 2 + 1; c.seg_off = seg_tot * 16; seg_tot += c.seg_cap; c.seg_first = 0;
                b->rr_stride[j] = c.rc_len + c.cr_len; b->rr_off[j] = rr_tot; rr_tot += lcd_align_up(2ull * (c.rc_len + c.cr_len) + 16, 16);
            }
            if (b->d_rr.ensure(rr_tot + 64)) return -11;
            b->rr_bytes = rr_tot;
            for (size_t j = 0; j < b->str_jobs.size(); ++j) cj[str_base[k] + j].out_off = b->d_rr.addr() + b->rr_off[j];
        }
        if (L->d_cmp_jobs.ensure(cj.size() * sizeof(CmpJob)) || L->d_cmp_outs.ensure(cj.size() * sizeof(CmpOut)) || L->d_cmp_seg.ensure(seg_tot * 16 + 64)) return -11;
        for (auto &c : cj) c.seg_off += L->d_cmp_seg.addr();
        HIPCHK(hipMemcpyAsync(L->d_cmp_jobs.p, cj.data(), cj.size() * sizeof(CmpJob), hipMemcpyHostToDevice, st));
        lcd_launch_compose((const CmpJob *)L->d_cmp_jobs.p, (CmpOut *)L->d_cmp_outs.p, nullptr, (int)cj.size(), 0, st);
        HIPCHK(hipGetLastError());
        std::vector<CmpOut> co(cj.size());
        std::vector<int> hseg(seg_tot * 4);
        HIPCHK(hipMemcpyAsync(co.data(), L->d_cmp_outs.p, cj.size() * sizeof(CmpOut), hipMemcpyDeviceToHost, st));
        if (seg_tot) HIPCHK(hipMemcpyAsync(hseg.data(), L->d_cmp_seg.p, seg_tot * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // the both-gap segments become one WFA stage (their rows go to a buffer of their own: d_wfa_out still holds the ref<->cons rows)
        std::vector<WfaJob> sj2; std::vector<CmpSeg> sres;
        for (size_t i = 0; i < cj.size(); ++i) {
            if (co[i].n_seg > cj[i].seg_cap) return set_err(-22, "ref<->read composition: segment list overflow");
            cj[i].seg_first = (int)sj2.size();
            const int *sg = hseg.data() + (cj[i].seg_off - L->d_cmp_seg.addr()) / 4;
            for (int q = 0; q < co[i].n_seg; ++q) {
                WfaJob w; w.p_off = cj[i].rc_t + sg[4 * q]; w.plen = sg[4 * q + 1]; w.t_off = cj[i].cr_q + sg[4 * q + 2]; w.tlen = sg[4 * q + 3];
                w.gap_aln = L->opt.gap_aln; w.want = 2; w.s_cap = wfa_default_scap(w.plen, w.tlen); w.ws_off = w.ws_bytes = w.out_off = 0;
                sj2.push_back(w);
            }
        }
        if (!sj2.empty()) {
            std::vector<WfaOut> so2;
            int rc2 = run_wfa_stage(st, sj2, L->d_wfa_jobs, L->d_poa_arena, L->d_seg_out, L->d_wfa_outs, so2, sc, env, nullptr);
            if (rc2) return rc2;
            sres.resize(sj2.size());
            for (size_t q = 0; q < sj2.size(); ++q) { sres[q].rows_off = sj2[q].out_off; sres[q].aln_len = so2[q].aln_len; sres[q].row_stride = sj2[q].plen + sj2[q].tlen + 1; }
            if (L->d_cmp_segres.ensure(sres.size() * sizeof(CmpSeg))) return -11;
            HIPCHK(hipMemcpyAsync(L->d_cmp_segres.p, sres.data(), sres.size() * sizeof(CmpSeg), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(L->d_cmp_jobs.p, cj.data(), cj.size() * sizeof(CmpJob), hipMemcpyHostToDevice, st));
        }
        lcd_launch_compose((const CmpJob *)L->d_cmp_jobs.p, (CmpOut *)L->d_cmp_outs.p, (const CmpSeg *)L->d_cmp_segres.p, (int)cj.size(), 1, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(co.data(), L->d_cmp_outs.p, cj.size() * sizeof(CmpOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < nb; ++k) for (size_t j = 0; j < bs[k]->str_jobs.size(); ++j) bs[k]->rr_len[j] = co[str_base[k] + j].aln_len;
        return 0;
    }

    // ---------------- S6 (opt.collect_noisy_vars): strings -> candidate variants + read x variant profile, SURVEY 8(f) f1 ----------------
    // make_vars_from_msa_cons_aln, src/collect_var.c:2279: the strings are still in HBM; only variants and alleles go back to the host.
    // Reads: rc_all, rc_base, str_base, the batches' rc / str tables.  Writes: the batches' vregs / vreg_of / d_var_out / var_bytes, the leader's variant buffers,
    // ms_vars; ev[6] and ev[7] on st (re-used: the POA rounds are over), synchronised.  Calling thread
    int candidate_vars() {
        for (int k = 0; k < nb; ++k) { bs[k]->vregs.clear(); bs[k]->vreg_of.assign(bs[k]->regs.size(), -1); bs[k]->var_bytes = 0; }
        if (!(L->opt.collect_noisy_vars && !rc_all.empty())) return 0;
        HIPCHK(hipEventRecord(L->ev[6], st));
        const size_t nj = rc_all.size();
        std::vector<VarScanJob> vj(nj); std::vector<VarScanOut> vo(nj);
        if (const int rc = scan_vars(vj, vo)) return rc;
        std::vector<VarRegJob> rj; std::vector<std::pair<int, int>> rj_owner;
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k];
            const size_t nk = b->regs.size() * 2; // (region, cluster) -> ref<->cons job, first string job, number of string jobs
            std::vector<int> rc_of(nk, -1), str_first(nk, 0), str_n(nk, 0);
            for (size_t i = 0; i < b->rc_jobs.size(); ++i) rc_of[(size_t)b->rc_region[i] * 2 + b->rc_clu[i]] = (int)i;
            for (size_t j = 0; j < b->str_jobs.size(); ++j) {
                const size_t key = (size_t)b->str_region[j] * 2 + b->str_clu[j];
                if (!str_n[key]) str_first[key] = (int)j;
                str_n[key]++;
            }
            uint64_t tot = 0;
            for (size_t ri = 0; ri < b->regs.size(); ++ri) {
                const RegionRec &R = b->regs[ri];
                if (R.n_cons <= 0) continue;
                VarRegJob J; memset(&J, 0, sizeof(J)); VarRegionRec V; memset(&V, 0, sizeof(V));
                J.n_cons = R.n_cons; V.region = (int)ri; V.n_cons = R.n_cons;
                int cap = 0, cols = 0, rows = 0;
                for (int c = 0; c < R.n_cons; ++c) {
                    const size_t key = ri * 2 + c;
                    if (rc_of[key] < 0) return set_err(-23, "candidate variants: a resolved region has no ref<->cons string");
                    const size_t g = rc_base[k] + rc_of[key];
                    J.rec[c] = vj[g].rec_off; J.cons[c] = vj[g].work_off + vj[g].row_cap; J.n_rec[c] = vo[g].n_vars;
                    J.rc_t[c] = vj[g].rc_t; J.rc_q[c] = vj[g].rc_q; J.rc_len[c] = vj[g].rc_len;
                    J.n_rows[c] = str_n[key]; J.str_first[c] = (int)(str_base[k] + str_first[key]);
                    V.rows[c] = J.n_rows[c]; cap += vo[g].n_vars; cols += vo[g].n_cols; rows += J.n_rows[c];
                }
                V.cap = cap;
                V.rec_off = tot; tot += lcd_align_up((uint64_t)cap * sizeof(VarRec) + 16, 16);
                V.alt_off = tot; tot += lcd_align_up((uint64_t)cols + 16, 16);
                V.prof_off = tot; tot += lcd_align_up((uint64_t)rows * cap + 16, 16);
                V.se_off = tot; tot += lcd_align_up((uint64_t)rows * 8 + 16, 16);
                b->vreg_of[ri] = (int)b->vregs.size(); b->vregs.push_back(V);
                rj.push_back(J); rj_owner.push_back({k, (int)b->vregs.size() - 1});
            }
            if (b->d_var_out.ensure(tot + 64)) return -11;
            b->var_bytes = tot;
        }
        for (size_t q = 0; q < rj.size(); ++q) {
            lcd_batch_t *b = bs[rj_owner[q].first]; const VarRegionRec &V = b->vregs[rj_owner[q].second]; const uint64_t base = b->d_var_out.addr();
            rj[q].out_rec = base + V.rec_off; rj[q].out_alt = base + V.alt_off; rj[q].out_prof = base + V.prof_off; rj[q].out_se = base + V.se_off;
        }
        if (rj.empty()) return 0;
        if (L->d_vreg_jobs.ensure(rj.size() * sizeof(VarRegJob)) || L->d_vreg_outs.ensure(rj.size() * sizeof(VarRegOut))) return -11;
        HIPCHK(hipMemcpyAsync(L->d_vreg_jobs.p, rj.data(), rj.size() * sizeof(VarRegJob), hipMemcpyHostToDevice, st));
        lcd_launch_vars_profile((const VarRegJob *)L->d_vreg_jobs.p, (VarRegOut *)L->d_vreg_outs.p, (const StrJob *)L->d_str_jobs.p, (const StrOut *)L->d_str_outs.p, (int)rj.size(), st);
        HIPCHK(hipGetLastError());
        std::vector<VarRegOut> ro(rj.size());
        HIPCHK(hipMemcpyAsync(ro.data(), L->d_vreg_outs.p, rj.size() * sizeof(VarRegOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(L->ev[7], st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t q = 0; q < rj.size(); ++q) { VarRegionRec &V = bs[rj_owner[q].first]->vregs[rj_owner[q].second]; V.n_vars = ro[q].n_vars; V.alt_bytes = ro[q].alt_bytes; }
        hipEventElapsedTime(&ms_vars, L->ev[6], L->ev[7]);
        return 0;
    }
    // S6's scan of every ref<->cons string: pass 0 counts the variants of every consensus, pass 1 writes the records into exactly sized lists.  Reads: the batches'
    // rc_jobs / rc_outs, rc_base.  Writes: vj, vo, the leader's d_var_jobs / d_var_outs / d_var_work; both launches on st, one synchronisation.  Calling thread
    int scan_vars(std::vector<VarScanJob> &vj, std::vector<VarScanOut> &vo) {
        const size_t nj = vj.size();
        uint64_t work_tot = 0;
        for (int k = 0; k < nb; ++k) for (size_t i = 0; i < bs[k]->rc_jobs.size(); ++i) {
            const WfaJob &wj = bs[k]->rc_jobs[i]; VarScanJob &v = vj[rc_base[k] + i];
            v.rc_t = wj.out_off; v.rc_q = wj.out_off + (uint64_t)(wj.plen + wj.tlen + 1); v.rc_len = bs[k]->rc_outs[i].aln_len;
            v.row_cap = (int)lcd_align_up((uint64_t)v.rc_len + 16, 16); v.work_off = work_tot; work_tot += 2ull * v.row_cap; v.rec_off = 0; v.rec_cap = 0; v.pad = 0;
        }
        if (L->d_var_jobs.ensure(nj * sizeof(VarScanJob)) || L->d_var_outs.ensure(nj * sizeof(VarScanOut)) || L->d_var_work.ensure(work_tot + 64)) return -11;
        for (auto &v : vj) v.work_off += L->d_var_work.addr();
        for (int pass = 0; pass < 2; ++pass) {
            HIPCHK(hipMemcpyAsync(L->d_var_jobs.p, vj.data(), nj * sizeof(VarScanJob), hipMemcpyHostToDevice, st));
            lcd_launch_vars_scan((const VarScanJob *)L->d_var_jobs.p, (VarScanOut *)L->d_var_outs.p, (int)nj, st);
            HIPCHK(hipGetLastError());
            if (pass == 1) break;
            HIPCHK(hipMemcpyAsync(vo.data(), L->d_var_outs.p, nj * sizeof(VarScanOut), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            uint64_t rec_tot = 0;
            for (size_t g = 0; g < nj; ++g) { vj[g].rec_cap = vo[g].n_vars; vj[g].rec_off = rec_tot; rec_tot += (uint64_t)vo[g].n_vars * sizeof(VarRec); }
            // the per-consensus lists live behind the compacted rows in the leader's work buffer (transient: consumed by the profile kernel;
            // ensure() may move the buffer -- nothing in it is live yet, pass 1 rewrites the rows)
            const uint64_t rec_base = lcd_align_up(work_tot + 64, 64);
            if (L->d_var_work.ensure(rec_base + rec_tot + 64)) return -11;
            uint64_t wo = 0;
            for (size_t g = 0; g < nj; ++g) { vj[g].work_off = L->d_var_work.addr() + wo; wo += 2ull * vj[g].row_cap; vj[g].rec_off += L->d_var_work.addr() + rec_base; }
        }
        return 0;
    }

    // ---- final statistics and the gather of the scattered result pieces.  Reads: the events ev[0..5], ms_vars, str_outs, str_base, the batches' couts.  Writes: the
    // batches' str_outs, stage times and POA totals, ran / downloaded / gathered; the gather launch on st, synchronised.  Calling thread ----
    int finish() {
        float ms_anchor = 0, ms_poa = 0, ms_wfa = 0, ms_str = 0, ms_tot = 0;
        hipEventElapsedTime(&ms_anchor, L->ev[0], L->ev[1]); hipEventElapsedTime(&ms_poa, L->ev[1], L->ev[2]);
        hipEventElapsedTime(&ms_wfa, L->ev[3], L->ev[4]); hipEventElapsedTime(&ms_str, L->ev[4], L->ev[5]); hipEventElapsedTime(&ms_tot, L->ev[0], L->ev[5]);
        const double host_ms = (now_ms() - t_begin) - ms_tot;
        for (int k = 0; k < nb; ++k) {
            lcd_batch_t *b = bs[k]; lcd_batch_stats_t &S = b->st;
            b->str_outs.assign(str_outs.begin() + str_base[k], str_outs.begin() + str_base[k + 1]);
            // stage times are those of the joint run (the same for every batch of the call)
            S.ms_anchor = ms_anchor; S.ms_poa = ms_poa; S.ms_wfa = ms_wfa; S.ms_strings = ms_str; S.ms_total = ms_tot + ms_vars; S.ms_host = host_ms - ms_vars; S.ms_vars = ms_vars;
            for (const PoaChainOut &o : b->couts) {
                S.poa_aligned_bases += o.aligned_bases; S.poa_cells += o.cells_alg; S.poa_cells_computed += o.cells;
                // B_poa = q + 5*N_sub + C + (q + N_sub) per aligned read; N_sub ~ final graph size (upper bound per read)
                S.poa_alg_bytes += 2 * o.aligned_bases + o.cells_alg + 6ull * (uint64_t)o.n_node * (uint64_t)o.n_aligned_reads;
            }
            b->ran = true; b->downloaded = false; b->gathered = false;
        }
        if (int rc = stage_gather_many(bs, nb, st)) return rc;
        if (env.mem_debug) fprintf(stderr, "[mem] device buffers of this process after the submission: %.2f GB (budget %.2f GB)\n", g_dev_bytes[L->device].load() / 1e9, dev_budget(L->device) / 1e9);
        if (env.placement) report_placement(*this);
        if (env.chain_times) report_chain_times(*this);
        if (env.profile_chains) report_profile_chains(*this);
        return 0;
    }
};

// ---- diagnostics of a submission: they read it and print; tools parse these lines (tools/occupancy.py and the tools that set LCD_PROFILE_CHAINS) ----
// LCD_MEM_DEBUG, per round: the arena layout and what it is made of
static void report_round_memory(const Submission &S, const PoaRound &R) {
    const ArenaPlan &P = R.P; const std::vector<size_t> &which = S.which;
    fprintf(stderr, "[mem] round %d arenas: %zu chains in %zu slot pools (%.2f GB), %zu with private arenas (%.2f GB)\n", R.round, P.n_pooled, P.n_pools, P.pool_bytes / 1e9, which.size() - P.n_pooled, P.private_bytes / 1e9);
    double cellb = 0, nodeb = 0; double worstc = 0; size_t nbig = 0;
    for (size_t i = 0; i < which.size(); ++i) { const PoaChain &pc = S.chain(which[i]); cellb += (pc.spill_x > 2 ? 5.0 + pc.spill_x : 4.0) * pc.cell_cap; PoaLayout Lay = poa_layout(pc.node_cap, pc.edge_cap, pc.rid_words, pc.max_len, 0, pc.n_reads); nodeb += (double)Lay.total; if (4.0 * pc.cell_cap > worstc) worstc = 4.0 * pc.cell_cap; nbig += 4.0 * pc.cell_cap > 64e6; }
    fprintf(stderr, "[mem] round %d: %zu chains, arena %.2f GB = DP regions %.2f GB (largest %.1f MB, %zu above 64 MB) + graph/plan arrays %.2f GB\n", R.round, which.size(), P.tot / 1e9, cellb / 1e9, worstc / 1e6, nbig, nodeb / 1e9);
}
// LCD_MEM_DEBUG, per round after the verdicts: certified bands, LCD_CERT_DEBUG / LCD_RETRY_DEBUG per chain, overflows by kind (S.which is still the round's set)
static void report_round_retries(const Submission &S, const PoaRound &R) {
    const int round = R.round; const std::vector<size_t> &which = S.which, &again = R.again; const PoaChainOut *const tmp = R.tmp;
    { size_t nc = 0; for (size_t g : which) nc += S.chain(g).cert != 0; fprintf(stderr, "[mem] round %d: %zu chains with a certified band, %zu sent back for full rows\n", round, nc, R.n_cert_fail); }
    if (S.env.cert_debug) for (size_t i = 0; i < which.size(); ++i) { const PoaChain &pc = S.chain(which[i]); if (!pc.cert) continue; const int k = S.chain_batch[which[i]];
        std::vector<int> ls; for (int r = 0; r < pc.n_reads; ++r) ls.push_back(S.preads[k][pc.read0 + r].len); std::sort(ls.begin(), ls.end());
        fprintf(stderr, "[cert] %s n %d max %d p75 %d med %d p25 %d min %d nodes %d\n", tmp[i].status == LCD_ERR_CERT ? "FAIL" : "ok  ", pc.n_reads, ls.back(), ls[ls.size() * 3 / 4], ls[ls.size() / 2], ls[ls.size() / 4], ls[0], tmp[i].n_node); if (tmp[i].status == LCD_ERR_CERT) fprintf(stderr, "[cert]    why %llu  attempt/qlen %llu  aligned reads %d hist?\n", tmp[i].t_plan, tmp[i].t_poll, tmp[i].n_aligned_reads); }
    if (S.env.retry_debug) for (size_t g : again) { const PoaChain &pc = S.chain(g); const PoaChainOut &o = S.out(g);
        fprintf(stderr, "[retry] round %d status %d: thr %d mode %d reads %d maxlen %d | caps nodes %d edges %d cells %llu (worst %llu) spill_x %d | reached nodes %d edges %d aligned reads %d cells %llu\n", round, o.status,
                chain_threads(pc), pc.mode, pc.n_reads, pc.max_len, pc.node_cap, pc.edge_cap, (unsigned long long)pc.cell_cap, (unsigned long long)pc.node_cap * (pc.max_len + 1), pc.spill_x, o.n_node, o.n_edge, o.n_aligned_reads, o.cells); }
    int c[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (size_t g : again) { const PoaChainOut &o = S.out(g); c[S.chain(g).mode ? 1 : 0][o.status == LCD_ERR_CELLS ? 0 : o.status == LCD_ERR_NODES ? 1 : 2]++; }
    { std::map<int, std::pair<int, int>> byc; for (size_t g : which) if (S.chain(g).mode) byc[chain_threads(S.chain(g))].second++; for (size_t g : again) if (S.chain(g).mode) byc[chain_threads(S.chain(g))].first++;
      for (auto &kv : byc) fprintf(stderr, "[mem]   K2 class %4d: %d of %d overflow\n", kv.first, kv.second.first, kv.second.second); }
    fprintf(stderr, "[mem] round %d overflows: K1 cells %d nodes %d edges %d | K2 cells %d nodes %d edges %d (hints: cells %d/%d nodes %d)\n", round, c[0][0], c[0][1], c[0][2], c[1][0], c[1][1], c[1][2],
            g_cell_hint[0].load(), g_cell_hint[1].load(), g_node_hint.load());
}
// LCD_DUMP_CHAIN: the failing chain's reads, for a replay in isolation (tools/replay_chain.py): header, then per read {len, skip, anchors, bases}
static void dump_failed_chain(const Submission &S, const size_t g, const int status) {
    const PoaChain &pc = S.chain(g);
    FILE *f = fopen(S.env.dump_chain, "wb");
    if (!f) return;
    const int hdr[8] = {0x4c434443, pc.mode, pc.n_reads, status, pc.threads, pc.wmax, pc.ring_k, pc.lds_words * 4};
    fwrite(hdr, sizeof(int), 8, f);
    const std::vector<PoaRead> &pr = S.preads[S.chain_batch[g]];
    for (int q = 0; q < pc.n_reads; ++q) {
        const PoaRead &r = pr[pc.read0 + q];
        const int rec[6] = {r.len, r.skip, r.ref_beg, r.ref_end, r.read_beg, r.read_end};
        fwrite(rec, sizeof(int), 6, f);
        std::vector<uint8_t> bases((size_t)std::max(r.len, 0));
        if (r.len > 0) (void)hipMemcpy(bases.data(), (const void *)(uintptr_t)r.seq_off, (size_t)r.len, hipMemcpyDeviceToHost);
        fwrite(bases.data(), 1, bases.size(), f);
    }
    fclose(f);
}
// the error text of a chain whose status ends the submission (o: its record of the round at hand)
static std::string failed_chain_text(const Submission &S, const size_t g, const PoaChainOut &o) {
    const PoaChain &pc = S.chain(g); const int k = S.chain_batch[g];
    return "POA kernel status " + std::to_string(o.status) + " on chain " + std::to_string(g - S.chain_base[k]) + " of batch " + std::to_string(k) + " (mode " + std::to_string(pc.mode) +
           ", " + std::to_string(pc.n_reads) + " reads, longest " + std::to_string(pc.max_len) + ", threads " + std::to_string(pc.threads) + ", window " + std::to_string(pc.wmax) + ", ring slots " +
           std::to_string(pc.ring_k) + ", LDS " + std::to_string(pc.lds_words * 4) + " B, nodes " + std::to_string(o.n_node) + "/" + std::to_string(pc.node_cap) + ", reads aligned " + std::to_string(o.n_aligned_reads) + ")" +
           (o.status == LCD_ERR_WATCHDOG ? [&] { std::string t = "; last backtrack states (row, column, state):"; const unsigned long long w[4] = {o.t_plan, o.t_poll, o.t_bp, o.t_add};
                for (int q = 0; q < 4; ++q) t += " (" + std::to_string((unsigned)(w[q] & 0xffffffffu)) + ", " + std::to_string((unsigned)((w[q] >> 32) & 0xffffff)) + ", " + std::to_string((unsigned)(w[q] >> 56)) + ")"; return t; }() : std::string());
}
// LCD_PLACEMENT, experiment: which CU did every wide chain run on, and when
static void report_placement(const Submission &S) {
    for (size_t g = 0; g < S.nC_all; ++g) { if (chain_threads(S.chain(g)) < 512) continue; const PoaChainOut &o = S.out(g);
        fprintf(stderr, "[place] thr %d xcc %u se %u sh %u cu %u simd %u  t %.1f..%.1f ms ticks %.3e\n", chain_threads(S.chain(g)), o.xcc_id & 15, (o.hw_id >> 13) & 7, (o.hw_id >> 12) & 1, (o.hw_id >> 8) & 15, (o.hw_id >> 4) & 3,
                o.rt_begin / 1e5, o.rt_end / 1e5, (double)o.t_total); }
}
// LCD_CHAIN_TIMES=<file>: every chain's class, pool, start and end (100 MHz device clock, relative to the first start): tools/occupancy.py
static void report_chain_times(const Submission &S) {
    FILE *f = fopen(S.env.chain_times, "w");
    if (!f) return;
    unsigned long long t0 = ~0ull;
    for (size_t g = 0; g < S.nC_all; ++g) t0 = std::min(t0, S.out(g).rt_begin);
    for (size_t g = 0; g < S.nC_all; ++g) { const PoaChainOut &o = S.out(g); const PoaChain &pc = S.chain(g);
        fprintf(f, "%d %d %d %llu %llu %u %u %d %d %d %llu %llu %llu %llu %llu\n", pc.threads, pc.lds_words * 4, pc.mode, o.rt_begin - t0, o.rt_end - t0, o.xcc_id & 15, (o.hw_id >> 8) & 15, pc.max_len, pc.n_reads, pc.cert, (unsigned long long)o.t_setup,
                (unsigned long long)o.t_total, (unsigned long long)o.t_dp, (unsigned long long)o.cells, (unsigned long long)o.t_bt); }
    fclose(f);
}
// LCD_PROFILE_CHAINS: the tail, CU-seconds per launch group, ticks per kind of chain and per workgroup class
static void report_profile_chains(const Submission &S) {
    const size_t nC_all = S.nC_all;
    { // the chains that end last: the tail of the submission (times on the device's 100 MHz clock, relative to the first chain's start)
        std::vector<size_t> ord(nC_all); unsigned long long t0 = ~0ull;
        for (size_t g = 0; g < nC_all; ++g) { ord[g] = g; t0 = std::min(t0, S.out(g).rt_begin); }
        std::sort(ord.begin(), ord.end(), [&](size_t a, size_t c) { return S.out(a).rt_end > S.out(c).rt_end; });
        for (size_t q = 0; q < std::min<size_t>(10, ord.size()); ++q) { const size_t g = ord[q]; const PoaChainOut &o = S.out(g); const PoaChain &pc = S.chain(g);
            fprintf(stderr, "[tail] thr %4d lds %3dK mode %d reads %3d maxlen %5d nodes %6d: %.1f .. %.1f ms  (dp %.0f%% bt %.0f%% graph %.0f%% out %.0f%%)  cells %.2e\n", chain_threads(pc), pc.lds_words * 4 >> 10, pc.mode, pc.n_reads, pc.max_len, o.n_node,
                    (o.rt_begin - t0) / 1e5, (o.rt_end - t0) / 1e5, 100.0 * o.t_dp / o.t_total, 100.0 * o.t_bt / o.t_total, 100.0 * o.t_graph / o.t_total, 100.0 * o.t_out / o.t_total, (double)o.cells); }
    }
    { // CU-seconds per launch group: sum of chain ticks / workgroups that fit a CU (LDS- or register-limited: 128 VGPRs are 16 wavefronts per CU)
        std::map<long long, std::pair<double, int>> gsum;
        for (size_t g = 0; g < nC_all; ++g) { auto &e = gsum[chain_group_key(S.chain(g))]; e.first += (double)S.out(g).t_total; e.second++; }
        double tot = 0;
        for (auto &kv : gsum) {
            const int thr = (int)(kv.first >> 20), lds = (int)(kv.first & ((1 << 20) - 1)) * 4;
            const int per_cu = chains_per_cu(lds, thr, kSchedOverhead);
            const double cus = kv.second.first / 2.4e9 / per_cu; tot += cus;
            fprintf(stderr, "[lcd] group thr %4d lds %3dK: %6d chains, %7.2f wg-s, %2d per CU -> %7.2f CU-s\n", thr, lds >> 10, kv.second.second, kv.second.first / 2.4e9, per_cu, cus);
        }
        fprintf(stderr, "[lcd] total %.2f CU-s = %.1f ms of %d CUs\n", tot, tot / g_n_cus * 1e3, g_n_cus);
    }
    // per (class, kind of chain): ticks per phase and cells -- kind 0: K1 (adaptive band), 1: K2 full rows, 2: K2 certified band, +4: long-chain (solo) workgroup
    {
        struct Acc { double n = 0, tt = 0, td = 0, tb = 0, tbp = 0, tad = 0, tso = 0, tse = 0, tsub = 0, to = 0, cells = 0, reads = 0, rows = 0; };
        std::map<int, Acc> by;
        for (size_t g = 0; g < nC_all; ++g) { const PoaChain &pc = S.chain(g); const PoaChainOut &o = S.out(g);
            Acc &a = by[chain_threads(pc) * 8 + (pc.mode ? (pc.cert ? 2 : 1) : 0) + (pc.solo ? 4 : 0)];
            a.n += 1; a.tt += (double)o.t_total; a.td += (double)o.t_dp; a.tb += (double)o.t_bt; a.tbp += (double)o.t_bp; a.tad += (double)o.t_add; a.tso += (double)o.t_sort; a.tse += (double)o.t_setup;
            a.tsub += (double)o.t_sub; a.to += (double)o.t_out; a.cells += (double)o.cells; a.reads += o.n_aligned_reads; a.rows += (double)o.n_aligned_reads * o.n_node; }
        for (auto &kv : by) { const Acc &a = kv.second;
            fprintf(stderr, "[kind] thr %4d kind %d: %6.0f chains %8.0f reads  ticks total %.3e | dp %.1f%% bt %.1f%% plan %.1f%% update %.1f%% re-sort %.1f%% setup %.1f%% sub %.1f%% out %.1f%% | cells %.3e  ticks/cell(dp) %.2f  ~rows %.3e\n",
                    kv.first >> 3, kv.first & 7, a.n, a.reads, a.tt, 100 * a.td / a.tt, 100 * a.tb / a.tt, 100 * a.tbp / a.tt, 100 * a.tad / a.tt, 100 * a.tso / a.tt, 100 * a.tse / a.tt, 100 * a.tsub / a.tt, 100 * a.to / a.tt,
                    a.cells, a.td / std::max(1.0, a.cells), a.rows); }
    }
    // per-phase shader-clock ticks, summed per workgroup class and for the slowest chain
    for (int cls : {64, 128, 256, 512, 1024}) {
        unsigned long long tt = 0, td = 0, tb = 0, tg = 0, to = 0, ts = 0, mx = 0, tbp = 0, tad = 0, tso = 0, tse = 0, tpl = 0; int cnt = 0; size_t mxc = 0;
        for (size_t g = 0; g < nC_all; ++g) { if (chain_threads(S.chain(g)) != cls) continue; const PoaChainOut &o = S.out(g); ++cnt;
            tt += o.t_total; td += o.t_dp; tb += o.t_bt; tg += o.t_graph; to += o.t_out; ts += o.t_sub; tbp += o.t_bp; tad += o.t_add; tso += o.t_sort; tse += o.t_setup; tpl += o.t_plan; if (o.t_total >= mx) { mx = o.t_total; mxc = g; } }
        if (!cnt) continue;
        fprintf(stderr, "[lcd] class %4d: row plan %.3e  graph update %.3e  re-sort %.3e  row setup %.3e  bound arrays %.3e\n", cls, (double)tbp, (double)tad, (double)tso, (double)tse, (double)tpl);
        if ((S.env.dbg & 32)) { // reads of certified-band chains by their widest interval (the t_setup slot carries five 12-bit counters per chain)
            unsigned long long h[5] = {0, 0, 0, 0, 0};
            for (size_t g = 0; g < nC_all; ++g) { if (chain_threads(S.chain(g)) != cls || !S.chain(g).cert) continue; const unsigned long long v = S.out(g).t_setup; for (int q = 0; q < 5; ++q) h[q] += (v >> (12 * q)) & 4095; }
            fprintf(stderr, "[lcd] class %4d: certified-band reads by widest interval <= 60 / 124 / 188 / 256 / wider: %llu / %llu / %llu / %llu / %llu\n", cls, h[0], h[1], h[2], h[3], h[4]);
        }
        { double tk = 0; for (size_t g = 0; g < nC_all; ++g) if (chain_threads(S.chain(g)) == cls) tk += (double)S.out(g).t_poll;
          fprintf(stderr, "[lcd] class %4d: %5d chains  sum ticks total %.3e dp %.3e bt %.3e graph %.3e (of which serial Kahn walk %.3e) sub %.3e out %.3e\n", cls, cnt, (double)tt, (double)td, (double)tb, (double)tg, tk, (double)ts, (double)to); }
        const PoaChainOut &o = S.out(mxc); const PoaChain &pm = S.chain(mxc);
        fprintf(stderr, "[lcd]   slowest chain %zu: mode %d reads %d maxlen %d nodes %d  total %.3e dp %.3e bt %.3e graph %.3e sub %.3e out %.3e cells %llu\n", mxc, pm.mode,
                pm.n_reads, pm.max_len, o.n_node, (double)o.t_total, (double)o.t_dp, (double)o.t_bt, (double)o.t_graph, (double)o.t_sub, (double)o.t_out, o.cells);
        fprintf(stderr, "[lcd]     of its dp: plan-window refreshes %.3e  mailbox polls %.3e (one wavefront)\n", (double)o.t_plan, (double)o.t_poll);
        fprintf(stderr, "[lcd]     row plan %.3e  graph update %.3e  re-sort %.3e  row setup %.3e\n", (double)o.t_bp, (double)o.t_add, (double)o.t_sort, (double)o.t_setup);
        if ((S.env.dbg & 32)) fprintf(stderr, "[lcd]     reads by widest interval <=60 / <=124 / <=188 / <=380 / wider: %llu %llu %llu %llu %llu\n", (unsigned long long)(o.t_setup & 4095), (unsigned long long)((o.t_setup >> 12) & 4095), (unsigned long long)((o.t_setup >> 24) & 4095), (unsigned long long)((o.t_setup >> 36) & 4095), (unsigned long long)((o.t_setup >> 48) & 4095));
    }
}

} // namespace

// The driver: the stages of a submission in order.  The preparation thread runs beside begin's tail and the anchor stage, the strings thread beside the
// ref<->cons WFA stage; both are joined here, and by the submission's destructor on an early return.
static int run_many_once(lcd_batch_t **bs, int nb) {
    if (nb <= 0) return 0;
    if (const int rc = Submission::validate(bs, nb)) return rc;
    Submission S(bs, nb);
    lcd_batch_t *const L = S.L;
    if (const int rc = S.begin()) return rc;
    if (const int rc = S.start_prep()) return rc;       // prep_chains (+ prepare_round0) on the preparation thread
    if (const int rc = S.anchor_stage()) return rc;     // S1; joins the preparation thread before it narrows the reads
    if (const int rc = S.join_prep()) return rc;
    HIPCHK(hipEventRecord(L->ev[1], S.st));
    S.tp0 = now_ms();
    if (S.env.time_host) fprintf(stderr, "[host] anchor stage: %.1f ms on the host clock\n", S.tp0 - S.t_begin);
    if (const int rc = S.poa_stage()) return rc;        // S2: read table, round 0's plan, the rounds
    if (S.env.time_host) fprintf(stderr, "[host] POA stage ends %.1f ms after its start\n", now_ms() - S.tp0);
    HIPCHK(hipEventRecord(L->ev[2], S.st));
    S.th0 = now_ms();
    if (const int rc = S.refcons_jobs()) return rc;     // S3's job table
    if (const int rc = S.start_strings()) return rc;    // S4 on the strings thread
    if (const int rc = S.wfa_stage()) return rc;        // S3
    if (const int rc = S.join_strings()) return rc;     // S4's end (LCD_STRINGS_SEQ: S4 itself)
    if (const int rc = S.compose_ref_read()) return rc; // S5
    if (const int rc = S.candidate_vars()) return rc;   // S6
    return S.finish();
}

int lcd_batch_run(lcd_batch_t *b) { return lcd_batch_run_many(&b, 1); }

// ---- one process, every GPU of the node: per-device submitter threads pulling from ONE cost-ordered queue of job buffers ----
// The reference's parallel strategy is kt_for: n_threads workers of one process taking the next chunk whenever they are free (work stealing,
// src/kthread.c:24-64, src/call_var_main.c:773).  Here the workers are the GPUs: the batches (host-only job buffers, LCD_DEVICE_ANY) are ordered by
// estimated DP work, longest first, and every device thread takes the next `coalesce` of them whenever its previous submission is done --
// upload, lcd_batch_run_many, download.  Chunks are independent until stitch_var_main: no device ever talks to another.
struct lcd_dispatch_s { std::vector<int> devs; int coalesce; int flags = 0; std::vector<double> busy_ms; std::vector<int> n_sub; };
static double batch_cost(const lcd_batch_t *b) { // DP cells, roughly: K1 chains = reads x length x band, K2 chains = reads x length^2
    double c = 0;
    for (const ChainRec &C : b->chains) {
        double sum = 0, maxl = 0;
        for (size_t k = 0; k < C.members.size(); ++k) { const double l = b->preads[C.read0 + k].len; sum += l; maxl = std::max(maxl, l); }
        c += sum * (C.mode == 0 ? std::min(maxl + 1, 2 * (10 + maxl / 100) + 1 + 64) : maxl + 1);
    }
    return c;
}
lcd_dispatch_t *lcd_dispatch_create(int n_devices, const int *devices, int coalesce) {
    if (init_default_device()) return nullptr;
    lcd_dispatch_t *d = new lcd_dispatch_s();
    if (n_devices <= 0) { for (int i = 0; i < g_n_devices; ++i) d->devs.push_back(i); }
    else for (int i = 0; i < n_devices; ++i) {
        const int dev = devices ? devices[i] : i;
        if (dev < 0 || dev >= g_n_devices) { set_err(-1, "lcd_dispatch_create: bad device index " + std::to_string(dev)); delete d; return nullptr; }
        d->devs.push_back(dev);
    }
    d->coalesce = coalesce > 0 ? coalesce : 16;
    return d;
}
void lcd_dispatch_destroy(lcd_dispatch_t *d) { delete d; }
int lcd_dispatch_n_devices(const lcd_dispatch_t *d) { return (int)d->devs.size(); }
double lcd_batch_cost(const lcd_batch_t *b) { return batch_cost(b); }
// the deterministic part, also used by the tests and by the multi-process sharding of bench.py: longest-processing-time assignment of costs to bins
void lcd_lpt_assign(int n, const double *cost, int n_bins, int *bin_of, double *bin_load) {
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    std::vector<double> load(n_bins, 0.0);
    for (int i : order) { int best = 0; for (int t = 1; t < n_bins; ++t) if (load[t] < load[best]) best = t; bin_of[i] = best; load[best] += cost[i]; }
    if (bin_load) for (int t = 0; t < n_bins; ++t) bin_load[t] = load[t];
}
// flags: bit 0 = leave the results on the device (no lcd_batch_download after a submission: a caller that times the kernels, or one that takes variants only later)
void lcd_dispatch_set_flags(lcd_dispatch_t *d, int flags) { if (d) d->flags = flags; }
// per device of the dispatcher (in its device order): milliseconds its submitter thread spent inside submissions during the LAST lcd_dispatch_run, and how many it made
int lcd_dispatch_busy(const lcd_dispatch_t *d, double *busy_ms, int *n_submissions) {
    if (!d) return 0;
    for (size_t q = 0; q < d->busy_ms.size(); ++q) { if (busy_ms) busy_ms[q] = d->busy_ms[q]; if (n_submissions) n_submissions[q] = d->n_sub[q]; }
    return (int)d->busy_ms.size();
}
int lcd_dispatch_run(lcd_dispatch_t *d, lcd_batch_t **bs, int n, int *device_of) {
    if (n <= 0) return 0;
    for (int i = 0; i < n; ++i) {
        if (bs[i]->device >= 0 && std::find(d->devs.begin(), d->devs.end(), bs[i]->device) == d->devs.end()) return set_err(-4, "lcd_dispatch_run: a batch is bound to a device outside the dispatcher");
        if (memcmp(&bs[i]->opt, &bs[0]->opt, sizeof(lcd_opt_t)) != 0) return set_err(-4, "lcd_dispatch_run: batches with different options");
    }
    std::vector<int> order(n);
    std::vector<double> cost(n);
    for (int i = 0; i < n; ++i) { order[i] = i; cost[i] = batch_cost(bs[i]); }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    std::map<int, int> slot_of; for (size_t q = 0; q < d->devs.size(); ++q) slot_of[d->devs[q]] = (int)q;
    d->busy_ms.assign(d->devs.size(), 0.0); d->n_sub.assign(d->devs.size(), 0);
    std::mutex mu; size_t n_left = (size_t)n; int first_err = 0; std::string err_msg;
    std::vector<char> taken((size_t)n, 0);
    const int n_dev = (int)d->devs.size();
    auto worker = [&](int dev) {
        std::vector<lcd_batch_t *> grp;
        for (;;) {
            grp.clear();
            {
                std::lock_guard<std::mutex> lk(mu);
                if (first_err) return;
                // take, in cost order, up to `coalesce` batches that are free or bound to THIS device -- never more than this device's fair share of what is left
                // (the tail of the queue is what balances the devices).  A batch bound to another GPU of the dispatcher is skipped: its own thread takes it, and a
                // thread that finds nothing it may take is done (no waiting on another device's submission)
                const size_t take = std::max<size_t>(1, std::min<size_t>((size_t)d->coalesce, (n_left + n_dev - 1) / n_dev));
                for (size_t q = 0; q < (size_t)n && grp.size() < take; ++q) {
                    if (taken[q]) continue;
                    lcd_batch_t *b = bs[order[q]];
                    if (b->device >= 0 && b->device != dev) continue;
                    taken[q] = 1; --n_left;
                    grp.push_back(b); if (device_of) device_of[order[q]] = dev;
                }
            }
            if (grp.empty()) return;
            const double tw0 = now_ms();
            int rc = 0;
            for (lcd_batch_t *b : grp) { if (b->device < 0 && (rc = bind_batch(b, dev))) break; if (!b->uploaded && (rc = lcd_batch_upload(b))) break; }
            if (!rc) rc = lcd_batch_run_many(grp.data(), (int)grp.size());
            for (size_t i = 0; i < grp.size() && !rc && !(d->flags & 1); ++i) rc = lcd_batch_download(grp[i]);
            { std::lock_guard<std::mutex> lk(mu); d->busy_ms[slot_of[dev]] += now_ms() - tw0; d->n_sub[slot_of[dev]] += 1; }
            if (rc) { std::lock_guard<std::mutex> lk(mu); if (!first_err) { first_err = rc; err_msg = g_err; } return; }
        }
    };
    std::vector<std::thread> ths;
    for (int dev : d->devs) ths.emplace_back(worker, dev);
    for (auto &t : ths) t.join();
    if (first_err) return set_err(first_err, err_msg);
    return 0;
}

// The scattered pieces of a batch's results -- the ref<->cons rows (one piece per region and cluster in the WFA output buffer) and the K2 chains' cluster lists (one
// piece per chain in the chain-output buffer) -- gathered into ONE staging block on the device.  Since round 4 this runs at the END OF THE RUN, on the submission's
// stream: a download is then DMA copies only.  (As a kernel inside lcd_batch_download it had to find a hardware queue next to another submission's chain kernels --
// four queues, all busy for the length of that submission -- so a download never overlapped the next submission: the pipeline of bench.py's pcie_inclusive.)
static int gather_plan(lcd_batch_t *b, std::vector<GatherJob> &gj_all) { // the batch's pieces appended to gj_all with absolute destinations in its own staging block
    const bool vars_only = b->opt.collect_noisy_vars == 2;
    const uint64_t final_bytes = vars_only ? 0 : b->final_bytes;
    uint64_t extra = 0;
    b->g_rc_off.assign(b->rc_jobs.size(), 0);
    std::vector<GatherJob> gj;
    for (size_t i = 0; i < b->rc_jobs.size(); ++i) {
        b->g_rc_off[i] = final_bytes + extra;
        if (!vars_only) { const uint64_t nbytes = 2ull * (b->rc_jobs[i].plen + b->rc_jobs[i].tlen + 1); gj.push_back({b->rc_jobs[i].out_off, extra, (uint32_t)nbytes, 0}); extra += lcd_align_up(nbytes, 16); }
    }
    b->g_clu_base = extra;
    b->clu_index.clear(); b->clu_gather_index.clear();
    {
        const int nC = (int)b->pchains.size();
        std::vector<char> seen((size_t)nC, 0);
        for (const RegionRec &R : b->regs) {
            if (R.branch != 2) continue;
            const int ch = R.chain[0]; const PoaChain &pc = b->pchains[ch];
            if (seen[ch]) continue;
            seen[ch] = 1;
            const uint64_t clu_addr = pc.out_off + lcd_align_up((uint64_t)(pc.n_reads + 4) * pc.node_cap, 16);
            b->clu_index.push_back({ch, (uint32_t)(extra - b->g_clu_base)});
            gj.push_back({clu_addr, extra, (uint32_t)(2 * (size_t)pc.n_reads * 4), 0}); extra += lcd_align_up(2ull * pc.n_reads * 4, 16);
        }
    }
    b->g_extra = extra;
    if (!gj.empty()) {
        if (b->d_gather.ensure(extra + 64)) return -11;
        for (auto &g : gj) g.dst += b->d_gather.addr();
        gj_all.insert(gj_all.end(), gj.begin(), gj.end());
    }
    return 0;
}
// one job table, one launch for all the batches of a submission (leader = bs[0] lends the table's buffer): per batch this was 20 x (upload, kernel, synchronize) =
// 3.4 ms at the end of a 20-batch run
static int stage_gather_many(lcd_batch_t **bs, int nb, hipStream_t st) {
    std::vector<GatherJob> gj;
    for (int k = 0; k < nb; ++k) if (int rc = gather_plan(bs[k], gj)) return rc;
    if (!gj.empty()) {
        lcd_batch_t *L = bs[0];
        if (L->d_gather_jobs.ensure(gj.size() * sizeof(GatherJob))) return -11;
        HIPCHK(hipMemcpyAsync(L->d_gather_jobs.p, gj.data(), gj.size() * sizeof(GatherJob), hipMemcpyHostToDevice, st));
        lcd_launch_gather((const GatherJob *)L->d_gather_jobs.p, (int)gj.size(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st)); // (gj is a local: the job table must have left the host before it goes out of scope)
    }
    for (int k = 0; k < nb; ++k) bs[k]->gathered = true;
    return 0;
}
static int stage_gather(lcd_batch_t *b, hipStream_t st) { return stage_gather_many(&b, 1, st); }

int lcd_batch_download(lcd_batch_t *b) {
    if (!b->ran) return set_err(-3, "lcd_batch_download before lcd_batch_run");
    if (use_device(b->device)) return -1;
    const double t0 = now_ms();
    hipStream_t st = b->stream;
    b->h_var.resize(b->var_bytes);
    if (b->var_bytes) HIPCHK(hipMemcpyAsync(b->h_var.data(), b->d_var_out.p, b->var_bytes, hipMemcpyDeviceToHost, st));
    const bool vars_only = b->opt.collect_noisy_vars == 2; // the alignment strings stay in HBM: only variants + alleles cross PCIe
    if (vars_only) b->final_bytes = 0;
    // ref<->cons rows and cluster lists are appended after the strings: the host block is sized ONCE, before any copy is queued into it (a resize between two
    // asynchronous copies would free the destination of the first).  The pieces themselves were gathered into one staging block at the end of the run.
    if (!b->gathered) { if (int rc = stage_gather(b, st)) return rc; }
    const uint64_t extra = b->g_extra, clu_base = b->g_clu_base;
    const std::vector<uint64_t> &rc_off = b->g_rc_off;
    b->h_final.resize(b->final_bytes + extra);
    if (b->final_bytes) HIPCHK(hipMemcpyAsync(b->h_final.data(), b->d_final.p, b->final_bytes, hipMemcpyDeviceToHost, st));
    if (extra) HIPCHK(hipMemcpyAsync(b->h_final.data() + b->final_bytes, b->d_gather.p, extra, hipMemcpyDeviceToHost, st));
    b->h_rr.resize(b->rr_bytes);
    if (b->rr_bytes) HIPCHK(hipMemcpyAsync(b->h_rr.data(), b->d_rr.p, b->rr_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    { // the cluster lists as lcd_batch_region_result reads them: [ch:int][n:int][ids...] per chain, found through clu_index
        b->h_poa_out.clear();
        if (b->clu_gather_index.empty() && !b->clu_index.empty()) b->clu_gather_index = b->clu_index; // (first download of this run: offsets into the staging block)
        b->clu_index = b->clu_gather_index;
        for (auto &ci : b->clu_index) {
            const PoaChain &pc = b->pchains[ci.first];
            int hdr[2] = {ci.first, 2 * pc.n_reads};
            const uint32_t at = (uint32_t)b->h_poa_out.size();
            const uint8_t *p = (const uint8_t *)hdr; b->h_poa_out.insert(b->h_poa_out.end(), p, p + 8);
            p = b->h_final.data() + b->final_bytes + clu_base + ci.second; b->h_poa_out.insert(b->h_poa_out.end(), p, p + (size_t)hdr[1] * 4);
            ci.second = at;
        }
        std::sort(b->clu_index.begin(), b->clu_index.end());
    }
    // remember where the ref<->cons rows are
    for (size_t i = 0; i < b->rc_jobs.size(); ++i) b->rc_jobs[i].ws_off = rc_off[i];
    b->downloaded = true;
    b->st.ms_download = now_ms() - t0;
    return 0;
}

static const std::vector<int> *clu_list(lcd_batch_t *b, int ch, std::vector<int> &tmp) {
    { // (binary search in the index lcd_batch_download made; the linear walk below is the fallback)
        auto it = std::lower_bound(b->clu_index.begin(), b->clu_index.end(), std::make_pair(ch, (uint32_t)0));
        if (it != b->clu_index.end() && it->first == ch && (size_t)it->second + 8 <= b->h_poa_out.size()) {
            int hdr[2]; memcpy(hdr, b->h_poa_out.data() + it->second, 8);
            if (hdr[0] == ch) { tmp.resize(hdr[1]); memcpy(tmp.data(), b->h_poa_out.data() + it->second + 8, (size_t)hdr[1] * 4); return &tmp; }
        }
    }
    const uint8_t *p = b->h_poa_out.data(), *e = p + b->h_poa_out.size();
    while (p < e) {
        int hdr[2]; memcpy(hdr, p, 8); p += 8;
        if (hdr[0] == ch) { tmp.resize(hdr[1]); memcpy(tmp.data(), p, (size_t)hdr[1] * 4); return &tmp; }
        p += (size_t)hdr[1] * 4;
    }
    return nullptr;
}

// One region's results in the reference's layout (src/collect_var.c:2670-2724).  `take(bytes, zero)` hands out the memory: libc malloc / calloc blocks the caller
// frees one by one (lcd_batch_region_result: the reference's ownership contract), or slices of ONE block per batch (lcd_batch_region_results_arena)
} // extern "C"
// DRY: only the sizes are asked for (`take` counts): nothing is copied and nothing is written through the returned pointers -- the sizing pass of the arena form
// used to do every copy twice
template <bool DRY = false, class Take>
static int region_result_impl(lcd_batch_t *b, int region, int *clu_n_seqs, int **clu_read_ids, lcd_aln_str_t **aln_strs, Take &&take) {
    if (!b->downloaded) return set_err(-3, "lcd_batch_region_result before lcd_batch_download");
    if (b->opt.collect_noisy_vars == 2) return set_err(-5, "lcd_batch_region_result: the strings were left in HBM (opt.collect_noisy_vars == 2)");
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    const RegionRec &R = b->regs[region];
    if (R.branch == 0) return 0;
    // src/align.c:832-834 / :907-920: clu_read_ids are filled whenever K1/K2 ran, even if the region ends with n_cons = 0
    std::vector<int> tmp;
    if (R.branch == 1) {
        for (int c = 0; c < 2; ++c) {
            const ChainRec &C = b->chains[R.chain[c]];
            clu_n_seqs[c] = (int)C.members.size();
            clu_read_ids[c] = (int *)take(C.members.size() * sizeof(int), false);
            if (!DRY) for (size_t k = 0; k < C.members.size(); ++k) clu_read_ids[c][k] = R.reads[C.members[k]].id;
        }
    } else {
        const ChainRec &C = b->chains[R.chain[0]]; const PoaChainOut &co = b->couts[R.chain[0]];
        const std::vector<int> *cl = DRY ? nullptr : clu_list(b, R.chain[0], tmp);
        if (co.n_cons == 2) {
            for (int c = 0; c < 2; ++c) {
                clu_n_seqs[c] = co.clu_n[c];
                clu_read_ids[c] = (int *)take((co.clu_n[c] > 0 ? co.clu_n[c] : 1) * sizeof(int), false);
                if (!DRY) for (int k = 0; k < co.clu_n[c]; ++k) clu_read_ids[c][k] = R.reads[C.members[(*cl)[(size_t)c * C.members.size() + k]]].id;
            }
        } else {
            clu_n_seqs[0] = (int)C.members.size();
            clu_read_ids[0] = (int *)take(C.members.size() * sizeof(int), false);
            if (!DRY) for (size_t k = 0; k < C.members.size(); ++k) clu_read_ids[0][k] = R.reads[C.members[k]].id;
        }
    }
    if (R.n_cons == 0) return 0;
    const bool have_ranges = b->reg_rc0.size() == b->regs.size() + 1;   // (job ranges per region: a scan over every job of the batch for every region was most of
    const size_t rc_lo = have_ranges ? b->reg_rc0[region] : 0, rc_hi = have_ranges ? b->reg_rc0[region + 1] : b->rc_jobs.size();  //  the 55 - 70 ms a batch's results cost)
    const size_t st_lo = have_ranges ? b->reg_str0[region] : 0, st_hi = have_ranges ? b->reg_str0[region + 1] : b->str_jobs.size();
    for (size_t i = rc_lo; i < rc_hi; ++i) {
        if (b->rc_region[i] != region) continue;
        const int c = b->rc_clu[i]; const WfaJob &wj = b->rc_jobs[i]; const WfaOut &wo = b->rc_outs[i];
        const int maxl = wj.plen + wj.tlen + 1; // wfa_collect_pretty_alignment layout, src/align.c:288-291
        uint8_t *mem = (uint8_t *)take(2 * (size_t)maxl, true);
        if (DRY) continue;
        memcpy(mem, b->h_final.data() + wj.ws_off, (size_t)wo.aln_len);
        memcpy(mem + maxl, b->h_final.data() + wj.ws_off + maxl, (size_t)wo.aln_len);
        lcd_aln_str_t &s = aln_strs[c][0];
        s.target_aln = mem; s.query_aln = mem + maxl; s.aln_len = wo.aln_len;
        s.target_beg = 0; s.target_end = wo.aln_len - 1; s.query_beg = 0; s.query_end = wo.aln_len - 1;
    }
    const uint64_t fbase = b->d_final.addr();
    for (size_t j = st_lo; j < st_hi; ++j) {
        if (b->str_region[j] != region) continue;
        const int c = b->str_clu[j], k = b->str_k[j]; const StrJob &sj = b->str_jobs[j]; const StrOut &so = b->str_outs[j];
        const uint8_t *src = b->h_final.data() + (sj.out_off - fbase);
        if (DRY) { (void)take(so.shift != 0 ? (size_t)so.aln_len * 2 + 1 : (size_t)sj.msa_len * 2 + 1, false); if (!b->rr_len.empty()) (void)take((size_t)b->rr_stride[j] * 2 + 1, false); continue; }
        lcd_aln_str_t &s = aln_strs[c][2 * k + 1];
        if (so.shift != 0) { // src/align.c:541-549: re-allocated compact block
            uint8_t *mem = (uint8_t *)take((size_t)so.aln_len * 2 + 1, false);
            memcpy(mem, src + so.shift, so.aln_len); memcpy(mem + so.aln_len, src + sj.msa_len + so.shift, so.aln_len);
            s.target_aln = mem; s.query_aln = mem + so.aln_len;
        } else {
            uint8_t *mem = (uint8_t *)take((size_t)sj.msa_len * 2 + 1, false);
            memcpy(mem, src, so.aln_len > 0 ? so.aln_len : 0); memcpy(mem + sj.msa_len, src + sj.msa_len, so.aln_len > 0 ? so.aln_len : 0);
            s.target_aln = mem; s.query_aln = mem + sj.msa_len;
        }
        s.aln_len = so.aln_len; s.target_beg = so.target_beg; s.target_end = so.target_end; s.query_beg = so.query_beg; s.query_end = so.query_end;
        if (!b->rr_len.empty()) { // ref<->read string, src/align.c:1056-1062 layout: one block of 2 * (rc_len + cr_len), query row at + max_len
            const int ml = b->rr_stride[j];
            uint8_t *mem = (uint8_t *)take((size_t)ml * 2 + 1, false);
            memcpy(mem, b->h_rr.data() + b->rr_off[j], (size_t)b->rr_len[j]); memcpy(mem + ml, b->h_rr.data() + b->rr_off[j] + ml, (size_t)b->rr_len[j]);
            lcd_aln_str_t &r2 = aln_strs[c][2 * k + 2];
            r2.target_aln = mem; r2.query_aln = mem + ml; r2.aln_len = b->rr_len[j];
            r2.target_beg = r2.target_end = r2.query_beg = r2.query_end = -1;
        }
    }
    return R.n_cons;
}

extern "C" {
int lcd_batch_region_result(lcd_batch_t *b, int region, int *clu_n_seqs, int **clu_read_ids, lcd_aln_str_t **aln_strs) {
    return region_result_impl(b, region, clu_n_seqs, clu_read_ids, aln_strs, [](size_t n, bool zero) { return zero ? calloc(n ? n : 1, 1) : malloc(n ? n : 1); });
}

// Every region's results of a batch in ONE host block (additive; the per-region entry above keeps the reference's malloc-per-row ownership): the table of
// lcd_region_result_t, the cluster id lists, the aln_str_t arrays (1 + 2 n_reads per cluster, zeroed like the caller's calloc at src/collect_var.c:2670-2679) and
// every alignment row live inside *arena_out; target_aln / query_aln / clu_read_ids are INTERIOR pointers -- free(*arena_out) frees everything, nothing else may be
// freed.  Two passes: sizes (the exact bytes region_result_impl asks for), then the regions filled by host threads.
int lcd_batch_region_results_arena(lcd_batch_t *b, lcd_region_result_t **results_out, void **arena_out, uint64_t *arena_bytes) {
    *results_out = nullptr; *arena_out = nullptr; if (arena_bytes) *arena_bytes = 0;
    if (!b->downloaded) return set_err(-3, "lcd_batch_region_results_arena before lcd_batch_download");
    if (b->opt.collect_noisy_vars == 2) return set_err(-5, "lcd_batch_region_results_arena: the strings were left in HBM (opt.collect_noisy_vars == 2)");
    const size_t nr = b->regs.size();
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    std::vector<uint64_t> off(nr + 1, 0);
    const size_t table = up(nr * sizeof(lcd_region_result_t));
    // pass 1: bytes per region (a dry run of the same code with a counting allocator that returns a scratch block)
    std::vector<uint64_t> need(nr, 0);
    auto run = [&](const bool dry, uint8_t *base, lcd_region_result_t *tab) {
        const int nth_max = host_arena_threads(HostSwitches::from_env()); // (read per call; a caller that materialises several batches at once on its own threads wants fewer per batch)
        const int nth = dry ? 1 : (int)std::max<size_t>(1, std::min<size_t>((size_t)nth_max, nr / 64 + 1)); // (the sizing pass is a few additions per row)
        std::atomic<size_t> next{0};
        auto work = [&]() {
            std::vector<uint8_t> scratch; std::vector<lcd_aln_str_t> dry_as;
            for (size_t ri; (ri = next.fetch_add(1)) < nr;) {
                const RegionRec &R = b->regs[ri];
                const size_t nas = 1 + 2 * (size_t)std::max(R.n_reads, 0);
                uint64_t used = 0;
                uint8_t *p = dry ? nullptr : base + off[ri];
                auto take = [&](size_t n, bool zero) -> void * {
                    const size_t a = up(n ? n : 1);
                    void *r;
                    if (dry) r = nullptr;
                    else { r = p + used; if (zero) memset(r, 0, a); }
                    used += a; return r;
                };
                lcd_region_result_t rr; memset(&rr, 0, sizeof(rr));
                lcd_aln_str_t *as[2];
                if (dry) { as[0] = as[1] = nullptr; used += 2 * up(nas * sizeof(lcd_aln_str_t)); }
                else { as[0] = (lcd_aln_str_t *)take(nas * sizeof(lcd_aln_str_t), true); as[1] = (lcd_aln_str_t *)take(nas * sizeof(lcd_aln_str_t), true); }
                rr.n_cons = dry ? region_result_impl<true>(b, (int)ri, rr.clu_n_seqs, rr.clu_read_ids, as, take) : region_result_impl<false>(b, (int)ri, rr.clu_n_seqs, rr.clu_read_ids, as, take);
                rr.aln_strs[0] = as[0]; rr.aln_strs[1] = as[1]; rr.n_aln_strs = (int)nas;
                if (dry) need[ri] = used; else tab[ri] = rr;
            }
        };
        if (nth == 1) work();
        else { std::vector<std::thread> ths; for (int t = 0; t < nth; ++t) ths.emplace_back(work); for (auto &t : ths) t.join(); }
    };
    run(true, nullptr, nullptr);
    off[0] = table;
    for (size_t ri = 0; ri < nr; ++ri) off[ri + 1] = off[ri] + need[ri];
    // (tens of megabytes per batch, touched once: on 2 MB pages -- where the host allows them for madvised ranges -- the first touch costs 4 ms instead of 10;
    //  posix_memalign'ed blocks are free()d like malloc'ed ones, so the caller's side of the contract does not change)
    uint8_t *arena = nullptr;
    if (off[nr] >= (8u << 20)) {
        void *pa = nullptr;
        if (posix_memalign(&pa, 2u << 20, (size_t)off[nr] + 16) == 0 && pa) { arena = (uint8_t *)pa; (void)madvise(pa, (size_t)off[nr] + 16, MADV_HUGEPAGE); }
    }
    if (!arena) arena = (uint8_t *)malloc((size_t)off[nr] + 16);
    if (!arena) return set_err(-12, "lcd_batch_region_results_arena: out of host memory");
    run(false, arena, (lcd_region_result_t *)arena);
    *results_out = (lcd_region_result_t *)arena; *arena_out = arena; if (arena_bytes) *arena_bytes = off[nr];
    return (int)nr;
}

// the outputs of make_vars_from_msa_cons_aln (src/collect_var.c:2279) for one region, from the S6 stage
int lcd_batch_region_vars(lcd_batch_t *b, int region, int64_t noisy_reg_beg, const uint8_t *chunk_ref_seq, int64_t chunk_ref_beg,
                          int64_t chunk_ref_len, lcd_noisy_var_t **vars, int *n_rows, int **row_read_ids, int **prof_start, int **prof_end,
                          int **prof_alleles) {
    *vars = nullptr; *n_rows = 0; *row_read_ids = *prof_start = *prof_end = *prof_alleles = nullptr;
    if (!b->downloaded) return set_err(-3, "lcd_batch_region_vars before lcd_batch_download");
    if (!b->opt.collect_noisy_vars) return set_err(-5, "lcd_batch_region_vars needs opt.collect_noisy_vars");
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    const RegionRec &R = b->regs[region];
    const int vi = b->vreg_of[region];
    if (R.n_cons <= 0 || vi < 0) return 0;
    const VarRegionRec &V = b->vregs[vi];
    const int rows = V.rows[0] + (V.n_cons == 2 ? V.rows[1] : 0), n = V.n_vars;
    { // rows = the reads of cluster 0, then of cluster 1, in clu_read_ids order (the same lists lcd_batch_region_result returns)
        int *ids = (int *)malloc((rows > 0 ? rows : 1) * sizeof(int)); int w = 0; std::vector<int> tmp;
        if (R.branch == 1) {
            for (int c = 0; c < 2; ++c) { const ChainRec &C = b->chains[R.chain[c]]; for (size_t k = 0; k < C.members.size(); ++k) ids[w++] = R.reads[C.members[k]].id; }
        } else {
            const ChainRec &C = b->chains[R.chain[0]]; const PoaChainOut &co = b->couts[R.chain[0]];
            if (co.n_cons == 2) {
                const std::vector<int> *cl = clu_list(b, R.chain[0], tmp);
                for (int c = 0; c < 2; ++c) for (int k = 0; k < co.clu_n[c]; ++k) ids[w++] = R.reads[C.members[(*cl)[(size_t)c * C.members.size() + k]]].id;
            } else for (size_t k = 0; k < C.members.size(); ++k) ids[w++] = R.reads[C.members[k]].id;
        }
        if (w != rows) { free(ids); return set_err(-23, "candidate variants: cluster rows do not match the string jobs"); }
        *row_read_ids = ids; *n_rows = rows;
    }
    int *ps = (int *)malloc((rows > 0 ? rows : 1) * sizeof(int)), *pe = (int *)malloc((rows > 0 ? rows : 1) * sizeof(int));
    int *pa = (int *)malloc(((size_t)rows * n + 1) * sizeof(int));
    const int *se = (const int *)(b->h_var.data() + V.se_off); const int8_t *prof = (const int8_t *)(b->h_var.data() + V.prof_off);
    for (int r = 0; r < rows; ++r) { ps[r] = se[2 * r]; pe[r] = se[2 * r + 1]; }
    for (size_t q = 0; q < (size_t)rows * n; ++q) pa[q] = prof[q] == -2 ? -1 : prof[q]; // init_read_var_profile: 0xFF fill (src/bam_utils.c:26)
    *prof_start = ps; *prof_end = pe; *prof_alleles = pa;
    lcd_noisy_var_t *out = (lcd_noisy_var_t *)calloc(n > 0 ? n : 1, sizeof(lcd_noisy_var_t));
    const VarRec *rec = (const VarRec *)(b->h_var.data() + V.rec_off); const uint8_t *pool = b->h_var.data() + V.alt_off;
    for (int i = 0; i < n; ++i) {
        const VarRec &v = rec[i]; lcd_noisy_var_t &o = out[i];
        o.pos = noisy_reg_beg + v.ref_off; o.var_type = v.type; o.ref_len = v.ref_len; o.alt_len = v.alt_len; o.cate = v.cate; o.from_cons = v.from_cons;
        o.ref_base = v.ref_base; o.alt_ref_base = v.alt_ref_base; o.total_cov = v.total_cov; o.alle_covs[0] = v.alle_cov0; o.alle_covs[1] = v.alle_cov1;
        if (v.alt_len > 0) { o.alt_seq = (uint8_t *)malloc(v.alt_len); memcpy(o.alt_seq, pool + v.alt_off, v.alt_len); }
        // var_is_homopolymer_indel, src/collect_var.c:1720-1744 (reads chunk reference bases beyond the region: host side, 5 bytes per indel);
        // gaps >= min_sv_len go to collect_te_info_from_cons instead (:1815, :1834 -- SURVEY a14, the caller's host code)
        o.is_homopolymer_indel = 0;
        const int gap = v.type == 1 ? v.alt_len : v.ref_len;
        const int64_t off = o.pos - chunk_ref_beg;
        if (v.type != 8 && gap < b->opt.min_sv_len && chunk_ref_seq && off >= 0 && off + 5 <= chunk_ref_len && (v.type == 1 || off + v.ref_len <= chunk_ref_len)) {
            const uint8_t b0 = v.type == 1 ? o.alt_seq[0] : chunk_ref_seq[off];
            int hp = 1;
            if (v.type == 1) { for (int k = 1; k < v.alt_len; ++k) hp &= o.alt_seq[k] == b0; }
            else { for (int k = 1; k < v.ref_len; ++k) hp &= chunk_ref_seq[off + k] == b0; }
            for (int k = 0; k < 5; ++k) hp &= chunk_ref_seq[off + k] == b0;
            o.is_homopolymer_indel = hp;
        }
    }
    *vars = out;
    return n;
}

int lcd_batch_region_ref_read_rows(lcd_batch_t *b, int region, int n_rows, int *aln_len, const uint8_t **target, const uint8_t **query) {
    const std::string W = "lcd_batch_region_ref_read_rows";
    if (!b || !b->downloaded) return set_err(-3, W + " before lcd_batch_download");
    if (!b->opt.collect_ref_read_aln_str || !b->opt.collect_noisy_vars) return set_err(-5, W + " needs opt.collect_ref_read_aln_str and opt.collect_noisy_vars");
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    const RegionRec &R = b->regs[region];
    const int vi = b->vreg_of[region];
    if (R.n_cons <= 0 || vi < 0) return 0;
    const VarRegionRec &V = b->vregs[vi];
    const int rows = V.rows[0] + (V.n_cons == 2 ? V.rows[1] : 0);
    if (n_rows < rows || !aln_len || !target || !query) return set_err(-4, W + ": fewer than the region's rows, or NULL arrays");
    if (b->rr_len.size() != b->str_jobs.size() || b->reg_str0.size() != b->regs.size() + 1) return set_err(-23, W + ": the run left no ref<->read rows");
    for (int r = 0; r < rows; ++r) aln_len[r] = -1;
    for (size_t j = b->reg_str0[region]; j < b->reg_str0[region + 1]; ++j) {
        if (b->str_region[j] != region) continue;
        const int c = b->str_clu[j], k = b->str_k[j];
        if (c < 0 || c >= V.n_cons || c > 1 || k < 0 || k >= V.rows[c]) continue;
        const int r = c == 0 ? k : V.rows[0] + k;
        if (b->rr_off[j] + 2ull * (uint64_t)b->rr_stride[j] > b->h_rr.size() || b->rr_len[j] < 0 || b->rr_len[j] > b->rr_stride[j]) return set_err(-23, W + ": rows outside the download");
        aln_len[r] = b->rr_len[j]; target[r] = b->h_rr.data() + b->rr_off[j]; query[r] = target[r] + b->rr_stride[j];
    }
    for (int r = 0; r < rows; ++r) if (aln_len[r] < 0) return set_err(-23, W + ": a read of a cluster has no ref<->read row");
    return rows;
}

int lcd_batch_region_sorted_ids(lcd_batch_t *b, int region, int *out) {
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    const RegionRec &R = b->regs[region];
    for (size_t i = 0; i < R.reads.size(); ++i) out[i] = R.reads[i].id;
    return (int)R.reads.size();
}

int lcd_batch_get_stats(lcd_batch_t *b, lcd_batch_stats_t *st) { *st = b->st; return 0; }

// the K4 (edlib NW + path) job set of the batch's anchor stage, as offsets into the batch's host pool: what bench.py times the reference's own
// edlib on (cpu_baseline.k4_reference) next to lcd_edlib_kernel
int lcd_batch_k4_jobs(lcd_batch_t *b, int cap, uint64_t *t_off, int *tlen, uint64_t *q_off, int *qlen, const uint8_t **pool, uint64_t *pool_len) {
    const int n = (int)b->ed_jobs.size();
    if (pool) *pool = b->h_pool.data();
    if (pool_len) *pool_len = b->h_pool.size();
    for (int i = 0; i < n && i < cap; ++i) { t_off[i] = b->ed_jobs[i].t_off; tlen[i] = b->ed_jobs[i].tlen; q_off[i] = b->ed_jobs[i].q_off; qlen[i] = b->ed_jobs[i].qlen; }
    return n;
}

// what a caller pays after lcd_batch_download to hold every result the way lcd_collect_noisy_reg_aln_strs hands it over: lcd_batch_region_result for every
// region (malloc()'d cluster id lists and aln_str_t rows), freed again; returns the bytes of alignment rows that were handed out.  (lcd_batch_digest does the same
// AND hashes every byte, which is most of its time: bench.py's PCIe-inclusive figures use this one for the clock and the digest for the check.)
uint64_t lcd_batch_materialize(lcd_batch_t *b) {
    if (!b->downloaded) return 0;
    uint64_t bytes = 0;
    for (size_t ri = 0; ri < b->regs.size(); ++ri) {
        const RegionRec &R = b->regs[ri];
        if (b->opt.collect_noisy_vars == 2) continue; // the strings stay in HBM: the variant records are already in the host block lcd_batch_download filled
        std::vector<int> cn(2, 0); std::vector<int *> ids(2, nullptr);
        std::vector<lcd_aln_str_t> a0(1 + 2 * (size_t)std::max(R.n_reads, 0)), a1(a0.size());
        memset(a0.data(), 0, a0.size() * sizeof(lcd_aln_str_t)); memset(a1.data(), 0, a1.size() * sizeof(lcd_aln_str_t));
        lcd_aln_str_t *as[2] = {a0.data(), a1.data()};
        lcd_batch_region_result(b, (int)ri, cn.data(), ids.data(), as);
        for (int c = 0; c < 2; ++c) {
            free(ids[c]);
            for (size_t j = 0; j < a0.size(); ++j) { lcd_aln_str_t &s = as[c][j]; if (!s.target_aln) continue; bytes += 2ull * (uint64_t)std::max(s.aln_len, 0); free(s.target_aln); }
        }
    }
    return bytes;
}
uint64_t lcd_batch_digest(lcd_batch_t *b) {
    if (!b->downloaded) return 0;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) { const uint8_t *q = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= q[i]; h *= 1099511628211ull; } };
    for (size_t ri = 0; ri < b->regs.size(); ++ri) {
        const RegionRec &R = b->regs[ri];
        std::vector<int> cn(2, 0); std::vector<int *> ids(2, nullptr);
        std::vector<lcd_aln_str_t> a0(1 + 2 * (size_t)std::max(R.n_reads, 0)), a1(a0.size());
        memset(a0.data(), 0, a0.size() * sizeof(lcd_aln_str_t)); memset(a1.data(), 0, a1.size() * sizeof(lcd_aln_str_t));
        lcd_aln_str_t *as[2] = {a0.data(), a1.data()};
        int nc = b->opt.collect_noisy_vars == 2 ? R.n_cons : lcd_batch_region_result(b, (int)ri, cn.data(), ids.data(), as);
        mix(&nc, 4);
        if (b->opt.collect_noisy_vars && b->vreg_of[ri] >= 0) { // stage S6 outputs: merged variants, alt pool, profile rows
            const VarRegionRec &V = b->vregs[b->vreg_of[ri]]; const int rows = V.rows[0] + (V.n_cons == 2 ? V.rows[1] : 0);
            mix(&V.n_vars, 4); mix(b->h_var.data() + V.rec_off, (size_t)V.n_vars * sizeof(VarRec)); mix(b->h_var.data() + V.alt_off, (size_t)V.alt_bytes);
            mix(b->h_var.data() + V.prof_off, (size_t)rows * V.n_vars); mix(b->h_var.data() + V.se_off, (size_t)rows * 8);
        }
        for (int c = 0; c < 2; ++c) {
            if (nc > 0 && c < nc) { mix(&cn[c], 4); mix(ids[c], (size_t)cn[c] * 4); }
            free(ids[c]);
            for (size_t j = 0; j < a0.size(); ++j) {
                lcd_aln_str_t &s = as[c][j];
                if (!s.target_aln) continue;
                if (nc > 0) { mix(&s.aln_len, 4); mix(&s.target_beg, 16); mix(s.target_aln, s.aln_len > 0 ? s.aln_len : 0); mix(s.query_aln, s.aln_len > 0 ? s.aln_len : 0); }
                free(s.target_aln);
            }
        }
    }
    return h;
}

// ---------------------------------------------------------------------------------------------------
// kernel-level batches
static int edlib_batch_mode(int mode, int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen, const uint64_t *t_off,
                            const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid, int *start, int *end);
int lcd_edlib_batch(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen, const uint64_t *t_off,
                    const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid) {
    return edlib_batch_mode(0, n, pool, pool_len, q_off, qlen, t_off, tlen, dist, xgaps, n_eq, n_xid, nullptr, nullptr);
}
int lcd_edlib_batch_hw(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen, const uint64_t *t_off,
                       const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid, int *start, int *end) {
    return edlib_batch_mode(1, n, pool, pool_len, q_off, qlen, t_off, tlen, dist, xgaps, n_eq, n_xid, start, end);
}
static int edlib_batch_mode(int mode, int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen, const uint64_t *t_off,
                            const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid, int *start, int *end) {
    if (ensure_init()) return -1;
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_pool, d_jobs, d_arena, d_outs;
    if (d_pool.ensure(pool_len + 64)) return -11;
    HIPCHK(hipMemcpyAsync(d_pool.p, pool, pool_len, hipMemcpyHostToDevice, st));
    std::vector<EdJob> jobs(n);
    for (int i = 0; i < n; ++i) { jobs[i].q_off = d_pool.addr() + q_off[i]; jobs[i].t_off = d_pool.addr() + t_off[i]; jobs[i].qlen = qlen[i]; jobs[i].tlen = tlen[i]; jobs[i].mode = mode; jobs[i].pad_ = 0; }
    std::vector<EdOut> outs;
    int rc = run_edlib_stage(st, jobs, d_jobs, d_arena, d_outs, outs);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        if (outs[i].status != LCD_OK) return set_err(-20, "edlib kernel status " + std::to_string(outs[i].status));
        if (dist) dist[i] = outs[i].dist;
        if (xgaps) xgaps[i] = outs[i].xgaps;
        if (n_eq) n_eq[i] = outs[i].n_eq;
        if (n_xid) n_xid[i] = outs[i].n_xid;
        if (start) start[i] = outs[i].start;
        if (end) end[i] = outs[i].end;
    }
    return 0;
}

// work-arena bytes of one alignment whose score bound is `score_bound` (what run_wfa_stage lays out for it): DESIGN / tests
uint64_t lcd_wfa_arena_bytes(int plen, int tlen, int score_bound, int b, int q, int e, int q2, int e2) {
    WfaJob j; memset(&j, 0, sizeof(j)); j.plen = plen; j.tlen = tlen;
    LcdScoring sc; sc.dbg = 0; sc.wd_s = 0; sc.match = 0; sc.mismatch = b; sc.o1 = q; sc.e1 = e; sc.o2 = q2; sc.e2 = e2;
    wfa_plan(j, sc, score_bound, HostSwitches::from_env());
    return j.ws_bytes;
}

int lcd_wfa_batch(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *p_off, const int *plen, const uint64_t *t_off, const int *tlen,
                  const int *gap_aln, int b, int q, int e, int q2, int e2, int want, int *score, uint32_t *cigars, int cigar_stride, int *n_cigar,
                  uint8_t *rows, int row_stride, int *aln_len) {
    if (ensure_init()) return -1;
    const HostSwitches sw = HostSwitches::from_env();
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_pool, d_jobs, d_arena, d_out, d_outs;
    if (d_pool.ensure(pool_len + 64)) return -11;
    HIPCHK(hipMemcpyAsync(d_pool.p, pool, pool_len, hipMemcpyHostToDevice, st));
    std::vector<WfaJob> jobs(n);
    for (int i = 0; i < n; ++i) {
        WfaJob &j = jobs[i];
        j.p_off = d_pool.addr() + p_off[i]; j.t_off = d_pool.addr() + t_off[i]; j.plen = plen[i]; j.tlen = tlen[i]; j.gap_aln = gap_aln[i]; j.want = want;
        j.s_cap = wfa_default_scap(plen[i], tlen[i]); j.ws_off = j.ws_bytes = j.out_off = 0;
    }
    LcdScoring sc; sc.dbg = 0; sc.wd_s = 0; sc.match = 0; sc.mismatch = b; sc.o1 = q; sc.e1 = e; sc.o2 = q2; sc.e2 = e2;
    std::vector<WfaOut> outs;
    int rc = run_wfa_stage(st, jobs, d_jobs, d_arena, d_out, d_outs, outs, sc, sw, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const uint64_t maxl = (uint64_t)plen[i] + tlen[i] + 1;
        uint64_t o = 0;
        if (score) score[i] = outs[i].score;
        if (want & 1) {
            if (n_cigar) n_cigar[i] = outs[i].n_cigar;
            if (outs[i].n_cigar > cigar_stride) { return set_err(-5, "cigar_stride too small"); }
            if (outs[i].n_cigar) HIPCHK(hipMemcpyAsync(cigars + (size_t)i * cigar_stride, (void *)(uintptr_t)jobs[i].out_off, (size_t)outs[i].n_cigar * 4, hipMemcpyDeviceToHost, st));
            o = lcd_align_up(maxl * 4, 16);
        }
        if (want & 2) {
            if (aln_len) aln_len[i] = outs[i].aln_len;
            if (outs[i].aln_len > row_stride) { return set_err(-5, "row_stride too small"); }
            if (outs[i].aln_len) {
                HIPCHK(hipMemcpyAsync(rows + (size_t)i * 2 * row_stride, (void *)(uintptr_t)(jobs[i].out_off + o), outs[i].aln_len, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(rows + (size_t)i * 2 * row_stride + row_stride, (void *)(uintptr_t)(jobs[i].out_off + o + maxl), outs[i].aln_len, hipMemcpyDeviceToHost, st));
            }
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// a region of the batch from the chunk in HBM: the slices (read_beg / read_end / cover, from lcd_chunk_region_slices) give the lengths and cover flags the host
// plans the chains with; the bases are unpacked on the device from the chunk's packed records into the batch's input pool at lcd_batch_upload -- no base crosses
// PCIe for a region.  Otherwise lcd_batch_add_region_from_chunk (same results).  The batch must live on the chunk's device.
int lcd_batch_add_region_from_chunk_dev(lcd_batch_t *b, const lcd_chunk_t *c, int64_t reg_beg, int64_t reg_end, int n, const int *read_ids, const int *read_beg,
                                        const int *read_end, const int *cover, const int *haps, const int64_t *phase_sets, const uint8_t *ref_seq, int ref_seq_len) {
    if (c->pending) return set_err(-4, "lcd_batch_add_region_from_chunk_dev: the chunk was opened and not resolved (lcd_chunk_resolve)");
    if (b->device >= 0 && b->device != c->device) return set_err(-4, "lcd_batch_add_region_from_chunk_dev: batch and chunk on different devices");
    std::vector<int> lens(n); std::vector<const uint8_t *> sp(n, nullptr), qp(n, nullptr);
    for (int i = 0; i < n; ++i) {
        const int r = read_ids[i];
        if (r < 0 || r >= c->n_reads) return set_err(-4, "lcd_batch_add_region_from_chunk_dev: read index out of range");
        lens[i] = read_end[i] - read_beg[i] + 1;
        qp[i] = lens[i] > 0 && !c->qual_base ? c->h_qual.data() + c->qual_off[r] + read_beg[i] : nullptr;
    }
    // the sampling rule of long regions (sort_noisy_region_reads by calc_read_error_rate, src/align.c:963-985, src/seq.c:429) on qualities that never left HBM
    std::vector<double> errs;
    if (c->qual_base && reg_end - reg_beg + 1 >= b->opt.min_noisy_reg_size_to_sample_reads && n > 0) {
        if (use_device(c->device)) return -1;
        errs.resize(n);
        std::vector<ErrJob> ej(n);
        for (int i = 0; i < n; ++i) { ej[i].qual = c->qual_base + c->qual_off[read_ids[i]] + (uint64_t)read_beg[i]; ej[i].len = lens[i]; ej[i].pad = 0; }
        double tab[256]; for (int q = 0; q < 256; ++q) tab[q] = pow(10.0, -((double)q) / 10.0);
        StreamGuard st; if (st.create()) return -10;
        DevBuf dj, dt, dout;
        if (dj.ensure(n * sizeof(ErrJob)) || dt.ensure(sizeof(tab)) || dout.ensure(n * sizeof(double))) return -11;
        HIPCHK(hipMemcpyAsync(dj.p, ej.data(), n * sizeof(ErrJob), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dt.p, tab, sizeof(tab), hipMemcpyHostToDevice, st));
        lcd_launch_errrate((const ErrJob *)dj.p, (const double *)dt.p, (double *)dout.p, n, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(errs.data(), dout.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const int ri = add_region_impl(b, reg_end - reg_beg + 1, n, read_ids, lens.data(), sp.data(), qp.data(), cover, haps, phase_sets, ref_seq, ref_seq_len, errs.empty() ? nullptr : errs.data());
    if (ri >= 0)
        for (RegRead &r : b->regs[ri].reads)
            for (int i = 0; i < n; ++i) if (read_ids[i] == r.id) {
                r.rb = read_beg[i]; r.re = read_end[i];
                if (r.len > 0) { UnpackJob j; j.src = c->seq_base + c->seq_off[r.id] + (uint64_t)(read_beg[i] >> 1); j.dst = r.off; j.first = read_beg[i] & 1; j.len = r.len; b->unpack_abs.push_back(j); }
                break;
            }
    return ri;
}

int lcd_poa_batch(const lcd_opt_t *opt, int n_chains, const int *mode, const int *chain_read0, const int *chain_n_reads, int n_reads_total,
                  const uint64_t *seq_off, const int *len, const int *skip, const int *anchors, const uint8_t *pool, uint64_t pool_len, int *status,
                  int *n_cons, int *cons_len, int *msa_len, int *clu_n, uint8_t *cons, int cons_stride, uint8_t *msa, int msa_stride, int max_reads,
                  int *clu_ids) {
    if (ensure_init()) return -1;
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_pool, d_chains, d_reads, d_arena, d_out, d_outs;
    if (d_pool.ensure(pool_len + 64)) return -11;
    HIPCHK(hipMemcpyAsync(d_pool.p, pool, pool_len, hipMemcpyHostToDevice, st));
    std::vector<PoaRead> preads(n_reads_total);
    for (int i = 0; i < n_reads_total; ++i) {
        PoaRead &r = preads[i]; r.seq_off = d_pool.addr() + seq_off[i]; r.len = len[i]; r.skip = skip ? skip[i] : 0;
        r.ref_beg = anchors[4 * i]; r.ref_end = anchors[4 * i + 1]; r.read_beg = anchors[4 * i + 2]; r.read_end = anchors[4 * i + 3];
    }
    const HostSwitches sw = HostSwitches::from_env(); const long long n_chains_unknown = 1ll << 40; // (no submission around these chains: the long ones take the four-wavefront pipeline, as in a crowded one)
    const PlanHints hints = learned_hints();
    std::vector<ChainRec> crec(n_chains); std::vector<PoaChain> pch(n_chains); std::vector<uint64_t> out_rel(n_chains);
    uint64_t out_tot = 0;
    for (int c = 0; c < n_chains; ++c) {
        crec[c].mode = mode[c]; crec[c].read0 = chain_read0[c]; crec[c].members.resize(chain_n_reads[c]);
        chain_caps(*opt, crec[c], preads, 1, n_chains_unknown, sw, hints, pch[c]);
        out_rel[c] = out_tot; out_tot += lcd_align_up(poa_out_bytes(pch[c].node_cap, pch[c].n_reads), 256);
    }
    if (d_out.ensure(out_tot) || d_reads.ensure(preads.size() * sizeof(PoaRead) + 16) || d_chains.ensure(n_chains * sizeof(PoaChain)) || d_outs.ensure(n_chains * sizeof(PoaChainOut))) return -11;
    HIPCHK(hipMemcpyAsync(d_reads.p, preads.data(), preads.size() * sizeof(PoaRead), hipMemcpyHostToDevice, st));
    std::vector<PoaChainOut> couts(n_chains);
    std::vector<int> which(n_chains);
    for (int c = 0; c < n_chains; ++c) which[c] = c;
    int scale = 1;
    std::vector<std::unique_ptr<DevBuf>> retry_out;
    const LcdScoring sc = scoring_of(*opt, sw);
    for (int round = 0; round < 12 && !which.empty(); ++round) {
        uint64_t tot = 0; std::vector<PoaChain> sub(which.size());
        for (size_t i = 0; i < which.size(); ++i) {
            PoaChain &pc = pch[which[i]];
            if (!round) pc.out_off = d_out.addr() + out_rel[which[i]];
            else {
                const int old_cap = pc.node_cap; const uint64_t keep = pc.out_off;
                chain_caps(*opt, crec[which[i]], preads, retry_scale(crec[which[i]], scale), n_chains_unknown, sw, learned_hints(), pc);
                pc.out_off = keep;
                if (pc.node_cap > old_cap) { // larger graph capacity -> larger output block
                    retry_out.emplace_back(new DevBuf());
                    if (retry_out.back()->ensure(poa_out_bytes(pc.node_cap, pc.n_reads) + 256)) return -11;
                    pc.out_off = retry_out.back()->addr();
                }
            }
            PoaLayout L = poa_layout(pc.node_cap, pc.edge_cap, pc.rid_words, pc.max_len, pc.cell_cap, pc.n_reads, pc.spill_x, pc.cert);
            pc.ws_off = tot; tot += L.total;
        }
        if (d_arena.ensure(tot)) return -11;
        for (size_t i = 0; i < which.size(); ++i) { pch[which[i]].ws_off += d_arena.addr(); sub[i] = pch[which[i]]; }
        { int rc2 = launch_poa_grouped(st, sub, d_chains, (const PoaRead *)d_reads.p, d_outs, sc, sw); if (rc2) return rc2; }
        std::vector<PoaChainOut> tmp(sub.size());
        HIPCHK(hipMemcpyAsync(tmp.data(), d_outs.p, sub.size() * sizeof(PoaChainOut), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int> again;
        for (size_t i = 0; i < which.size(); ++i) {
            couts[which[i]] = tmp[i];
            if (chain_goes_back(tmp[i].status, pch[which[i]], crec[which[i]], round)) again.push_back(which[i]);
        }
        if (!again.empty()) scale *= 2;
        which.swap(again);
    }
    for (int c = 0; c < n_chains; ++c) {
        const PoaChainOut &o = couts[c]; const PoaChain &pc = pch[c];
        status[c] = o.status; n_cons[c] = o.n_cons; cons_len[2 * c] = o.cons_len[0]; cons_len[2 * c + 1] = o.cons_len[1]; msa_len[c] = o.msa_len;
        clu_n[2 * c] = o.clu_n[0]; clu_n[2 * c + 1] = o.clu_n[1];
        if (o.status != LCD_OK) continue;
        if (o.msa_len > msa_stride || o.cons_len[0] > cons_stride || o.cons_len[1] > cons_stride || pc.n_reads > max_reads) { return set_err(-5, "output strides too small"); }
        for (int k = 0; k < o.n_cons; ++k)
            if (o.cons_len[k]) HIPCHK(hipMemcpyAsync(cons + ((size_t)2 * c + k) * cons_stride, (void *)(uintptr_t)(pc.out_off + (uint64_t)k * pc.node_cap), o.cons_len[k], hipMemcpyDeviceToHost, st));
        for (int r = 0; r < pc.n_reads + o.n_cons; ++r)
            if (o.msa_len) HIPCHK(hipMemcpyAsync(msa + ((size_t)c * (max_reads + 2) + r) * msa_stride, (void *)(uintptr_t)(pc.out_off + 2ull * pc.node_cap + (uint64_t)r * pc.node_cap), o.msa_len, hipMemcpyDeviceToHost, st));
        const uint64_t clu_addr = pc.out_off + lcd_align_up((uint64_t)(pc.n_reads + 4) * pc.node_cap, 16);
        for (int k = 0; k < o.n_cons; ++k)
            if (o.clu_n[k]) HIPCHK(hipMemcpyAsync(clu_ids + ((size_t)2 * c + k) * max_reads, (void *)(uintptr_t)(clu_addr + (uint64_t)k * pc.n_reads * 4), (size_t)o.clu_n[k] * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int lcd_batch_region_n_cons(lcd_batch_t *b, int region) {
    if (!b->downloaded) return set_err(-3, "lcd_batch_region_n_cons before lcd_batch_download");
    if (region < 0 || region >= (int)b->regs.size()) return set_err(-4, "bad region index");
    return b->regs[region].n_cons > 0 ? b->regs[region].n_cons : 0;
}
int lcd_batch_add_planned(lcd_batch_t *b, const lcd_chunk_t *c, const lcd_pass_plan_t *plan, const int *haps, const int64_t *phase_sets, const uint8_t *ref_seq,
                          int64_t ref_beg, int *region_idx_out) {
    if (!b || !c || !plan || !haps || !phase_sets || !ref_seq) return set_err(-4, "lcd_batch_add_planned: NULL argument");
    if (c->pending) return set_err(-4, "lcd_batch_add_planned: the chunk was opened and not resolved (lcd_chunk_resolve)");
    if (plan->n_regs < 0 || (plan->n_regs > 0 && (!plan->status || !plan->beg || !plan->end || !plan->read_off))) return set_err(-4, "lcd_batch_add_planned: incomplete plan");
    for (int i = 0; i < plan->n_regs; ++i) {
        if (plan->status[i] != LCD_PLAN_SUBMIT) continue;
        if (plan->beg[i] < ref_beg || plan->end[i] < plan->beg[i] || plan->read_off[i + 1] < plan->read_off[i]) return set_err(-4, "lcd_batch_add_planned: region " + std::to_string(i) + " outside the reference or with a decreasing read_off");
        for (uint64_t k = plan->read_off[i]; k < plan->read_off[i + 1]; ++k)
            if (plan->read_ids[k] < 0 || plan->read_ids[k] >= c->n_reads) return set_err(-4, "lcd_batch_add_planned: read id outside [0, n_reads)");
    }
    int added = 0; std::vector<int> hp; std::vector<int64_t> ps;
    for (int i = 0; i < plan->n_regs; ++i) {
        if (region_idx_out) region_idx_out[i] = -1;
        if (plan->status[i] != LCD_PLAN_SUBMIT) continue;
        const uint64_t k0 = plan->read_off[i]; const int n = (int)(plan->read_off[i + 1] - k0);
        hp.resize(n); ps.resize(n);
        for (int k = 0; k < n; ++k) { hp[k] = haps[plan->read_ids[k0 + k]]; ps[k] = phase_sets[plan->read_ids[k0 + k]]; }
        const int ri = lcd_batch_add_region_from_chunk_dev(b, c, plan->beg[i], plan->end[i], n, plan->read_ids + k0, plan->read_beg + k0, plan->read_end + k0, plan->cover + k0,
                                                           hp.data(), ps.data(), ref_seq + (plan->beg[i] - ref_beg), (int)(plan->end[i] - plan->beg[i] + 1));
        if (ri < 0) return ri;
        if (region_idx_out) region_idx_out[i] = ri;
        ++added;
    }
    return added;
}

// ---- the planner's probes (declared in lcd_host_internal.h only; tests/test_chain_plan.py): what chain_caps / wfa_plan decide for one chain / job, with the
// switches read from the environment at this call.  No device is touched ----
int lcd_plan_chain_probe(const lcd_opt_t *opt, int mode, int n_reads, const int *read_len, int scale, int cert_level, int solo, long long n_chains, const int *hints, int64_t *out) {
    std::vector<PoaRead> preads(n_reads);
    for (int i = 0; i < n_reads; ++i) { memset(&preads[i], 0, sizeof(PoaRead)); preads[i].len = read_len[i]; }
    ChainRec C; C.region = 0; C.clu = 0; C.mode = mode; C.members.resize(n_reads); C.read0 = 0; C.cert_level = cert_level; C.solo = solo;
    PlanHints h = learned_hints();
    if (hints) { h.cell[0] = hints[0]; h.cell[1] = hints[1]; h.node = hints[2]; }
    PoaChain pc; memset(&pc, 0, sizeof(pc));
    chain_caps(*opt, C, preads, scale, n_chains, HostSwitches::from_env(), h, pc);
    out[0] = pc.threads; out[1] = pc.wmax; out[2] = (int64_t)pc.lds_words * 4; out[3] = pc.ring_k; out[4] = pc.ring16; out[5] = pc.solo; out[6] = pc.cert;
    out[7] = pc.node_cap; out[8] = pc.edge_cap; out[9] = (int64_t)pc.cell_cap; out[10] = pc.spill_x; out[11] = pc.min_w;
    return 0;
}
// (s_want <= 0: wfa_default_scap, of an anchor-stage job where anchor != 0; wfa_hint < 0: the learned level; scoring: mismatch, o1, e1, o2, e2)
int lcd_plan_wfa_probe(int plen, int tlen, long long s_want, int anchor, int wfa_hint, const int *scoring, int64_t *out) {
    const HostSwitches sw = HostSwitches::from_env();
    WfaJob j; memset(&j, 0, sizeof(j)); j.plen = plen; j.tlen = tlen;
    LcdScoring sc; memset(&sc, 0, sizeof(sc)); sc.mismatch = scoring[0]; sc.o1 = scoring[1]; sc.e1 = scoring[2]; sc.o2 = scoring[3]; sc.e2 = scoring[4];
    if (s_want <= 0) s_want = wfa_default_scap(plen, tlen, !anchor ? 0 : wfa_hint >= 0 ? wfa_hint : learned_hints().wfa);
    wfa_plan(j, sc, s_want, sw);
    out[0] = j.lds; out[1] = j.s_cap; out[2] = j.blk_rows; out[3] = j.n_ckpt; out[4] = (int64_t)j.ws_bytes; out[5] = wfa_class(j, sc, sw);
    return 0;
}

} // extern "C"
