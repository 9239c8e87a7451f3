// lcd_mods.cpp -- lcd_chunk_mod_pileup: the per-haplotype CpG methylation table of a device-resident chunk from the MM / ML tags of its kept records, read where
// the inflate left them (mods_kernel.hip).  Per chunk: the window and one job per kept record go up, the site map, its scan, the pile-up and the compaction run,
// the statistics and the non-empty rows come down.  The options' check, the strand combination and the text are host code in lcd_mods_format.cpp.
#include "lcd_host_internal.h"

using namespace lcd_internal;

struct lcd_mods_s { std::vector<int64_t> pos; std::vector<char> strand; std::vector<uint32_t> counts; };

// ---- the table of a driver run ----
namespace lcd_internal __attribute__((visibility("hidden"))) {
int ModsSink::parse(const std::string &W, const lcd_run_ext2_t *ext2, lcd_run_ext2_t *x2, lcd_mods_opt_t *mo) {
    memset(x2, 0, sizeof(*x2));
    lcd_mods_opt_default(mo);
    if (!ext2) return 0;
    // the caller's struct may be older (shorter) or newer (longer) than this one: what lies behind its `size` reads as zero, what lies behind ours is not looked at
    if (ext2->size < offsetof(lcd_run_ext2_t, mods_path) + sizeof(x2->mods_path)) return set_err(-4, W + ": lcd_run_ext2_t.size does not reach its first option");
    memcpy(x2, ext2, std::min(ext2->size, sizeof(*x2)));
    if (x2->mods_stats) memset(x2->mods_stats, 0, sizeof(*x2->mods_stats));
    if (!x2->mods_path) return 0;
    if (x2->mods_code) mo->code = x2->mods_code;
    if (x2->mods_threshold) mo->threshold = x2->mods_threshold;
    mo->combine_strands = x2->mods_combine_strands != 0;
    if (lcd_mods_opt_check(mo)) return set_err(-4, W + ": the methylation table's code must be m or h and its threshold 128 ... 255");
    if (!x2->mods_path[0] || !strcmp(x2->mods_path, "-")) return set_err(-4, W + ": the methylation table goes to a file (mods_path is empty or \"-\")");
    return 0;
}
int ModsSink::open(const std::string &W, const lcd_run_ext2_t &x2, const lcd_mods_opt_t &mo) {
    opt = mo; memset(&sum, 0, sizeof(sum)); stats_out = x2.mods_stats; path = x2.mods_path; head = held = false;
    f = fopen(path.c_str(), "wb");
    return f ? 0 : set_err(-30, W + ": cannot open " + path + " for writing");
}
int ModsSink::put(int n, const int64_t *pos, const char *strand, const uint32_t *cnt, const char *chrom) {
    char *text = nullptr;
    if (int rc = lcd_mods_format(n, pos, strand, cnt, chrom, opt.code, head ? 0 : 1, &text)) return set_err(rc, "formatting the methylation table failed");
    head = true;
    const size_t len = strlen(text);
    const bool ok = fwrite(text, 1, len, f) == len;
    free(text);
    sum.n_rows += n;
    return ok ? 0 : set_err(-30, "short write on the methylation table " + path);
}
int ModsSink::flush_held() {
    if (!held) return 0;
    held = false;
    const char dot = '.';
    return put(1, &held_pos, &dot, held_cnt, held_chrom.c_str());
}
int ModsSink::chunk(const lcd_chunk_t *handle, const lcd_first_chunk_t &x, const char *chrom) {
    lcd_mods_opt_t o = opt; o.ref_seq = (const char *)x.ref_seq; o.ref_beg = x.ref_beg; o.ref_end = x.ref_end;
    lcd_mods_stats_t ms;
    lcd_mods_t *m = mod_pileup_core(handle, x.state ? x.state->haps : nullptr, &o, &ms, scratch);
    if (!m) return -1;
    const int n = lcd_mods_n_rows(m);
    std::vector<int64_t> pos((size_t)n + 1); std::vector<char> strand((size_t)n + 1); std::vector<uint32_t> cnt(9 * ((size_t)n + 1));
    lcd_mods_rows_to_host(m, pos.data(), strand.data(), cnt.data());
    lcd_mods_free(m);
    int64_t *a = &sum.n_records; const int64_t *b = &ms.n_records;
    for (int k = 0; k < 13; ++k) a[k] += b[k];                                  // (the counters in front of n_rows, which counts the lines written)
    sum.ms_site_map += ms.ms_site_map; sum.ms_pileup += ms.ms_pileup; sum.ms_compact += ms.ms_compact;
    // combine_strands: a CpG cut by the end of the chunk before left its row held back; it is this chunk's first row when contig and key are equal
    int first = 0;
    if (held && n > 0 && held_chrom == chrom && held_pos == pos[0]) { for (int z = 0; z < 9; ++z) held_cnt[z] += cnt[z]; first = 1; }
    if (n - first > 0 || (held && held_chrom != chrom)) if (int rc = flush_held()) return rc;
    int last = n;
    if (opt.combine_strands && n - first > 0) { last = n - 1; held = true; held_chrom = chrom; held_pos = pos[last]; memcpy(held_cnt, &cnt[9 * (size_t)last], 36); }
    if (last - first > 0) return put(last - first, pos.data() + first, strand.data() + first, cnt.data() + 9 * (size_t)first, chrom);
    return 0;
}
int ModsSink::finish(bool ok) {
    if (!f) return 0;
    int rc = 0;
    if (ok) { rc = flush_held(); if (!rc && !head) rc = put(0, nullptr, nullptr, nullptr, ""); }     // (a table without a row still has its header line)
    if (fclose(f) != 0 && ok && !rc) rc = set_err(-30, "closing the methylation table " + path + " failed");
    f = nullptr;
    if (!ok || rc) { remove(path.c_str()); return rc ? -30 : 0; }
    if (stats_out) *stats_out = sum;
    return 0;
}

lcd_mods_t *mod_pileup_core(const lcd_chunk_t *c, const int *haps, const lcd_mods_opt_t *opt, lcd_mods_stats_t *stats, ModsScratch &B) {
    const std::string W = "lcd_chunk_mod_pileup";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->pending) { set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)"); return nullptr; }
    if (!opt || lcd_mods_opt_check(opt)) { set_err(-4, W + ": NULL options, a code outside m / h or a threshold outside 128 ... 255"); return nullptr; }
    if (!opt->ref_seq || opt->ref_end < opt->ref_beg) { set_err(-4, W + ": no reference window"); return nullptr; }
    if (c->n_reads > 0 && !haps) { set_err(-4, W + ": NULL haps"); return nullptr; }
    for (int r = 0; r < c->n_reads; ++r) if (haps[r] < 0 || haps[r] > 2) { set_err(-4, W + ": a haplotype outside 0 ... 2"); return nullptr; }
    const int64_t reg_beg = c->reg_beg, reg_end = c->reg_end, n_pos = reg_end - reg_beg + 1;
    if (n_pos < 1 || n_pos > (int64_t)INT32_MAX - 1024) { set_err(-4, W + ": the chunk's region is empty or longer than 2^31"); return nullptr; }
    std::unique_ptr<lcd_mods_s> h(new lcd_mods_s());
    // one job per kept record, its class bytes in one arena (l_seq bytes each)
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    std::vector<ModsJob> jobs; uint64_t arena = 0;
    for (size_t i = 0; i < c->rec_beg.size(); ++i) {
        const int r = c->rec_read[i];
        if (r < 0) continue;
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads || c->qlen[r] < 0) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        ModsJob j; j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.cap = (uint32_t)c->qlen[r]; j.hap = haps[r]; j.pad = 0; j.cls = arena;
        arena += lcd_align_up((uint64_t)j.cap, 16);
        jobs.push_back(j);
    }
    const int n = (int)jobs.size();
    if (use_device(c->device)) return nullptr;
    StreamGuard st; if (st.create()) return nullptr;
    const size_t ref_len = (size_t)(opt->ref_end - opt->ref_beg + 1);
    DevBuf &d_jobs = B.d_jobs, &d_cls = B.d_cls, &d_ref = B.d_ref, &d_idx = B.d_idx, &d_small = B.d_small, &d_tab = B.d_tab, &d_rows = B.d_rows;
    if (d_jobs.ensure((size_t)std::max(n, 1) * sizeof(ModsJob)) || d_cls.ensure((size_t)arena + 64) || d_ref.ensure(ref_len + 64) || d_idx.ensure((size_t)n_pos * 4 + 64) ||
        d_small.ensure(256)) return nullptr;
    for (ModsJob &j : jobs) j.cls += d_cls.addr();
    std::vector<uint8_t> codes(ref_len);                                // the window as codes 0-4, whatever it came as
    for (size_t k = 0; k < ref_len; ++k) {
        const uint8_t b = (uint8_t)opt->ref_seq[k];
        codes[k] = b <= 4 ? b : (b == 'A' || b == 'a') ? 0 : (b == 'C' || b == 'c') ? 1 : (b == 'G' || b == 'g') ? 2 : (b == 'T' || b == 't') ? 3 : 4;
    }
    auto hipfail = [&](const char *what) -> lcd_mods_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define MCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    // d_small: [0, 96) the twelve statistics, [96] the number of sites, [100] the number of rows
    unsigned long long *d_stats = (unsigned long long *)d_small.p; int *d_nsites = (int *)((uint8_t *)d_small.p + 96), *d_nrows = d_nsites + 1;
    ModsIn in; memset(&in, 0, sizeof(in));
    in.jobs = (const ModsJob *)d_jobs.p; in.ref = (const uint8_t *)d_ref.p; in.site_idx = (const int *)d_idx.p; in.stats = d_stats;
    in.ref_beg = opt->ref_beg; in.ref_end = opt->ref_end; in.reg_beg = reg_beg; in.reg_end = reg_end; in.n_jobs = n; in.code = opt->code; in.threshold = opt->threshold;
    const double w0 = now_ms();
    MCHK(hipMemsetAsync(d_small.p, 0, 256, st));
    MCHK(hipMemcpyAsync(d_ref.p, codes.data(), ref_len, hipMemcpyHostToDevice, st));
    if (n) MCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(ModsJob), hipMemcpyHostToDevice, st));
    lcd_launch_mods_sites(in, (int *)d_idx.p, n_pos, st);
    MCHK(hipGetLastError());
    lcd_launch_cv_scan((int *)d_idx.p, (int)n_pos, d_nsites, st);
    MCHK(hipGetLastError());
    int n_sites = 0;
    MCHK(hipMemcpyAsync(&n_sites, d_nsites, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    const double w1 = now_ms();
    if (n_sites < 0 || n_sites > n_pos) { set_err(-24, W + ": inconsistent site map"); return nullptr; }
    if (d_tab.ensure((size_t)std::max(n_sites, 1) * 36 + 64) || d_rows.ensure((size_t)std::max(n_sites, 1) * sizeof(ModsRow))) return nullptr;
    in.tab = (unsigned *)d_tab.p;
    MCHK(hipMemsetAsync(d_tab.p, 0, (size_t)std::max(n_sites, 1) * 36, st));
    lcd_launch_mods_pileup(in, st);
    MCHK(hipGetLastError());
    MCHK(hipStreamSynchronize(st));
    const double w2 = now_ms();
    int n_rows = 0; unsigned long long S[12];
    if (n_sites) { lcd_launch_mods_compact(in, n_pos, (ModsRow *)d_rows.p, d_nrows, st); MCHK(hipGetLastError()); }
    MCHK(hipMemcpyAsync(S, d_stats, sizeof(S), hipMemcpyDeviceToHost, st));
    MCHK(hipMemcpyAsync(&n_rows, d_nrows, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    if (n_rows < 0 || n_rows > n_sites) { set_err(-24, W + ": inconsistent compaction"); return nullptr; }
    std::vector<ModsRow> rows((size_t)n_rows);
    if (n_rows) MCHK(hipMemcpy(rows.data(), d_rows.p, (size_t)n_rows * sizeof(ModsRow), hipMemcpyDeviceToHost));
#undef MCHK
    std::sort(rows.begin(), rows.end(), [](const ModsRow &a, const ModsRow &b) { return a.pos < b.pos; });      // (a position holds at most one site)
    h->pos.resize(n_rows); h->strand.resize(n_rows); h->counts.resize((size_t)n_rows * 9);
    for (int k = 0; k < n_rows; ++k) { h->pos[k] = rows[k].pos; h->strand[k] = rows[k].strand == 1 ? '+' : '-'; memcpy(&h->counts[(size_t)k * 9], rows[k].count, 36); }
    if (opt->combine_strands && n_rows) {
        const int m = lcd_mods_combine_rows(n_rows, h->pos.data(), h->strand.data(), h->counts.data());
        h->pos.resize(m); h->strand.resize(m); h->counts.resize((size_t)m * 9);
    }
    if (stats) {
        int64_t *f = &stats->n_records;
        for (int k = 0; k < 12; ++k) f[k] = (int64_t)S[k];
        stats->n_sites = n_sites; stats->n_rows = (int64_t)h->pos.size();
        stats->ms_site_map = w1 - w0; stats->ms_pileup = w2 - w1; stats->ms_compact = now_ms() - w2;
    }
    return h.release();
}
} // namespace lcd_internal

extern "C" {

lcd_mods_t *lcd_chunk_mod_pileup(const lcd_chunk_t *c, const int *haps, const lcd_mods_opt_t *opt, lcd_mods_stats_t *stats) {
    ModsScratch B;
    return mod_pileup_core(c, haps, opt, stats, B);
}
int lcd_mods_n_rows(const lcd_mods_t *m) { return m ? (int)m->pos.size() : 0; }
int lcd_mods_rows_to_host(const lcd_mods_t *m, int64_t *pos, char *strand, uint32_t *counts) {
    if (!m) return set_err(-4, "lcd_mods_rows_to_host: NULL table");
    const size_t n = m->pos.size();
    if (n && (!pos || !strand || !counts)) return set_err(-4, "lcd_mods_rows_to_host: NULL output");
    if (n) { memcpy(pos, m->pos.data(), n * 8); memcpy(strand, m->strand.data(), n); memcpy(counts, m->counts.data(), n * 36); }
    return (int)n;
}
void lcd_mods_free(lcd_mods_t *m) { delete m; }

} // extern "C"
