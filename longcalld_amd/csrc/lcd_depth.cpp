// lcd_depth.cpp -- lcd_chunk_depth: the per-haplotype depth track of a device-resident chunk from the CIGARs of its kept records, read where the inflate left
// them (depth_kernel.hip).  Per chunk: one job per kept record goes up, the mark launch fills the difference array, the tile partials, their scan and the row
// launch turn it into rows; the statistics and the rows come down.  The options' check, the window rule and the text are host code in lcd_depth_format.cpp.
#include "lcd_host_internal.h"

using namespace lcd_internal;

struct lcd_depth_s { std::vector<int64_t> beg, end; std::vector<uint32_t> depth; };

// ---- the track of a driver run ----
namespace lcd_internal __attribute__((visibility("hidden"))) {
int DepthSink::parse(const std::string &W, const lcd_run_ext2_t &x2) {
    if (x2.depth_stats) memset(x2.depth_stats, 0, sizeof(*x2.depth_stats));
    if (!x2.depth_path) return 0;
    lcd_depth_opt_t o; lcd_depth_opt_default(&o); o.window = x2.depth_window;
    if (lcd_depth_opt_check(&o)) return set_err(-4, W + ": the depth track's window must be 0 ... 2^30");
    if (!x2.depth_path[0] || !strcmp(x2.depth_path, "-")) return set_err(-4, W + ": the depth track goes to a file (depth_path is empty or \"-\")");
    if (x2.mods_path && !strcmp(x2.depth_path, x2.mods_path)) return set_err(-4, W + ": the depth track and the methylation table name one file (depth_path equals mods_path)");
    return 0;
}
int DepthSink::open(const std::string &W, const lcd_run_ext2_t &x2) {
    lcd_depth_opt_default(&opt); opt.window = x2.depth_window; opt.skip_dels = x2.depth_skip_dels != 0;
    memset(&sum, 0, sizeof(sum)); stats_out = x2.depth_stats; path = x2.depth_path; head = held = false;
    f = fopen(path.c_str(), "wb");
    return f ? 0 : set_err(-30, W + ": cannot open " + path + " for writing");
}
int DepthSink::put(int n, const int64_t *beg, const int64_t *end, const uint64_t *val, const char *chrom) {
    std::vector<uint32_t> d;
    if (!opt.window) { d.resize(3 * (size_t)n + 3); for (size_t k = 0; k < 3 * (size_t)n; ++k) d[k] = (uint32_t)val[k]; }      // (per base the values are depths)
    char *text = nullptr;
    if (int rc = lcd_depth_format(n, beg, end, opt.window ? nullptr : d.data(), opt.window ? val : nullptr, chrom, head ? 0 : 1, &text)) return set_err(rc, "formatting the depth track failed");
    head = true;
    const size_t len = strlen(text);
    const bool ok = fwrite(text, 1, len, f) == len;
    free(text);
    sum.n_rows += n;
    return ok ? 0 : set_err(-30, "short write on the depth track " + path);
}
int DepthSink::flush_held() {
    if (!held) return 0;
    held = false;
    return put(1, &held_beg, &held_end, held_val, held_chrom.c_str());
}
int DepthSink::chunk(const lcd_chunk_t *handle, const lcd_first_chunk_t &x, const char *chrom) {
    lcd_depth_stats_t ds;
    lcd_depth_t *d = depth_core(handle, x.state ? x.state->haps : nullptr, &opt, &ds, scratch);
    if (!d) return -1;
    int n = lcd_depth_n_rows(d);
    std::vector<int64_t> beg = std::move(d->beg), end = std::move(d->end); std::vector<uint64_t> val(d->depth.begin(), d->depth.end());
    lcd_depth_free(d);
    int64_t *a = &sum.n_records; const int64_t *b = &ds.n_records;
    for (int k = 0; k < 8; ++k) a[k] += b[k];                                   // (the counters in front of n_rows, which counts the lines written)
    sum.ms_mark += ds.ms_mark; sum.ms_rows += ds.ms_rows;
    if (opt.window) {
        std::vector<uint32_t> dep(val.begin(), val.end());
        int64_t *wb = nullptr, *we = nullptr; uint64_t *ws = nullptr;
        const int m = lcd_depth_windows(n, beg.data(), end.data(), dep.data(), opt.window, &wb, &we, &ws);
        if (m < 0) return set_err(m, "lcd_depth_windows failed on a chunk's rows");
        beg.assign(wb, wb + m); end.assign(we, we + m); val.assign(ws, ws + 3 * (size_t)m); n = m;
        free(wb); free(we); free(ws);
    }
    if (n < 1) return set_err(-24, "a chunk without depth rows");             // (the rows tile the region)
    // the row held back joins this chunk's first row, or is written as it is
    if (held) {
        bool join = held_chrom == chrom && held_end + 1 == beg[0];
        if (join) join = opt.window ? (held_beg - 1) / opt.window == (beg[0] - 1) / opt.window : (held_val[0] == val[0] && held_val[1] == val[1] && held_val[2] == val[2]);
        if (join) { beg[0] = held_beg; if (opt.window) for (int h = 0; h < 3; ++h) val[h] += held_val[h]; held = false; }
        else if (int rc = flush_held()) return rc;
    }
    if (n > 1) if (int rc = put(n - 1, beg.data(), end.data(), val.data(), chrom)) return rc;
    held = true; held_chrom = chrom; held_beg = beg[n - 1]; held_end = end[n - 1]; memcpy(held_val, &val[3 * (size_t)(n - 1)], 24);
    return 0;
}
int DepthSink::finish(bool ok) {
    if (!f) return 0;
    int rc = 0;
    if (ok) { rc = flush_held(); if (!rc && !head) rc = put(0, nullptr, nullptr, nullptr, ""); }     // (a track without a row still has its header line)
    if (fclose(f) != 0 && ok && !rc) rc = set_err(-30, "closing the depth track " + path + " failed");
    f = nullptr;
    if (!ok || rc) { remove(path.c_str()); return rc ? -30 : 0; }
    if (stats_out) *stats_out = sum;
    return 0;
}

lcd_depth_t *depth_core(const lcd_chunk_t *c, const int *haps, const lcd_depth_opt_t *opt, lcd_depth_stats_t *stats, DepthScratch &B) {
    const std::string W = "lcd_chunk_depth";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->pending) { set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)"); return nullptr; }
    if (!opt) { set_err(-4, W + ": NULL options"); return nullptr; }
    if (c->n_reads > 0 && !haps) { set_err(-4, W + ": NULL haps"); return nullptr; }
    for (int r = 0; r < c->n_reads; ++r) if (haps[r] < 0 || haps[r] > 2) { set_err(-4, W + ": a haplotype outside 0 ... 2"); return nullptr; }
    const int64_t reg_beg = c->reg_beg, reg_end = c->reg_end, n_pos = reg_end - reg_beg + 1;
    if (n_pos < 1 || n_pos > (int64_t)INT32_MAX - 1024) { set_err(-4, W + ": the chunk's region is empty or longer than 2^31 - 1024"); return nullptr; }
    std::unique_ptr<lcd_depth_s> h(new lcd_depth_s());
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    std::vector<DepthJob> jobs;
    for (size_t i = 0; i < c->rec_beg.size(); ++i) {
        const int r = c->rec_read[i];
        if (r < 0) continue;
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads || c->qlen[r] < 0) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        DepthJob j; j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.cap = (uint32_t)c->qlen[r]; j.hap = haps[r]; j.pad = 0;
        jobs.push_back(j);
    }
    const int n = (int)jobs.size();
    if (use_device(c->device)) return nullptr;
    StreamGuard st; if (st.create()) return nullptr;
    const int64_t T = LCD_DEPTH_TILE, n_tiles = (n_pos + T - 1) / T, pitch = n_tiles * T;
    DevBuf &d_jobs = B.d_jobs, &d_diff = B.d_diff, &d_parts = B.d_parts, &d_small = B.d_small, &d_rows = B.d_rows;
    if (d_jobs.ensure((size_t)std::max(n, 1) * sizeof(DepthJob)) || d_diff.ensure((size_t)pitch * 12) || d_parts.ensure((size_t)n_tiles * sizeof(DepthPart)) || d_small.ensure(256)) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_depth_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define DCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    // d_small: [0, 64) the eight statistics in front of n_rows, [64] the number of rows
    unsigned long long *d_stats = (unsigned long long *)d_small.p; int *d_nrows = (int *)((uint8_t *)d_small.p + 64);
    DepthIn in; memset(&in, 0, sizeof(in));
    in.jobs = (const DepthJob *)d_jobs.p; in.diff = (int *)d_diff.p; in.stats = d_stats; in.reg_beg = reg_beg; in.reg_end = reg_end; in.n_pos = n_pos; in.pitch = pitch;
    in.n_jobs = n; in.skip_dels = opt->skip_dels != 0;
    const double w0 = now_ms();
    DCHK(hipMemsetAsync(d_small.p, 0, 256, st));
    DCHK(hipMemsetAsync(d_diff.p, 0, (size_t)pitch * 12, st));
    if (n) DCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(DepthJob), hipMemcpyHostToDevice, st));
    lcd_launch_depth_mark(in, st);
    DCHK(hipGetLastError());
    DCHK(hipStreamSynchronize(st));
    const double w1 = now_ms();
    lcd_launch_depth_tiles(in, (DepthPart *)d_parts.p, st);
    DCHK(hipGetLastError());
    lcd_launch_depth_scan((DepthPart *)d_parts.p, n_tiles, d_nrows, st);
    DCHK(hipGetLastError());
    int n_rows = 0; unsigned long long S[8];
    DCHK(hipMemcpyAsync(&n_rows, d_nrows, 4, hipMemcpyDeviceToHost, st));
    DCHK(hipMemcpyAsync(S, d_stats, sizeof(S), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    if (n_rows < 1 || n_rows > n_pos) { set_err(-24, W + ": inconsistent row count"); return nullptr; }
    if (d_rows.ensure((size_t)n_rows * sizeof(DepthRow))) return nullptr;
    lcd_launch_depth_rows(in, (const DepthPart *)d_parts.p, (DepthRow *)d_rows.p, n_rows, st);
    DCHK(hipGetLastError());
    std::vector<DepthRow> rows((size_t)n_rows);
    DCHK(hipMemcpyAsync(rows.data(), d_rows.p, (size_t)n_rows * sizeof(DepthRow), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
#undef DCHK
    h->beg.resize(n_rows); h->end.resize(n_rows); h->depth.resize((size_t)n_rows * 3);
    for (int k = 0; k < n_rows; ++k) {                                          // (position order: a row ends in front of the next one)
        if (rows[k].beg < reg_beg || rows[k].beg > reg_end || (k > 0 && rows[k].beg <= rows[k - 1].beg)) { set_err(-24, W + ": rows out of order"); return nullptr; }
        h->beg[k] = rows[k].beg; h->end[k] = k + 1 < n_rows ? rows[k + 1].beg - 1 : reg_end; memcpy(&h->depth[(size_t)k * 3], rows[k].d, 12);
    }
    if (stats) {
        int64_t *f = &stats->n_records;
        for (int k = 0; k < 8; ++k) f[k] = (int64_t)S[k];
        stats->n_rows = n_rows; stats->ms_mark = w1 - w0; stats->ms_rows = now_ms() - w1;
    }
    return h.release();
}
} // namespace lcd_internal

extern "C" {

lcd_depth_t *lcd_chunk_depth(const lcd_chunk_t *c, const int *haps, const lcd_depth_opt_t *opt, lcd_depth_stats_t *stats) {
    DepthScratch B;
    return depth_core(c, haps, opt, stats, B);
}
int lcd_depth_n_rows(const lcd_depth_t *d) { return d ? (int)d->beg.size() : 0; }
int lcd_depth_rows_to_host(const lcd_depth_t *d, int64_t *beg, int64_t *end, uint32_t *depth) {
    if (!d) return set_err(-4, "lcd_depth_rows_to_host: NULL track");
    const size_t n = d->beg.size();
    if (n && (!beg || !end || !depth)) return set_err(-4, "lcd_depth_rows_to_host: NULL output");
    if (n) { memcpy(beg, d->beg.data(), n * 8); memcpy(end, d->end.data(), n * 8); memcpy(depth, d->depth.data(), n * 12); }
    return (int)n;
}
void lcd_depth_free(lcd_depth_t *d) { delete d; }

} // extern "C"
