// lcd_split.cpp -- lcd_chunk_split_reads: the records of a device-resident chunk as per-haplotype FASTQ entries and haplotag list lines, formatted where the
// inflate left them (split_kernel.hip).  Per chunk: one job per record of the plan goes up, the measure pass's rows come down, the host's prefix sums go back in
// them and the emit pass fills the four buffers; only rows, statistics and (compressed) text cross PCIe.  The options' check, the paths and the prefix sums are
// host code in lcd_split_format.cpp.
#include "lcd_host_internal.h"

using namespace lcd_internal;

struct lcd_split_s { DevBuf buf[4]; size_t size[4] = {0, 0, 0, 0}; int device = 0; };

// ---- the read sets of a driver run ----
namespace lcd_internal __attribute__((visibility("hidden"))) {
int SplitSink::parse(const std::string &W, const lcd_run_ext2_t *ext2, lcd_run_ext2_split_t *xs, int n_other, const char *const *other) {
    memset(xs, 0, sizeof(*xs));
    // a caller that knows the shorter struct gets a run without read sets; so does one whose size lies beyond this struct: it holds a layout this library does
    // not know, and only the bytes of lcd_run_ext2_t are certain to be there
    if (!ext2 || ext2->size <= sizeof(lcd_run_ext2_t) || ext2->size > sizeof(*xs)) return 0;
    memcpy(xs, ext2, ext2->size);
    if (xs->split_stats) memset(xs->split_stats, 0, sizeof(*xs->split_stats));
    if (!xs->split_prefix && (xs->split_gz || xs->split_comment)) return set_err(-4, W + ": split_gz / split_comment need split_prefix");
    if (!xs->split_prefix && !xs->haplotag_path) return 0;
    if (xs->split_prefix && (!xs->split_prefix[0] || !strcmp(xs->split_prefix, "-"))) return set_err(-4, W + ": the read sets go to files (split_prefix is empty or \"-\")");
    if (xs->haplotag_path && (!xs->haplotag_path[0] || !strcmp(xs->haplotag_path, "-"))) return set_err(-4, W + ": the haplotag list goes to a file (haplotag_path is empty or \"-\")");
    std::vector<const char *> all(other, other + n_other);
    all.push_back(xs->haplotag_path);
    char *p[3];
    const int rc = lcd_split_paths(xs->split_prefix, xs->split_gz, (int)all.size(), all.data(), p);
    for (char *q : p) free(q);
    if (rc) return set_err(rc, W + ": the read sets, the haplotag list and the other outputs of the run name one file");
    return 0;
}
int SplitSink::open(const std::string &W, const lcd_run_ext2_split_t &xs, int n_ref, const char *const *ref_names, int sort) {
    lcd_split_opt_default(&opt); opt.comment = xs.split_comment != 0; opt.list = xs.haplotag_path != nullptr;
    memset(&sum, 0, sizeof(sum)); stats_out = xs.split_stats; gz = xs.split_gz != 0; sort_output = sort;
    if (opt.list) { names = lcd_sam_names_create(n_ref, ref_names); if (!names) return -30; }
    if (xs.split_prefix) {
        char *p[3];
        if (int rc = lcd_split_paths(xs.split_prefix, gz, 0, nullptr, p)) return set_err(rc, W + ": no paths for the read sets");
        for (int s = 0; s < 3; ++s) { path[s] = p[s]; free(p[s]); }
    }
    if (opt.list) path[3] = xs.haplotag_path;
    for (int s = 0; s < 4; ++s) {
        if (path[s].empty()) continue;
        f[s] = fopen(path[s].c_str(), "wb");
        if (!f[s]) { const int rc = set_err(-30, W + ": cannot open " + path[s] + " for writing"); const std::string m = g_err; drop(); g_err = m; return rc; }
    }
    static const char head[] = "#readname\thaplotype\tphaseset\tchromosome\n";
    if (f[3] && fwrite(head, 1, sizeof(head) - 1, f[3]) != sizeof(head) - 1) return set_err(-30, W + ": short write on " + path[3]);
    return 0;
}
void SplitSink::drop() {
    for (int s = 0; s < 4; ++s) if (f[s]) { fclose(f[s]); remove(path[s].c_str()); f[s] = nullptr; }
    if (names) { lcd_sam_names_free(names); names = nullptr; }
}
// stream s of a chunk's result to its file
int SplitSink::put(int s, const lcd_split_t *h) {
    const size_t n = lcd_split_size(h, s);
    if (!f[s] || !n) return 0;
    std::vector<uint8_t> host;
    if (gz && s < 3) {
        const double t0 = now_ms();
        lcd_deflated_t *d = lcd_bgzf_deflate_dev_ptr(lcd_split_dev_ptr(h, s), n, 0, 0);
        if (!d) return -30;
        const double t1 = now_ms();
        host.resize(lcd_deflated_size(d));
        const int rc = lcd_deflated_to_host(d, 0, host.size(), host.data());
        lcd_deflated_free(d);
        if (rc) return rc;
        sum.ms_deflate += t1 - t0;
    } else {
        host.resize(n);
        if (int rc = lcd_split_to_host(h, s, 0, n, host.data())) return rc;
    }
    const double t2 = now_ms();
    if (fwrite(host.data(), 1, host.size(), f[s]) != host.size()) return set_err(-30, "short write on " + path[s]);
    sum.ms_download_write += now_ms() - t2;
    return 0;
}
int SplitSink::window(int n, const lcd_call_chunk_t *chunks, const int *tids, const lcd_stitch_carry_t *prev) {
    for (int c = 0; c < n; ++c) {
        const lcd_first_chunk_t &x = chunks[c].first; const lcd_chunk_s *k = x.chunk;
        if (!k) return set_err(-4, "the read sets: a chunk without its handle");
        // the plan of lcd_bam_writer_append for this chunk (rules 4 and 5), whether or not that writer runs
        bool has_prev = c > 0 && (!tids || tids[c - 1] == tids[c]);
        int64_t pb = has_prev ? chunks[c - 1].first.reg_beg : 0, pe = has_prev ? chunks[c - 1].first.reg_end : 0;
        if (c == 0 && prev && prev->valid && (!tids || prev->tid == tids[0])) { has_prev = true; pb = prev->reg_beg; pe = prev->reg_end; }
        const int n_rec = (int)k->rec_beg.size();
        std::vector<uint8_t> skip((size_t)n_rec + 1); std::vector<int> order((size_t)n_rec + 1);
        const int n_out = lcd_merged_record_plan(n_rec, k->rec_file.data(), k->rec_pos0.data(), k->rec_endpos.data(), has_prev, pb, pe, sort_output != 0, skip.data(), order.data());
        if (n_out < 0) return n_out;
        lcd_split_stats_t ss;
        lcd_split_t *h = lcd_chunk_split_reads(k, x.state ? x.state->haps : nullptr, x.state ? x.state->phase_sets : nullptr, skip.data(), order.data(), names, &opt, &ss);
        if (!h) return -30;
        int rc = 0;
        for (int s = 0; s < 4 && !rc; ++s) rc = put(s, h);
        lcd_split_free(h);
        if (rc) return rc;
        int64_t *a = &sum.n_records; const int64_t *b = &ss.n_records;
        for (int i = 0; i < 14; ++i) a[i] += b[i];                               // (every counter in front of the times)
        sum.ms_measure += ss.ms_measure; sum.ms_emit += ss.ms_emit;
    }
    return 0;
}
int SplitSink::finish(bool ok) {
    if (!active()) return 0;
    int rc = 0;
    if (ok && gz) {                                                              // the EOF member of every FASTQ file
        lcd_deflated_t *d = lcd_bgzf_deflate_dev(nullptr, 0, 0, 1);
        uint8_t eof[28];
        if (!d || lcd_deflated_size(d) != 28 || lcd_deflated_to_host(d, 0, 28, eof)) rc = -30;
        lcd_deflated_free(d);
        for (int s = 0; s < 3 && !rc; ++s) if (f[s] && fwrite(eof, 1, 28, f[s]) != 28) rc = set_err(-30, "short write on " + path[s]);
    }
    if (ok && !rc) {
        for (int s = 0; s < 4; ++s) {
            if (!f[s]) continue;
            const bool bad = fclose(f[s]) != 0;
            f[s] = nullptr;
            if (bad) { rc = set_err(-30, "closing " + path[s] + " failed"); break; }
        }
    }
    if (!ok || rc) {
        const std::string m = g_err;
        drop();
        for (int s = 0; s < 4; ++s) if (!path[s].empty()) remove(path[s].c_str());       // (the files closed before the one that failed)
        g_err = m;
        return rc ? -30 : 0;
    }
    if (names) { lcd_sam_names_free(names); names = nullptr; }
    if (stats_out) *stats_out = sum;
    return 0;
}
} // namespace lcd_internal

extern "C" {

lcd_split_t *lcd_chunk_split_reads(const lcd_chunk_t *c, const int *haps, const int64_t *phase_sets, const uint8_t *skip, const int *order, const lcd_sam_names_t *names,
                                   const lcd_split_opt_t *opt, lcd_split_stats_t *stats) {
    const std::string W = "lcd_chunk_split_reads";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->pending) { set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)"); return nullptr; }
    if (!opt || lcd_split_opt_check(opt)) { set_err(-4, W + ": NULL options, or comment / list outside 0 and 1"); return nullptr; }
    if (c->n_reads > 0 && !haps) { set_err(-4, W + ": NULL haps"); return nullptr; }
    for (int r = 0; r < c->n_reads; ++r) if (haps[r] < 0 || haps[r] > 2) { set_err(-4, W + ": a haplotype outside 0 ... 2"); return nullptr; }
    if (opt->list && !names) { set_err(-4, W + ": the list needs the contigs' names (lcd_sam_names_create)"); return nullptr; }
    if (opt->list && names->device != c->device) { set_err(-4, W + ": the chunk and the names are on different devices"); return nullptr; }
    std::vector<int> pick;
    if (pick_selected(W, c, skip, order, pick)) return nullptr;
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    const int n = (int)pick.size();
    std::vector<SplitJob> jobs((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int i = pick[k], r = c->rec_read[i];
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        SplitJob &j = jobs[k];
        j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.hap = r >= 0 ? haps[r] : 0; j.ps = r >= 0 && phase_sets ? phase_sets[r] : 0;
    }
    if (use_device(c->device)) return nullptr;
    std::unique_ptr<lcd_split_s> h(new lcd_split_s());
    h->device = c->device;
    lcd_split_stats_t s; memset(&s, 0, sizeof(s));
    s.n_records = n;
    if (n == 0) { if (stats) *stats = s; return h.release(); }
    StreamGuard st; if (st.create()) return nullptr;
    DevBuf d_jobs, d_rows;
    if (d_jobs.ensure((size_t)n * sizeof(SplitJob), 31) || d_rows.ensure((size_t)n * sizeof(SplitRow), 31)) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_split_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define PCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    SplitIn in; memset(&in, 0, sizeof(in));
    in.jobs = (const SplitJob *)d_jobs.p; in.n_jobs = n; in.comment = opt->comment; in.list = opt->list;
    if (opt->list) { in.names = (const uint8_t *)names->pool.p; in.name_off = (const unsigned *)names->offs.p; in.n_ref = names->n_ref; }
    const double w0 = now_ms();
    PCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(SplitJob), hipMemcpyHostToDevice, st));
    lcd_launch_split_measure(in, (SplitRow *)d_rows.p, st);
    PCHK(hipGetLastError());
    std::vector<SplitRow> rows((size_t)n);
    PCHK(hipMemcpyAsync(rows.data(), d_rows.p, (size_t)n * sizeof(SplitRow), hipMemcpyDeviceToHost, st));
    PCHK(hipStreamSynchronize(st));
    const double w1 = now_ms();
    std::vector<int> stream((size_t)n); std::vector<uint64_t> fl((size_t)n), ll((size_t)n), fo((size_t)n), lo((size_t)n);
    const size_t name_max = opt->list ? names->pool_bytes : 0;
    for (int k = 0; k < n; ++k) {
        const SplitRow &o = rows[k];
        // what the emit pass writes is what was measured: an entry is two copies of l_seq <= the record's bytes, a name and at most 64 more; a line is a name,
        // a contig's name and at most 64 more
        const bool in_out = o.stream >= 0;
        if (o.stream < -1 || o.stream > 2 || (in_out && o.stream != jobs[k].hap) || (!in_out && (o.fq_len || o.list_len || !(o.flags & 3u))) || (in_out && (o.flags & 3u)) ||
            o.fq_len > 4ull * jobs[k].len + 320 || o.list_len > 320ull + name_max || (in_out && !o.fq_len != !!(o.flags & LCD_SPLIT_NO_SEQ)) || (in_out && !o.list_len != !opt->list)) {
            set_err(-24, W + ": inconsistent measure pass"); return nullptr;
        }
        stream[k] = o.stream; fl[k] = o.fq_len; ll[k] = o.list_len;
        if (!in_out) { ++((o.flags & LCD_SPLIT_NOT_PRIMARY) ? s.n_not_primary : s.n_bad_layout); continue; }
        ++s.n_selected; ++s.n_hap[o.stream];
        s.n_filtered_primary += c->rec_read[pick[k]] < 0; s.n_reverse += (o.flags & LCD_SPLIT_REVERSE) != 0; s.n_no_seq += (o.flags & LCD_SPLIT_NO_SEQ) != 0;
    }
    uint64_t tot[4];
    if (lcd_split_offsets(n, stream.data(), fl.data(), ll.data(), fo.data(), lo.data(), tot)) { set_err(-24, W + ": the lengths do not add up"); return nullptr; }
    for (int k = 0; k < n; ++k) { rows[k].fq_off = fo[k]; rows[k].list_off = lo[k]; }
    for (int b = 0; b < 4; ++b) { h->size[b] = (size_t)tot[b]; if (h->buf[b].ensure((size_t)tot[b] + 64, 31)) return nullptr; }
    for (int b = 0; b < 3; ++b) s.bytes_fastq[b] = (int64_t)tot[b];
    s.bytes_list = (int64_t)tot[3];
    PCHK(hipMemcpyAsync(d_rows.p, rows.data(), (size_t)n * sizeof(SplitRow), hipMemcpyHostToDevice, st));
    lcd_launch_split_emit(in, (const SplitRow *)d_rows.p, (uint8_t *)h->buf[0].p, (uint8_t *)h->buf[1].p, (uint8_t *)h->buf[2].p, (uint8_t *)h->buf[3].p, st);
    PCHK(hipGetLastError());
    PCHK(hipStreamSynchronize(st));
#undef PCHK
    s.ms_measure = w1 - w0; s.ms_emit = now_ms() - w1;
    if (stats) *stats = s;
    return h.release();
}
size_t lcd_split_size(const lcd_split_t *h, int stream) { return h && stream >= 0 && stream < 4 ? h->size[stream] : 0; }
uint64_t lcd_split_dev_ptr(const lcd_split_t *h, int stream) { return h && stream >= 0 && stream < 4 ? h->buf[stream].addr() : 0; }
int lcd_split_to_host(const lcd_split_t *h, int stream, size_t off, size_t n, uint8_t *out) {
    if (!h || stream < 0 || stream > 3 || off > h->size[stream] || n > h->size[stream] - off || (n && !out)) return set_err(-41, "lcd_split_to_host: no such stream, or a range past its end");
    if (n == 0) return 0;
    if (use_device(h->device)) return -1;
    HIPCHK(hipMemcpy(out, (const uint8_t *)h->buf[stream].p + off, n, hipMemcpyDeviceToHost));
    return 0;
}
void lcd_split_free(lcd_split_t *h) { delete h; }

} // extern "C"
