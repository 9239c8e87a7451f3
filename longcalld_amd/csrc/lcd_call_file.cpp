// lcd_call_file.cpp -- a whole BAM in one call (longcallD call ref.fa in.bam -o out.vcf -b out.bam): the chunk plan of collect_regions (src/call_var_main.c:404-634),
// the BAM header's contigs and sample name, the VCF writer, and the driver that runs call_var_worker_pipeline (:762-815) for the germline path over windows of
// chunks: load (lcd_chunk_open_from_bam / lcd_fasta_fetch / lcd_chunk_resolve), call (chunks_call_core with the stitch carried across windows), write (the VCF and
// the appendable BAM writer).  Everything here composes exports that exist; no kernel is launched from this file.
// lcd_call_files runs the same driver over the alignment files of one sample (-X / -L, src/call_var_main.c:361-400, 640-741): every chunk is opened from all files at once
// (lcd_chunk_open_from_bams), file 0 gives the contigs, the headers and the sample name, every further file must carry its reference table (LCD_ERR_INPUT_HEADERS).
// lcd_haplotag_files is the same run with another middle stage: files_run() takes the stage as a parameter (TagStage: lcd_chunk_haplotag against a phased VCF
// instead of chunks_call_core) and writes no VCF; plan, windows, load, write and the closing order are shared.
#include <condition_variable>
#include <ctime>
#include "lcd_host_internal.h"

using namespace lcd_internal;

struct lcd_vcf_writer_s {
    FILE *f = nullptr; bool own = false, bgzf = false; std::string path;
    // lcd_vcf_writer_open_idx: the builder of the output's .tbi / .csi (NULL: none, or given up), where the index goes, the file offset of the next member, the
    // append's text in HBM (uploaded once: the deflater and the builder read the same buffer)
    lcd_vcf_index_builder_t *vidx = nullptr; std::string index_path; uint64_t file_off = 0; lcd_vcf_index_stats_t *vstats = nullptr; DevBuf d_text; int device = 0;
    ~lcd_vcf_writer_s() { lcd_vcf_index_builder_destroy(vidx); }
};

namespace {
char *dup_str(const std::string &s) { char *p = (char *)malloc(s.size() + 1); memcpy(p, s.c_str(), s.size() + 1); return p; }
template <class T> T *dup_vec(const std::vector<T> &v) { T *p = (T *)malloc((v.size() + 1) * sizeof(T)); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

// the header block of a BAM: its text and its reference table
int bam_header_parts(const char *bam_path, std::string &text, std::vector<std::string> &names, std::vector<int64_t> &lens, const std::string &W) {
    std::vector<uint8_t> hdr;
    if (lcd_io_bam_header(bam_path, hdr)) return set_err(-30, W + ": " + lcd_io_last_error());
    int l_text = 0; memcpy(&l_text, hdr.data() + 4, 4);
    text.assign((const char *)hdr.data() + 8, (size_t)l_text);
    while (!text.empty() && text.back() == 0) text.pop_back();
    size_t o = 8 + (size_t)l_text;
    int n_ref = 0; memcpy(&n_ref, hdr.data() + o, 4); o += 4;
    for (int i = 0; i < n_ref; ++i) {
        int ln = 0; memcpy(&ln, hdr.data() + o, 4); o += 4;
        names.emplace_back((const char *)hdr.data() + o, (size_t)std::max(ln - 1, 0)); o += (size_t)ln;
        int tl = 0; memcpy(&tl, hdr.data() + o, 4); o += 4;
        lens.push_back(tl);
    }
    return 0;
}

// classify_chromosome, src/call_var_main.c:411-446: 0 autosome, 1 sex chromosome, 2 other
int classify_chromosome(const std::string &name) {
    std::string s = name.substr(0, name.find(':'));
    if (s.compare(0, 3, "chr") == 0) s = s.substr(3);
    if (s == "X" || s == "Y") return 1;
    if (s == "MT" || s == "M") return 2;
    char *end = nullptr;
    const long num = strtol(s.c_str(), &end, 10);
    return (*end == '\0' && num >= 1) ? 0 : 2;
}

struct Reg { int tid; int64_t beg, end; };
// "1,234" -> 1234; false when the text is not a number
bool parse_pos(std::string s, int64_t &v) {
    s.erase(std::remove(s.begin(), s.end(), ','), s.end());
    if (s.empty()) return false;
    char *end = nullptr;
    v = strtoll(s.c_str(), &end, 10);
    return *end == '\0';
}
} // namespace

extern "C" {

int lcd_bam_contigs(const char *bam_path, int *n, char ***names, int64_t **lens) {
    const std::string W = "lcd_bam_contigs";
    if (n) *n = 0;
    if (names) *names = nullptr;
    if (lens) *lens = nullptr;
    if (!bam_path || !n || !names || !lens) return set_err(-4, W + ": NULL argument");
    std::string text; std::vector<std::string> nm; std::vector<int64_t> ln;
    if (int rc = bam_header_parts(bam_path, text, nm, ln, W)) return rc;
    char **out = (char **)malloc((nm.size() + 1) * sizeof(char *));
    for (size_t i = 0; i < nm.size(); ++i) out[i] = dup_str(nm[i]);
    *n = (int)nm.size(); *names = out; *lens = dup_vec(ln);
    return 0;
}
void lcd_bam_contigs_free(int n, char **names, int64_t *lens) {
    for (int i = 0; names && i < n; ++i) free(names[i]);
    free(names); free(lens);
}

int lcd_bam_sample_name(const char *bam_path, char **name) {
    const std::string W = "lcd_bam_sample_name";
    if (name) *name = nullptr;
    if (!bam_path || !name) return set_err(-4, W + ": NULL argument");
    std::string text; std::vector<std::string> nm; std::vector<int64_t> ln;
    if (int rc = bam_header_parts(bam_path, text, nm, ln, W)) return rc;
    for (size_t o = 0; o < text.size();) {
        size_t e = text.find('\n', o); if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(o, e - o); o = e + 1;
        if (line.compare(0, 4, "@RG\t") != 0) continue;
        for (size_t f = 4; f <= line.size();) {
            size_t t = line.find('\t', f); if (t == std::string::npos) t = line.size();
            if (t - f >= 3 && line.compare(f, 3, "SM:") == 0) { *name = dup_str(line.substr(f + 3, t - f - 3)); return 0; }   // the first one is kept whatever follows
            f = t + 1;
        }
    }
    return 0;
}

void lcd_chunk_plan_free(lcd_chunk_plan_t *p) {
    if (!p) return;
    free(p->tid); free(p->reg_beg); free(p->reg_end);
    memset(p, 0, sizeof(*p));
}

int lcd_plan_chunks(int n_contigs, const char *const *names, const int64_t *lens, int contig_mode, int n_exclude, const char *const *exclude, int n_regions,
                    const char *const *regions, const char *bed_path, int64_t chunk_len, lcd_chunk_plan_t *out) {
    const std::string W = "lcd_plan_chunks";
    if (out) memset(out, 0, sizeof(*out));
    if (!out || n_contigs < 0 || (n_contigs > 0 && (!names || !lens)) || n_exclude < 0 || (n_exclude > 0 && !exclude) || n_regions < 0 || (n_regions > 0 && !regions))
        return set_err(-4, W + ": bad argument");
    if (contig_mode != LCD_CTG_AUTOSOME_XY && contig_mode != LCD_CTG_AUTOSOME && contig_mode != LCD_CTG_ALL) return set_err(-4, W + ": unknown contig mode");
    if (chunk_len < 0) return set_err(-4, W + ": chunk_len < 0");
    const int64_t L = chunk_len ? chunk_len : 500000;
    auto tid_of = [&](const std::string &s) { for (int i = 0; i < n_contigs; ++i) if (s == names[i]) return i; return -1; };
    // skip_target_region, :464-470
    auto skipped = [&](int tid, int mode) {
        const int t = classify_chromosome(names[tid]);
        if (mode == LCD_CTG_AUTOSOME && t != 0) return true;
        if (mode == LCD_CTG_AUTOSOME_XY && t != 0 && t != 1) return true;
        for (int i = 0; i < n_exclude; ++i) if (!strcmp(names[tid], exclude[i])) return true;
        return false;
    };
    std::vector<int> p_tid; std::vector<int64_t> p_beg, p_end;
    auto cut = [&](int tid, int64_t beg, int64_t end) { for (int64_t b = beg; b <= end; b += L) { p_tid.push_back(tid); p_beg.push_back(b); p_end.push_back(std::min(b + L - 1, end)); } };
    auto whole = [&](int mode) { for (int i = 0; i < n_contigs; ++i) if (!skipped(i, mode)) cut(i, 1, lens[i]); };
    // a list of regions: per contig in header order, sorted by begin, overlapping ones merged; each cut from its own begin
    auto from_regs = [&](std::vector<Reg> &regs) {
        std::vector<Reg> keep;
        for (Reg r : regs) {
            if (skipped(r.tid, LCD_CTG_ALL)) continue;
            r.beg = std::max<int64_t>(1, r.beg); r.end = std::min(r.end, lens[r.tid]);
            if (r.beg <= r.end) keep.push_back(r);
        }
        std::stable_sort(keep.begin(), keep.end(), [](const Reg &a, const Reg &b) { return a.tid != b.tid ? a.tid < b.tid : a.beg < b.beg; });
        std::vector<Reg> merged;
        for (const Reg &r : keep) {
            if (!merged.empty() && merged.back().tid == r.tid && r.beg <= merged.back().end) merged.back().end = std::max(merged.back().end, r.end);
            else merged.push_back(r);
        }
        for (const Reg &r : merged) cut(r.tid, r.beg, r.end);
    };
    if (n_regions > 0) {
        std::vector<Reg> regs;
        for (int i = 0; i < n_regions; ++i) {
            if (!regions[i]) return set_err(-4, W + ": NULL region string");
            const std::string s = regions[i];
            int tid = tid_of(s);
            if (tid >= 0) { regs.push_back(Reg{tid, 1, lens[tid]}); continue; }
            const size_t colon = s.rfind(':');
            if (colon == std::string::npos || (tid = tid_of(s.substr(0, colon))) < 0) continue;      // an unknown contig plans nothing
            const std::string iv = s.substr(colon + 1);
            const size_t dash = iv.find('-');
            int64_t beg = 1, end = lens[tid];
            if (!parse_pos(iv.substr(0, dash), beg)) continue;
            if (dash != std::string::npos && dash + 1 < iv.size() && !parse_pos(iv.substr(dash + 1), end)) continue;
            regs.push_back(Reg{tid, beg, end});
        }
        from_regs(regs);
    } else if (bed_path) {
        FILE *fp = fopen(bed_path, "r");
        if (!fp) return set_err(-30, W + ": cannot open the region file " + bed_path);
        std::vector<Reg> regs; std::string line; int ch;
        auto take = [&]() {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '#') return;
            std::vector<std::string> col;
            for (size_t f = 0; f <= line.size();) { size_t t = line.find('\t', f); if (t == std::string::npos) t = line.size(); if (t > f) col.push_back(line.substr(f, t - f)); f = t + 1; }   // (strtok joins empty fields)
            if (col.empty()) return;
            const int tid = tid_of(col[0]);
            if (tid < 0) return;
            int64_t beg = 1, end = lens[tid];
            if (col.size() > 1) { beg = (int64_t)atoi(col[1].c_str()) + 1; if (col.size() > 2) end = atoi(col[2].c_str()); }
            if (beg > end || beg <= 0 || end <= 0) return;
            regs.push_back(Reg{tid, beg, end});
        };
        while ((ch = fgetc(fp)) != EOF) { if (ch == '\n') { take(); line.clear(); } else line += (char)ch; }
        take();                                                    // (a last line without a newline)
        fclose(fp);
        from_regs(regs);
    } else whole(contig_mode);
    if (p_tid.empty()) {   // :744-749: nothing found -- the entire file, the classes off
        whole(LCD_CTG_ALL);
        out->fallback = 1;
    }
    out->n = (int)p_tid.size(); out->tid = dup_vec(p_tid); out->reg_beg = dup_vec(p_beg); out->reg_end = dup_vec(p_end);
    return out->n;
}

} // extern "C"

// ---- the VCF writer ----
namespace {
// LCD_ERR_VIDX_ORDER / LCD_ERR_VIDX_CSI: the VCF goes on without an index (the BAM writer's out_bai_skipped behaviour); anything else is the caller's error
int vcf_index_give_up(lcd_vcf_writer_s *w, int rc) {
    if (rc != LCD_ERR_VIDX_ORDER && rc != LCD_ERR_VIDX_CSI) return rc;
    if (w->vstats) { w->vstats->skipped = rc; snprintf(w->vstats->skip_reason, sizeof(w->vstats->skip_reason), "%s", g_err.c_str()); }
    lcd_vcf_index_builder_destroy(w->vidx); w->vidx = nullptr;
    remove(w->index_path.c_str());
    return 0;
}
} // namespace
extern "C" {
lcd_vcf_writer_t *lcd_vcf_writer_open_idx(const char *path, int bgzf, const char *header_text, const lcd_vcf_index_opt_t *vi) {
    const std::string W = "lcd_vcf_writer_open";
    if (vi) {
        if (vi->stats) memset(vi->stats, 0, sizeof(*vi->stats));
        if (!bgzf || !path || !strcmp(path, "-")) { set_err(-4, W + "_idx: an index needs a BGZF-compressed VCF (bgzf = 1) that goes to a file"); return nullptr; }
        if (vi->format != LCD_VIDX_TBI && vi->format != LCD_VIDX_CSI) { set_err(-4, W + "_idx: format must be LCD_VIDX_TBI or LCD_VIDX_CSI"); return nullptr; }
    }
    std::unique_ptr<lcd_vcf_writer_s> w(new lcd_vcf_writer_s());
    w->bgzf = bgzf != 0;
    if (!path || !strcmp(path, "-")) { w->f = stdout; w->path = "-"; }
    else { w->f = fopen(path, "wb"); w->own = true; w->path = path; }
    if (!w->f) { set_err(-30, W + ": cannot open " + path + " for writing"); return nullptr; }
    if (vi) {
        w->index_path = vi->index_path ? std::string(vi->index_path) : w->path + (vi->format == LCD_VIDX_CSI ? ".csi" : ".tbi");
        w->vstats = vi->stats;
        remove(w->index_path.c_str());
        w->vidx = lcd_vcf_index_builder_create(vi->format);
        if (!w->vidx) { lcd_vcf_writer_t *p = w.release(); lcd_vcf_writer_abort(p); return nullptr; }
        w->device = cur_device();
    }
    if (header_text && header_text[0] && lcd_vcf_writer_append(w.get(), header_text)) { lcd_vcf_writer_t *p = w.release(); lcd_vcf_writer_abort(p); return nullptr; }
    return w.release();
}
lcd_vcf_writer_t *lcd_vcf_writer_open(const char *path, int bgzf, const char *header_text) { return lcd_vcf_writer_open_idx(path, bgzf, header_text, nullptr); }
int lcd_vcf_writer_append(lcd_vcf_writer_t *w, const char *text) {
    const std::string W = "lcd_vcf_writer_append";
    if (!w || !w->f) return set_err(-4, W + ": NULL writer");
    const size_t n = text ? strlen(text) : 0;
    if (!n) return 0;
    if (!w->bgzf) return fwrite(text, 1, n, w->f) == n ? 0 : set_err(-30, W + ": short write on " + w->path);
    lcd_deflated_t *d = nullptr;
    if (w->vidx) {      // one upload: the deflater and the index builder read the same text in HBM
        if (text[n - 1] != '\n') return set_err(-4, W + ": with an index every append ends with a line end");
        if (use_device(w->device)) return -1;
        if (w->d_text.ensure(n + 64, 31)) return -1;
        if (hipMemcpy(w->d_text.p, text, n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return set_err(-10, W + ": upload failed"); }
        d = lcd_bgzf_deflate_dev_ptr(w->d_text.addr(), n, 0, 0);
    } else d = lcd_bgzf_deflate_dev((const uint8_t *)text, n, 0, 0);
    if (!d) return -30;
    const size_t sz = lcd_deflated_size(d);
    if (w->vidx) {
        const size_t nb = lcd_deflated_n_blocks(d);
        std::vector<lcd_bai_member_t> tab(nb);
        uint64_t u = 0, c = w->file_off;
        for (size_t k = 0; k < nb; ++k) {
            uint32_t payload = 0, bsize = 0; int kind = 0;
            if (lcd_deflated_block_info(d, k, &payload, &bsize, &kind)) { lcd_deflated_free(d); return -24; }
            tab[k].uoff = u; tab[k].coff = c; tab[k].ulen = payload; tab[k].pad = 0; u += payload; c += bsize;
        }
        size_t next = 0;
        int rc = (u == n && c == w->file_off + sz) ? lcd_vcf_index_builder_add_stream(w->vidx, w->d_text.addr(), n, 0, nb, tab.data(), w->file_off + sz, &next)
                                                   : set_err(-24, W + ": the deflater's member table does not add up to the append");
        if (rc) rc = vcf_index_give_up(w, rc);
        if (rc) { lcd_deflated_free(d); return rc; }
    }
    std::vector<uint8_t> buf(sz + 1);
    int rc = lcd_deflated_to_host(d, 0, sz, buf.data());
    lcd_deflated_free(d);
    if (!rc && fwrite(buf.data(), 1, sz, w->f) != sz) rc = set_err(-30, W + ": short write on " + w->path);
    if (!rc) w->file_off += sz;
    return rc;
}
void lcd_vcf_writer_abort(lcd_vcf_writer_t *w) {
    if (!w) return;
    const std::string m = g_err;
    if (w->f) { if (w->own) fclose(w->f); else fflush(w->f); }
    if (!w->index_path.empty()) remove(w->index_path.c_str());
    delete w;
    g_err = m;
}
int lcd_vcf_writer_close(lcd_vcf_writer_t *w) {
    const std::string W = "lcd_vcf_writer_close";
    if (!w) return set_err(-4, W + ": NULL writer");
    int rc = 0;
    if (w->bgzf) {
        static const uint8_t eof_member[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (fwrite(eof_member, 1, 28, w->f) != 28) rc = set_err(-30, W + ": short write on " + w->path);
    }
    if ((w->own ? fclose(w->f) : fflush(w->f)) != 0 && !rc) rc = set_err(-30, W + ": closing " + w->path + " failed");
    if (w->vidx && !rc) {      // the index after the EOF member
        rc = lcd_vcf_index_builder_finish(w->vidx, w->index_path.c_str());
        if (!rc) { if (w->vstats) { lcd_vcf_index_builder_counts(w->vidx, w->vstats); w->vstats->wrote = 1; } }
        else rc = vcf_index_give_up(w, rc);
    }
    if (rc && !w->index_path.empty()) remove(w->index_path.c_str());
    delete w;
    return rc;
}
} // extern "C"
extern "C" {

void lcd_file_job_default(lcd_file_job_t *job) { memset(job, 0, sizeof(*job)); job->overlap = -1; }
void lcd_file_stats_free(lcd_file_stats_t *s) {
    if (!s) return;
    free(s->chunk_tid); free(s->chunk_reg_beg); free(s->chunk_reg_end); free(s->chunk_n_reads); free(s->chunk_n_passes); free(s->chunk_flip_hap); free(s->chunk_n_records);
    free(s->chunk_flip_pre_PS); free(s->chunk_flip_cur_PS);
    lcd_free_variants(s->records, s->n_kept_records);
    memset(s, 0, sizeof(*s));
}

} // extern "C"

namespace {
// one window of the plan: its inputs (load), its results (call); everything is released with it
struct Window {
    int first = 0, n = 0;
    std::vector<lcd_chunk_t *> handles; std::vector<uint8_t *> refs; std::vector<lcd_bam_reads_t> metas;
    std::vector<lcd_call_chunk_t> chunks; std::vector<int> tids; std::vector<const char *> chroms;
    lcd_var1_t *records = nullptr; int n_records = 0; char *text = nullptr; bool called = false;
    lcd_stitch_carry_t prev;      // the region of the chunk in front of the window (valid / tid / reg_beg / reg_end only): what the BAM writer leaves out
    explicit Window(int first_, int n_) : first(first_), n(n_), handles(n_, nullptr), refs(n_, nullptr), metas(n_), chunks(n_), tids(n_, 0), chroms(n_, nullptr) {
        memset(&prev, 0, sizeof(prev));
        for (int c = 0; c < n; ++c) { memset(&metas[c], 0, sizeof(lcd_bam_reads_t)); memset(&chunks[c], 0, sizeof(lcd_call_chunk_t)); }
    }
    ~Window() {
        if (called) lcd_call_free(n, chunks.data(), records, n_records, text);
        for (int c = 0; c < n; ++c) { if (handles[c]) lcd_chunk_destroy(handles[c]); free(refs[c]); lcd_bam_reads_free(&metas[c]); }
    }
    Window(const Window &) = delete; Window &operator=(const Window &) = delete;
};

// a queue of depth one between two stages; close() ends it (pop then returns NULL once it is empty)
struct Slot {
    std::mutex mu; std::condition_variable cv; std::unique_ptr<Window> w; bool full = false, closed = false;
    bool push(std::unique_ptr<Window> x) {     // false: closed, the window was dropped
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !full || closed; });
        if (closed) return false;
        w = std::move(x); full = true; cv.notify_all();
        return true;
    }
    std::unique_ptr<Window> pop() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return full || closed; });
        if (!full) return nullptr;
        full = false; cv.notify_all();
        return std::move(w);
    }
    void close() { std::lock_guard<std::mutex> lk(mu); closed = true; cv.notify_all(); }
    void abort() { std::lock_guard<std::mutex> lk(mu); closed = true; full = false; w.reset(); cv.notify_all(); }
};
// at most `n` windows alive
struct Tokens {
    std::mutex mu; std::condition_variable cv; int free_; bool stop = false;
    explicit Tokens(int n) : free_(n) {}
    bool take() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return free_ > 0 || stop; }); if (stop) return false; --free_; return true; }
    void give() { std::lock_guard<std::mutex> lk(mu); ++free_; cv.notify_all(); }
    void halt() { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); }
};

// the middle stage of lcd_haplotag_files: the site tables of the phased VCF (contig i of the tables is contig i of the BAM header), the options, the sums
struct TagStage { lcd_phased_vcf_t *vcf = nullptr; lcd_haplotag_opt_t opt; lcd_haplotag_stats_t sum; ~TagStage() { lcd_phased_vcf_free(vcf); } };

struct Run {
    const lcd_file_job_t *job; const lcd_cfg_t *cfg; lcd_file_stats_t *st;
    TagStage *tag = nullptr;               // NULL: a calling run
    std::vector<std::string> bams, bais; std::vector<const char *> bam_p, bai_p;     // the input files of the one sample, in input order
    std::vector<int64_t> reads_per_file;
    int is_ont = 0, device = 0, loader_threads = 1;
    std::vector<std::string> names; std::vector<int64_t> lens;
    lcd_chunk_plan_t plan;
    lcd_stitch_carry_t carry;
    lcd_vcf_writer_t *vcf = nullptr; lcd_bam_writer_t *bam = nullptr;
    std::vector<lcd_var1_t> kept;          // keep_records
    bool refine = false;                   // refined alignments in the alignment output: every chunk's rounds write their log
    FieldsRun *fields = nullptr;           // the TE library and the names mode of the call (read-only here; its counters belong to the call stage)
    ModsSink mods;                         // the methylation table (lcd_run_ext2_t.mods_path): written by the write stage, chunk by chunk in plan order
    DepthSink depth;                       // the depth track (lcd_run_ext2_t.depth_path): likewise
    SplitSink split;                       // the per-haplotype read sets and the haplotag list (lcd_run_ext2_split_t): likewise, with the alignment writer's plan
    // the first error of any stage
    std::mutex err_mu; int err_code = 0; std::string err_msg; std::atomic<bool> failed{false};
    std::atomic<long long> peak{0};
    void fail(int code, const std::string &m) { std::lock_guard<std::mutex> lk(err_mu); if (!err_code) { err_code = code ? code : -1; err_msg = m; } failed = true; }
    void sample_peak() { const long long b = g_dev_bytes[device].load(); long long p = peak.load(); while (b > p && !peak.compare_exchange_weak(p, b)) {} }

    // ---- load: open every chunk, fetch its reference window around the reads' span, resolve it with that window ----
    int load(Window &w) {
        const double t0 = now_ms();
        lcd_digar_opt_t dopt; lcd_digar_opt_default(&dopt, is_ont);
        dopt.min_bq = cfg->clean.min_bq; dopt.noisy_reg_max_xgaps = cfg->clean.noisy_reg_max_xgaps;   // (one -B / one window rule for the digars and the first round; equal by default)
        std::vector<int> rc(w.n, 0); std::vector<std::string> msg(w.n);
        std::atomic<bool> stop{false};
        par_chunks((size_t)w.n, loader_threads, 1, [&](size_t lo, size_t hi, int t) {
            if (t > 0 && lcd_set_thread_device(device)) { for (size_t c = lo; c < hi; ++c) { rc[c] = -1; msg[c] = g_err; } stop = true; return; }
            for (size_t c = lo; c < hi; ++c) {
                if (stop || failed) { rc[c] = 1; continue; }       // (after an error nothing more is launched)
                const int e = plan.tid[w.first + (int)c]; const int64_t rb = plan.reg_beg[w.first + (int)c], re = plan.reg_end[w.first + (int)c];
                const char *chrom = names[e].c_str();
                auto bad = [&](int code, const std::string &m) { rc[c] = code ? code : -1; msg[c] = m; stop = true; };
                w.handles[c] = lcd_chunk_open_from_bams(&dopt, (int)bam_p.size(), bam_p.data(), bai_p.data(), chrom, rb, re, job->min_mapq, 1, &w.metas[c]);
                if (!w.handles[c]) { bad(-30, g_err); continue; }
                int64_t lo1 = rb, hi1 = re;
                for (int r = 0; r < w.metas[c].n_reads; ++r) { lo1 = std::min(lo1, w.metas[c].pos0[r] + 1); hi1 = std::max(hi1, w.metas[c].end_pos[r]); }
                // get_bam_chunk_reg_ref_seq0 (src/bam_utils.c:1558-1571): 0-based [max(flank, beg - 1) - flank, min(len - flank - 1, end - 1) + flank], cut to the contig
                const int64_t flank = 50000, len = w.metas[c].target_len;
                const int64_t b0 = std::max<int64_t>(flank, lo1 - 1) - flank, e0 = std::min<int64_t>(len - flank - 1, hi1 - 1) + flank;
                const int64_t got = lcd_fasta_fetch(job->fasta_path, chrom, b0 + 1, e0 + 1, &w.refs[c]);
                if (got <= 0) { bad(got < 0 ? (int)got : -30, std::string("lcd_call_files: no reference sequence for ") + chrom + ":" + std::to_string(rb) + "-" + std::to_string(re) + " (" + (got < 0 ? lcd_io_last_error() : "empty window") + ")"); continue; }
                lcd_chunk_src_t src; src.ref_seq = (const char *)w.refs[c]; src.ref_beg = b0 + 1; src.ref_end = b0 + got; src.is_ont = is_ont;
                if (int r2 = lcd_chunk_resolve(w.handles[c], &src)) { bad(r2, g_err); continue; }
                if (refine) if (int r3 = lcd_chunk_set_refine(w.handles[c], 1)) { bad(r3, g_err); continue; }
                lcd_first_chunk_t &x = w.chunks[c].first;
                x.chunk = w.handles[c]; x.ref_seq = w.refs[c]; x.ref_beg = b0 + 1; x.ref_end = b0 + got; x.reg_beg = rb; x.reg_end = re; x.is_ont = is_ont;
                x.ordered_read_ids = nullptr; x.is_rev = nullptr; x.meta = &w.metas[c];
                w.tids[c] = e; w.chroms[c] = chrom;
            }
        });
        sample_peak();
        for (int c = 0; c < w.n; ++c) if (rc[c] < 0) { fail(rc[c], msg[c]); return rc[c]; }
        if (stop) return -1;
        {
            std::lock_guard<std::mutex> lk(err_mu);     // (the counters are written by one stage each; the lock only orders them with the final read)
            st->n_region_loads += w.n; st->n_windows += 1;
            for (int c = 0; c < w.n; ++c) {
                if (w.handles[c]->n_reads > 0) ++st->n_loaded; else ++st->n_empty;
                st->n_reads += w.handles[c]->n_reads;
                for (const int f : w.handles[c]->read_file) ++reads_per_file[f];
            }
            st->ms_load += now_ms() - t0;
        }
        return 0;
    }
    // ---- call: the body of lcd_chunks_call, linked to the carried chunk and to the next planned region ----
    int call(Window &w) {
        const double t0 = now_ms();
        w.prev.valid = carry.valid; w.prev.tid = carry.tid; w.prev.reg_beg = carry.reg_beg; w.prev.reg_end = carry.reg_end;
        CallLinks links; links.chroms = w.chroms.data(); links.tids = w.tids.data(); links.carry_in = &carry; links.carry_out = &carry;
        const int nx = w.first + w.n;
        links.next_tid = nx < plan.n ? plan.tid[nx] : -1; links.next_beg = nx < plan.n ? plan.reg_beg[nx] : 0; links.next_end = nx < plan.n ? plan.reg_end[nx] : 0;
        const int rc = chunks_call_core(w.n, w.chunks.data(), cfg, nullptr, &links, fields, &w.records, &w.n_records, &w.text);
        sample_peak();
        if (rc) { fail(rc, g_err); return rc; }
        w.called = true;
        std::lock_guard<std::mutex> lk(err_mu);
        st->n_records += w.n_records; st->ms_call += now_ms() - t0;
        return 0;
    }
    // ---- tag (lcd_haplotag_files' middle stage): every chunk's reads against the phased sites of its contig; the answer is handed on as the chunk's K5 state.  A
    // record that two overlapping chunks hold gets the same answer in both (it depends on the record and the table alone): no stitch, no flip, nothing carried
    // but the region in front of the window, which the writers leave out ----
    int tag_window(Window &w) {
        const double t0 = now_ms();
        w.prev.valid = carry.valid; w.prev.tid = carry.tid; w.prev.reg_beg = carry.reg_beg; w.prev.reg_end = carry.reg_end;
        w.called = true;                                            // (the window frees the states made below)
        for (int c = 0; c < w.n; ++c) {
            lcd_first_chunk_t &x = w.chunks[c].first;
            lcd_haplotag_stats_t hs;
            lcd_haplotag_t *h = lcd_chunk_haplotag(w.handles[c], tag->vcf, w.tids[c], &tag->opt, &hs);
            if (!h) { fail(-1, g_err); return -1; }
            const int n = lcd_haplotag_n_reads(h);
            x.state = (lcd_hap_state_t *)calloc(1, sizeof(lcd_hap_state_t));
            int rc = x.state ? lcd_hap_state_init(n, 0, x.state) : set_err(-11, "lcd_haplotag_files: out of memory");
            if (!rc) rc = lcd_haplotag_to_host(h, x.state->haps, x.state->phase_sets, nullptr, nullptr) == n ? 0 : -24;
            lcd_haplotag_free(h);
            if (rc) { fail(rc, g_err); return rc; }
            x.n_reads = n;
            int64_t *a = &tag->sum.n_records; const int64_t *b = &hs.n_records;
            for (int k = 0; k < 14; ++k) a[k] += b[k];
            tag->sum.ms_measure += hs.ms_measure; tag->sum.ms_mark += hs.ms_mark; tag->sum.ms_reduce += hs.ms_reduce;
        }
        carry.valid = 1; carry.tid = w.tids[w.n - 1]; carry.reg_beg = w.chunks[w.n - 1].first.reg_beg; carry.reg_end = w.chunks[w.n - 1].first.reg_end;
        sample_peak();
        std::lock_guard<std::mutex> lk(err_mu);
        st->ms_call += now_ms() - t0;
        return 0;
    }
    int middle(Window &w) { return tag ? tag_window(w) : call(w); }
    // ---- write: the text, the window's records of the alignment output; the caller frees the window ----
    int write(Window &w) {
        const double t0 = now_ms();
        int rc = vcf ? lcd_vcf_writer_append(vcf, w.text) : 0;
        if (!rc && bam) rc = lcd_bam_writer_append(bam, w.n, w.chunks.data(), w.tids.data(), &w.prev);
        if (mods.active()) for (int c = 0; c < w.n && !rc; ++c) rc = mods.chunk(w.handles[c], w.chunks[c].first, w.chroms[c]);
        if (depth.active()) for (int c = 0; c < w.n && !rc; ++c) rc = depth.chunk(w.handles[c], w.chunks[c].first, w.chroms[c]);
        if (split.active() && !rc) rc = split.window(w.n, w.chunks.data(), w.tids.data(), &w.prev);
        sample_peak();
        if (rc) { fail(rc, g_err); return rc; }
        std::lock_guard<std::mutex> lk(err_mu);
        for (const char *p = w.text; p && *p; ++p) if (*p == '\n') ++st->n_vcf_lines;
        if (job->keep_records) {
            for (int c = 0; c < w.n; ++c) {
                const int i = w.first + c; const lcd_call_chunk_t &x = w.chunks[c];
                st->chunk_tid[i] = w.tids[c]; st->chunk_reg_beg[i] = x.first.reg_beg; st->chunk_reg_end[i] = x.first.reg_end; st->chunk_n_reads[i] = w.handles[c]->n_reads;
                st->chunk_n_passes[i] = x.n_passes; st->chunk_flip_hap[i] = x.flip_hap; st->chunk_n_records[i] = x.n_records;
                st->chunk_flip_pre_PS[i] = x.flip_pre_PS; st->chunk_flip_cur_PS[i] = x.flip_cur_PS;
            }
            for (int i = 0; i < w.n_records; ++i) kept.push_back(w.records[i]);
            free(w.records); w.records = nullptr; w.n_records = 0;      // (the members moved into `kept`)
        }
        st->ms_write += now_ms() - t0;
        return 0;
    }
};
} // namespace

// the whole-file run over the input files of one sample; in == NULL: the one file of the job
extern "C" int lcd_call_files(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out) {
    return lcd_call_files_ext(in, job, cfg, opt, stats, out, nullptr);
}
extern "C" int lcd_call_files_ext(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                                  const lcd_run_ext_t *ext) {
    return lcd_call_files_ext2(in, job, cfg, opt, stats, out, ext, nullptr);
}
static int files_run(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                     const lcd_run_ext_t *ext, const lcd_run_ext2_t *ext2, const lcd_haplotag_run_t *hopt);
extern "C" int lcd_call_files_ext2(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                                   const lcd_run_ext_t *ext, const lcd_run_ext2_t *ext2) {
    return files_run(in, job, cfg, opt, stats, out, ext, ext2, nullptr);
}
extern "C" int lcd_haplotag_files(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_haplotag_run_t *hopt, const lcd_run_opt_t *opt,
                                  lcd_file_stats_t *stats, const lcd_run_out_t *out, const lcd_run_ext2_t *ext2) {
    if (hopt) {
        if (hopt->stats) memset(hopt->stats, 0, sizeof(*hopt->stats));
        if (hopt->size >= offsetof(lcd_haplotag_run_t, vcf_stats) + sizeof(void *) && hopt->vcf_stats) memset(hopt->vcf_stats, 0, sizeof(*hopt->vcf_stats));
    }
    if (!hopt || hopt->size < offsetof(lcd_haplotag_run_t, vcf_path) + sizeof(char *)) return set_err(-4, "lcd_haplotag_files: NULL options, or a size that does not reach vcf_path");
    return files_run(in, job, cfg, opt, stats, out, nullptr, ext2, hopt);
}
// hopt == NULL: a calling run (lcd_call_files_ext2); else lcd_haplotag_files: the middle stage is TagStage and no VCF is written
static int files_run(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                     const lcd_run_ext_t *ext, const lcd_run_ext2_t *ext2, const lcd_haplotag_run_t *hopt) {
    const std::string W = hopt ? "lcd_haplotag_files" : "lcd_call_files";
    lcd_haplotag_run_t hx; memset(&hx, 0, sizeof(hx));
    if (hopt) memcpy(&hx, hopt, std::min(hopt->size, sizeof(hx)));     // (what lies behind `size` reads as zero)
    lcd_run_ext2_t x2; lcd_mods_opt_t mods_opt;
    if (int rc = ModsSink::parse(W, ext2, &x2, &mods_opt)) return rc;
    if (int rc = DepthSink::parse(W, x2)) return rc;
    lcd_run_ext2_split_t xs;
    {
        const char *other[4] = {job ? job->vcf_path : nullptr, job && job->bam_out ? job->bam_out->path : nullptr, x2.mods_path, x2.depth_path};
        if (int rc = SplitSink::parse(W, ext2, &xs, 4, other)) return rc;
    }
    const lcd_index_opt_t *idx = opt ? opt->idx : nullptr;
    const lcd_vcf_fields_t *fields = opt ? opt->fields : nullptr;
    lcd_vcf_fields_out_t *fields_out = out ? out->fields_out : nullptr;
    int64_t *n_reads_per_file = out ? out->n_reads_per_file : nullptr;
    zero_run_out(out);
    if (ext && ext->vcf_idx_stats) memset(ext->vcf_idx_stats, 0, sizeof(*ext->vcf_idx_stats));
    if (stats) memset(stats, 0, sizeof(*stats));
    lcd_index_stats_t ist_local; memset(&ist_local, 0, sizeof(ist_local));
    lcd_index_stats_t *ist = out && out->idx_stats ? out->idx_stats : &ist_local;
    if (int rc = check_aln_opt(W, opt)) return rc;
    TagStage tag;
    if (hopt) {
        if (!hx.vcf_path) return set_err(-4, W + ": no phased VCF (vcf_path)");
        if (job && job->vcf_path) return set_err(-4, W + ": a haplotag run writes no VCF (job->vcf_path)");
        if (opt && opt->fields) return set_err(-4, W + ": a haplotag run has no VCF fields (opt->fields)");
        if (opt && opt->aln && opt->aln->refine) return set_err(-4, W + ": a haplotag run does not refine alignments (opt->aln->refine)");
        if (hx.max_indel < 0 || hx.min_diff < 0 || hx.min_bq < 0 || hx.min_bq > 254) return set_err(-4, W + ": max_indel / min_diff below 0 (0: the default), or min_bq outside 0 ... 254");
        if (!(job && job->bam_out) && !x2.mods_path && !x2.depth_path && !xs.split_prefix && !xs.haplotag_path) return set_err(-4, W + ": no output requested");
        lcd_haplotag_opt_default(&tag.opt); tag.opt.min_bq = hx.min_bq; if (hx.min_diff) tag.opt.min_diff = hx.min_diff;
        memset(&tag.sum, 0, sizeof(tag.sum));
    }
    if (idx && idx->write_out_bai && (!job || !job->bam_out)) return set_err(-4, W + ": write_out_bai needs bam_out");
    if (idx && idx->slab_members < 0) return set_err(-4, W + ": negative slab_members");
    const lcd_vcf_index_opt_t *vcf_idx = ext ? ext->vcf_idx : nullptr;
    if (vcf_idx && (!job || !job->vcf_bgzf || !job->vcf_path || !strcmp(job->vcf_path, "-"))) return set_err(-4, W + ": vcf_idx needs a BGZF-compressed VCF (vcf_bgzf) that goes to a file");
    if (vcf_idx && vcf_idx->format != LCD_VIDX_TBI && vcf_idx->format != LCD_VIDX_CSI) return set_err(-4, W + ": vcf_idx->format must be LCD_VIDX_TBI or LCD_VIDX_CSI");
    if (!job || !cfg || !stats || (!in && !job->bam_path) || !job->fasta_path) return set_err(-4, W + ": NULL argument");
    if (in) {
        if (in->n < 1 || in->n > LCD_MAX_INPUTS || !in->bam_paths) return set_err(-4, W + ": the number of inputs must be 1 ... LCD_MAX_INPUTS, with their paths");
        for (int f = 0; f < in->n; ++f) if (!in->bam_paths[f]) return set_err(-4, W + ": NULL input path");
        if (job->bam_path && strcmp(job->bam_path, in->bam_paths[0]) != 0) return set_err(-4, W + ": job->bam_path must be NULL or the first input");
        if (job->bai_path && in->bai_paths && in->bai_paths[0] && strcmp(job->bai_path, in->bai_paths[0]) != 0) return set_err(-4, W + ": job->bai_path must be NULL or the first input's index");
    }
    if (job->bam_out && !job->bam_out->path) return set_err(-4, W + ": bam_out without a path");
    const bool sam = opt && opt->aln && opt->aln->format == LCD_ALN_SAM && job->bam_out;
    if (sam && idx && idx->write_out_bai) return set_err(-4, W + ": a SAM output has no index (write_out_bai)");
    if (!hopt && sam && !strcmp(job->bam_out->path, "-") && (!job->vcf_path || !strcmp(job->vcf_path, "-"))) return set_err(-4, W + ": the SAM output and the VCF cannot both go to stdout");
    if (job->window_chunks < 0 || job->loader_threads < 0 || job->chunk_len < 0 || job->overlap < -1 || job->overlap > 1) return set_err(-4, W + ": negative window_chunks / loader_threads / chunk_len, or overlap outside -1 ... 1");
    if (cfg->clean.out_somatic || cfg->opt.collect_ref_read_aln_str) return set_err(-2, W + ": somatic / refine mode is not supported");
    const double t_wall = now_ms();
    FieldsRun fr; fr.collect_rnames = fields_out != nullptr && job->keep_records;
    if (int rc = fr.open(fields, W)) return rc;     // (an unreadable TE file: before an index is built or an output file is created)
    Run R; R.job = job; R.cfg = cfg; R.st = stats; R.fields = &fr; R.tag = hopt ? &tag : nullptr;
    R.refine = opt && opt->aln && opt->aln->refine && job->bam_out;     // (without an alignment output the option has no effect, as in the reference)
    memset(&R.plan, 0, sizeof(R.plan)); memset(&R.carry, 0, sizeof(R.carry));
    const int n_in = in ? in->n : 1;
    for (int f = 0; f < n_in; ++f) {
        R.bams.push_back(in ? in->bam_paths[f] : job->bam_path);
        const char *b = in && in->bai_paths && in->bai_paths[f] ? in->bai_paths[f] : f == 0 ? job->bai_path : nullptr;
        R.bais.push_back(b ? std::string(b) : R.bams[f] + ".bai");
    }
    for (int f = 0; f < n_in; ++f) { R.bam_p.push_back(R.bams[f].c_str()); R.bai_p.push_back(R.bais[f].c_str()); }
    R.reads_per_file.assign(n_in, 0);
    if (n_reads_per_file) for (int f = 0; f < n_in; ++f) n_reads_per_file[f] = 0;
    const char *bam0 = R.bam_p[0];
    R.is_ont = cfg->clean.is_ont != 0;
    // an index that exists is read as it is; a missing one is built only when the caller asks for it (lcd_index_opt_t), at the path that would have been read
    for (int which = 0; which <= n_in; ++which) {     // every input's .bai, then the .fai
        const bool is_bai = which < n_in;
        const std::string p = is_bai ? R.bais[which] : std::string(job->fasta_path) + ".fai";
        FILE *f = fopen(p.c_str(), "rb");
        if (f) { fclose(f); continue; }
        if (!idx) return set_err(-30, W + ": cannot open the index " + p + " (the library does not build indexes here: lcd_run_opt_t.idx / --make-index does)");
        if (!(is_bai ? idx->build_missing_bai : idx->build_missing_fai))
            return set_err(-30, W + ": cannot open the index " + p + " (lcd_index_opt_t." + (is_bai ? "build_missing_bai" : "build_missing_fai") + " would build it)");
        const double t0 = now_ms();
        if (is_bai) {
            lcd_bai_opt_t bo; bo.slab_members = idx->slab_members; bo.verify_crc = 0;
            if (int rc = lcd_bai_build(R.bam_p[which], p.c_str(), &bo, nullptr)) return rc;
            ist->built_bai = 1; ist->ms_build_bai += now_ms() - t0;
        } else {
            const int rc = lcd_fai_build(job->fasta_path, p.c_str());
            if (rc < 0) return rc;
            ist->built_fai = 1; ist->ms_build_fai = now_ms() - t0;
        }
    }
    std::string text;
    if (int rc = bam_header_parts(bam0, text, R.names, R.lens, W)) return rc;
    // PROJECT RULE: every further file carries file 0's reference table -- names, lengths, order (the reference uses file 0's tids for every file unchecked)
    for (int f = 1; f < n_in; ++f) {
        std::string t2; std::vector<std::string> nm2; std::vector<int64_t> ln2;
        if (int rc = bam_header_parts(R.bam_p[f], t2, nm2, ln2, W)) return rc;
        const size_t m = std::min(nm2.size(), R.names.size());
        size_t i = 0;
        while (i < m && nm2[i] == R.names[i] && ln2[i] == R.lens[i]) ++i;
        if (i < m || nm2.size() != R.names.size()) {
            auto ent = [&](const std::vector<std::string> &nm, const std::vector<int64_t> &ln) { return i < nm.size() ? nm[i] + " (" + std::to_string((long long)ln[i]) + ")" : std::string("nothing"); };
            return set_err(LCD_ERR_INPUT_HEADERS, W + ": " + R.bams[f] + " does not carry the reference table of " + R.bams[0] + ": entry " + std::to_string(i) + " is " + ent(nm2, ln2) +
                                                      ", the first file has " + ent(R.names, R.lens));
        }
    }
    if (hopt) {     // the site tables: contig i of the BAM header is contig i of the tables
        std::vector<const char *> nm; for (const std::string &s : R.names) nm.push_back(s.c_str());
        lcd_hapvcf_opt_t vo; lcd_hapvcf_opt_default(&vo); if (hx.max_indel) vo.max_indel = hx.max_indel; vo.snvs_only = hx.snvs_only != 0;
        tag.vcf = lcd_phased_vcf_read(hx.vcf_path, hx.sample, (int)nm.size(), nm.data(), &vo, hx.vcf_stats);
        if (!tag.vcf) return set_err(lcd_phased_vcf_errno() ? lcd_phased_vcf_errno() : -30, W + ": " + lcd_phased_vcf_error());
    }
    {
        std::vector<const char *> nm; for (const std::string &s : R.names) nm.push_back(s.c_str());
        const int rc = lcd_plan_chunks((int)nm.size(), nm.data(), R.lens.data(), job->contig_mode, job->n_exclude, job->exclude, job->n_regions, job->regions, job->region_bed_path,
                                       job->chunk_len, &R.plan);
        if (rc < 0) return rc;
    }
    struct PlanGuard { lcd_chunk_plan_t *p; lcd_stitch_carry_t *c; ~PlanGuard() { lcd_chunk_plan_free(p); lcd_stitch_carry_free(c); } } guard{&R.plan, &R.carry};
    stats->n_planned = R.plan.n; stats->plan_fallback = R.plan.fallback;
    const int window = job->window_chunks ? job->window_chunks : (R.is_ont ? 16 : 32);
    // the defaults come from profiles/NOTES_call_file.md: pipelining did not win reliably there, so -1 runs the stages in turn; four loader threads shortened the load stage
    const bool overlap = job->overlap == 1;
    R.loader_threads = job->loader_threads ? std::min(job->loader_threads, 16) : std::max(1, std::min(4, host_cpus()));
    if (R.plan.n > 0 && ensure_init()) return -1;
    R.device = cur_device();
    if (job->keep_records) {
        const size_t n = (size_t)R.plan.n + 1;
        stats->n_chunks = R.plan.n;
        stats->chunk_tid = (int *)calloc(n, sizeof(int)); stats->chunk_reg_beg = (int64_t *)calloc(n, 8); stats->chunk_reg_end = (int64_t *)calloc(n, 8);
        stats->chunk_n_reads = (int *)calloc(n, sizeof(int)); stats->chunk_n_passes = (int *)calloc(n, sizeof(int)); stats->chunk_flip_hap = (int *)calloc(n, sizeof(int));
        stats->chunk_n_records = (int *)calloc(n, sizeof(int)); stats->chunk_flip_pre_PS = (int64_t *)calloc(n, 8); stats->chunk_flip_cur_PS = (int64_t *)calloc(n, 8);
    }
    // the outputs: the header names every contig of the BAM header, in header order (src/vcf_utils.c:46-49)
    {
        char *hdr = nullptr, *sm = nullptr;
        if (!hopt && !job->no_vcf_header) {
            if (!job->sample_name && lcd_bam_sample_name(bam0, &sm)) return -30;
            std::string joined;     // src/call_var_main.c:733-735: without an SM, the input paths
            for (int f = 0; f < n_in; ++f) joined += (f ? "," : "") + R.bams[f];
            std::vector<const char *> nm; for (const std::string &s : R.names) nm.push_back(s.c_str());
            char date[16] = "";
            if (!job->date_yyyymmdd) { const time_t now = time(nullptr); struct tm tmv; localtime_r(&now, &tmv); strftime(date, sizeof(date), "%Y%m%d", &tmv); }
            lcd_vcf_header(job->source_version ? job->source_version : lcd_version(), job->cmdline ? job->cmdline : "", job->date_yyyymmdd ? job->date_yyyymmdd : date, (int)nm.size(),
                           nm.data(), R.lens.data(), job->sample_name ? job->sample_name : sm ? sm : joined.c_str(), &hdr);
        }
        lcd_vcf_index_opt_t vio; memset(&vio, 0, sizeof(vio));
        if (vcf_idx) { vio = *vcf_idx; vio.stats = ext->vcf_idx_stats; }
        if (!hopt) R.vcf = lcd_vcf_writer_open_idx(job->vcf_path, job->vcf_bgzf, hdr, vcf_idx ? &vio : nullptr);
        free(hdr); free(sm);
        if (!hopt && !R.vcf) { lcd_file_stats_free(stats); return -30; }
        if (job->bam_out) {
            lcd_writer_opt_t wo; memset(&wo, 0, sizeof(wo));
            wo.format = sam ? LCD_ALN_SAM : LCD_ALN_BAM; wo.sort_output = in ? in->sort_output : 0;
            if (idx && idx->write_out_bai) { wo.write_index = 1; wo.index_path = idx->out_bai_path; wo.idx_stats = ist; }
            if (R.refine) wo.refine_stats = out ? out->refine_stats : nullptr;
            if (sam) wo.sam_stats = out ? out->sam_stats : nullptr;
            R.bam = lcd_bam_writer_open(bam0, job->bam_out, &wo);
            if (!R.bam) { lcd_vcf_writer_abort(R.vcf); lcd_file_stats_free(stats); return -30; }
        }
        std::vector<const char *> ref_names; for (const std::string &s : R.names) ref_names.push_back(s.c_str());
        if ((x2.mods_path && R.mods.open(W, x2, mods_opt)) || (x2.depth_path && R.depth.open(W, x2)) ||
            ((xs.split_prefix || xs.haplotag_path) && R.split.open(W, xs, (int)ref_names.size(), ref_names.data(), in ? in->sort_output : 0))) {
            const std::string m0 = g_err;
            if (R.mods.active()) R.mods.finish(false);
            if (R.depth.active()) R.depth.finish(false);
            if (R.bam) lcd_bam_writer_abort(R.bam);
            lcd_vcf_writer_abort(R.vcf); lcd_file_stats_free(stats);
            return set_err(-30, m0);
        }
    }
    const int n_windows = (R.plan.n + window - 1) / window;
    auto make = [&](int k) { return std::unique_ptr<Window>(new Window(k * window, std::min(window, R.plan.n - k * window))); };
    if (!overlap) {
        for (int k = 0; k < n_windows && !R.failed; ++k) {
            std::unique_ptr<Window> w = make(k);
            if (R.load(*w) || R.middle(*w) || R.write(*w)) break;
        }
    } else {
        Slot loaded, called; Tokens alive(3);
        std::thread loader([&] {
            if (lcd_set_thread_device(R.device)) R.fail(-1, g_err);
            for (int k = 0; k < n_windows && !R.failed; ++k) {
                if (!alive.take()) break;
                std::unique_ptr<Window> w = make(k);
                if (R.load(*w)) { w.reset(); alive.give(); break; }
                if (!loaded.push(std::move(w))) { alive.give(); break; }
            }
            loaded.close();
        });
        std::thread writer([&] {
            if (lcd_set_thread_device(R.device)) R.fail(-1, g_err);
            for (;;) {
                std::unique_ptr<Window> w = called.pop();
                if (!w) break;
                if (!R.failed) R.write(*w);
                w.reset(); alive.give();
            }
        });
        for (;;) {      // the call stage runs on the calling thread
            std::unique_ptr<Window> w = loaded.pop();
            if (!w) break;
            if (R.failed || R.middle(*w)) { w.reset(); alive.give(); break; }
            if (!called.push(std::move(w))) { alive.give(); break; }
        }
        if (R.failed) { alive.halt(); loaded.abort(); }     // (the loader may be waiting for a token or for the slot)
        called.close();
        loader.join(); writer.join();
    }
    int rc = 0;
    if (R.failed) {
        if (R.bam) lcd_bam_writer_abort(R.bam);
        lcd_vcf_writer_abort(R.vcf);
        rc = R.err_code;
    } else {
        if (R.bam) rc = lcd_bam_writer_close(R.bam);
        const int rc2 = R.vcf ? lcd_vcf_writer_close(R.vcf) : 0;
        if (!rc) rc = rc2;
        if (rc) R.err_msg = g_err;
    }
    // the table is finished after the other outputs: a run that fails anywhere, their close included, leaves no table and no statistics of it
    if (R.mods.active()) { const int rc3 = R.mods.finish(!rc); if (!rc && rc3) { rc = rc3; R.err_msg = g_err; } }
    if (R.depth.active()) { const int rc3 = R.depth.finish(!rc); if (!rc && rc3) { rc = rc3; R.err_msg = g_err; } }
    if (R.split.active()) { const int rc3 = R.split.finish(!rc); if (!rc && rc3) { rc = rc3; R.err_msg = g_err; } }
    if (job->keep_records) {
        stats->records = dup_vec(R.kept); stats->n_kept_records = (int)R.kept.size();
    }
    if (!rc) fr.give(fields_out);
    if (!rc && hopt && hx.stats) *hx.stats = tag.sum;
    stats->peak_device_bytes = R.peak.load();
    if (n_reads_per_file) for (int f = 0; f < n_in; ++f) n_reads_per_file[f] = R.reads_per_file[f];
    stats->ms_wall = now_ms() - t_wall;
    return rc ? set_err(rc, R.err_msg) : 0;
}
