// lcd_call.cpp -- the germline path joined end to end: lcd_chunks_call (first round, noisy-region rounds, cross-chunk stitch, genotype records, VCF body lines
// for a pipeline step's chunks of one contig), lcd_call_bam_regions (the same from an indexed BAM and a FASTA) and the phased alignment file beside it
// (the appendable writer lcd_bam_writer_*, lcd_write_phased).  chunks_call_core is the body of lcd_chunks_call that lcd_call_files
// (lcd_call_file.cpp) runs per window of chunks.  Every stage is an export of its own
// (lcd_first_round.cpp, lcd_chunk_vars.cpp, lcd_emit.cpp, lcd_chunk.cpp, lcd_io.cpp); this file only composes them as collect_var_main / stitch_var_main /
// make_var_main do (src/collect_var.c:2897-3000).
#include "lcd_host_internal.h"

using namespace lcd_internal;

extern "C" {

void lcd_cfg_default(lcd_cfg_t *cfg, int is_ont) {
    lcd_clean_opt_default(&cfg->clean, is_ont); lcd_opt_default(&cfg->opt); cfg->opt.is_ont = is_ont != 0; lcd_pass_opt_default(&cfg->pass); lcd_call_opt_default(&cfg->call);
}

void lcd_call_free(int n, lcd_call_chunk_t *chunks, lcd_var1_t *records, int n_records, char *vcf_body) {
    for (int c = 0; chunks && c < n; ++c) { lcd_first_round_free(&chunks[c].first); chunks[c].n_passes = chunks[c].flip_hap = chunks[c].n_records = 0; chunks[c].flip_pre_PS = chunks[c].flip_cur_PS = -1; }
    lcd_free_variants(records, n_records);
    free(vcf_body);
}

int lcd_chunks_call(int n, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, lcd_var1_t **records, int *n_records, char **vcf_body) {
    return lcd_chunks_call_fields(n, chunks, cfg, chrom, nullptr, records, n_records, vcf_body, nullptr);
}
int lcd_chunks_call_refine(int n, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, lcd_var1_t **records, int *n_records, char **vcf_body) {
    for (int c = 0; chunks && c < n; ++c) if (chunks[c].first.chunk) if (int rc = lcd_chunk_set_refine(const_cast<lcd_chunk_t *>(chunks[c].first.chunk), 1)) return rc;
    return lcd_chunks_call(n, chunks, cfg, chrom, records, n_records, vcf_body);
}
int lcd_chunks_call_fields(int n, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, const lcd_vcf_fields_t *fields, lcd_var1_t **records, int *n_records,
                           char **vcf_body, lcd_vcf_fields_out_t *fields_out) {
    if (fields_out) memset(fields_out, 0, sizeof(*fields_out));
    FieldsRun fr; fr.collect_rnames = fields_out != nullptr;
    if (int rc = fr.open(fields, "lcd_chunks_call")) { if (records) *records = nullptr; if (n_records) *n_records = 0; if (vcf_body) *vcf_body = nullptr; return rc; }
    const int rc = chunks_call_core(n, chunks, cfg, chrom, nullptr, &fr, records, n_records, vcf_body);
    if (!rc) fr.give(fields_out);
    return rc;
}

void lcd_vcf_fields_out_free(lcd_vcf_fields_out_t *o) {
    if (!o) return;
    for (int i = 0; o->te_names && i < o->n_te_seqs; ++i) free(o->te_names[i]);
    for (int i = 0; o->rnames && i < o->n_rnames; ++i) free(o->rnames[i]);
    free(o->te_names); free(o->rnames);
    memset(o, 0, sizeof(*o));
}

} // extern "C"

int lcd_internal::FieldsRun::open(const lcd_vcf_fields_t *f, const std::string &W) {
    if (!f) return 0;
    if (f->rnames_mode < LCD_RNAMES_NONE || f->rnames_mode > LCD_RNAMES_ALL) return set_err(-4, W + ": rnames_mode must be 0 (none), 1 (SV records) or 2 (all records)");
    if (f->te_kmer_len < 0 || f->te_kmer_len > 15) return set_err(-4, W + ": te_kmer_len must be 0 (15) or 1 ... 15");
    rnames_mode = f->rnames_mode;
    if (!f->te_fasta_path) return 0;
    return lcd_te_lib_from_fasta(f->te_fasta_path, f->te_kmer_len, &lib, &te_names, nullptr, &n_te);
}
void lcd_internal::FieldsRun::give(lcd_vcf_fields_out_t *out) {
    if (!out) return;
    out->n_te_seqs = n_te; out->te_names = te_names; te_names = nullptr;
    out->n_mei_lines = n_mei;
    if (collect_rnames && rnames_mode) {
        out->n_rnames = (int)rnames.size();
        out->rnames = (char **)malloc((rnames.size() + 1) * sizeof(char *));
        if (!rnames.empty()) memcpy(out->rnames, rnames.data(), rnames.size() * sizeof(char *));
        rnames.clear();
    }
}
lcd_internal::FieldsRun::~FieldsRun() {
    for (char *p : rnames) free(p);
    for (int i = 0; te_names && i < n_te; ++i) free(te_names[i]);
    free(te_names);
    lcd_te_lib_destroy(lib);
}

// the body of lcd_chunks_call.  links == NULL: n chunks of the one contig `chrom`.  With links (lcd_call_files' window): a contig name and tid per chunk, the first
// chunk's up list against the carried region, the last chunk's down list against the next planned region, the stitch carried in and out
int lcd_internal::chunks_call_core(int n, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, const CallLinks *links, FieldsRun *fields, lcd_var1_t **records,
                                   int *n_records, char **vcf_body) {
    const std::string W = "lcd_chunks_call";
    if (records) *records = nullptr;
    if (n_records) *n_records = 0;
    if (vcf_body) *vcf_body = nullptr;
    if (!records || !n_records || !vcf_body || !cfg || (!chrom && !links)) return set_err(-4, W + ": NULL argument");
    if (n < 0 || (n > 0 && !chunks)) return set_err(-4, W + ": bad chunk list");
    if (cfg->clean.out_somatic || cfg->opt.collect_ref_read_aln_str) return set_err(-2, W + ": somatic / refine mode is not supported");
    for (int c = 0; c < n; ++c) { lcd_call_chunk_t &x = chunks[c]; x.n_passes = x.flip_hap = x.n_records = 0; x.flip_pre_PS = x.flip_cur_PS = -1; }
    // 1. the head of collect_var_main
    std::vector<lcd_first_chunk_t> f(n);
    for (int c = 0; c < n; ++c) f[c] = chunks[c].first;
    int rc = lcd_chunks_first_round(n, f.data(), &cfg->clean);
    for (int c = 0; c < n; ++c) chunks[c].first = f[c];      // (on failure the out members are NULL / 0)
    if (rc) return rc;
    auto fail = [&](int code) { const std::string m = g_err; lcd_call_free(n, chunks, nullptr, 0, nullptr); g_err = m; return code; };
    // 2. the noisy-region loop
    {
        std::vector<lcd_rounds_chunk_t> r(n);
        for (int c = 0; c < n; ++c) {
            const lcd_first_chunk_t &x = chunks[c].first;
            memset(&r[c], 0, sizeof(lcd_rounds_chunk_t));
            r[c].chunk = x.chunk; r[c].vars = x.vars; r[c].state = x.state; r[c].ordered_read_ids = x.order; r[c].is_skipped = x.is_skipped;
            r[c].ref_seq = x.ref_seq; r[c].ref_beg = x.ref_beg; r[c].ref_end = x.ref_end; r[c].is_ont = x.is_ont;
        }
        std::vector<lcd_refine_log_t *> logs(n + 1, nullptr);      // the chunks a driver asked refined alignments for (lcd_chunk_set_refine): their rounds write the log
        for (int c = 0; c < n; ++c) logs[c] = chunks[c].first.chunk ? chunks[c].first.chunk->refine_log : nullptr;
        rc = lcd_chunks_noisy_rounds_log(n, r.data(), &cfg->opt, &cfg->pass, logs.data());
        if (rc) return fail(rc);
        for (int c = 0; c < n; ++c) { chunks[c].n_passes = r[c].n_passes; free(r[c].done); free(r[c].first_to_final); }
    }
    // 3. stitch_var_main: the phase sets of neighbours joined through the reads they share
    {
        std::vector<lcd_chunk_phase_t> ph(n); std::vector<std::vector<int>> up(n), down(n);
        const lcd_stitch_carry_t *cin = links ? links->carry_in : nullptr;
        for (int c = 0; c < n; ++c) {
            const lcd_first_chunk_t &x = chunks[c].first; const lcd_chunk_s *k = x.chunk;
            const int tid = links ? links->tids[c] : 0;
            // the neighbours' regions: the chunk beside it, or across the window's border the carried / the next planned region; none on another contig
            bool has_up = c > 0 && (!links || links->tids[c - 1] == tid), has_down = c + 1 < n && (!links || links->tids[c + 1] == tid);
            int64_t ub = has_up ? chunks[c - 1].first.reg_beg : 0, ue = has_up ? chunks[c - 1].first.reg_end : 0;
            int64_t db = has_down ? chunks[c + 1].first.reg_beg : 0, de = has_down ? chunks[c + 1].first.reg_end : 0;
            if (c == 0 && cin && cin->valid && cin->tid == tid) { has_up = true; ub = cin->reg_beg; ue = cin->reg_end; }
            if (c == n - 1 && links && links->next_tid == tid) { has_down = true; db = links->next_beg; de = links->next_end; }
            for (int r = 0; r < k->n_reads; ++r) {
                const int64_t rb = k->beg[r], re = k->end[r];
                if (has_up && !(re < ub || rb > ue)) up[c].push_back(r);
                if (has_down && !(re < db || rb > de)) down[c].push_back(r);
            }
            lcd_chunk_phase_t &p = ph[c]; memset(&p, 0, sizeof(p));
            p.tid = tid; p.n_reads = x.vars->n_reads; p.n_vars = x.vars->n_vars; p.ordered_read_ids = x.order; p.is_skipped = x.is_skipped;
            p.haps = x.state->haps; p.phase_sets = x.state->phase_sets; p.var_phase_set = x.state->var_phase_set; p.hap_to_cons_alle = x.state->hap_to_cons_alle;
            p.n_up_ovlp = (int)up[c].size(); p.n_down_ovlp = (int)down[c].size(); p.up_ovlp_read_i = up[c].data(); p.down_ovlp_read_i = down[c].data();
            p.flip_hap = 0; p.flip_pre_PS = p.flip_cur_PS = -1;
        }
        rc = links ? lcd_stitch_chunks_carry(ph.data(), n, 1, links->carry_in, links->carry_out) : lcd_stitch_chunks(ph.data(), n, 1);
        if (!rc && links && links->carry_out && n > 0) { links->carry_out->reg_beg = chunks[n - 1].first.reg_beg; links->carry_out->reg_end = chunks[n - 1].first.reg_end; }
        if (rc) return fail(set_err(rc, W + ": neighbouring chunks disagree on the reads they share (the overlap counts differ)"));
        for (int c = 0; c < n; ++c) { chunks[c].flip_hap = ph[c].flip_hap; chunks[c].flip_pre_PS = ph[c].flip_pre_PS; chunks[c].flip_cur_PS = ph[c].flip_cur_PS; }
    }
    // 4. make_var_main per chunk, records appended in chunk order; the VCF body lines
    std::vector<lcd_var1_t> all;
    lcd_te_opt_t te; lcd_te_opt_default(&te);
    for (int c = 0; c < n; ++c) {
        const lcd_first_chunk_t &x = chunks[c].first; const lcd_clean_vars_t *v = x.vars;
        lcd_hap_problem_t p; memset(&p, 0, sizeof(p));
        std::vector<int> alle_off(v->n_vars + 1), allele_off(v->n_reads + 1);
        lcd_clean_vars_hap_problem(v, x.is_ont, x.order, x.is_skipped, alle_off.data(), allele_off.data(), &p);
        const lcd_hap_state_t &s = *x.state;
        p.haps = s.haps; p.phase_sets = s.phase_sets; p.n_clean_agree_snps = s.n_clean_agree_snps; p.n_clean_conflict_snps = s.n_clean_conflict_snps;
        p.var_phase_set = s.var_phase_set; p.hap_to_cons_alle = s.hap_to_cons_alle; p.hap_to_alle_profile = s.hap_to_alle_profile;
        std::vector<uint8_t> unknown;
        if (!v->alt_ref_base) unknown.assign((size_t)v->n_vars + 1, 4);
        lcd_var1_t *recs = nullptr;
        const int m = lcd_make_variants(&cfg->call, &p, v->ref_len, v->alt_len, v->alt_off, v->alt_pool, v->alt_ref_base ? v->alt_ref_base : unknown.data(), (const char *)x.ref_seq,
                                        x.ref_beg, x.reg_beg, x.reg_end, &recs);
        if (m < 0) {   // (the reference exits: more reads carry the alt allele than its coverage says)
            lcd_var1_t *tmp = (lcd_var1_t *)malloc((all.size() + 1) * sizeof(lcd_var1_t));
            if (!all.empty()) memcpy(tmp, all.data(), all.size() * sizeof(lcd_var1_t));
            lcd_free_variants(tmp, (int)all.size());
            return fail(set_err(m, W + ": lcd_make_variants failed on chunk " + std::to_string(c)));
        }
        if (m > 0) lcd_annotate_te(&cfg->call, &te, fields ? fields->lib : nullptr, (const char *)x.ref_seq, x.ref_beg, x.ref_end, recs, m);
        for (int i = 0; i < m; ++i) all.push_back(recs[i]);
        free(recs);                                            // (the members moved into `all`)
        chunks[c].n_records = m;
    }
    lcd_var1_t *out = (lcd_var1_t *)malloc((all.size() + 1) * sizeof(lcd_var1_t));
    if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(lcd_var1_t));
    char *text = nullptr;
    if (fields && fields->active()) {   // MEI / REPNAME from the library's names; ALTREADS: every chunk's records against that chunk's own read names
        std::string t; size_t at = 0; const size_t rn0 = fields->rnames.size();
        auto drop = [&](int code) { const std::string m = g_err; for (size_t i = rn0; i < fields->rnames.size(); ++i) free(fields->rnames[i]); fields->rnames.resize(rn0); lcd_free_variants(out, (int)all.size()); g_err = m; return fail(code); };
        int64_t n_mei = 0;
        for (int c = 0; c < n; ++c) {
            const int m = chunks[c].n_records; const lcd_bam_reads_t *meta = chunks[c].first.meta;
            if (m > 0 && fields->rnames_mode && (!meta || (meta->n_reads > 0 && (!meta->name_off || !meta->name_pool))))
                return drop(set_err(-4, W + ": read names are wanted and chunk " + std::to_string(c) + " has no name table (first.meta with name_off / name_pool)"));
            char *one = nullptr; int mei = 0;
            const int nl = lcd_format_vcf_fields(&cfg->call, links ? links->chroms[c] : chrom, out + at, m, fields->te_names, fields->rnames_mode, meta ? meta->n_reads : 0,
                                                 meta ? meta->name_off : nullptr, meta ? meta->name_pool : nullptr, &one, &mei);
            if (nl < 0) return drop(nl);
            if (one) t += one;
            free(one); n_mei += mei;
            for (int i = 0; fields->collect_rnames && fields->rnames_mode && i < m; ++i) {
                const lcd_var1_t &v = out[at + (size_t)i]; char *s = nullptr;
                if ((fields->rnames_mode == LCD_RNAMES_ALL || v.is_sv) && lcd_alt_read_names(&v, meta->n_reads, meta->name_off, meta->name_pool, &s)) return drop(-4);
                fields->rnames.push_back(s);
            }
            at += (size_t)m;
        }
        fields->n_mei += n_mei;
        text = (char *)malloc(t.size() + 1); memcpy(text, t.c_str(), t.size() + 1);
    } else if (!links) {
        const int nl = lcd_format_vcf(&cfg->call, chrom, out, (int)all.size(), &text);
        if (nl < 0) { lcd_free_variants(out, (int)all.size()); return fail(nl); }
    } else {   // the lines of every chunk under its own contig name
        std::string t; size_t at = 0;
        for (int c = 0; c < n; ++c) {
            char *one = nullptr;
            const int nl = lcd_format_vcf(&cfg->call, links->chroms[c], out + at, chunks[c].n_records, &one);
            if (nl < 0) { lcd_free_variants(out, (int)all.size()); return fail(nl); }
            if (one) t += one;
            free(one); at += (size_t)chunks[c].n_records;
        }
        text = (char *)malloc(t.size() + 1); memcpy(text, t.c_str(), t.size() + 1);
    }
    *records = out; *n_records = (int)all.size(); *vcf_body = text;
    return 0;
}

extern "C" {

// write_read_to_bam for every region of a call (src/bam_utils.c:1944-2048, called from the output step at src/call_var_main.c:801): the input's header block plus
// one @PG line, then per region its records with HP:i / PS:i rewritten in HBM (lcd_chunk_tag_records) and compressed there (lcd_bgzf_deflate_dev_ptr); only
// compressed bytes come down, and they go to the file with fwrite.  A region leaves out the records the region before it already wrote: its kept and its filtered
// records that overlap that region's [reg_beg, reg_end] (is_ovlp_with_prev_region, src/bam_utils.c:1684-1691) -- in a sorted file they are the first ones.
struct lcd_bam_writer_s {
    FILE *f = nullptr; lcd_bam_out_t *out = nullptr; std::string path; std::vector<uint8_t> buf;
    lcd_writer_opt_t o;      // the options of the open (all zero for none): the format, sort_output, where the sums over the appends go
    // write_index: the builder of the output's .bai (NULL: none, or given up), where the index goes; the file offset of the next member
    lcd_bai_builder_t *bai = nullptr; std::string index_path; uint64_t file_off = 0;
    // LCD_ALN_SAM: the records go out as SAM text (lcd_tagged_to_sam) instead of BGZF members; f may be stdout
    bool sam = false, own_f = true; lcd_sam_names_t *names = nullptr;
    ~lcd_bam_writer_s() { lcd_sam_names_free(names); lcd_bai_builder_destroy(bai); }
};
namespace {
// a += one append's statistics (the log counters of lcd_refine_stats_t are the writer's own and are added where the log is read)
void add_refine_stats(lcd_refine_stats_t &a, const lcd_refine_stats_t &b) {
    a.n_records += b.n_records; a.n_kept += b.n_kept; a.n_refined += b.n_refined; a.n_identical += b.n_identical; a.n_unrefined += b.n_unrefined; a.n_pos_moved += b.n_pos_moved;
    a.n_no_digars += b.n_no_digars; a.n_qlen_mismatch += b.n_qlen_mismatch; a.n_bad_pos += b.n_bad_pos; a.n_too_many_ops += b.n_too_many_ops; a.n_cg_cigar += b.n_cg_cigar;
    a.n_nm_replaced += b.n_nm_replaced; a.n_md_replaced += b.n_md_replaced; a.n_cs_replaced += b.n_cs_replaced; a.n_touched += b.n_touched;
    a.bytes_digars_up += b.bytes_digars_up; a.bytes_ref_up += b.bytes_ref_up; a.ms_measure += b.ms_measure; a.ms_emit += b.ms_emit;
}
void add_sam_stats(lcd_sam_stats_t &a, const lcd_sam_stats_t &b) {
    a.n_records += b.n_records; a.bytes_records += b.bytes_records; a.bytes_text += b.bytes_text; a.n_float_values += b.n_float_values; a.n_cg_cigar += b.n_cg_cigar;
    a.n_walk_stopped += b.n_walk_stopped; a.n_bad_layout += b.n_bad_layout; a.ms_measure += b.ms_measure; a.ms_emit += b.ms_emit; a.ms_download_write += b.ms_download_write;
}
// download + fwrite of one compressed image, then free
int writer_put(lcd_bam_writer_s *w, lcd_deflated_t *d, const std::string &W) {
    if (!d) return -1;
    lcd_bam_out_t *out = w->out;
    const double t0 = now_ms();
    const size_t sz = lcd_deflated_size(d);
    w->buf.resize(sz + 1);
    int rc = lcd_deflated_to_host(d, 0, sz, w->buf.data());
    if (!rc && sz && fwrite(w->buf.data(), 1, sz, w->f) != sz) rc = set_err(-30, W + ": short write on " + w->path);
    out->ms_deflate += lcd_deflated_kernel_ms(d); out->bytes_file += (int64_t)sz; w->file_off += sz;
    lcd_deflated_free(d);
    out->ms_download_write += now_ms() - t0;
    return rc;
}
// the output's index gives up (rule 3: an input with records out of order inside a region, or chunks appended out of order; a position outside the header's
// contigs): the BAM goes on, no index file stays, the statistics say why
void writer_skip_index(lcd_bam_writer_s *w, int code) {
    if (lcd_index_stats_t *ist = w->o.idx_stats) { ist->out_bai_skipped = code; snprintf(ist->out_bai_skip_reason, sizeof(ist->out_bai_skip_reason), "%s", g_err.c_str()); }
    lcd_bai_builder_destroy(w->bai); w->bai = nullptr;
    remove(w->index_path.c_str());
}
// the records of one append (a tagged stream in HBM, about to be written as the members of d at the writer's file offset) into the output's index
int writer_index_stream(lcd_bam_writer_s *w, const lcd_tagged_t *t, const lcd_deflated_t *d) {
    const double t0 = now_ms();
    const size_t nb = lcd_deflated_n_blocks(d);
    std::vector<lcd_bai_member_t> tab(nb);
    uint64_t u = 0, c = w->file_off;
    for (size_t i = 0; i < nb; ++i) {
        uint32_t payload = 0, bsize = 0;
        if (int rc = lcd_deflated_block_info(d, i, &payload, &bsize, nullptr)) return rc;
        tab[i].uoff = u; tab[i].coff = c; tab[i].ulen = payload; tab[i].pad = 0; u += payload; c += bsize;
    }
    size_t next = 0;
    const int rc = lcd_bai_builder_add_stream(w->bai, lcd_tagged_dev_ptr(t), lcd_tagged_size(t), 0, nb, tab.data(), w->file_off + lcd_deflated_size(d), &next);
    if (w->o.idx_stats) w->o.idx_stats->ms_out_bai += now_ms() - t0;
    if (rc == LCD_ERR_BAI_ORDER || rc == LCD_ERR_BAI_CSI || rc == LCD_ERR_BAI_CONTIG) { writer_skip_index(w, rc); return 0; }
    if (!rc && next != lcd_tagged_size(t)) return set_err(-24, "lcd_bam_writer_append: the tagged stream ends inside a record");
    return rc;
}
// the SAM writer's append: the tagged stream as text, download + fwrite
int writer_put_sam(lcd_bam_writer_s *w, const lcd_tagged_t *t, const std::string &W) {
    lcd_bam_out_t *out = w->out;
    lcd_sam_stats_t ss;
    lcd_sam_text_t *x = lcd_tagged_to_sam(t, w->names, &ss);
    if (!x) return -30;
    const double t0 = now_ms();
    const size_t sz = lcd_sam_text_size(x);
    w->buf.resize(sz + 1);
    int rc = lcd_sam_text_to_host(x, 0, sz, w->buf.data());
    if (!rc && sz && fwrite(w->buf.data(), 1, sz, w->f) != sz) rc = set_err(-30, W + ": short write on " + w->path);
    lcd_sam_text_free(x);
    out->bytes_file += (int64_t)sz; w->file_off += sz;
    ss.ms_download_write = now_ms() - t0; out->ms_download_write += ss.ms_download_write;
    if (w->o.sam_stats) add_sam_stats(*w->o.sam_stats, ss);
    return rc;
}
// pg_line as a line of its own behind the header text of `hdr` (the BAM header block), in front of the text's NUL padding; returns where the text then ends
size_t header_add_pg(std::vector<uint8_t> &hdr, const char *pg_line) {
    int l_text = 0; memcpy(&l_text, hdr.data() + 4, 4);
    size_t te = 8 + (size_t)l_text;
    while (te > 8 && hdr[te - 1] == 0) --te;
    if (!pg_line || !pg_line[0]) return te;
    std::string add = (te > 8 && hdr[te - 1] != '\n') ? "\n" : "";
    add += pg_line; add += '\n';
    hdr.insert(hdr.begin() + (long)te, add.begin(), add.end());
    l_text += (int)add.size(); memcpy(hdr.data() + 4, &l_text, 4);
    return te + add.size();
}
// the SAM header, in place: `text` comes in as the header text without its padding, the @PG line added
void sam_header_text(std::string &text, int n_ref, char **names, const int64_t *lens) {
    if (!text.empty() && text.back() != '\n') text += '\n';
    const bool have_sq = text.compare(0, 4, "@SQ\t") == 0 || text.find("\n@SQ\t") != std::string::npos;      // a line that starts with it
    if (!have_sq && n_ref > 0) {
        std::string sq;
        for (int r = 0; r < n_ref; ++r) sq += std::string("@SQ\tSN:") + names[r] + "\tLN:" + std::to_string((long long)lens[r]) + "\n";
        const size_t at = text.compare(0, 3, "@HD") == 0 && (text.size() == 3 || text[3] == '\t' || text[3] == '\n') ? text.find('\n') + 1 : 0;
        text.insert(at, sq);
    }
}
// what an open refuses before it reads or creates anything; then the one reset of *out's counters and of the statistics the options name
int writer_begin(const std::string &W, const char *in_bam_path, lcd_bam_out_t *out, const lcd_writer_opt_t &o) {
    if (o.refine_stats) memset(o.refine_stats, 0, sizeof(*o.refine_stats));
    if (o.sam_stats) memset(o.sam_stats, 0, sizeof(*o.sam_stats));
    if (!in_bam_path || !out || !out->path) return set_err(-4, W + ": NULL argument");
    out->n_records_out = out->n_filtered_out = out->bytes_inflated = out->bytes_file = 0; out->ms_tag = out->ms_deflate = out->ms_download_write = 0;
    if (o.format != LCD_ALN_BAM && o.format != LCD_ALN_SAM) return set_err(-4, W + ": format must be LCD_ALN_BAM or LCD_ALN_SAM");
    if (o.format == LCD_ALN_SAM && o.write_index) return set_err(-4, W + ": a SAM output has no index (write_index)");
    if (o.format == LCD_ALN_BAM && (out->block_payload < 0 || out->block_payload > 0xff00)) return set_err(-4, W + ": block_payload must be 0 or 1 ... 0xff00");
    return 0;
}
int writer_check_chunks(const std::string &W, int n, const lcd_call_chunk_t *chunks) {
    for (int c = 0; c < n; ++c) {
        const lcd_chunk_s *k = chunks[c].first.chunk;
        if (!k || !k->from_bam) return set_err(-4, W + ": chunk " + std::to_string(c) + " was not made from a BAM");
        if (k->n_reads > 0 && (!chunks[c].first.state || !chunks[c].first.state->haps || !chunks[c].first.state->phase_sets || chunks[c].first.state->n_reads != k->n_reads))
            return set_err(-4, W + ": chunk " + std::to_string(c) + " has no final haplotypes (call lcd_chunks_call first)");
    }
    return 0;
}
} // namespace

lcd_bam_writer_t *lcd_bam_writer_open(const char *in_bam_path, lcd_bam_out_t *out, const lcd_writer_opt_t *wopt) {
    const std::string W = "lcd_bam_writer_open";
    std::unique_ptr<lcd_bam_writer_s> w(new lcd_bam_writer_s());
    if (wopt) w->o = *wopt; else memset(&w->o, 0, sizeof(w->o));
    if (writer_begin(W, in_bam_path, out, w->o)) return nullptr;
    w->sam = w->o.format == LCD_ALN_SAM; w->out = out; w->path = out->path;
    std::vector<uint8_t> hdr;
    if (lcd_io_bam_header(in_bam_path, hdr)) { set_err(-30, W + ": " + lcd_io_last_error()); return nullptr; }
    const size_t text_end = header_add_pg(hdr, out->pg_line);
    std::string text;
    if (w->sam || w->o.write_index) {     // the contigs: their names for the SAM lines, their lengths for the index builder
        int n_ref = 0; char **names = nullptr; int64_t *lens = nullptr;
        if (lcd_bam_contigs(in_bam_path, &n_ref, &names, &lens)) return nullptr;
        if (w->sam) {
            text.assign((const char *)hdr.data() + 8, text_end - 8);
            sam_header_text(text, n_ref, names, lens);
            w->names = lcd_sam_names_create(n_ref, names);
        } else w->bai = lcd_bai_builder_create(n_ref, lens);
        lcd_bam_contigs_free(n_ref, names, lens);
        if (w->sam ? !w->names : !w->bai) return nullptr;
    }
    if (w->sam && !strcmp(out->path, "-")) { w->f = stdout; w->own_f = false; }
    else w->f = fopen(out->path, "wb");
    if (!w->f) { set_err(-30, W + ": cannot open " + out->path + " for writing"); return nullptr; }
    int rc = 0;
    if (w->sam) {
        if (!text.empty() && fwrite(text.data(), 1, text.size(), w->f) != text.size()) rc = set_err(-30, W + ": short write on " + w->path);
        out->bytes_file += (int64_t)text.size(); w->file_off += text.size();
    } else {
        rc = writer_put(w.get(), lcd_bgzf_deflate_dev(hdr.data(), hdr.size(), out->block_payload, 0), W);
        out->bytes_inflated += (int64_t)hdr.size();
    }
    if (rc) { const std::string m = g_err; if (w->own_f) fclose(w->f); g_err = m; return nullptr; }
    if (w->bai) {
        w->index_path = w->o.index_path ? std::string(w->o.index_path) : std::string(out->path) + ".bai";
        remove(w->index_path.c_str());     // (an index of an earlier file at this path would not describe the one being written)
    }
    return w.release();
}
int lcd_bam_writer_append(lcd_bam_writer_t *w, int n, const lcd_call_chunk_t *chunks, const int *tids, const lcd_stitch_carry_t *prev) {
    const std::string W = "lcd_bam_writer_append";
    if (!w || !w->f || n < 0 || (n > 0 && !chunks)) return set_err(-4, W + ": NULL argument");
    if (int rc = writer_check_chunks(W, n, chunks)) return rc;
    lcd_bam_out_t *out = w->out;
    for (int c = 0; c < n; ++c) {
        const lcd_first_chunk_t &x = chunks[c].first; const lcd_chunk_s *k = x.chunk;
        bool has_prev = c > 0 && (!tids || tids[c - 1] == tids[c]);
        int64_t pb = has_prev ? chunks[c - 1].first.reg_beg : 0, pe = has_prev ? chunks[c - 1].first.reg_end : 0;
        if (c == 0 && prev && prev->valid && (!tids || prev->tid == tids[0])) { has_prev = true; pb = prev->reg_beg; pe = prev->reg_end; }
        // the plan of the merged output: a record is left out iff it overlaps the region before (per record, whatever file it came from); the rest in table
        // (file-major) order, or sorted by position
        const int n_rec = (int)k->rec_beg.size();
        std::vector<uint8_t> skip((size_t)n_rec + 1); std::vector<int> order((size_t)n_rec + 1);
        const int n_out = lcd_merged_record_plan(n_rec, k->rec_file.data(), k->rec_pos0.data(), k->rec_endpos.data(), has_prev, pb, pe, w->o.sort_output != 0, skip.data(), order.data());
        if (n_out < 0) return n_out;
        const double t0 = now_ms();
        lcd_tagged_t *t = nullptr;
        if (k->refine_log) {     // refined alignments: the log of the chunk's rounds on a host copy of its digars, then the records from the final lists
            int n_touched = 0; int *t_reads = nullptr; uint64_t *t_off = nullptr, *d_off = nullptr; lcd_digar_t *t_dg = nullptr, *dg = nullptr; int64_t n_rej = 0;
            int rc = 0;
            if (lcd_refine_log_n_entries(k->refine_log) > 0) {
                rc = lcd_chunk_digars(k, &d_off, &dg);         // (returns the number of reads)
                if (rc >= 0) rc = lcd_refine_log_apply(k->refine_log, k->n_reads, d_off, dg, k->qlen.data(), &n_touched, &t_reads, &t_off, &t_dg, &n_rej);
            }
            lcd_refine_stats_t rs;
            if (!rc) t = lcd_chunk_refine_records(k, n_touched, t_reads, t_off, t_dg, x.ref_seq, x.ref_beg, x.ref_end, x.state ? x.state->haps : nullptr,
                                                  x.state ? x.state->phase_sets : nullptr, skip.data(), order.data(), &rs);
            free(t_reads); free(t_off); free(t_dg); free(d_off); free(dg);
            if (!t) return rc ? rc : -30;
            if (lcd_refine_stats_t *a = w->o.refine_stats) {
                add_refine_stats(*a, rs);
                a->n_log_entries += lcd_refine_log_n_entries(k->refine_log); a->bytes_log_down += lcd_refine_log_row_bytes(k->refine_log); a->n_log_rejected += n_rej;
            }
        } else t = lcd_chunk_tag_records_sel(k, x.state ? x.state->haps : nullptr, x.state ? x.state->phase_sets : nullptr, skip.data(), order.data());
        if (!t) return -30;
        out->ms_tag += now_ms() - t0;
        for (int i = 0; i < n_rec; ++i) if (!skip[i]) ++(k->rec_read[i] >= 0 ? out->n_records_out : out->n_filtered_out);
        out->bytes_inflated += (int64_t)lcd_tagged_size(t);
        if (w->sam) {
            const int rc = lcd_tagged_size(t) ? writer_put_sam(w, t, W) : 0;
            lcd_tagged_free(t);
            if (rc) return rc;
            continue;
        }
        lcd_deflated_t *d = lcd_tagged_size(t) ? lcd_bgzf_deflate_dev_ptr(lcd_tagged_dev_ptr(t), lcd_tagged_size(t), out->block_payload, 0) : nullptr;
        int rc = 0;
        if (lcd_tagged_size(t) && d && w->bai) rc = writer_index_stream(w, t, d);
        if (rc) { lcd_deflated_free(d); lcd_tagged_free(t); return rc; }
        rc = lcd_tagged_size(t) ? writer_put(w, d, W) : 0;
        lcd_tagged_free(t);
        if (rc) return rc;
    }
    return 0;
}
void lcd_bam_writer_abort(lcd_bam_writer_t *w) {
    if (!w) return;
    const std::string m = g_err;
    if (w->f && w->own_f) fclose(w->f); else if (w->f) fflush(w->f);
    if (w->bai) remove(w->index_path.c_str());
    delete w;
    g_err = m;
}
int lcd_bam_writer_close(lcd_bam_writer_t *w) {
    const std::string W = "lcd_bam_writer_close";
    if (!w) return set_err(-4, W + ": NULL argument");
    if (!w->sam) if (int rc = writer_put(w, lcd_bgzf_deflate_dev(nullptr, 0, w->out->block_payload, 1), W)) { lcd_bam_writer_abort(w); return rc; }   // the EOF member
    const std::string path = w->path;
    int rc = w->own_f ? fclose(w->f) : fflush(w->f);
    w->f = nullptr;
    if (rc != 0) { lcd_bam_writer_abort(w); return set_err(-30, W + ": closing " + path + " failed"); }
    if (w->bai) {   // the index after the EOF member
        const double t0 = now_ms();
        rc = lcd_bai_builder_finish(w->bai, w->index_path.c_str());
        lcd_index_stats_t *ist = w->o.idx_stats;
        if (!rc && ist) {
            const uint8_t *bytes = nullptr; size_t n = 0;
            (void)lcd_bai_builder_bytes(w->bai, &bytes, &n);
            ist->wrote_out_bai = 1; ist->out_bai_bytes = (int64_t)n;
            if (n >= 8) { uint64_t nc = 0; memcpy(&nc, bytes + n - 8, 8); ist->out_n_no_coor = (int64_t)nc; }
            ist->out_n_indexed = w->out->n_records_out + w->out->n_filtered_out - ist->out_n_no_coor;
            ist->ms_out_bai += now_ms() - t0;
        }
    }
    delete w;
    return rc;
}
int lcd_write_phased(const char *in_bam_path, int n, const lcd_call_chunk_t *chunks, lcd_bam_out_t *out, const lcd_writer_opt_t *wopt) {
    const std::string W = "lcd_write_phased";
    lcd_writer_opt_t o;
    if (wopt) o = *wopt; else memset(&o, 0, sizeof(o));
    if (int rc = writer_begin(W, in_bam_path, out, o)) return rc;
    if (n < 0 || (n > 0 && !chunks)) return set_err(-4, W + ": NULL argument");
    if (int rc = writer_check_chunks(W, n, chunks)) return rc;     // (before the output file is touched)
    lcd_bam_writer_t *w = lcd_bam_writer_open(in_bam_path, out, &o);
    if (!w) return -30;
    if (int rc = lcd_bam_writer_append(w, n, chunks, nullptr, nullptr)) { lcd_bam_writer_abort(w); return rc; }
    return lcd_bam_writer_close(w);
}

int lcd_call_bam_regions(const char *bam_path, const char *bai_path, const char *fasta_path, const char *chrom, int n, const int64_t *reg_beg, const int64_t *reg_end,
                         int min_mapq, const lcd_cfg_t *cfg, lcd_call_chunk_t *chunks, lcd_var1_t **records, int *n_records, char **vcf_body, lcd_bam_out_t *bam_out,
                         const lcd_run_opt_t *opt, const lcd_run_out_t *out) {
    return lcd_call_bam_regions_ext2(bam_path, bai_path, fasta_path, chrom, n, reg_beg, reg_end, min_mapq, cfg, chunks, records, n_records, vcf_body, bam_out, opt, out, nullptr);
}
// ... with lcd_run_ext2_t: the contig's methylation table, every region's chunk piled up with its final haplotypes, in region order
int lcd_call_bam_regions_ext2(const char *bam_path, const char *bai_path, const char *fasta_path, const char *chrom, int n, const int64_t *reg_beg, const int64_t *reg_end,
                              int min_mapq, const lcd_cfg_t *cfg, lcd_call_chunk_t *chunks, lcd_var1_t **records, int *n_records, char **vcf_body, lcd_bam_out_t *bam_out,
                              const lcd_run_opt_t *opt, const lcd_run_out_t *out, const lcd_run_ext2_t *ext2) {
    const std::string W = "lcd_call_bam_regions";
    if (records) *records = nullptr;
    if (n_records) *n_records = 0;
    if (vcf_body) *vcf_body = nullptr;
    zero_run_out(out);
    lcd_run_ext2_t x2; lcd_mods_opt_t mods_opt;
    if (int rc = ModsSink::parse(W, ext2, &x2, &mods_opt)) return rc;
    if (int rc = DepthSink::parse(W, x2)) return rc;
    lcd_run_ext2_split_t xs;
    {
        const char *other[3] = {bam_out ? bam_out->path : nullptr, x2.mods_path, x2.depth_path};
        if (int rc = SplitSink::parse(W, ext2, &xs, 3, other)) return rc;
    }
    if (int rc = check_aln_opt(W, opt)) return rc;
    if (opt && opt->aln && opt->aln->format == LCD_ALN_SAM) return set_err(-2, W + ": SAM text is not supported by this driver (lcd_write_phased on the called chunks writes it)");
    if (opt && opt->idx) return set_err(-4, W + ": index options are not supported by this driver");
    const lcd_vcf_fields_t *fields = opt ? opt->fields : nullptr;
    lcd_vcf_fields_out_t *fields_out = out ? out->fields_out : nullptr;
    const bool refine = opt && opt->aln && opt->aln->refine && bam_out;     // (without -b the option has no effect, as in the reference: no log is written)
    if (!bam_path || !bai_path || !fasta_path || !chrom || !cfg || !records || !n_records || !vcf_body) return set_err(-4, W + ": NULL argument");
    if (bam_out && !bam_out->path) return set_err(-4, W + ": bam_out without a path");
    if (n < 0 || (n > 0 && (!reg_beg || !reg_end || !chunks))) return set_err(-4, W + ": bad region list");
    for (int c = 0; c < n; ++c) if (reg_beg[c] < 1 || reg_end[c] < reg_beg[c] || (c > 0 && reg_beg[c] <= reg_end[c - 1])) return set_err(-4, W + ": regions must be 1-based, non-empty and in genome order");
    if (cfg->clean.out_somatic || cfg->opt.collect_ref_read_aln_str) return set_err(-2, W + ": somatic / refine mode is not supported");
    FieldsRun fr; fr.collect_rnames = fields_out != nullptr;
    if (int rc0 = fr.open(fields, W)) return rc0;
    const int is_ont = cfg->clean.is_ont != 0;
    lcd_digar_opt_t dopt; lcd_digar_opt_default(&dopt, is_ont);
    std::vector<lcd_chunk_t *> handles(n, nullptr); std::vector<uint8_t *> refs(n, nullptr); std::vector<lcd_bam_reads_t> metas(n);
    for (int c = 0; c < n; ++c) { memset(&chunks[c], 0, sizeof(lcd_call_chunk_t)); memset(&metas[c], 0, sizeof(lcd_bam_reads_t)); }
    auto drop_inputs = [&]() {
        for (int c = 0; c < n; ++c) {
            if (handles[c]) lcd_chunk_destroy(handles[c]);
            free(refs[c]); lcd_bam_reads_free(&metas[c]);
            handles[c] = nullptr; refs[c] = nullptr; chunks[c].first.chunk = nullptr; chunks[c].first.ref_seq = nullptr; chunks[c].first.meta = nullptr;
        }
    };
    auto fail = [&](int code) { const std::string m = g_err; drop_inputs(); g_err = m; return code; };
    for (int c = 0; c < n; ++c) {
        // a first pass on the device for the reads' span (and, for EQX data, the chunk itself)
        handles[c] = lcd_chunk_create_from_bam(&dopt, bam_path, bai_path, chrom, reg_beg[c], reg_end[c], min_mapq, 1, &metas[c]);
        if (!handles[c]) return fail(-30);
        int64_t lo = reg_beg[c], hi = reg_end[c];
        for (int r = 0; r < metas[c].n_reads; ++r) { lo = std::min(lo, metas[c].pos0[r] + 1); hi = std::max(hi, metas[c].end_pos[r]); }
        // get_bam_chunk_reg_ref_seq0 (src/bam_utils.c:1558-1571): 0-based [max(flank, beg - 1) - flank, min(len - flank - 1, end - 1) + flank], cut to the contig
        const int64_t flank = 50000, len = metas[c].target_len;
        const int64_t b0 = std::max<int64_t>(flank, lo - 1) - flank, e0 = std::min<int64_t>(len - flank - 1, hi - 1) + flank;
        const int64_t got = lcd_fasta_fetch(fasta_path, chrom, b0 + 1, e0 + 1, &refs[c]);
        if (got <= 0) return fail(set_err(got < 0 ? (int)got : -30, W + ": no reference sequence for the region (" + (got < 0 ? lcd_io_last_error() : "empty window") + ")"));
        bool again = is_ont;
        for (int r = 0; r < handles[c]->n_reads && !again; ++r) again = handles[c]->status[r] == -2;
        if (again) {
            lcd_chunk_destroy(handles[c]); handles[c] = nullptr; lcd_bam_reads_free(&metas[c]); memset(&metas[c], 0, sizeof(lcd_bam_reads_t));
            lcd_chunk_src_t src; src.ref_seq = (const char *)refs[c]; src.ref_beg = b0 + 1; src.ref_end = b0 + got; src.is_ont = is_ont;
            handles[c] = lcd_chunk_create_from_bam_src(&dopt, bam_path, bai_path, chrom, reg_beg[c], reg_end[c], min_mapq, 1, &src, &metas[c]);
            if (!handles[c]) return fail(-30);
        }
        if (refine && lcd_chunk_set_refine(handles[c], 1)) return fail(-11);
        lcd_first_chunk_t &x = chunks[c].first;
        x.chunk = handles[c]; x.ref_seq = refs[c]; x.ref_beg = b0 + 1; x.ref_end = b0 + got; x.reg_beg = reg_beg[c]; x.reg_end = reg_end[c]; x.is_ont = is_ont;
        x.ordered_read_ids = nullptr; x.is_rev = nullptr; x.meta = &metas[c];
    }
    int rc = chunks_call_core(n, chunks, cfg, chrom, nullptr, &fr, records, n_records, vcf_body);
    if (rc == 0) fr.give(fields_out);
    ModsSink mods;               // (created after the refusals and the call; removed when anything behind it fails)
    if (rc == 0 && x2.mods_path) {
        rc = mods.open(W, x2, mods_opt);
        for (int c = 0; c < n && !rc; ++c) rc = mods.chunk(handles[c], chunks[c].first, chrom);
    }
    DepthSink depth;             // the depth track, by the same order of events
    if (rc == 0 && x2.depth_path) {
        rc = depth.open(W, x2);
        for (int c = 0; c < n && !rc; ++c) rc = depth.chunk(handles[c], chunks[c].first, chrom);
    }
    SplitSink split;             // the read sets and the haplotag list, likewise; the plan is lcd_write_phased's: one contig, file order
    if (rc == 0 && (xs.split_prefix || xs.haplotag_path)) {
        int n_ref = 0; char **names = nullptr; int64_t *lens = nullptr;
        rc = xs.haplotag_path ? lcd_bam_contigs(bam_path, &n_ref, &names, &lens) : 0;
        if (!rc) rc = split.open(W, xs, n_ref, names, 0);
        if (names) lcd_bam_contigs_free(n_ref, names, lens);
        if (!rc) rc = split.window(n, chunks, nullptr, nullptr);
    }
    if (rc == 0 && bam_out) {   // (a failure here leaves the records and the text valid)
        lcd_writer_opt_t wo; memset(&wo, 0, sizeof(wo)); wo.refine_stats = out ? out->refine_stats : nullptr;
        rc = lcd_write_phased(bam_path, n, chunks, bam_out, &wo);
    }
    if (mods.active()) { const std::string m0 = g_err; const int rc3 = mods.finish(rc == 0); if (!rc) rc = rc3; else g_err = m0; }
    if (depth.active()) { const std::string m0 = g_err; const int rc3 = depth.finish(rc == 0); if (!rc) rc = rc3; else g_err = m0; }
    if (split.active()) { const std::string m0 = g_err; const int rc3 = split.finish(rc == 0); if (!rc) rc = rc3; else g_err = m0; }
    const std::string m = g_err;
    drop_inputs();
    g_err = m;
    return rc;
}

} // extern "C"
