// lcd_chunk.cpp -- digars (collect_digar_from_* for all reads of a chunk) and the device-resident chunk, lcd_chunk_t: creation from host arrays or from an
// indexed BAM, the host's view of it and the (region, read) slices cut in HBM.  The struct itself is in lcd_host_internal.h.
#include <cmath>
#include "lcd_host_internal.h"
#include "tag_words.h"

using namespace lcd_internal;

extern "C" {

// SURVEY 8(f) f2, first part: collect_digar_from_eqx_cigar (src/bam_utils.c:701-842) for all reads of a chunk
void lcd_digar_opt_default(lcd_digar_opt_t *o, int is_ont) {
    o->min_bq = 10; o->noisy_reg_max_xgaps = 5; o->noisy_reg_slide_win = is_ont ? 25 : 100; o->end_clip_reg = 30; o->end_clip_reg_flank_win = 100;
    o->max_noisy_frac_per_read = 0.5; o->max_var_ratio_per_read = 0.05;
}
// the four collect_digar_from_* entry points share everything behind the CIGAR-shaped operation words: `words` are host words (h_pool) or words already in
// HBM (d_words: the reference-comparison rewrite) with their per-read digar / event counts; clip_rule as DigarJob; rlen_true: bam_cigar2rlen of the BAM
// CIGAR where the words were derived from a tag instead (digar->end = bam_endpos(read), src/bam_utils.c:852)
namespace {
struct DigarWords {
    const uint32_t *h_pool = nullptr; const uint64_t *off = nullptr; const int *n_cigar = nullptr;
    const DevBuf *d_words = nullptr; const RefCmpOut *counts = nullptr;
    int clip_rule = 0; const int64_t *rlen_true = nullptr; const int *pre_status = nullptr;
    const int *n_indel = nullptr; // with counts: how many of the window events are insertions / deletions (tighter window capacity)
    uint64_t d_qual_base = 0;   // != 0: the qualities are already in HBM (qual_off relative to this address; qual_pool unused)
    // a chunk that mixes the four sources (lcd_chunk_create_from_bam_src): per read the device address of its words (they lie in several pools) and its clip rule
    const uint64_t *addr = nullptr; const int *clip_rule_r = nullptr;
};
// keep: the digars stay in HBM (a device-resident chunk, lcd_chunk_t): `keep->d_dig` receives them, nothing of them is downloaded, *digars_out stays NULL and
// keep->slot / keep->n_digar say where read r's digars are (record index into d_dig, count)
struct DigarKeep { DevBuf *d_dig; std::vector<uint64_t> slot; std::vector<int> n_digar; };
int digar_batch_core(const lcd_digar_opt_t *opt, int n, const int64_t *pos0, const DigarWords &W,
                    const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags, int64_t reg_beg, int64_t reg_end,
                    int64_t whole_ref_len, uint64_t **digar_off_out, lcd_digar_t **digars_out, uint64_t **iv_off_out, lcd_noisy_iv_t **ivs_out,
                    uint8_t **iv_in_chunk_out, int *status, int64_t *beg, int64_t *end, int *n_cand_vars, hipStream_t st, DigarKeep *keep = nullptr) {
    const uint32_t *cigar_pool = W.h_pool; const uint64_t *cigar_off = W.off; const int *n_cigar = W.n_cigar;
    static_assert(sizeof(lcd_digar_t) == sizeof(DigarRec) && sizeof(lcd_noisy_iv_t) == sizeof(IvRec), "ABI structs mirror the device records");
    // capacities from one pass over the CIGAR words (the host has them in hand anyway), or from the rewrite's count pass
    std::vector<DigarJob> jobs(n);
    uint64_t cig_words = 0, qual_bytes = 0, dtot = 0, itot = 0, etot = 0;
    for (int r = 0; r < n; ++r) { cig_words = std::max<uint64_t>(cig_words, cigar_off[r] + n_cigar[r]); qual_bytes = std::max<uint64_t>(qual_bytes, qual_off[r] + qlen[r]); }
    for (int r = 0; r < n; ++r) {
        DigarJob &j = jobs[r];
        long long nd = 0, nev = 0, nid = -1; // digars; window events; of those insertions / deletions (-1: not counted)
        if (W.counts) { nd = W.counts[r].nd; nev = W.counts[r].nev; if (W.n_indel) nid = W.n_indel[r]; }
        else { nid = 0; for (int i = 0; i < n_cigar[r]; ++i) { const uint32_t c = cigar_pool[cigar_off[r] + i]; const int op = c & 0xf, len = (int)(c >> 4); if (op == 8) { nd += len; nev += len; } else if (op != 3 && op != 9) { ++nd; if (op == 1 || op == 2) { ++nev; ++nid; } } } }
        j.n_cigar = n_cigar[r]; j.qlen = qlen[r]; j.pos0 = pos0[r]; j.left_pal = pal_flags ? pal_flags[r] & 1 : 0; j.right_pal = pal_flags ? (pal_flags[r] >> 1) & 1 : 0;
        j.digar_cap = (int)nd; j.ev_cap = (int)nev + 1; j.clip_rule = W.clip_rule_r ? W.clip_rule_r[r] : W.clip_rule;
        // windows are disjoint and each holds events of total weight > max_xgaps (a mismatch weighs 1, an insertion / deletion its length): at most one per
        // indel event plus one per max_xgaps + 1 mismatches, plus the two clip flanks
        j.iv_cap = (int)(nid >= 0 ? nid + (nev - nid) / (opt->noisy_reg_max_xgaps + 1) : nev) + 4;
        j.cigar_off = W.addr ? W.addr[r] : cigar_off[r] * 4; j.qual_off = qual_off[r];
        j.digar_off = dtot * sizeof(DigarRec); dtot += nd; j.iv_off = itot * sizeof(IvRec); itot += j.iv_cap; j.ev_off = etot * 16; etot += j.ev_cap;
    }
    DevBuf d_cig, d_qual, d_jobs, d_outs, d_dig_local, d_iv, d_ev;
    DevBuf &d_dig = keep ? *keep->d_dig : d_dig_local;
    if ((!W.d_words && d_cig.ensure(cig_words * 4 + 64)) || (!W.d_qual_base && d_qual.ensure(qual_bytes + 64)) || d_jobs.ensure(n * sizeof(DigarJob)) || d_outs.ensure(n * sizeof(DigarOut)) ||
        d_dig.ensure(dtot * sizeof(DigarRec) + 64) || d_iv.ensure(itot * sizeof(IvRec) + 64) || d_ev.ensure(etot * 16 + 64)) return -11;
    const uint64_t cig_base = W.d_words ? W.d_words->addr() : d_cig.addr();
    for (DigarJob &j : jobs) { if (!W.addr) j.cigar_off += cig_base; j.qual_off += W.d_qual_base ? W.d_qual_base : d_qual.addr(); j.digar_off += d_dig.addr(); j.iv_off += d_iv.addr(); j.ev_off += d_ev.addr(); }
    if (!W.d_words) HIPCHK(hipMemcpyAsync(d_cig.p, cigar_pool, cig_words * 4, hipMemcpyHostToDevice, st));
    if (!W.d_qual_base) HIPCHK(hipMemcpyAsync(d_qual.p, qual_pool, qual_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(DigarJob), hipMemcpyHostToDevice, st));
    DigarOpt dopt; dopt.min_bq = opt->min_bq; dopt.max_xgaps = opt->noisy_reg_max_xgaps; dopt.win = opt->noisy_reg_slide_win; dopt.end_clip_reg = opt->end_clip_reg;
    dopt.end_clip_flank = opt->end_clip_reg_flank_win; dopt.pad = 0; dopt.whole_ref_len = whole_ref_len;
    lcd_launch_digar((const DigarJob *)d_jobs.p, (DigarOut *)d_outs.p, dopt, n, st);
    HIPCHK(hipGetLastError());
    std::vector<DigarOut> outs(n);
    std::vector<DigarRec> hd(keep ? 1 : dtot + 1); std::vector<IvRec> hiv(itot + 1);
    HIPCHK(hipMemcpyAsync(outs.data(), d_outs.p, n * sizeof(DigarOut), hipMemcpyDeviceToHost, st));
    if (dtot && !keep) { HIPCHK(hipMemcpyAsync(hd.data(), d_dig.p, dtot * sizeof(DigarRec), hipMemcpyDeviceToHost, st)); g_copy_bytes[0] += dtot * sizeof(DigarRec); }
    if (itot) HIPCHK(hipMemcpyAsync(hiv.data(), d_iv.p, itot * sizeof(IvRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t *doff = (uint64_t *)malloc((n + 1) * sizeof(uint64_t)), *ioff = (uint64_t *)malloc((n + 1) * sizeof(uint64_t));
    uint64_t niv = 0;
    for (int r = 0; r < n; ++r) { if (outs[r].status == -3) { free(doff); free(ioff); return set_err(-24, "digar batch: capacity estimate too small"); } niv += outs[r].n_iv; }
    lcd_digar_t *dg = keep ? nullptr : (lcd_digar_t *)malloc((dtot + 1) * sizeof(lcd_digar_t));
    if (keep) { keep->slot.resize(n); keep->n_digar.resize(n); }
    lcd_noisy_iv_t *iv = (lcd_noisy_iv_t *)malloc((niv + 1) * sizeof(lcd_noisy_iv_t)); uint8_t *inc = (uint8_t *)calloc(niv + 1, 1);
    uint64_t dw = 0, iw = 0;
    for (int r = 0; r < n; ++r) {
        const DigarJob &j = jobs[r]; const DigarOut &o = outs[r];
        doff[r] = dw; ioff[r] = iw;
        if (keep) { keep->slot[r] = (j.digar_off - d_dig.addr()) / sizeof(DigarRec); keep->n_digar[r] = o.n_digar; }
        else memcpy(dg + dw, hd.data() + (j.digar_off - d_dig.addr()) / sizeof(DigarRec), (size_t)o.n_digar * sizeof(DigarRec));
        dw += o.n_digar;
        const IvRec *src = hiv.data() + (j.iv_off - d_iv.addr()) / sizeof(IvRec);
        std::vector<IvRec> v(src, src + o.n_iv);
        // cr_index (src/cgranges.c): intervals stay as added when their starts are non-decreasing, otherwise they are sorted by start --
        // an insertion sort for up to 64 of them, i.e. stable (longer unsorted lists: radix passes whose tie order is not reproduced here;
        // a tie needs a window starting exactly where the right-clip flank starts)
        // (starts are >= 0: the kernel clamps like cr_add does, src/cgranges.c:146)
        auto key = [](const IvRec &a) { return (uint64_t)(long long)(int)a.st; };
        bool sorted = true; for (int k = 1; k < o.n_iv; ++k) if (key(v[k]) < key(v[k - 1])) sorted = false;
        if (!sorted) std::stable_sort(v.begin(), v.end(), [&](const IvRec &a, const IvRec &b) { return key(a) < key(b); });
        long long total = 0;
        for (const IvRec &x : v) total += x.en - x.st + 1;                     // collect_noisy_region_len (:631)
        beg[r] = j.pos0 + 1; end[r] = j.pos0 + (W.rlen_true ? W.rlen_true[r] : o.rlen); n_cand_vars[r] = o.n_cand;
        const long long mapped = end[r] - beg[r] + 1;
        const bool skip = (double)total > mapped * opt->max_noisy_frac_per_read || (double)o.n_cand > mapped * opt->max_var_ratio_per_read; // (:811)
        status[r] = (o.status == -2 || (W.pre_status && W.pre_status[r])) ? -2 : skip ? -1 : 0;
        for (int k = 0; k < o.n_iv; ++k) {
            iv[iw + k].start = v[k].st; iv[iw + k].end = v[k].en; iv[iw + k].label = v[k].label; iv[iw + k].pad = 0;
            inc[iw + k] = !skip && !(v[k].st + 1 > reg_end || v[k].en < reg_beg);    // is_overlap_reg(start + 1, end, ...) (:820)
        }
        iw += o.n_iv;
    }
    doff[n] = dw; ioff[n] = iw;
    *digar_off_out = doff; *digars_out = dg; *iv_off_out = ioff; *ivs_out = iv; *iv_in_chunk_out = inc;
    return 0;
}

// (the host side of the cs / MD paths, cs_to_words / md_to_words: tag_words.h)
using lcd_tag_words::cs_to_words; using lcd_tag_words::md_to_words;
} // namespace

int lcd_digar_batch(const lcd_digar_opt_t *opt, int n, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off, const int *n_cigar,
                    const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags, int64_t reg_beg, int64_t reg_end,
                    int64_t whole_ref_len, uint64_t **digar_off_out, lcd_digar_t **digars_out, uint64_t **iv_off_out, lcd_noisy_iv_t **ivs_out,
                    uint8_t **iv_in_chunk_out, int *status, int64_t *beg, int64_t *end, int *n_cand_vars) {
    *digar_off_out = *iv_off_out = nullptr; *digars_out = nullptr; *ivs_out = nullptr; *iv_in_chunk_out = nullptr;
    if (ensure_init()) return -1;
    if (n <= 0) return 0;
    StreamGuard st; if (st.create()) return -10;
    DigarWords W; W.h_pool = cigar_pool; W.off = cigar_off; W.n_cigar = n_cigar;
    return digar_batch_core(opt, n, pos0, W, qual_pool, qual_off, qlen, pal_flags, reg_beg, reg_end, whole_ref_len, digar_off_out, digars_out, iv_off_out, ivs_out,
                            iv_in_chunk_out, status, beg, end, n_cand_vars, st);
}

// ---- a DEVICE-RESIDENT chunk (SURVEY 8f f2 -> region jobs without the host round trips): the reads' CIGARs, qualities and 4-bit bases go up ONCE, the digars are
// made and KEPT in HBM, the (region, read) slices are cut there and a batch's read slices are unpacked from there -- the host sees what its glue needs (per-read
// status / span / candidate count, the noisy intervals: tens per read; per slice two offsets and a cover flag) and never a digar or a base.
// Reference: collect_digar_from_eqx_cigar src/bam_utils.c:701-842, collect_noisy_read_info src/align.c:1377-1461. ----
lcd_chunk_t *lcd_chunk_create(const lcd_digar_opt_t *opt, int n, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off, const int *n_cigar,
                              const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags, const uint8_t *seq_pool,
                              const uint64_t *seq_off, int64_t reg_beg, int64_t reg_end, int64_t whole_ref_len) {
    if (ensure_init() || n <= 0) return nullptr;
    std::unique_ptr<lcd_chunk_s> c(new lcd_chunk_s());
    c->device = cur_device(); c->n_reads = n; c->opt = *opt;
    c->qlen.assign(qlen, qlen + n); c->seq_off.assign(seq_off, seq_off + n); c->qual_off.assign(qual_off, qual_off + n);
    uint64_t seq_bytes = 0, qual_bytes = 0;
    for (int r = 0; r < n; ++r) { seq_bytes = std::max<uint64_t>(seq_bytes, seq_off[r] + (uint64_t)(qlen[r] + 1) / 2); qual_bytes = std::max<uint64_t>(qual_bytes, qual_off[r] + (uint64_t)qlen[r]); }
    c->h_qual.assign(qual_pool, qual_pool + qual_bytes);
    StreamGuard st; if (st.create()) return nullptr;
    if (c->d_seq.ensure(seq_bytes + 64)) return nullptr;
    if (hipMemcpyAsync(c->d_seq.p, seq_pool, seq_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { set_err(-10, "lcd_chunk_create: upload failed"); return nullptr; }
    g_copy_bytes[2] += seq_bytes; // the records' bases: once per chunk, 4-bit packed
    c->status.resize(n); c->n_cand.resize(n); c->beg.resize(n); c->end.resize(n);
    DigarWords W; W.h_pool = cigar_pool; W.off = cigar_off; W.n_cigar = n_cigar;
    DigarKeep keep; keep.d_dig = &c->d_dig;
    uint64_t *doff = nullptr; lcd_digar_t *dg = nullptr;
    const int rc = digar_batch_core(opt, n, pos0, W, qual_pool, qual_off, qlen, pal_flags, reg_beg, reg_end, whole_ref_len, &doff, &dg, &c->iv_off, &c->ivs, &c->iv_in_chunk,
                                    c->status.data(), c->beg.data(), c->end.data(), c->n_cand.data(), st, &keep);
    free(doff);
    if (rc) return nullptr;
    if (hipStreamSynchronize(st) != hipSuccess) { set_err(-10, "lcd_chunk_create: synchronize failed"); return nullptr; }
    c->slot.swap(keep.slot); c->n_digar.swap(keep.n_digar);
    c->seq_base = c->d_seq.addr();
    return c.release();
}
// f3 on the device, in front of the chunk: the region's BGZF blocks (through the .bai) are read from the file and uploaded compressed, inflated by
// lcd_inflate_kernel, the records are found / measured / filtered in HBM (bam_kernel.hip) and their digars made there -- what sam_itr_queryi + sam_itr_next
// (htslib: bgzf_read_block, inflate, bam_read1) and the record loop of collect_ref_seq_bam_main (src/bam_utils.c:1672-1706) followed by
// collect_digar_from_eqx_cigar (:701-842) do for the reference on the calling thread.  The host sees 40 + 40 bytes per record (descriptor, CIGAR statistics),
// never a base, a quality or a digar.  Records, filters, order and stop rule are lcd_bam_load_region_indexed's (Collector::take).
//
// With `src` every read gets the source the reference would choose for it (collect_digar_from_bam, src/collect_var.c:1072-1079): lcd_bam_aux_kernel hops the kept
// records' auxiliary fields in HBM; reads compared with the reference go through the lcd_refcmp_kernel passes on the CIGAR words and the 4-bit bases where the
// inflate left them; the cs / MD VALUES (O(events) bytes, the only record bytes that cross PCIe) come to the host, are parsed by cs_to_words / md_to_words and go
// back as EQX-shaped words; ONE digar launch covers all reads.  src == NULL is lcd_chunk_create_from_bam as it always was.
//
// Several files of one sample (collect_ref_seq_bam_main's loop over the files, src/bam_utils.c:1659-1716): the files' region images are appended in file order and
// inflated in ONE launch; every index range is one walk job that ends at its own file's segment of the stream; the loader's rule runs file by file (its stop rule and
// the contig's tid, looked up by name in every header, restart at each file), so the chunk's reads and its record table are file-major.  Nothing behind this function
// knows about files: no kernel takes a file index.  lcd_chunk_open_from_bam is the n = 1 case.
namespace {
lcd_chunk_t *chunk_open_files(const lcd_digar_opt_t *opt, int n_bams, const char *const *bam_paths, const char *const *bai_paths, const char *chrom, int64_t reg_beg,
                              int64_t reg_end, int min_mapq, int verify_crc, lcd_bam_reads_t *meta) {
    if (ensure_init()) return nullptr;
    LcdRegionImage im;
    if (lcd_io_region_images(n_bams, bam_paths, bai_paths, chrom, reg_beg, reg_end, im)) { set_err(-30, std::string("lcd_chunk_create_from_bam: ") + lcd_io_last_error()); return nullptr; }
    std::unique_ptr<lcd_chunk_s> c(new lcd_chunk_s());
    c->device = cur_device(); c->n_reads = 0; c->opt = *opt; c->from_bam = true; c->n_files = n_bams; c->reg_beg = reg_beg; c->reg_end = reg_end;
    c->pending.reset(new ChunkPending());
    ChunkPending &P = *c->pending; P.reg_beg = reg_beg; P.reg_end = reg_end; P.tlen = im.tlen;
    if (meta) { meta->tid = im.tid; meta->n_targets = im.n_ref; meta->target_len = im.tlen; }
    if (im.image.empty() || im.ranges.empty()) return c.release();
    c->stream = lcd_bgzf_inflate_dev(im.image.data(), im.image.size(), verify_crc);
    if (!c->stream) { set_err(-32, std::string("lcd_chunk_create_from_bam: ") + lcd_io_last_error()); return nullptr; }
    const uint64_t base = lcd_inflated_dev_ptr(c->stream), usize = lcd_inflated_size(c->stream);
    if (!usize) return c.release();
    StreamGuard st; if (st.create()) return nullptr;
    auto fail = [&](int code, const std::string &m) -> lcd_chunk_t * { set_err(code, "lcd_chunk_create_from_bam: " + m); return nullptr; };
#define CHK(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return fail(-10, "HIP call failed: " #x); } } while (0)
    // 1. the records of every range: one serial hop per record on the device
    const int nr = (int)im.ranges.size();
    std::vector<int> file_of(nr, 0);     // the file a range belongs to
    for (int f = 0; f < n_bams; ++f) for (size_t k = 0; k < im.files[f].range_n; ++k) file_of[im.files[f].range_first + k] = f;
    std::vector<BamWalkJob> wj(nr); std::vector<BamWalkOut> wo(nr);
    std::vector<BamRecDesc> descs; std::vector<size_t> first(nr + 1, 0);
    DevBuf d_desc, d_wj, d_wo;
    for (int attempt = 0; attempt < 2; ++attempt) {
        size_t tot = 0;
        for (int k = 0; k < nr; ++k) {
            const uint64_t len = im.ranges[k].second > im.ranges[k].first ? im.ranges[k].second - im.ranges[k].first : 0;
            const size_t cap = attempt == 0 ? (size_t)(len / 256 + 1024) : (size_t)(len / 36 + 2); // (a record is at least 36 bytes; long reads are tens of kilobytes)
            first[k] = tot; tot += cap; wj[k].cap = (int)cap;
        }
        first[nr] = tot;
        if (d_desc.ensure(tot * sizeof(BamRecDesc)) || d_wj.ensure(nr * sizeof(BamWalkJob)) || d_wo.ensure(nr * sizeof(BamWalkOut))) return nullptr;
        for (int k = 0; k < nr; ++k) {
            // a walk ends at its FILE's segment of the stream, not at the stream's end: behind the segment lie the next file's bytes
            const uint64_t fend = std::min<uint64_t>(im.files[file_of[k]].uend, usize);
            wj[k].stream = base; wj[k].ubeg = std::min<uint64_t>(im.ranges[k].first, fend); wj[k].uend = std::min<uint64_t>(im.ranges[k].second, fend); wj[k].usize = fend;
            wj[k].descs = d_desc.addr() + first[k] * sizeof(BamRecDesc); wj[k].reg_end = reg_end; wj[k].tid = im.files[file_of[k]].tid;
        }
        CHK(hipMemcpyAsync(d_wj.p, wj.data(), nr * sizeof(BamWalkJob), hipMemcpyHostToDevice, st));
        lcd_launch_bam_walk((const BamWalkJob *)d_wj.p, (BamWalkOut *)d_wo.p, nr, st);
        CHK(hipGetLastError());
        CHK(hipMemcpyAsync(wo.data(), d_wo.p, nr * sizeof(BamWalkOut), hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        bool over = false; for (int k = 0; k < nr; ++k) if (wo[k].status == 3) over = true;
        if (!over) break;
        if (attempt == 1) return fail(-24, "record descriptor capacity");
    }
    size_t nrec = 0; std::vector<size_t> at(nr + 1, 0);
    for (int k = 0; k < nr; ++k) { at[k] = nrec; nrec += (size_t)wo[k].n; } at[nr] = nrec;
    descs.resize(nrec + 1);
    for (int k = 0; k < nr; ++k) if (wo[k].n) CHK(hipMemcpyAsync(descs.data() + at[k], (const uint8_t *)d_desc.p + first[k] * sizeof(BamRecDesc), (size_t)wo[k].n * sizeof(BamRecDesc), hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    // 2. CIGAR statistics of the wanted reference's records
    std::vector<int> stat_of(nrec, -1); std::vector<BamStatJob> sj;
    std::vector<int> tid_of(nrec + 1, -1);     // per record the wanted contig's tid in its own file
    for (int k = 0; k < nr; ++k) for (size_t i = at[k]; i < at[k + 1]; ++i) tid_of[i] = im.files[file_of[k]].tid;
    for (size_t i = 0; i < nrec; ++i) if (descs[i].refid == tid_of[i]) {
        BamStatJob j; j.rec = base + descs[i].off; j.bs = descs[i].bs; j.lname = descs[i].lname; j.nc = descs[i].nc; j.lseq = descs[i].lseq;
        stat_of[i] = (int)sj.size(); sj.push_back(j);
    }
    std::vector<BamStatOut> so(sj.size() + 1);
    DevBuf d_sj, d_so;
    if (!sj.empty()) {
        if (d_sj.ensure(sj.size() * sizeof(BamStatJob)) || d_so.ensure(sj.size() * sizeof(BamStatOut))) return nullptr;
        CHK(hipMemcpyAsync(d_sj.p, sj.data(), sj.size() * sizeof(BamStatJob), hipMemcpyHostToDevice, st));
        lcd_launch_bam_stat((const BamStatJob *)d_sj.p, (BamStatOut *)d_so.p, (int)sj.size(), st);
        CHK(hipGetLastError());
        CHK(hipMemcpyAsync(so.data(), d_so.p, sj.size() * sizeof(BamStatOut), hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
    }
    // 3. the loader's rule, record by record in file order (Collector::take in lcd_io.cpp)
    std::vector<int64_t> &pos0 = P.pos0, &rl_true = P.rl_true; std::vector<int> &ncig = P.ncig, &qlen = P.qlen, &nindel = P.nindel; std::vector<uint64_t> &coff = P.coff, &soff = P.soff, &qoff = P.qoff;
    std::vector<RefCmpOut> &counts = P.counts; std::vector<BamAuxJob> &auxj = P.auxj; DevBuf &d_cig = P.d_cig;   // (kept for lcd_chunk_resolve)
    std::vector<int64_t> endp; std::vector<int> mapq, flag; std::vector<uint64_t> noff; std::vector<GatherJob> gj, nj;
    uint64_t cw = 0, nbytes = 0;
    const char *malformed = "malformed BAM record (a field runs past the record, or a placeholder CIGAR without its CG tag)";
    for (int f = 0; f < n_bams; ++f) {
        const int ftid = im.files[f].tid; const size_t n_before = pos0.size();     // (the stop rules see this file's reads only)
        bool done = false;
        for (int k = (int)im.files[f].range_first; k < (int)(im.files[f].range_first + im.files[f].range_n) && !done; ++k) {
            for (size_t i = at[k]; i < at[k + 1] && !done; ++i) {
                const BamRecDesc &d = descs[i];
                if (d.refid != ftid) { if ((d.refid > ftid || d.refid < 0) && pos0.size() > n_before) done = true; continue; }
                const BamStatOut &x = so[stat_of[i]];
                if (x.kind == -2) return fail(-33, malformed);
                const int64_t e0 = (int64_t)d.pos + (x.rl > 0 ? x.rl : 1);
                if (d.pos >= reg_end) { done = true; break; }
                // the record table of the alignment output: the iterator's overlap test applies whatever the flags say; PROJECT RULE (htslib is not in the checkout): a
                // record with the unmapped flag spans one base, like one whose CIGAR consumes no reference (bam_endpos)
                const int64_t e0_any = (d.flag & 0x4) ? (int64_t)d.pos + 1 : e0;
                const bool kept = e0 > reg_beg - 1 && !((d.flag & (0x4 | 0x100 | 0x800)) || (int)d.mapq < min_mapq);
                if (e0_any > reg_beg - 1) {
                    c->rec_beg.push_back(d.off - 4); c->rec_stop.push_back(d.off + (uint64_t)d.bs); c->rec_read.push_back(kept ? (int)pos0.size() : -1);
                    c->rec_pos0.push_back(d.pos); c->rec_endpos.push_back(e0_any); c->rec_file.push_back(f);
                }
                if (e0 <= reg_beg - 1) continue;
                if ((d.flag & (0x4 | 0x100 | 0x800)) || (int)d.mapq < min_mapq) continue;
                c->read_file.push_back(f);
                pos0.push_back(d.pos); endp.push_back(e0); mapq.push_back(d.mapq); flag.push_back(d.flag); ncig.push_back(x.nc); qlen.push_back(d.lseq);
                const uint64_t sq = d.off + 32 + d.lname + 4ull * d.nc;
                soff.push_back(sq); qoff.push_back(sq + ((uint64_t)d.lseq + 1) / 2);
                c->aux_off.push_back(sq + ((uint64_t)d.lseq + 1) / 2 + (uint64_t)d.lseq); c->rec_end.push_back(d.off + (uint64_t)d.bs); // (the walk checked: the fixed fields end inside the record)
                coff.push_back(cw); { GatherJob g; g.src = x.cig_src; g.dst = cw * 4; g.bytes = (uint32_t)x.nc * 4u; g.pad_ = 0; gj.push_back(g); } cw += (uint64_t)x.nc;
                RefCmpOut rc; rc.n_ops = x.nc; rc.nd = (int)x.nd; rc.nev = (int)x.nev; rc.pad = 0; counts.push_back(rc); nindel.push_back((int)x.nid);
                {
                    BamAuxJob a; a.rec = base + d.off; a.cig = x.cig_src; a.bs = d.bs; a.lname = d.lname; a.nc16 = d.nc; a.lseq = d.lseq; a.nc = x.nc; a.flag = d.flag; a.prim_pos = (long long)d.pos + 1; a.prim_end = e0;
                    auxj.push_back(a); rl_true.push_back(x.rl);
                }
                noff.push_back(nbytes); { GatherJob g; g.src = base + d.off + 32; g.dst = nbytes; g.bytes = d.lname; g.pad_ = 0; nj.push_back(g); } nbytes += d.lname;
            }
            if (!done) {
                if (wo[k].status == 1) return fail(-33, "truncated BAM record");
                if (wo[k].status == 2) return fail(-33, malformed);
            }
        }
    }
    const int n = (int)pos0.size();
    c->n_reads = n;
    // read names: one gather + one copy (the only record bytes that come to the host)
    std::vector<char> names(nbytes + 1, 0);
    DevBuf d_gj, d_names;
    if (n > 0) {
        if (d_cig.ensure(cw * 4 + 64) || d_gj.ensure((size_t)n * sizeof(GatherJob)) || d_names.ensure(nbytes + 64)) return nullptr;
        for (GatherJob &g : gj) g.dst += d_cig.addr();
        CHK(hipMemcpyAsync(d_gj.p, gj.data(), (size_t)n * sizeof(GatherJob), hipMemcpyHostToDevice, st));
        lcd_launch_bam_cigar((const GatherJob *)d_gj.p, n, st);
        CHK(hipGetLastError());
        if (meta) {
            CHK(hipStreamSynchronize(st)); // (d_gj is reused)
            for (GatherJob &g : nj) g.dst += d_names.addr();
            CHK(hipMemcpyAsync(d_gj.p, nj.data(), (size_t)n * sizeof(GatherJob), hipMemcpyHostToDevice, st));
            lcd_launch_gather((const GatherJob *)d_gj.p, n, st);
            CHK(hipGetLastError());
            CHK(hipMemcpyAsync(names.data(), d_names.p, nbytes, hipMemcpyDeviceToHost, st));
            CHK(hipStreamSynchronize(st));
        }
    }
    auto dupv = [](const auto &v) { using T = typename std::decay<decltype(v[0])>::type; T *p = (T *)malloc((v.size() + 1) * sizeof(T)); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; };
    if (meta) {
        meta->n_reads = n; meta->pos0 = dupv(pos0); meta->end_pos = dupv(endp); meta->mapq = dupv(mapq); meta->flag = dupv(flag); meta->n_cigar = dupv(ncig); meta->qlen = dupv(qlen);
        meta->cigar_off = dupv(coff); meta->seq_off = dupv(soff); meta->qual_off = dupv(qoff); meta->name_off = dupv(noff); meta->name_pool = dupv(names);
        // (cigar_pool / seq_pool / qual_pool stay NULL: those bytes are in HBM; seq_off / qual_off are offsets of the inflated stream)
    }
    if (n > 0 && hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); if (meta) { lcd_bam_reads_free(meta); memset(meta, 0, sizeof(*meta)); } return fail(-10, "HIP call failed: hipStreamSynchronize"); }
#undef CHK
    return c.release();
}
} // namespace

lcd_chunk_t *lcd_chunk_open_from_bam(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end,
                                     int min_mapq, int verify_crc, lcd_bam_reads_t *meta) {
    if (meta) memset(meta, 0, sizeof(*meta));
    if (!opt || !bam_path || !bai_path || !chrom) { set_err(-4, "lcd_chunk_create_from_bam: NULL argument"); return nullptr; }
    return chunk_open_files(opt, 1, &bam_path, &bai_path, chrom, reg_beg, reg_end, min_mapq, verify_crc, meta);
}
lcd_chunk_t *lcd_chunk_open_from_bams(const lcd_digar_opt_t *opt, int n_bams, const char *const *bam_paths, const char *const *bai_paths, const char *chrom, int64_t reg_beg,
                                      int64_t reg_end, int min_mapq, int verify_crc, lcd_bam_reads_t *meta) {
    if (meta) memset(meta, 0, sizeof(*meta));
    if (!opt || !bam_paths || !chrom || n_bams < 1 || n_bams > LCD_MAX_INPUTS) { set_err(-4, "lcd_chunk_open_from_bams: NULL argument, or n_bams outside 1 ... LCD_MAX_INPUTS"); return nullptr; }
    std::vector<std::string> bai(n_bams); std::vector<const char *> bp(n_bams);
    for (int f = 0; f < n_bams; ++f) {
        if (!bam_paths[f]) { set_err(-4, "lcd_chunk_open_from_bams: NULL path"); return nullptr; }
        bai[f] = bai_paths && bai_paths[f] ? std::string(bai_paths[f]) : std::string(bam_paths[f]) + ".bai"; bp[f] = bai[f].c_str();
    }
    return chunk_open_files(opt, n_bams, bam_paths, bp.data(), chrom, reg_beg, reg_end, min_mapq, verify_crc, meta);
}
int lcd_chunk_n_files(const lcd_chunk_t *c) { return c ? c->n_files : 0; }
// per kept read the index of the file it came from (a chunk made from host arrays, or from one BAM: 0)
int lcd_chunk_read_files(const lcd_chunk_t *c, int *file_of_read) {
    if (!c) return set_err(-4, "lcd_chunk_read_files: NULL chunk");
    if (c->n_reads > 0 && !file_of_read) return set_err(-4, "lcd_chunk_read_files: NULL output");
    for (int r = 0; r < c->n_reads; ++r) file_of_read[r] = r < (int)c->read_file.size() ? c->read_file[r] : 0;
    return c->n_reads;
}
int lcd_chunk_resolve(lcd_chunk_t *c, const lcd_chunk_src_t *src) {
    if (!c || !c->pending) return set_err(-4, "lcd_chunk_resolve: the handle was not opened by lcd_chunk_open_from_bam, or is resolved already");
    if (use_device(c->device)) return -1;
    ChunkPending &P = *c->pending;
    const int n = c->n_reads;
    if (n == 0) { c->pending.reset(); return 0; }
    const int64_t reg_beg = P.reg_beg, reg_end = P.reg_end;
    const lcd_digar_opt_t *opt = &c->opt;
    const uint64_t base = lcd_inflated_dev_ptr(c->stream);
    std::vector<int64_t> &pos0 = P.pos0, &rl_true = P.rl_true; std::vector<int> &ncig = P.ncig, &qlen = P.qlen, &nindel = P.nindel; std::vector<uint64_t> &coff = P.coff, &soff = P.soff, &qoff = P.qoff;
    std::vector<RefCmpOut> &counts = P.counts; std::vector<BamAuxJob> &auxj = P.auxj; DevBuf &d_cig = P.d_cig;
    StreamGuard st; if (st.create()) return -10;
    auto fail = [&](int code, const std::string &m) -> int { return set_err(code, "lcd_chunk_create_from_bam: " + m); };
    // 3b. the reads' sources: what the words of the digar launch are made from
    std::vector<uint8_t> pal; std::vector<int> pre, clip, nw; std::vector<uint64_t> waddr;
    DevBuf d_aj, d_ao, d_ref, d_rj, d_rc, d_rw, d_tg, d_tpool, d_tw;
    double t0 = now_ms();
    if (src) {
        c->source.assign(n, 0); c->pal.assign(n, 0); pal.assign(n, 0); pre.assign(n, 0); clip.assign(n, 0); nw = ncig; waddr.resize(n);
        std::vector<BamAuxOut> ao(n);
        if (d_aj.ensure((size_t)n * sizeof(BamAuxJob)) || d_ao.ensure((size_t)n * sizeof(BamAuxOut))) return -11;
#define CHKM(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return fail(-10, "HIP call failed: " #x); } } while (0)
        CHKM(hipMemcpyAsync(d_aj.p, auxj.data(), (size_t)n * sizeof(BamAuxJob), hipMemcpyHostToDevice, st));
        lcd_launch_bam_aux((const BamAuxJob *)d_aj.p, (BamAuxOut *)d_ao.p, src->is_ont != 0, n, st);
        CHKM(hipGetLastError());
        CHKM(hipMemcpyAsync(ao.data(), d_ao.p, (size_t)n * sizeof(BamAuxOut), hipMemcpyDeviceToHost, st));
        CHKM(hipStreamSynchronize(st));
        c->stage_ms[0] = now_ms() - t0; t0 = now_ms();
        const bool have_ref = src->ref_seq && src->ref_end >= src->ref_beg;
        std::vector<int> ref_reads, tag_reads;
        for (int r = 0; r < n; ++r) {
            c->source[r] = ao[r].source; c->pal[r] = ao[r].pal != 0; pal[r] = ao[r].pal; waddr[r] = d_cig.addr() + coff[r] * 4;
            // a read compared with the reference needs the window, and a CIGAR that consumes exactly the record's bases (the comparison reads them in place)
            if (ao[r].source == LCD_SRC_REF) { if (!have_ref || ao[r].cig_qlen != (long long)qlen[r]) pre[r] = 1; else ref_reads.push_back(r); }
            else if (ao[r].source != LCD_SRC_EQX) { if (ao[r].bad_type) pre[r] = 1; else tag_reads.push_back(r); }
        }
        if (!ref_reads.empty()) {
            const int m = (int)ref_reads.size(); const uint64_t ref_len = (uint64_t)(src->ref_end - src->ref_beg + 1);
            if (d_ref.ensure(ref_len + 64) || d_rj.ensure((size_t)m * sizeof(RefCmpJob)) || d_rc.ensure((size_t)m * sizeof(RefCmpOut))) return -11;
            std::vector<RefCmpJob> rj(m); std::vector<RefCmpOut> cnt(m);
            for (int k = 0; k < m; ++k) { const int r = ref_reads[k]; RefCmpJob &j = rj[k]; j.cigar_off = waddr[r]; j.seq_off = base + soff[r]; j.out_off = 0; j.n_cigar = ncig[r]; j.pad = 0; j.pos0 = pos0[r]; }
            CHKM(hipMemcpyAsync(d_ref.p, src->ref_seq, ref_len, hipMemcpyHostToDevice, st));
            CHKM(hipMemcpyAsync(d_rj.p, rj.data(), (size_t)m * sizeof(RefCmpJob), hipMemcpyHostToDevice, st));
            lcd_launch_refcmp(false, (const RefCmpJob *)d_rj.p, (RefCmpOut *)d_rc.p, (const char *)d_ref.p, src->ref_beg, src->ref_end, m, st);
            CHKM(hipGetLastError());
            CHKM(hipMemcpyAsync(cnt.data(), d_rc.p, (size_t)m * sizeof(RefCmpOut), hipMemcpyDeviceToHost, st));
            CHKM(hipStreamSynchronize(st));
            uint64_t tot = 0;
            for (int k = 0; k < m; ++k) tot += (uint64_t)cnt[k].n_ops;
            if (d_rw.ensure(tot * 4 + 64)) return -11;
            tot = 0;
            for (int k = 0; k < m; ++k) { const int r = ref_reads[k]; rj[k].out_off = d_rw.addr() + tot * 4; waddr[r] = rj[k].out_off; nw[r] = cnt[k].n_ops; counts[r] = cnt[k]; tot += (uint64_t)cnt[k].n_ops; }
            CHKM(hipMemcpyAsync(d_rj.p, rj.data(), (size_t)m * sizeof(RefCmpJob), hipMemcpyHostToDevice, st));
            lcd_launch_refcmp(true, (const RefCmpJob *)d_rj.p, (RefCmpOut *)d_rc.p, (const char *)d_ref.p, src->ref_beg, src->ref_end, m, st);
            CHKM(hipGetLastError());
            CHKM(hipStreamSynchronize(st));
        }
        c->stage_ms[1] = now_ms() - t0; t0 = now_ms();
        std::vector<uint32_t> words;
        if (!tag_reads.empty()) {
            // one pool: per read its CIGAR words (4-byte aligned), then the tag value with its NUL
            const int m = (int)tag_reads.size();
            std::vector<GatherJob> tj(2 * (size_t)m); std::vector<uint64_t> at_cig(m), at_tag(m);
            uint64_t tb = 0;
            for (int k = 0; k < m; ++k) {
                const int r = tag_reads[k];
                at_cig[k] = tb; tj[2 * k] = GatherJob{waddr[r], tb, (uint32_t)ncig[r] * 4u, 0}; tb += (uint64_t)ncig[r] * 4;
                at_tag[k] = tb; tj[2 * k + 1] = GatherJob{ao[r].tag, tb, ao[r].tag_len + 1u, 0}; tb = lcd_align_up(tb + ao[r].tag_len + 1, 4);
                c->tag_bytes += ao[r].tag_len;
            }
            if (d_tpool.ensure(tb + 64) || d_tg.ensure(tj.size() * sizeof(GatherJob))) return -11;
            for (GatherJob &g : tj) g.dst += d_tpool.addr();
            std::vector<uint8_t> hp(tb + 4);
            CHKM(hipMemcpyAsync(d_tg.p, tj.data(), tj.size() * sizeof(GatherJob), hipMemcpyHostToDevice, st));
            lcd_launch_gather((const GatherJob *)d_tg.p, (int)tj.size(), st);
            CHKM(hipGetLastError());
            CHKM(hipMemcpyAsync(hp.data(), d_tpool.p, tb, hipMemcpyDeviceToHost, st));
            CHKM(hipStreamSynchronize(st));
            std::vector<uint64_t> woff(m);
            for (int k = 0; k < m; ++k) {
                const int r = tag_reads[k];
                const uint32_t *cig = (const uint32_t *)(hp.data() + at_cig[k]); char *tag = (char *)(hp.data() + at_tag[k]);
                tag[ao[r].tag_len] = 0;
                woff[k] = words.size();
                const bool ok = ao[r].source == LCD_SRC_CS ? cs_to_words(cig, ncig[r], tag, words) : md_to_words(cig, ncig[r], tag, words);
                if (!ok) { pre[r] = 1; words.resize(woff[k]); }     // the reference stops the program here: status -2, no digars
                long long nd = 0, nev = 0, nid = 0;                 // (lcd_digar_batch's capacity pass)
                for (size_t i = woff[k]; i < words.size(); ++i) { const uint32_t w = words[i]; const int op = w & 0xf, len = (int)(w >> 4); if (op == 8) { nd += len; nev += len; } else if (op != 3 && op != 9) { ++nd; if (op == 1 || op == 2) { ++nev; ++nid; } } }
                nw[r] = (int)(words.size() - woff[k]); counts[r].n_ops = nw[r]; counts[r].nd = (int)nd; counts[r].nev = (int)nev; nindel[r] = (int)nid;
                clip[r] = ao[r].source == LCD_SRC_CS;
            }
            words.push_back(0);
            if (d_tw.ensure(words.size() * 4 + 64)) return -11;
            CHKM(hipMemcpyAsync(d_tw.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
            for (int k = 0; k < m; ++k) waddr[tag_reads[k]] = d_tw.addr() + woff[k] * 4;
        }
        for (int r = 0; r < n; ++r) if (pre[r] && c->source[r] != LCD_SRC_EQX) { nw[r] = 0; counts[r].n_ops = counts[r].nd = counts[r].nev = 0; nindel[r] = 0; }
        CHKM(hipStreamSynchronize(st));   // (`words` leaves scope below)
#undef CHKM
        c->stage_ms[2] = now_ms() - t0; t0 = now_ms();
    }
    // 4. digars, kept in HBM; bases and qualities are read in place
    c->qlen = qlen; c->seq_off = soff; c->qual_off = qoff; c->seq_base = base; c->qual_base = base;
    c->status.resize(n); c->n_cand.resize(n); c->beg.resize(n); c->end.resize(n);
    DigarWords W; W.off = coff.data(); W.n_cigar = ncig.data(); W.d_words = &d_cig; W.counts = counts.data(); W.n_indel = nindel.data(); W.d_qual_base = base;
    if (src) { W.n_cigar = nw.data(); W.addr = waddr.data(); W.clip_rule_r = clip.data(); W.rlen_true = rl_true.data(); W.pre_status = pre.data(); }
    DigarKeep keep; keep.d_dig = &c->d_dig;
    uint64_t *doff = nullptr; lcd_digar_t *dg = nullptr;
    const int rc = digar_batch_core(opt, n, pos0.data(), W, nullptr, qoff.data(), qlen.data(), src ? pal.data() : nullptr, reg_beg, reg_end, P.tlen, &doff, &dg, &c->iv_off, &c->ivs, &c->iv_in_chunk,
                                    c->status.data(), c->beg.data(), c->end.data(), c->n_cand.data(), st, &keep);
    free(doff);
    if (rc) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return fail(-10, "HIP call failed: hipStreamSynchronize"); }
    c->slot.swap(keep.slot); c->n_digar.swap(keep.n_digar);
    if (src) c->stage_ms[3] = now_ms() - t0;
    c->pending.reset();
    return 0;
}
lcd_chunk_t *lcd_chunk_create_from_bam_src(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end,
                                           int min_mapq, int verify_crc, const lcd_chunk_src_t *src, lcd_bam_reads_t *meta) {
    lcd_chunk_t *c = lcd_chunk_open_from_bam(opt, bam_path, bai_path, chrom, reg_beg, reg_end, min_mapq, verify_crc, meta);
    if (!c) return nullptr;
    if (lcd_chunk_resolve(c, src)) {
        const std::string m = g_err;
        lcd_chunk_destroy(c);
        if (meta) { lcd_bam_reads_free(meta); memset(meta, 0, sizeof(*meta)); }   // (the caller's arrays were handed out by the first phase)
        g_err = m;
        return nullptr;
    }
    return c;
}
lcd_chunk_t *lcd_chunk_create_from_bam(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end,
                                       int min_mapq, int verify_crc, lcd_bam_reads_t *meta) {
    return lcd_chunk_create_from_bam_src(opt, bam_path, bai_path, chrom, reg_beg, reg_end, min_mapq, verify_crc, nullptr, meta);
}
// per read the source the reference would choose (LCD_SRC_*; a chunk made without `src`: LCD_SRC_EQX), chunk->is_ont_palindrome, and the cs / MD bytes that came
// to the host when the chunk was made
int lcd_chunk_read_sources(const lcd_chunk_t *c, uint8_t *source, uint8_t *is_ont_palindrome, uint64_t *tag_bytes_d2h) {
    for (int r = 0; r < c->n_reads; ++r) { if (source) source[r] = c->source.empty() ? LCD_SRC_EQX : c->source[r]; if (is_ont_palindrome) is_ont_palindrome[r] = c->pal.empty() ? 0 : c->pal[r]; }
    if (tag_bytes_d2h) *tag_bytes_d2h = c->tag_bytes;
    return c->n_reads;
}
// bam_get_NM (src/bam_utils.c:1632-1639) per kept read of a chunk made from a BAM, on the records where the inflate left them (lcd_bam_nm_kernel): 16 bytes per read go
// up, 4 come back.  A chunk made from host arrays has no records: -4.
int lcd_chunk_read_nm(const lcd_chunk_t *c, int *nm_out) {
    if (!c || !c->from_bam) return set_err(-4, "lcd_chunk_read_nm: the chunk was not made from a BAM");
    const int n = c->n_reads;
    if (n <= 0) return 0;
    if (!nm_out) return set_err(-4, "lcd_chunk_read_nm: NULL output");
    if (!c->stream || (int)c->aux_off.size() != n || (int)c->rec_end.size() != n) return set_err(-4, "lcd_chunk_read_nm: the chunk has no record stream");
    if (use_device(c->device)) return -1;
    const uint64_t base = lcd_inflated_dev_ptr(c->stream), usize = lcd_inflated_size(c->stream);
    std::vector<BamNmJob> jobs(n);
    for (int r = 0; r < n; ++r) {
        if (c->aux_off[r] > c->rec_end[r] || c->rec_end[r] > usize) return set_err(-4, "lcd_chunk_read_nm: record outside the stream");
        jobs[r].aux = base + c->aux_off[r]; jobs[r].end = base + c->rec_end[r];
    }
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_jobs, d_nm;
    if (d_jobs.ensure((size_t)n * sizeof(BamNmJob)) || d_nm.ensure((size_t)n * 4)) return -11;
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(BamNmJob), hipMemcpyHostToDevice, st));
    lcd_launch_bam_nm((const BamNmJob *)d_jobs.p, (int *)d_nm.p, n, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(nm_out, d_nm.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return n;
}
// sort_chunk_reads (src/bam_utils.c:1616-1656), host code: comp_bam_read_sort's keys -- pos ascending, end DESCENDING, NM ascending, strcmp of the names -- and, where
// all four are equal (qsort leaves that order open), file order
int lcd_sort_chunk_reads(int n, const int64_t *pos0, const int64_t *end_pos, const int *nm, const uint64_t *name_off, const char *name_pool, int *order_out) {
    if (n < 0) return set_err(-4, "lcd_sort_chunk_reads: n < 0");
    if (n == 0) return 0;
    if (!pos0 || !end_pos || !nm || !name_off || !name_pool || !order_out) return set_err(-4, "lcd_sort_chunk_reads: NULL argument");
    std::vector<int> o(n);
    for (int i = 0; i < n; ++i) o[i] = i;
    std::stable_sort(o.begin(), o.end(), [&](const int a, const int b) {
        if (pos0[a] != pos0[b]) return pos0[a] < pos0[b];
        if (end_pos[a] != end_pos[b]) return end_pos[a] > end_pos[b];
        if (nm[a] != nm[b]) return nm[a] < nm[b];
        return strcmp(name_pool + name_off[a], name_pool + name_off[b]) < 0;
    });
    memcpy(order_out, o.data(), (size_t)n * sizeof(int));
    return n;
}
void lcd_chunk_stage_ms(const lcd_chunk_t *c, double out[4]) { for (int k = 0; k < 4; ++k) out[k] = c->stage_ms[k]; }
// the chunk's digars as lcd_digar_batch returns them (tests and debugging: everything else reads them in HBM)
int lcd_chunk_digars(const lcd_chunk_t *c, uint64_t **digar_off, lcd_digar_t **digars) {
    *digar_off = nullptr; *digars = nullptr;
    if (c->pending) return set_err(-4, "lcd_chunk_digars: the chunk was opened and not resolved (lcd_chunk_resolve)");
    if (use_device(c->device)) return -1;
    const int n = c->n_reads;
    uint64_t span = 0, tot = 0;
    for (int r = 0; r < n; ++r) { span = std::max<uint64_t>(span, c->slot[r] + (uint64_t)c->n_digar[r]); tot += (uint64_t)c->n_digar[r]; }
    if (span * sizeof(DigarRec) > c->d_dig.cap) return set_err(-4, "lcd_chunk_digars: digar slots outside the chunk's buffer");
    std::vector<DigarRec> h(span + 1);
    if (span) { HIPCHK(hipMemcpy(h.data(), c->d_dig.p, span * sizeof(DigarRec), hipMemcpyDeviceToHost)); g_copy_bytes[0] += span * sizeof(DigarRec); }
    uint64_t *off = (uint64_t *)malloc(((size_t)n + 1) * sizeof(uint64_t)); lcd_digar_t *dg = (lcd_digar_t *)malloc((tot + 1) * sizeof(lcd_digar_t));
    if (!off || !dg) { free(off); free(dg); return set_err(-11, "lcd_chunk_digars: out of memory"); }
    uint64_t w = 0;
    for (int r = 0; r < n; ++r) { off[r] = w; if (c->n_digar[r]) memcpy(dg + w, h.data() + c->slot[r], (size_t)c->n_digar[r] * sizeof(DigarRec)); w += (uint64_t)c->n_digar[r]; }
    off[n] = w;
    *digar_off = off; *digars = dg;
    return n;
}
void lcd_chunk_destroy(lcd_chunk_t *c) { delete c; }
int lcd_chunk_n_reads(const lcd_chunk_t *c) { return c ? c->n_reads : 0; }
int lcd_chunk_set_refine(lcd_chunk_t *c, int on) {
    if (!c) return set_err(-4, "lcd_chunk_set_refine: NULL chunk");
    lcd_refine_log_free(c->refine_log); c->refine_log = nullptr;
    if (on && !(c->refine_log = lcd_refine_log_create())) return set_err(-11, "lcd_chunk_set_refine: out of memory");
    return 0;
}
lcd_refine_log_t *lcd_chunk_refine_log(const lcd_chunk_t *c) { return c ? c->refine_log : nullptr; }
// what collect_digar_from_eqx_cigar leaves on the host side of the reference: per read 0 / -1 (skipped as too noisy) / -2 ('M' operation), digar->beg / end, the number
// of candidate variants; the reads' noisy windows in cr_index order (CSR; pointers into the chunk, valid until it is destroyed) and which of them enter chunk_noisy_regs
int lcd_chunk_read_info(const lcd_chunk_t *c, int *status, int64_t *beg, int64_t *end, int *n_cand_vars, int *n_digars) {
    if (c->pending) return set_err(-4, "lcd_chunk_read_info: the chunk was opened and not resolved (lcd_chunk_resolve)");
    for (int r = 0; r < c->n_reads; ++r) { if (status) status[r] = c->status[r]; if (beg) beg[r] = c->beg[r]; if (end) end[r] = c->end[r]; if (n_cand_vars) n_cand_vars[r] = c->n_cand[r]; if (n_digars) n_digars[r] = c->n_digar[r]; }
    return c->n_reads;
}
int lcd_chunk_intervals(const lcd_chunk_t *c, const uint64_t **iv_off, const lcd_noisy_iv_t **ivs, const uint8_t **iv_in_chunk) {
    *iv_off = nullptr; *ivs = nullptr; *iv_in_chunk = nullptr;
    if (c->pending) return set_err(-4, "lcd_chunk_intervals: the chunk was opened and not resolved (lcd_chunk_resolve)");
    *iv_off = c->iv_off; *ivs = c->ivs; *iv_in_chunk = c->iv_in_chunk;
    return c->n_reads;
}
// collect_noisy_read_info's digar walk (src/align.c:1392-1456) for many (region, read) pairs, on the digars in HBM: out per pair the read's query interval over the
// region and the cover flag -- 12 bytes per pair come back
int lcd_chunk_region_slices(const lcd_chunk_t *c, int n_pairs, const int *pair_read, const int64_t *pair_reg_beg, const int64_t *pair_reg_end, int noisy_reg_flank_len,
                            int *read_beg, int *read_end, int *cover) {
    if (n_pairs <= 0) return 0;
    if (c->pending) return set_err(-4, "lcd_chunk_region_slices: the chunk was opened and not resolved (lcd_chunk_resolve)");
    if (use_device(c->device)) return -1;
    std::vector<SliceJob> jobs(n_pairs);
    for (int i = 0; i < n_pairs; ++i) {
        const int r = pair_read[i];
        if (r < 0 || r >= c->n_reads) return set_err(-4, "lcd_chunk_region_slices: read index out of range");
        SliceJob &j = jobs[i]; j.digar_off = c->slot[r]; j.n_digar = c->n_digar[r]; j.qlen = c->qlen[r]; j.reg_beg = pair_reg_beg[i]; j.reg_end = pair_reg_end[i];
    }
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_jobs, d_outs;
    if (d_jobs.ensure(n_pairs * sizeof(SliceJob)) || d_outs.ensure(n_pairs * sizeof(SliceOut))) return -11;
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n_pairs * sizeof(SliceJob), hipMemcpyHostToDevice, st));
    lcd_launch_slices((const SliceJob *)d_jobs.p, (SliceOut *)d_outs.p, (const DigarRec *)c->d_dig.p, noisy_reg_flank_len, n_pairs, st);
    HIPCHK(hipGetLastError());
    std::vector<SliceOut> outs(n_pairs);
    HIPCHK(hipMemcpyAsync(outs.data(), d_outs.p, n_pairs * sizeof(SliceOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n_pairs; ++i) { read_beg[i] = outs[i].read_beg; read_end[i] = outs[i].read_end; cover[i] = outs[i].cover; }
    return 0;
}

int lcd_digar_batch_tags(const lcd_digar_opt_t *opt, int mode, int n, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off, const int *n_cigar,
                         const char *const *tags, const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags, int64_t reg_beg,
                         int64_t reg_end, int64_t whole_ref_len, uint64_t **digar_off_out, lcd_digar_t **digars_out, uint64_t **iv_off_out,
                         lcd_noisy_iv_t **ivs_out, uint8_t **iv_in_chunk_out, int *status, int64_t *beg, int64_t *end, int *n_cand_vars) {
    *digar_off_out = *iv_off_out = nullptr; *digars_out = nullptr; *ivs_out = nullptr; *iv_in_chunk_out = nullptr;
    if (mode != LCD_DIGAR_CS && mode != LCD_DIGAR_MD) return set_err(-2, "lcd_digar_batch_tags: mode is LCD_DIGAR_CS or LCD_DIGAR_MD");
    if (ensure_init()) return -1;
    if (n <= 0) return 0;
    StreamGuard st; if (st.create()) return -10;
    std::vector<uint32_t> words; std::vector<uint64_t> off(n); std::vector<int> cnt(n), pre(n, 0); std::vector<int64_t> rlen(n);
    for (int r = 0; r < n; ++r) {
        const uint32_t *cig = cigar_pool + cigar_off[r];
        off[r] = words.size();
        const bool ok = mode == LCD_DIGAR_CS ? cs_to_words(cig, n_cigar[r], tags[r], words) : md_to_words(cig, n_cigar[r], tags[r], words);
        if (!ok) { pre[r] = 1; words.resize(off[r]); }           // the reference stops the program here; the read comes back with status -2 and no digars
        cnt[r] = (int)(words.size() - off[r]);
        long long rl = 0;
        for (int i = 0; i < n_cigar[r]; ++i) { const int op = cig[i] & 0xf; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cig[i] >> 4; }
        rlen[r] = rl;
    }
    words.push_back(0);
    DigarWords W; W.h_pool = words.data(); W.off = off.data(); W.n_cigar = cnt.data(); W.clip_rule = mode == LCD_DIGAR_CS ? 1 : 0; W.rlen_true = rlen.data(); W.pre_status = pre.data();
    return digar_batch_core(opt, n, pos0, W, qual_pool, qual_off, qlen, pal_flags, reg_beg, reg_end, whole_ref_len, digar_off_out, digars_out, iv_off_out, ivs_out,
                            iv_in_chunk_out, status, beg, end, n_cand_vars, st);
}

int lcd_digar_batch_ref(const lcd_digar_opt_t *opt, int n, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off, const int *n_cigar,
                        const uint8_t *seq_pool, const uint64_t *seq_off, const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags,
                        const char *ref_seq, int64_t ref_beg, int64_t ref_end, int64_t reg_beg, int64_t reg_end, int64_t whole_ref_len, uint64_t **digar_off_out,
                        lcd_digar_t **digars_out, uint64_t **iv_off_out, lcd_noisy_iv_t **ivs_out, uint8_t **iv_in_chunk_out, int *status, int64_t *beg,
                        int64_t *end, int *n_cand_vars) {
    *digar_off_out = *iv_off_out = nullptr; *digars_out = nullptr; *ivs_out = nullptr; *iv_in_chunk_out = nullptr;
    if (ensure_init()) return -1;
    if (n <= 0) return 0;
    if (ref_end < ref_beg) return set_err(-2, "lcd_digar_batch_ref: empty reference window");
    StreamGuard st; if (st.create()) return -10;
    uint64_t cig_words = 0, seq_bytes = 0;
    for (int r = 0; r < n; ++r) { cig_words = std::max<uint64_t>(cig_words, cigar_off[r] + n_cigar[r]); seq_bytes = std::max<uint64_t>(seq_bytes, seq_off[r] + (uint64_t)(qlen[r] + 1) / 2); }
    const uint64_t ref_len = (uint64_t)(ref_end - ref_beg + 1);
    DevBuf d_cig, d_seq, d_ref, d_jobs, d_cnt, d_words;
    if (d_cig.ensure(cig_words * 4 + 64) || d_seq.ensure(seq_bytes + 64) || d_ref.ensure(ref_len + 64) || d_jobs.ensure(n * sizeof(RefCmpJob)) || d_cnt.ensure(n * sizeof(RefCmpOut))) return -11;
    std::vector<RefCmpJob> jobs(n);
    for (int r = 0; r < n; ++r) { RefCmpJob &j = jobs[r]; j.cigar_off = d_cig.addr() + cigar_off[r] * 4; j.seq_off = d_seq.addr() + seq_off[r]; j.out_off = 0; j.n_cigar = n_cigar[r]; j.pad = 0; j.pos0 = pos0[r]; }
    HIPCHK(hipMemcpyAsync(d_cig.p, cigar_pool, cig_words * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_seq.p, seq_pool, seq_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ref.p, ref_seq, ref_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(RefCmpJob), hipMemcpyHostToDevice, st));
    lcd_launch_refcmp(false, (const RefCmpJob *)d_jobs.p, (RefCmpOut *)d_cnt.p, (const char *)d_ref.p, ref_beg, ref_end, n, st);
    HIPCHK(hipGetLastError());
    std::vector<RefCmpOut> cnt(n);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, n * sizeof(RefCmpOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<uint64_t> off(n); std::vector<int> nw(n); uint64_t tot = 0;
    for (int r = 0; r < n; ++r) { off[r] = tot; nw[r] = cnt[r].n_ops; tot += (uint64_t)cnt[r].n_ops; }
    if (d_words.ensure(tot * 4 + 64)) return -11;
    for (int r = 0; r < n; ++r) jobs[r].out_off = d_words.addr() + off[r] * 4;
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(RefCmpJob), hipMemcpyHostToDevice, st));
    lcd_launch_refcmp(true, (const RefCmpJob *)d_jobs.p, (RefCmpOut *)d_cnt.p, (const char *)d_ref.p, ref_beg, ref_end, n, st);
    HIPCHK(hipGetLastError());
    DigarWords W; W.off = off.data(); W.n_cigar = nw.data(); W.d_words = &d_words; W.counts = cnt.data();
    return digar_batch_core(opt, n, pos0, W, qual_pool, qual_off, qlen, pal_flags, reg_beg, reg_end, whole_ref_len, digar_off_out, digars_out, iv_off_out, ivs_out,
                            iv_in_chunk_out, status, beg, end, n_cand_vars, st);
}

} // extern "C"
