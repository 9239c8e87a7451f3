// lcd_bam_out.cpp -- the device side of the phased alignment output (longcallD call -b): BGZF members compressed in HBM (deflate_kernel.hip) and the HP:i / PS:i
// rewrite of a chunk's records where the inflate left them (bam_tag_kernel.hip).  The writer that joins them into a file is lcd_write_phased (lcd_call.cpp).
// The same records as SAM text lines (bam_sam_kernel.hip): lcd_tagged_to_sam / lcd_records_to_sam, behind the writer's LCD_ALN_SAM format.
#include "lcd_host_internal.h"

using namespace lcd_internal;

struct lcd_deflated_s {
    DevBuf image; size_t size = 0, n_blocks = 0; double ms_kernel = 0; int device = 0; bool eof = false;
    std::vector<DeflateOut> outs; std::vector<uint32_t> payloads;
};
// offs: where record k starts in `out` (n_records + 1 entries, what the emit pass was given); d_offs: the same in HBM, uploaded by the first lcd_tagged_to_sam
struct lcd_tagged_s { DevBuf out; size_t size = 0; int n_records = 0, device = 0; std::vector<unsigned long long> offs; mutable DevBuf d_offs; mutable bool offs_up = false; };
struct lcd_sam_text_s { DevBuf text; size_t size = 0; int device = 0; };

namespace {
const uint8_t EOF_MEMBER[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
unsigned gf2_mulmod_h(unsigned a, unsigned b) { unsigned m = 1u << 31, p = 0; for (;;) { if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; } m >>= 1; b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1; } return p; }

// d_data: n bytes in HBM (readable as they are: the kernel never reads behind them)
lcd_deflated_t *deflate_dev(const uint8_t *d_data, size_t n, int block_payload, int add_eof, hipStream_t st) {
    const std::string W = "lcd_bgzf_deflate_dev";
    if (block_payload == 0) block_payload = 0xff00;
    if (block_payload < 1 || block_payload > 0xff00) { set_err(-4, W + ": block_payload must be 0 or 1 ... 0xff00"); return nullptr; }
    const size_t nb = (n + (size_t)block_payload - 1) / (size_t)block_payload;
    if (nb > (size_t)1 << 30) { set_err(-4, W + ": too many blocks"); return nullptr; }
    std::unique_ptr<lcd_deflated_s> h(new lcd_deflated_s());
    h->device = cur_device(); h->n_blocks = nb; h->eof = add_eof != 0;
    auto hipfail = [&](const char *what) -> lcd_deflated_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define DCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    std::vector<unsigned long long> offs(nb + 1, 0);
    if (nb) {
        const unsigned stride = (unsigned)lcd_align_up((uint64_t)block_payload + 5 + 16, 16);
        const int grid = (int)std::min<size_t>(nb, 2048);
        DevBuf d_slots, d_toks, d_outs, d_offs;
        if (d_slots.ensure(nb * (size_t)stride + 64, 31) || d_toks.ensure((size_t)grid * (size_t)block_payload * 4 + 64, 31) || d_outs.ensure(nb * sizeof(DeflateOut), 31) ||
            d_offs.ensure(nb * 8, 31)) return nullptr;
        { unsigned t[32]; unsigned p = 1u << 30; t[0] = p; for (int k = 1; k < 32; ++k) t[k] = p = gf2_mulmod_h(p, p); lcd_deflate_set_x2n(t, st); }
        hipEvent_t ev[2] = {nullptr, nullptr};
        DCHK(hipEventCreate(&ev[0]));
        if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipEventDestroy(ev[0]); return hipfail("hipEventCreate"); }
        auto drop = [&]() { (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); };
#define ECHK(x) do { if ((x) != hipSuccess) { drop(); return hipfail(#x); } } while (0)
        ECHK(hipEventRecord(ev[0], st));
        lcd_launch_deflate(d_data, (unsigned long long)n, block_payload, (int)nb, (uint8_t *)d_slots.p, stride, (unsigned *)d_toks.p, (DeflateOut *)d_outs.p, grid, st);
        ECHK(hipGetLastError());
        h->outs.resize(nb);
        ECHK(hipMemcpyAsync(h->outs.data(), d_outs.p, nb * sizeof(DeflateOut), hipMemcpyDeviceToHost, st));
        ECHK(hipStreamSynchronize(st));
        h->payloads.resize(nb);
        for (size_t i = 0; i < nb; ++i) {
            h->payloads[i] = (uint32_t)std::min<size_t>((size_t)block_payload, n - i * (size_t)block_payload);
            if (h->outs[i].clen > h->payloads[i] + 5u) { drop(); set_err(-24, W + ": a member exceeds its stored size"); return nullptr; }
            offs[i + 1] = offs[i] + 18ull + h->outs[i].clen + 8ull;
        }
        h->size = (size_t)offs[nb] + (add_eof ? 28 : 0);
        if (h->image.ensure(h->size + 64, 31)) { drop(); return nullptr; }
        ECHK(hipMemcpyAsync(d_offs.p, offs.data(), nb * 8, hipMemcpyHostToDevice, st));
        lcd_launch_deflate_pack((const uint8_t *)d_slots.p, stride, (const DeflateOut *)d_outs.p, (const unsigned long long *)d_offs.p, (uint8_t *)h->image.p, (unsigned long long)n,
                                block_payload, (int)nb, st);
        ECHK(hipGetLastError());
        ECHK(hipEventRecord(ev[1], st));
        if (add_eof) ECHK(hipMemcpyAsync((uint8_t *)h->image.p + offs[nb], EOF_MEMBER, 28, hipMemcpyHostToDevice, st));
        ECHK(hipStreamSynchronize(st));
        float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[1]);     // both kernels and the size round trip between them
        h->ms_kernel = ms;
        drop();
#undef ECHK
    } else {
        h->size = add_eof ? 28 : 0;
        if (h->size) { if (h->image.ensure(h->size + 64, 31)) return nullptr; DCHK(hipMemcpyAsync(h->image.p, EOF_MEMBER, 28, hipMemcpyHostToDevice, st)); DCHK(hipStreamSynchronize(st)); }
    }
#undef DCHK
    return h.release();
}
} // namespace

extern "C" {

lcd_deflated_t *lcd_bgzf_deflate_dev_ptr(uint64_t dev_ptr, size_t n, int block_payload, int add_eof) {
    if (ensure_init()) return nullptr;
    if (n && !dev_ptr) { set_err(-4, "lcd_bgzf_deflate_dev_ptr: NULL device pointer"); return nullptr; }
    StreamGuard st; if (st.create()) return nullptr;
    return deflate_dev((const uint8_t *)(uintptr_t)dev_ptr, n, block_payload, add_eof, st);
}
lcd_deflated_t *lcd_bgzf_deflate_dev(const uint8_t *data, size_t n, int block_payload, int add_eof) {
    if (ensure_init()) return nullptr;
    if (n && !data) { set_err(-4, "lcd_bgzf_deflate_dev: NULL data"); return nullptr; }
    StreamGuard st; if (st.create()) return nullptr;
    DevBuf d_in;
    if (n) {
        if (d_in.ensure(n + 64, 31)) return nullptr;
        if (hipMemcpyAsync(d_in.p, data, n, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); set_err(-10, "lcd_bgzf_deflate_dev: upload failed"); return nullptr; }
    }
    return deflate_dev((const uint8_t *)d_in.p, n, block_payload, add_eof, st);   // (synchronised before d_in leaves scope)
}
size_t lcd_deflated_size(const lcd_deflated_t *h) { return h ? h->size : 0; }
size_t lcd_deflated_n_blocks(const lcd_deflated_t *h) { return h ? h->n_blocks : 0; }
double lcd_deflated_kernel_ms(const lcd_deflated_t *h) { return h ? h->ms_kernel : 0; }
int lcd_deflated_block_info(const lcd_deflated_t *h, size_t i, uint32_t *payload, uint32_t *bsize, int *kind) {
    if (!h || i >= h->n_blocks) return set_err(-4, "lcd_deflated_block_info: no such block");
    if (payload) *payload = h->payloads[i];
    if (bsize) *bsize = 18u + h->outs[i].clen + 8u;
    if (kind) *kind = (int)h->outs[i].kind;
    return 0;
}
int lcd_deflated_to_host(const lcd_deflated_t *h, size_t off, size_t n, uint8_t *out) {
    if (!h || off + n > h->size) return set_err(-41, "lcd_deflated_to_host: range past the end of the image");
    if (n == 0) return 0;
    if (use_device(h->device)) return -1;
    HIPCHK(hipMemcpy(out, (const uint8_t *)h->image.p + off, n, hipMemcpyDeviceToHost));
    return 0;
}
void lcd_deflated_free(lcd_deflated_t *h) { delete h; }

// ---- which records of a chunk's table are written, and in which order (rules 4 and 5 of the merged alignment output; pure host code) ----
int lcd_merged_record_plan(int n_rec, const int *rec_file, const int64_t *rec_pos0, const int64_t *rec_endpos, int has_prev, int64_t prev_beg, int64_t prev_end,
                           int sort_output, uint8_t *skip, int *order) {
    const std::string W = "lcd_merged_record_plan";
    if (n_rec < 0 || (n_rec > 0 && (!rec_pos0 || !rec_endpos || !skip || !order))) return set_err(-4, W + ": n_rec < 0 or NULL argument");
    int m = 0;
    for (int i = 0; i < n_rec; ++i) {
        skip[i] = has_prev && !(rec_endpos[i] < prev_beg || rec_pos0[i] + 1 > prev_end);     // is_ovlp_with_prev_region on [pos0 + 1, bam_endpos]
        if (!skip[i]) order[m++] = i;
    }
    if (sort_output)
        std::stable_sort(order, order + m, [&](const int a, const int b) {
            if (rec_pos0[a] != rec_pos0[b]) return rec_pos0[a] < rec_pos0[b];
            const int fa = rec_file ? rec_file[a] : 0, fb = rec_file ? rec_file[b] : 0;
            return fa != fb ? fa < fb : a < b;                                                 // (the table index is the position in the file)
        });
    for (int i = m; i < n_rec; ++i) order[i] = -1;
    return m;
}

// ---- HP / PS rewrite of a chunk's records ----
namespace {
// the records `pick` names (indices of the chunk's record table), rewritten in that order
lcd_tagged_t *tag_records_core(const std::string &W, const lcd_chunk_t *c, const int *haps, const int64_t *phase_sets, const std::vector<int> &pick) {
    if (use_device(c->device)) return nullptr;
    std::unique_ptr<lcd_tagged_s> h(new lcd_tagged_s());
    h->device = c->device;
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    std::vector<BamTagJob> jobs;
    for (const int i : pick) {
        const int r = c->rec_read[i];
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        BamTagJob j; j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.kept = r >= 0; j.hap = r >= 0 ? haps[r] : 0; j.pad = 0; j.ps = r >= 0 ? phase_sets[r] : 0;
        jobs.push_back(j);
    }
    const int n = (int)jobs.size();
    h->n_records = n;
    if (n == 0) return h.release();
    StreamGuard st; if (st.create()) return nullptr;
    DevBuf d_jobs, d_outs;
    if (d_jobs.ensure((size_t)n * sizeof(BamTagJob), 31) || d_outs.ensure((size_t)n * sizeof(BamTagOut), 31)) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_tagged_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define TCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    TCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(BamTagJob), hipMemcpyHostToDevice, st));
    lcd_launch_bam_tag_measure((const BamTagJob *)d_jobs.p, (BamTagOut *)d_outs.p, n, st);
    TCHK(hipGetLastError());
    std::vector<BamTagOut> outs(n);
    TCHK(hipMemcpyAsync(outs.data(), d_outs.p, (size_t)n * sizeof(BamTagOut), hipMemcpyDeviceToHost, st));
    TCHK(hipStreamSynchronize(st));
    uint64_t tot = 0;
    for (int i = 0; i < n; ++i) {
        const BamTagOut &o = outs[i];
        if (o.hp_end < o.hp_beg || o.ps_end < o.ps_beg || o.hp_end > jobs[i].len || o.ps_end > jobs[i].len || o.new_len < 36 || o.new_len > jobs[i].len + 14) { set_err(-24, W + ": inconsistent measure pass"); return nullptr; }
        outs[i].dst = tot; h->offs.push_back(tot); tot += o.new_len;
    }
    h->offs.push_back(tot);
    h->size = (size_t)tot;
    if (h->out.ensure((size_t)tot + 64, 31)) return nullptr;
    TCHK(hipMemcpyAsync(d_outs.p, outs.data(), (size_t)n * sizeof(BamTagOut), hipMemcpyHostToDevice, st));
    lcd_launch_bam_tag_emit((const BamTagJob *)d_jobs.p, (const BamTagOut *)d_outs.p, (uint8_t *)h->out.p, n, st);
    TCHK(hipGetLastError());
    TCHK(hipStreamSynchronize(st));
#undef TCHK
    return h.release();
}
} // namespace

lcd_tagged_t *lcd_chunk_tag_records(const lcd_chunk_t *c, const int *haps, const int64_t *phase_sets, int n_skip_kept, int n_skip_filtered) {
    const std::string W = "lcd_chunk_tag_records";
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->n_reads > 0 && (!haps || !phase_sets)) { set_err(-4, W + ": NULL haps / phase_sets"); return nullptr; }
    if (n_skip_kept < 0 || n_skip_filtered < 0) { set_err(-4, W + ": negative skip count"); return nullptr; }
    std::vector<int> pick;
    int sk = n_skip_kept, sf = n_skip_filtered;
    for (size_t i = 0; i < c->rec_beg.size(); ++i) {
        const int r = c->rec_read[i];
        if (r >= 0 ? sk > 0 : sf > 0) { --(r >= 0 ? sk : sf); continue; }
        pick.push_back((int)i);
    }
    return tag_records_core(W, c, haps, phase_sets, pick);
}
lcd_tagged_t *lcd_chunk_tag_records_sel(const lcd_chunk_t *c, const int *haps, const int64_t *phase_sets, const uint8_t *skip, const int *order) {
    const std::string W = "lcd_chunk_tag_records_sel";
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->n_reads > 0 && (!haps || !phase_sets)) { set_err(-4, W + ": NULL haps / phase_sets"); return nullptr; }
    std::vector<int> pick;
    if (pick_selected(W, c, skip, order, pick)) return nullptr;
    return tag_records_core(W, c, haps, phase_sets, pick);
}
// ---- refined alignments: the records rewritten from their reads' final digars (bam_refine_kernel.hip) ----
lcd_tagged_t *lcd_chunk_refine_records(const lcd_chunk_t *c, int n_touched, const int *touched_reads, const uint64_t *touched_off, const lcd_digar_t *touched_digars,
                                       const uint8_t *ref_seq, int64_t ref_beg, int64_t ref_end, const int *haps, const int64_t *phase_sets, const uint8_t *skip,
                                       const int *order, lcd_refine_stats_t *stats) {
    const std::string W = "lcd_chunk_refine_records";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->pending) { set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)"); return nullptr; }
    if (c->n_reads > 0 && (!haps || !phase_sets)) { set_err(-4, W + ": NULL haps / phase_sets"); return nullptr; }
    if (n_touched < 0 || (n_touched > 0 && (!touched_reads || !touched_off || (touched_off[n_touched] > touched_off[0] && !touched_digars)))) {
        set_err(-4, W + ": n_touched < 0 or NULL digar arrays"); return nullptr;
    }
    static_assert(sizeof(lcd_digar_t) == sizeof(DigarRec), "lcd_digar_t is uploaded as DigarRec");
    std::vector<int> touched_of(c->n_reads, -1);
    for (int k = 0; k < n_touched; ++k) {
        const int r = touched_reads[k];
        if (r < 0 || r >= c->n_reads || touched_of[r] >= 0 || touched_off[k + 1] < touched_off[k] || touched_off[k + 1] - touched_off[k] > (uint64_t)INT32_MAX) {
            set_err(-4, W + ": touched_reads must name reads of the chunk once each, touched_off must not fall"); return nullptr;
        }
        touched_of[r] = k;
        uint64_t sum = 0;                                        // (the kernels' running sums are 32-bit: a list stays below 2^28 bases in all, as every CIGAR word must)
        for (uint64_t d = touched_off[k]; d < touched_off[k + 1]; ++d) {
            const lcd_digar_t &g = touched_digars[d];
            // (qi is taken as it is: the reference's rewrite leaves '=' digars with qi -1 behind a right-cover walk; the kernels read a base outside the read as n)
            if (g.type < 0 || g.type > 8 || g.len < 0 || g.len >= (1 << 28) || (sum += (uint64_t)g.len) >= (1u << 28)) {
                set_err(-4, W + ": a digar with an unknown type, or lengths that are negative or reach 2^28 in all"); return nullptr;
            }
        }
    }
    const bool have_ref = ref_seq && ref_end >= ref_beg;
    std::vector<int> pick;
    if (pick_selected(W, c, skip, order, pick)) return nullptr;
    if (use_device(c->device)) return nullptr;
    std::unique_ptr<lcd_tagged_s> h(new lcd_tagged_s());
    h->device = c->device;
    const int n = (int)pick.size();
    h->n_records = n;
    if (n == 0) return h.release();
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    const uint64_t t0 = n_touched ? touched_off[0] : 0, n_up = n_touched ? touched_off[n_touched] - t0 : 0;
    DevBuf d_jobs, d_outs, d_up, d_words, d_ref;
    // the word arena: one word per digar of every record written, each record's share at a 16-byte boundary and 16 bytes behind the last one
    std::vector<BamRefineJob> jobs(n);
    uint64_t arena = 0;
    for (int k = 0; k < n; ++k) {
        const int i = pick[k], r = c->rec_read[i];
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        BamRefineJob &j = jobs[k];
        j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.kept = r >= 0; j.hap = r >= 0 ? haps[r] : 0; j.ps = r >= 0 ? phase_sets[r] : 0;
        j.pad = 0; j.skipped = r >= 0 && c->status[r] != 0; j.n_digar = 0; j.dig = 0; j.words = arena;
        if (r >= 0 && touched_of[r] >= 0) { const int t = touched_of[r]; j.n_digar = (int)(touched_off[t + 1] - touched_off[t]); j.dig = (touched_off[t] - t0) * sizeof(DigarRec); j.pad = 1; }
        else if (r >= 0) {
            j.n_digar = j.skipped ? 0 : std::max(0, c->n_digar[r]); j.dig = c->d_dig.addr() + c->slot[r] * sizeof(DigarRec);
            if (j.n_digar && (c->slot[r] + (uint64_t)j.n_digar) * sizeof(DigarRec) > c->d_dig.cap) { set_err(-4, W + ": digar slots outside the chunk's buffer"); return nullptr; }
        }
        arena += lcd_align_up((uint64_t)std::max(0, j.n_digar) * 4, 16);
    }
    if (d_jobs.ensure((size_t)n * sizeof(BamRefineJob), 31) || d_outs.ensure((size_t)n * sizeof(BamRefineOut), 31) || d_words.ensure((size_t)arena + 64, 31) ||
        d_up.ensure((size_t)n_up * sizeof(DigarRec) + 64, 31) || d_ref.ensure((have_ref ? (size_t)(ref_end - ref_beg + 1) : 0) + 64, 31)) return nullptr;
    for (BamRefineJob &j : jobs) { j.words += d_words.addr(); if (j.pad) { j.dig += d_up.addr(); j.pad = 0; } }
    std::vector<uint8_t> codes;                                        // the window as codes 0-4, whatever it came as
    if (have_ref) {
        codes.resize((size_t)(ref_end - ref_beg + 1));
        for (size_t k = 0; k < codes.size(); ++k) {
            const uint8_t b = ref_seq[k];
            codes[k] = b <= 4 ? b : (b == 'A' || b == 'a') ? 0 : (b == 'C' || b == 'c') ? 1 : (b == 'G' || b == 'g') ? 2 : (b == 'T' || b == 't') ? 3 : 4;
        }
    }
    StreamGuard st; if (st.create()) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_tagged_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define RCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    const double w0 = now_ms();
    RCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n * sizeof(BamRefineJob), hipMemcpyHostToDevice, st));
    if (n_up) { RCHK(hipMemcpyAsync(d_up.p, touched_digars + t0, (size_t)n_up * sizeof(DigarRec), hipMemcpyHostToDevice, st)); g_copy_bytes[1] += n_up * sizeof(DigarRec); }
    if (have_ref) RCHK(hipMemcpyAsync(d_ref.p, codes.data(), codes.size(), hipMemcpyHostToDevice, st));
    const long long rb = have_ref ? ref_beg : 1, re = have_ref ? ref_end : 0;    // (no window: every position reads as N)
    lcd_launch_bam_refine_measure((const BamRefineJob *)d_jobs.p, (BamRefineOut *)d_outs.p, (const uint8_t *)d_ref.p, rb, re, n, st);
    RCHK(hipGetLastError());
    std::vector<BamRefineOut> outs(n);
    RCHK(hipMemcpyAsync(outs.data(), d_outs.p, (size_t)n * sizeof(BamRefineOut), hipMemcpyDeviceToHost, st));
    RCHK(hipStreamSynchronize(st));
    const double w1 = now_ms();
    uint64_t tot = 0;
    lcd_refine_stats_t s; memset(&s, 0, sizeof(s));
    for (int k = 0; k < n; ++k) {
        BamRefineOut &o = outs[k]; const BamRefineJob &j = jobs[k];
        // what the emit pass writes is what was measured: the deleted fields lie inside the record, ascending and apart, and the length adds up
        uint64_t gone = 0, prev = 36; bool ok = o.state <= LCD_REFINE_CG && o.n_ops <= 65535 && (o.state == LCD_REFINE_CHANGED || !(o.flags & 39u));
        for (int d = 0; d < 5; ++d) { ok = ok && o.del_beg[d] >= prev && o.del_end[d] >= o.del_beg[d] && o.del_end[d] <= j.len; prev = o.del_end[d]; gone += o.del_end[d] - o.del_beg[d]; }
        const uint64_t app = ((o.flags & 1u) ? 7 : 0) + ((o.flags & 2u) ? 4ull + o.md_len : 0) + ((o.flags & 4u) ? 4ull + o.cs_len : 0) + ((o.flags & 8u) ? 7 : 0) + ((o.flags & 16u) ? 7 : 0);
        const uint64_t nc_old = ((uint64_t)j.len + 4ull * o.n_ops + app - gone - (uint64_t)o.new_len);     // 4 * the record's own n_cigar
        ok = ok && (uint64_t)o.new_len + gone >= 36 + app && nc_old % 4 == 0 && nc_old <= 4ull * 65535 && ((o.flags & 32u) || nc_old == 4ull * o.n_ops) &&
             (!(o.flags & 32u) || (int)o.n_ops <= j.n_digar);
        if (!ok) { set_err(-24, W + ": inconsistent measure pass"); return nullptr; }
        o.dst = tot; h->offs.push_back(tot); tot += o.new_len;
        ++s.n_records; s.n_kept += j.kept; s.n_pos_moved += o.pos_moved != 0;
        switch (o.state) {
        case LCD_REFINE_CHANGED: ++s.n_refined; s.n_nm_replaced += o.flags & 1u; s.n_md_replaced += (o.flags >> 1) & 1u; s.n_cs_replaced += (o.flags >> 2) & 1u; break;
        case LCD_REFINE_IDENTICAL: ++s.n_identical; break;
        case LCD_REFINE_NO_DIGARS: ++s.n_no_digars; break;
        case LCD_REFINE_QLEN: ++s.n_qlen_mismatch; break;
        case LCD_REFINE_POS: ++s.n_bad_pos; break;
        case LCD_REFINE_OPS: ++s.n_too_many_ops; break;
        case LCD_REFINE_CG: ++s.n_cg_cigar; break;
        default: break;
        }
    }
    s.n_unrefined = s.n_no_digars + s.n_qlen_mismatch + s.n_bad_pos + s.n_too_many_ops + s.n_cg_cigar;
    s.n_touched = n_touched; s.bytes_digars_up = (int64_t)(n_up * sizeof(DigarRec)); s.bytes_ref_up = (int64_t)codes.size();
    h->offs.push_back(tot);
    h->size = (size_t)tot;
    if (h->out.ensure((size_t)tot + 64, 31)) return nullptr;
    RCHK(hipMemcpyAsync(d_outs.p, outs.data(), (size_t)n * sizeof(BamRefineOut), hipMemcpyHostToDevice, st));
    lcd_launch_bam_refine_emit((const BamRefineJob *)d_jobs.p, (const BamRefineOut *)d_outs.p, (const uint8_t *)d_ref.p, rb, re, (uint8_t *)h->out.p, n, st);
    RCHK(hipGetLastError());
    RCHK(hipStreamSynchronize(st));
#undef RCHK
    s.ms_measure = w1 - w0; s.ms_emit = now_ms() - w1;
    if (stats) *stats = s;
    return h.release();
}
uint64_t lcd_tagged_dev_ptr(const lcd_tagged_t *h) { return h ? h->out.addr() : 0; }
size_t lcd_tagged_size(const lcd_tagged_t *h) { return h ? h->size : 0; }
int lcd_tagged_n_records(const lcd_tagged_t *h) { return h ? h->n_records : 0; }
int lcd_tagged_to_host(const lcd_tagged_t *h, size_t off, size_t n, uint8_t *out) {
    if (!h || off + n > h->size) return set_err(-41, "lcd_tagged_to_host: range past the end of the records");
    if (n == 0) return 0;
    if (use_device(h->device)) return -1;
    HIPCHK(hipMemcpy(out, (const uint8_t *)h->out.p + off, n, hipMemcpyDeviceToHost));
    return 0;
}
void lcd_tagged_free(lcd_tagged_t *h) { delete h; }

// ---- records as SAM text (bam_sam_kernel.hip) ----
lcd_sam_names_t *lcd_sam_names_create(int n_ref, const char *const *names) {
    const std::string W = "lcd_sam_names_create";
    if (n_ref < 0 || (n_ref > 0 && !names)) { set_err(-4, W + ": n_ref < 0 or NULL names"); return nullptr; }
    for (int r = 0; r < n_ref; ++r) if (!names[r]) { set_err(-4, W + ": NULL name"); return nullptr; }
    if (ensure_init()) return nullptr;
    std::vector<unsigned> offs((size_t)n_ref + 1, 0u); std::string pool;
    for (int r = 0; r < n_ref; ++r) {
        pool += names[r];
        if (pool.size() > (size_t)1 << 31) { set_err(-4, W + ": the names exceed 2 GB"); return nullptr; }
        offs[(size_t)r + 1] = (unsigned)pool.size();
    }
    std::unique_ptr<lcd_sam_names_s> h(new lcd_sam_names_s());
    h->n_ref = n_ref; h->device = cur_device(); h->pool_bytes = pool.size();
    if (h->pool.ensure(pool.size() + 64, 31) || h->offs.ensure(offs.size() * 4, 31)) return nullptr;
    if ((pool.size() && hipMemcpy(h->pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(h->offs.p, offs.data(), offs.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); set_err(-10, W + ": upload failed"); return nullptr;
    }
    return h.release();
}
void lcd_sam_names_free(lcd_sam_names_t *h) { delete h; }

namespace {
// the records [offs[k], offs[k + 1]) of d_base (readable for 8 bytes behind the last one) as text; the calling thread's device is the buffers' device
lcd_sam_text_t *sam_core(const std::string &W, const uint8_t *d_base, const unsigned long long *d_offs, const std::vector<unsigned long long> &offs,
                         const lcd_sam_names_t *names, lcd_sam_stats_t *stats) {
    std::unique_ptr<lcd_sam_text_s> h(new lcd_sam_text_s());
    h->device = cur_device();
    const size_t n = offs.empty() ? 0 : offs.size() - 1;
    if (n > (size_t)INT32_MAX) { set_err(-4, W + ": too many records"); return nullptr; }
    if (n == 0) return h.release();
    StreamGuard st; if (st.create()) return nullptr;
    DevBuf d_outs, d_toff;
    if (d_outs.ensure(n * sizeof(BamSamOut), 31) || d_toff.ensure((n + 1) * 8, 31)) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_sam_text_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define SCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    BamSamIn in; in.base = d_base; in.rec_off = d_offs; in.names = (const uint8_t *)names->pool.p; in.name_off = (const unsigned *)names->offs.p;
    in.n_ref = names->n_ref; in.n_rec = (int)n;
    const double w0 = now_ms();
    lcd_launch_bam_sam_measure(in, (BamSamOut *)d_outs.p, st);
    SCHK(hipGetLastError());
    std::vector<BamSamOut> outs(n);
    SCHK(hipMemcpyAsync(outs.data(), d_outs.p, n * sizeof(BamSamOut), hipMemcpyDeviceToHost, st));
    SCHK(hipStreamSynchronize(st));
    const double w1 = now_ms();
    lcd_sam_stats_t s; memset(&s, 0, sizeof(s));
    std::vector<unsigned long long> toff(n + 1, 0);
    for (size_t k = 0; k < n; ++k) {
        const BamSamOut &o = outs[k];
        // a line is at least its eleven one-byte columns, ten tabs and the newline; an array element of one byte prints as at most five, and two names come from the pool
        if (o.len < 22 || o.len > 64 + 5 * (offs[k + 1] - offs[k]) + 2 * names->pool_bytes) { set_err(-24, W + ": inconsistent measure pass"); return nullptr; }
        toff[k + 1] = toff[k] + o.len;
        s.n_float_values += o.n_float; s.n_cg_cigar += o.flags & 1u; s.n_walk_stopped += (o.flags >> 1) & 1u; s.n_bad_layout += (o.flags >> 2) & 1u;
    }
    s.n_records = (int64_t)n; s.bytes_records = (int64_t)(offs[n] - offs[0]); s.bytes_text = (int64_t)toff[n];
    h->size = (size_t)toff[n];
    if (h->text.ensure(h->size + 64, 31)) return nullptr;
    SCHK(hipMemcpyAsync(d_toff.p, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    lcd_launch_bam_sam_emit(in, (const unsigned long long *)d_toff.p, (uint8_t *)h->text.p, st);
    SCHK(hipGetLastError());
    SCHK(hipStreamSynchronize(st));
#undef SCHK
    s.ms_measure = w1 - w0; s.ms_emit = now_ms() - w1;
    if (stats) *stats = s;
    return h.release();
}
} // namespace

lcd_sam_text_t *lcd_tagged_to_sam(const lcd_tagged_t *t, const lcd_sam_names_t *names, lcd_sam_stats_t *stats) {
    const std::string W = "lcd_tagged_to_sam";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!t || !names) { set_err(-4, W + ": NULL argument"); return nullptr; }
    if (t->device != names->device) { set_err(-4, W + ": the records and the names are on different devices"); return nullptr; }
    if (t->n_records > 0 && t->offs.size() != (size_t)t->n_records + 1) { set_err(-24, W + ": the stream has no record offsets"); return nullptr; }
    if (use_device(t->device)) return nullptr;
    if (t->n_records > 0 && !t->offs_up) {
        if (t->d_offs.ensure(t->offs.size() * 8, 31)) return nullptr;
        if (hipMemcpy(t->d_offs.p, t->offs.data(), t->offs.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); set_err(-10, W + ": upload failed"); return nullptr; }
        t->offs_up = true;
    }
    static const std::vector<unsigned long long> none;
    return sam_core(W, (const uint8_t *)t->out.p, (const unsigned long long *)t->d_offs.p, t->n_records > 0 ? t->offs : none, names, stats);
}
lcd_sam_text_t *lcd_records_to_sam(const uint8_t *records, size_t n_bytes, const lcd_sam_names_t *names, lcd_sam_stats_t *stats) {
    const std::string W = "lcd_records_to_sam";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!names || (n_bytes && !records)) { set_err(-4, W + ": NULL argument"); return nullptr; }
    std::vector<unsigned long long> offs(1, 0ull);
    for (size_t o = 0; o < n_bytes;) {
        uint32_t bs = 0;
        if (n_bytes - o >= 4) memcpy(&bs, records + o, 4);
        if (n_bytes - o < 4 || bs < 32 || bs > (uint32_t)INT32_MAX || n_bytes - o - 4 < bs) { set_err(-24, W + ": the stream ends inside a record, or a record is shorter than its fixed fields"); return nullptr; }
        o += 4 + (size_t)bs; offs.push_back(o);
    }
    if (use_device(names->device)) return nullptr;
    DevBuf d_in, d_offs;
    if (n_bytes) {
        if (d_in.ensure(n_bytes + 64, 31) || d_offs.ensure(offs.size() * 8, 31)) return nullptr;
        if (hipMemcpy(d_in.p, records, n_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_offs.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError(); set_err(-10, W + ": upload failed"); return nullptr;
        }
    }
    return sam_core(W, (const uint8_t *)d_in.p, (const unsigned long long *)d_offs.p, offs, names, stats);   // (synchronised before d_in leaves scope)
}
size_t lcd_sam_text_size(const lcd_sam_text_t *h) { return h ? h->size : 0; }
uint64_t lcd_sam_text_dev_ptr(const lcd_sam_text_t *h) { return h ? h->text.addr() : 0; }
int lcd_sam_text_to_host(const lcd_sam_text_t *h, size_t off, size_t n, uint8_t *out) {
    if (!h || off > h->size || n > h->size - off || (n && !out)) return set_err(-41, "lcd_sam_text_to_host: range past the end of the text");
    if (n == 0) return 0;
    if (use_device(h->device)) return -1;
    HIPCHK(hipMemcpy(out, (const uint8_t *)h->text.p + off, n, hipMemcpyDeviceToHost));
    return 0;
}
void lcd_sam_text_free(lcd_sam_text_t *h) { delete h; }

} // extern "C"
