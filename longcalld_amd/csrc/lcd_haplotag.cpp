// lcd_haplotag.cpp -- lcd_chunk_haplotag: the kept records of a device-resident chunk against the phased sites of their contig (haplotag_kernel.hip; the rules:
// include/lcd_hotpath.h).  A contig's table goes up once per device, into a cache the lcd_phased_vcf_t owns, and is reused by every later chunk.  Per chunk: one
// job per kept record goes up; measure + scan give the candidates' total, the only number the host waits for in between (it sizes the pair bytes); mark and
// reduce follow; the four per-read arrays and the statistics come down.  The pair arrays stay in HBM until lcd_haplotag_pairs_to_host asks for them.
#include <map>
#include "lcd_host_internal.h"
#include "lcd_phased_vcf.h"

using namespace lcd_internal;

namespace {
struct DevTable { DevBuf blob; HtagSites t; };
struct DevCache { std::map<std::pair<int, int>, std::unique_ptr<DevTable>> tabs; };     // (device, contig)
void dev_cache_free(void *p) { delete (DevCache *)p; }

// the contig's table on the current device `dev`: uploaded by the first call, on stream st (synchronised here)
const HtagSites *table_on_device(lcd_phased_vcf_s *v, int contig, int dev, hipStream_t st, const std::string &W) {
    std::lock_guard<std::mutex> g(v->dev_lock);
    if (!v->dev) { v->dev = new DevCache(); v->dev_free = dev_cache_free; }
    DevCache *dc = (DevCache *)v->dev;
    auto it = dc->tabs.find({dev, contig});
    if (it != dc->tabs.end()) return &it->second->t;
    const lcd_hapvcf_contig &c = v->contigs[(size_t)contig];
    const size_t n = c.pos.size();
    std::unique_ptr<DevTable> d(new DevTable());
    std::vector<uint8_t> hb; StagePut put{hb};
    std::vector<unsigned> meta(n);
    for (size_t i = 0; i < n; ++i) meta[i] = (unsigned)c.kind[i] | ((unsigned)c.hap_of_alt[i] << 2) | ((unsigned)c.ref_code[i] << 4) | ((unsigned)c.alt_code[i] << 8);
    const uint64_t o_pos = put(c.pos.data(), n * 8), o_ins = put(c.ins_off.data(), n * 8), o_psv = put(c.ps_value.data(), c.ps_value.size() * 8), o_len = put(c.len.data(), n * 4),
                   o_psi = put(c.ps_idx.data(), n * 4), o_meta = put(meta.data(), n * 4), o_pool = put(c.pool.data(), c.pool.size());
    d->blob.dev = dev;
    if (d->blob.ensure(hb.size() + 16, 63)) return nullptr;
    if (!hb.empty() && (hipMemcpyAsync(d->blob.p, hb.data(), hb.size(), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        (void)hipGetLastError(); set_err(-10, W + ": uploading the site table failed"); return nullptr;
    }
    const uint8_t *b = (const uint8_t *)d->blob.p;
    HtagSites &t = d->t;
    t.pos = (const long long *)(b + o_pos); t.ins_off = (const long long *)(b + o_ins); t.ps_value = (const long long *)(b + o_psv); t.len = (const int *)(b + o_len);
    t.ps_idx = (const int *)(b + o_psi); t.meta = (const unsigned *)(b + o_meta); t.pool = b + o_pool;
    t.n_sites = (long long)n; t.pool_size = (long long)c.pool.size(); t.max_fp = c.max_footprint; t.n_ps = (int)c.ps_value.size();
    const HtagSites *out = &d->t;
    dc->tabs[{dev, contig}] = std::move(d);
    return out;
}
} // namespace

struct lcd_haplotag_s {
    std::vector<int> haps, n1, n2; std::vector<int64_t> ps;
    int n_jobs = 0, device = -1; uint64_t total = 0;
    DevBuf d_jobs, d_recs, d_off, d_bits, d_verdict, d_out, d_small;
};

extern "C" {

void lcd_haplotag_opt_default(lcd_haplotag_opt_t *o) { if (o) { memset(o, 0, sizeof(*o)); o->min_diff = 1; } }
int lcd_haplotag_opt_check(const lcd_haplotag_opt_t *o) {
    if (!o) return -4;
    if (o->min_diff < 1 || o->min_bq < 0 || o->min_bq > 254) return -4;
    return 0;
}

lcd_haplotag_t *lcd_chunk_haplotag(const lcd_chunk_t *c, const lcd_phased_vcf_t *vcf, int contig, const lcd_haplotag_opt_t *opt_in, lcd_haplotag_stats_t *stats) {
    const std::string W = "lcd_chunk_haplotag";
    if (stats) memset(stats, 0, sizeof(*stats));
    lcd_haplotag_opt_t opt; lcd_haplotag_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    if (!c || !c->from_bam) { set_err(-4, W + ": the chunk was not made from a BAM"); return nullptr; }
    if (c->pending) { set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)"); return nullptr; }
    if (!vcf) { set_err(-4, W + ": NULL site tables"); return nullptr; }
    if (contig < 0 || (size_t)contig >= vcf->contigs.size()) { set_err(-4, W + ": contig outside the site tables'"); return nullptr; }
    if (opt.min_diff < 1) { set_err(-4, W + ": min_diff must be at least 1"); return nullptr; }
    if (opt.min_bq < 0 || opt.min_bq > 254) { set_err(-4, W + ": min_bq must be 0 ... 254"); return nullptr; }
    if (vcf->contigs[(size_t)contig].pos.size() >= (size_t)INT32_MAX) { set_err(-4, W + ": a contig with 2^31 - 1 sites or more"); return nullptr; }
    const uint64_t base = c->stream ? lcd_inflated_dev_ptr(c->stream) : 0, usize = c->stream ? lcd_inflated_size(c->stream) : 0;
    std::vector<HtagJob> jobs;
    for (size_t i = 0; i < c->rec_beg.size(); ++i) {
        const int r = c->rec_read[i];
        if (r < 0) continue;                                                    // (filtered by the loader: no read)
        if (c->rec_stop[i] > usize || c->rec_beg[i] + 36 > c->rec_stop[i] || r >= c->n_reads || c->qlen[r] < 0) { set_err(-4, W + ": record outside the stream"); return nullptr; }
        HtagJob j; j.src = base + c->rec_beg[i]; j.len = (uint32_t)(c->rec_stop[i] - c->rec_beg[i]); j.cap = (uint32_t)c->qlen[r]; j.read = r; j.pad = 0;
        jobs.push_back(j);
    }
    const int n = (int)jobs.size(), n_reads = c->n_reads;
    std::unique_ptr<lcd_haplotag_s> h(new lcd_haplotag_s());
    h->haps.assign((size_t)n_reads, 0); h->n1.assign((size_t)n_reads, 0); h->n2.assign((size_t)n_reads, 0); h->ps.assign((size_t)n_reads, 0); h->n_jobs = n;
    if (use_device(c->device)) return nullptr;
    h->device = cur_device();
    StreamGuard st; if (st.create()) return nullptr;
    const HtagSites *tab = table_on_device(const_cast<lcd_phased_vcf_s *>(vcf), contig, h->device, st, W);
    if (!tab) return nullptr;
    // d_out: haps, n1, n2 (ints), then the phase sets (64-bit) -- per read, zeroed: a read without a job keeps 0
    const size_t out_ints = lcd_align_up((size_t)std::max(n_reads, 1) * 12, 16), out_bytes = out_ints + (size_t)std::max(n_reads, 1) * 8;
    if (h->d_jobs.ensure((size_t)std::max(n, 1) * sizeof(HtagJob), 63) || h->d_recs.ensure((size_t)std::max(n, 1) * sizeof(HtagRec), 63) || h->d_off.ensure(((size_t)n + 1) * 8, 63) ||
        h->d_out.ensure(out_bytes, 63) || h->d_small.ensure(256, 63)) return nullptr;
    auto hipfail = [&](const char *what) -> lcd_haplotag_t * { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed: " + what); return nullptr; };
#define HCHK(x) do { if ((x) != hipSuccess) return hipfail(#x); } while (0)
    HtagIn in; memset(&in, 0, sizeof(in));
    in.jobs = (const HtagJob *)h->d_jobs.p; in.recs = (HtagRec *)h->d_recs.p; in.cand_off = (unsigned long long *)h->d_off.p; in.stats = (unsigned long long *)h->d_small.p;
    in.haps = (int *)h->d_out.p; in.n1 = in.haps + n_reads; in.n2 = in.n1 + n_reads; in.ps = (long long *)((uint8_t *)h->d_out.p + out_ints);
    in.t = *tab; in.n_jobs = n; in.min_bq = opt.min_bq; in.min_diff = opt.min_diff;
    const double w0 = now_ms();
    HCHK(hipMemsetAsync(h->d_small.p, 0, 256, st));
    HCHK(hipMemsetAsync(h->d_out.p, 0, out_bytes, st));
    if (n) HCHK(hipMemcpyAsync(h->d_jobs.p, jobs.data(), (size_t)n * sizeof(HtagJob), hipMemcpyHostToDevice, st));
    lcd_launch_htag_measure(in, st);
    HCHK(hipGetLastError());
    lcd_launch_htag_scan(in, st);
    HCHK(hipGetLastError());
    unsigned long long total = 0;
    HCHK(hipMemcpyAsync(&total, in.cand_off + n, 8, hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
    if (total > (unsigned long long)n * 0x7fffffffull) { set_err(-24, W + ": inconsistent candidate count"); return nullptr; }
    h->total = total;
    const size_t words = (size_t)((total + 3) / 4) + 1;
    if (h->d_bits.ensure(words * 4, 63) || h->d_verdict.ensure((size_t)total + 16, 63)) return nullptr;
    in.bits = (unsigned *)h->d_bits.p; in.verdict = (uint8_t *)h->d_verdict.p;
    const double w1 = now_ms();
    HCHK(hipMemsetAsync(h->d_bits.p, 0, words * 4, st));
    lcd_launch_htag_mark(in, st);
    HCHK(hipGetLastError());
    HCHK(hipStreamSynchronize(st));
    const double w2 = now_ms();
    lcd_launch_htag_reduce(in, st);
    HCHK(hipGetLastError());
    unsigned long long S[14];
    if (n_reads) {
        HCHK(hipMemcpyAsync(h->haps.data(), in.haps, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
        HCHK(hipMemcpyAsync(h->n1.data(), in.n1, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
        HCHK(hipMemcpyAsync(h->n2.data(), in.n2, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
        HCHK(hipMemcpyAsync(h->ps.data(), in.ps, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
    }
    HCHK(hipMemcpyAsync(S, in.stats, sizeof(S), hipMemcpyDeviceToHost, st));
    HCHK(hipStreamSynchronize(st));
#undef HCHK
    for (int r = 0; r < n_reads; ++r) if (h->haps[r] < 0 || h->haps[r] > 2) { set_err(-24, W + ": a haplotype outside 0 ... 2 came back"); return nullptr; }
    if (stats) {
        int64_t *f = &stats->n_records;
        for (int k = 0; k < 14; ++k) f[k] = (int64_t)S[k];
        stats->ms_measure = w1 - w0; stats->ms_mark = w2 - w1; stats->ms_reduce = now_ms() - w2;
    }
    return h.release();
}

int lcd_haplotag_n_reads(const lcd_haplotag_t *h) { return h ? (int)h->haps.size() : 0; }
int lcd_haplotag_to_host(const lcd_haplotag_t *h, int *haps, int64_t *phase_sets, int *n1, int *n2) {
    if (!h) return set_err(-4, "lcd_haplotag_to_host: NULL handle");
    const size_t n = h->haps.size();
    if (n) {
        if (haps) memcpy(haps, h->haps.data(), n * 4);
        if (phase_sets) memcpy(phase_sets, h->ps.data(), n * 8);
        if (n1) memcpy(n1, h->n1.data(), n * 4);
        if (n2) memcpy(n2, h->n2.data(), n * 4);
    }
    return (int)n;
}
int lcd_haplotag_n_records(const lcd_haplotag_t *h) { return h ? h->n_jobs : 0; }
int64_t lcd_haplotag_n_candidates(const lcd_haplotag_t *h) { return h ? (int64_t)h->total : 0; }
int lcd_haplotag_pairs_to_host(const lcd_haplotag_t *h, int64_t *first_site, int64_t *cand_off, uint8_t *verdict) {
    if (!h) return set_err(-4, "lcd_haplotag_pairs_to_host: NULL handle");
    if (use_device(h->device)) return -10;
    const int n = h->n_jobs;
    if (first_site && n) {
        std::vector<HtagRec> recs((size_t)n);
        HIPCHK(hipMemcpy(recs.data(), h->d_recs.p, (size_t)n * sizeof(HtagRec), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) first_site[i] = recs[i].lo;
    }
    if (cand_off) HIPCHK(hipMemcpy(cand_off, h->d_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    if (verdict && h->total) HIPCHK(hipMemcpy(verdict, h->d_verdict.p, (size_t)h->total, hipMemcpyDeviceToHost));
    return n;
}
void lcd_haplotag_free(lcd_haplotag_t *h) { delete h; }

} // extern "C"
