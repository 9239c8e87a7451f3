// lcd_chunk_vars.cpp -- the collect_var_main port on device-resident chunks: the clean-region variants of the first round, the merge of a pass's region variants,
// the pass plan, the K5 state across a merge and lcd_chunks_noisy_rounds, which composes them with the region-batch ABI of lcd_host.cpp.
#include <cfloat>
#include <cmath>
#include <numeric>
#include "lcd_host_internal.h"

using namespace lcd_internal;

extern "C" {

// ---- the first round of collect_var_main on a device-resident chunk (src/collect_var.c:2897-2980, steps 1.2 - 3.1), see include/lcd_hotpath.h ----
void lcd_clean_opt_default(lcd_clean_opt_t *o, int is_ont) {
    o->min_dp = 5; o->min_alt_dp = 2; o->min_bq = 10; o->min_sv_len = 30; o->noisy_reg_max_xgaps = 5; o->noisy_reg_flank_len = 10; o->noisy_reg_merge_dis = 500;
    o->is_ont = is_ont ? 1 : 0; o->out_somatic = 0; o->min_af = 0.20; o->max_af = 0.80; o->strand_bias_pval = 0.01f;
}
namespace {
constexpr int CV_NON_VAR = 0x800, CV_LOW_COV = 0x001, CV_STRAND_BIAS = 0x002, CV_LOW_AF = 0x400, CV_REP_HET = 0x010, CV_NOT_CAND = 0x800 | 0x001 | 0x002;
// fisher_exact_test (src/math_utils.c:119-168; fast_lgamma is lgamma: its cache holds lgamma(i))
double cv_log_hyper(int a, int b, int c, int d) {
    const int n1 = a + b, n2 = c + d, m1 = a + c, m2 = b + d, N = n1 + n2;
    if (n1 > n2) return cv_log_hyper(c, d, a, b);
    if (m1 > m2) return cv_log_hyper(b, a, d, c);
    return lgamma(n1 + 1) + lgamma(n2 + 1) + lgamma(m1 + 1) + lgamma(m2 + 1) - (lgamma(a + 1) + lgamma(b + 1) + lgamma(c + 1) + lgamma(d + 1) + lgamma(N + 1));
}
double cv_fisher(int a, int b, int c, int d) {
    const double p_obs = exp(cv_log_hyper(a, b, c, d));
    double total = 0.0;
    const int min_a = (0 > (a + c) - (a + b + c + d)) ? 0 : (a + c) - (b + d), max_a = (a + b) < (a + c) ? (a + b) : (a + c);
    const int mode_a = (int)((a + b) * (a + c) / (double)(a + b + c + d));
    auto term = [&](int ca) {
        const int cb = (a + b) - ca, cc = (a + c) - ca, cd = (b + d) - cb;
        if (cb >= 0 && cc >= 0 && cd >= 0) { const double p = exp(cv_log_hyper(ca, cb, cc, cd)); if (p <= p_obs + DBL_EPSILON) total += p; }
    };
    for (int delta = 0; delta <= max_a - min_a; delta++) {
        if (mode_a + delta <= max_a) term(mode_a + delta);
        if (delta > 0 && mode_a - delta >= min_a) term(mode_a - delta);
    }
    return total;
}
int cv_strand_bias(const CvCov &v, float pval) { // var_is_strand_bias (src/collect_var.c:270)
    const int f = v.strand[1], r = v.strand[3], e = (f + r) / 2;
    if (e == 0) return 0;
    const float p = (float)cv_fisher(f, r, e, e);
    return p < pval;
}
// intervals [st, en) sorted by start, for counting overlaps with short queries (cr_overlap's count)
struct CvOvl {
    std::vector<long long> st, en; long long maxlen = 0;
    void build(std::vector<std::pair<long long, long long>> v) {
        std::sort(v.begin(), v.end());
        for (auto &x : v) { st.push_back(x.first); en.push_back(x.second); maxlen = std::max(maxlen, x.second - x.first); }
    }
    long long count(long long qs, long long qe) const {
        long long n = 0;
        for (long long i = (long long)(std::lower_bound(st.begin(), st.end(), qe) - st.begin()) - 1; i >= 0 && st[i] >= qs - maxlen; --i) if (qs < en[i]) n++;
        return n;
    }
};
} // namespace

static int clean_vars_one(const lcd_chunk_t *c0, const lcd_clean_opt_t *opt, const int *ordered, const uint8_t *is_rev, const uint8_t *ref_seq, int64_t ref_beg,
                          int64_t ref_end, int64_t reg_beg, int64_t reg_end, const lcd_noisy_iv_t *pre_regs, int n_pre, const int64_t *low_comp, int n_low,
                          lcd_clean_vars_t *out) {
    memset(out, 0, sizeof(*out));
    lcd_chunk_s *c = const_cast<lcd_chunk_s *>(c0);
    if (!c || !opt || !out) return set_err(-4, "lcd_chunk_clean_vars: NULL argument");
    if (opt->out_somatic) return set_err(-2, "lcd_chunk_clean_vars: somatic mode (out_somatic) is not supported");
    if (use_device(c->device)) return -1;
    const int n = c->n_reads;
    if (reg_beg < 1 || reg_end < reg_beg || reg_end - reg_beg > (1ll << 28)) return set_err(-4, "lcd_chunk_clean_vars: region [reg_beg, reg_end] out of range");
    if (!ref_seq || ref_end < ref_beg) return set_err(-4, "lcd_chunk_clean_vars: no reference");
    if (n > 0 && !ordered) return set_err(-4, "lcd_chunk_clean_vars: no ordered_read_ids");
    // the reads as the kernels see them; the qualities of a host-array chunk go up once
    std::vector<CvRead> reads(n + 1);
    uint64_t qbase = c->qual_base;
    if (n > 0 && !qbase) {
        std::lock_guard<std::mutex> lk(c->qual_mu);
        if (!c->d_qual.p) {
            if (c->d_qual.ensure(c->h_qual.size() + 64)) return -11;
            if (!c->h_qual.empty() && hipMemcpy(c->d_qual.p, c->h_qual.data(), c->h_qual.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); c->d_qual.release(); return set_err(-10, "lcd_chunk_clean_vars: quality upload failed"); }
            out->qual_upload_bytes = c->h_qual.size();
        }
        qbase = c->d_qual.addr();
    }
    uint64_t n_rec = 0;
    for (int r = 0; r < n; ++r) {
        CvRead &x = reads[r];
        x.dig = c->slot[r]; x.n_digar = c->n_digar[r]; x.seq = c->seq_base + c->seq_off[r]; x.qual = qbase + c->qual_off[r]; x.beg = c->beg[r]; x.end = c->end[r];
        x.qlen = c->qlen[r]; x.strand = is_rev ? (is_rev[r] != 0) : 0; x.iv = c->iv_off[r]; x.n_iv = (int)(c->iv_off[r + 1] - c->iv_off[r]);
        n_rec = std::max<uint64_t>(n_rec, x.dig + (uint64_t)x.n_digar);
    }
    std::vector<int> order;
    for (int i = 0; i < n; ++i) {
        const int r = ordered[i];
        if (r < 0 || r >= n) return set_err(-4, "lcd_chunk_clean_vars: ordered_read_ids out of range");
        if (c->status[r] != -1) order.push_back(r);
    }
    const int m = (int)order.size();
    CvOpt o; o.min_dp = opt->min_dp; o.min_alt_dp = opt->min_alt_dp; o.min_bq = opt->min_bq; o.min_sv_len = opt->min_sv_len; o.max_xgaps = opt->noisy_reg_max_xgaps; o.pad = 0;
    o.min_af = opt->min_af; o.max_af = opt->max_af; o.reg_beg = reg_beg; o.reg_end = reg_end; o.ref_beg = ref_beg; o.ref_end = ref_end;
    const uint64_t n_iv = n > 0 ? c->iv_off[n] : 0, ref_len = (uint64_t)(ref_end - ref_beg + 1);
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_reads, d_order, d_ivs, d_ref, d_cnt, d_tot;
    if (d_reads.ensure((n + 1) * sizeof(CvRead)) || d_order.ensure((m + 1) * 4ull) || d_ivs.ensure((n_iv + 1) * sizeof(IvRec)) || d_ref.ensure(ref_len + 64) ||
        d_cnt.ensure((m + 1) * 4ull) || d_tot.ensure(64)) return -11;
    const DigarRec *dg = (const DigarRec *)c->d_dig.p;
    HIPCHK(hipMemcpyAsync(d_reads.p, reads.data(), (n + 1) * sizeof(CvRead), hipMemcpyHostToDevice, st));
    if (m) HIPCHK(hipMemcpyAsync(d_order.p, order.data(), m * 4ull, hipMemcpyHostToDevice, st));
    if (n_iv) HIPCHK(hipMemcpyAsync(d_ivs.p, c->ivs, n_iv * sizeof(IvRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ref.p, ref_seq, ref_len, hipMemcpyHostToDevice, st));
    const CvRead *R = (const CvRead *)d_reads.p; const int *O = (const int *)d_order.p;
    // 1.2 candidate sites: count, offsets, emit with the key histogram, counting sort + bucket rank sort, dedup, compaction
    lcd_launch_cv_count(R, O, m, dg, reg_beg, reg_end, (int *)d_cnt.p, st);
    HIPCHK(hipGetLastError());
    std::vector<int> cnt(m + 1, 0);
    if (m) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, m * 4ull, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    long long n_raw = 0;
    for (int k = 0; k < m; ++k) { const int x = cnt[k]; cnt[k] = (int)n_raw; n_raw += x; }
    if (n_raw > (1ll << 30)) return set_err(-4, "lcd_chunk_clean_vars: too many site records");
    const int nr = (int)n_raw;
    const long long key0 = reg_beg - 1; const int nb = (int)(((reg_end - reg_beg + 1) >> 6) + 1); // (64 position keys per bucket, clean_vars_kernel.hip)
    DevBuf d_off, d_sites, d_hist, d_fill, d_tmp, d_sorted, d_keep, d_kidx, d_u, d_cov, d_cate;
    if (d_off.ensure((m + 1) * 4ull) || d_sites.ensure((nr + 1) * sizeof(CvSite)) || d_hist.ensure((nb + 2) * 4ull) || d_fill.ensure((nb + 2) * 4ull) ||
        d_tmp.ensure((nr + 1) * 4ull) || d_sorted.ensure((nr + 1) * 4ull) || d_keep.ensure((nr + 1) * 4ull) || d_kidx.ensure((nr + 1) * 4ull)) return -11;
    if (m) HIPCHK(hipMemcpyAsync(d_off.p, cnt.data(), m * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_hist.p, 0, (nb + 2) * 4ull, st));
    HIPCHK(hipMemsetAsync(d_fill.p, 0, (nb + 2) * 4ull, st));
    lcd_launch_cv_emit(R, O, m, dg, reg_beg, reg_end, (const int *)d_off.p, (CvSite *)d_sites.p, (int *)d_hist.p, key0, st);
    lcd_launch_cv_scan((int *)d_hist.p, nb + 1, (int *)d_tot.p, st);
    lcd_launch_cv_sort((const CvSite *)d_sites.p, nr, R, (const int *)d_hist.p, (int *)d_fill.p, (int *)d_tmp.p, (int *)d_sorted.p, key0, nb, (int *)d_keep.p,
                       opt->min_sv_len, st);
    HIPCHK(hipGetLastError());
    int ns = 0;
    if (nr) {
        HIPCHK(hipMemcpyAsync(d_kidx.p, d_keep.p, nr * 4ull, hipMemcpyDeviceToDevice, st));
        lcd_launch_cv_scan((int *)d_kidx.p, nr, (int *)d_tot.p, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&ns, d_tot.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (d_u.ensure((ns + 1) * sizeof(CvSite)) || d_cov.ensure((ns + 1) * sizeof(CvCov)) || d_cate.ensure((ns + 1) * 4ull)) return -11;
    const CvSite *U = (const CvSite *)d_u.p;
    lcd_launch_cv_compact((const CvSite *)d_sites.p, (const int *)d_sorted.p, (const int *)d_keep.p, (const int *)d_kidx.p, nr, (CvSite *)d_u.p, st);
    // 1.3 pile-up and 2.2 per-site classification
    HIPCHK(hipMemsetAsync(d_cov.p, 0, (ns + 1) * sizeof(CvCov), st));
    lcd_launch_cv_pileup(R, O, m, dg, U, ns, (CvCov *)d_cov.p, o, st);
    lcd_launch_cv_classify(U, R, (const CvCov *)d_cov.p, ns, (const unsigned char *)d_ref.p, o, (int *)d_cate.p, st);
    HIPCHK(hipGetLastError());
    std::vector<CvSite> sites(ns + 1); std::vector<CvCov> cov(ns + 1); std::vector<int> cate(ns + 1);
    if (ns) {
        HIPCHK(hipMemcpyAsync(sites.data(), d_u.p, ns * sizeof(CvSite), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(cov.data(), d_cov.p, ns * sizeof(CvCov), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(cate.data(), d_cate.p, ns * 4ull, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    // 2.2 / 2.3 classify_cand_vars (:902-1040), host side: the ONT strand-bias test, var_pos_cr, the noisy-region tests, cr_add_var_cr, cr_merge2, post_process
    std::vector<std::pair<long long, long long>> vp;
    for (int i = 0; i < ns; ++i) {
        if (opt->is_ont && cate[i] != CV_LOW_COV && cv_strand_bias(cov[i], opt->strand_bias_pval)) cate[i] = CV_STRAND_BIAS;
        if (cate[i] == CV_LOW_COV) continue;
        if (opt->is_ont && cate[i] == CV_STRAND_BIAS) continue;
        const CvSite &v = sites[i];
        const long long a = std::max<long long>(0, v.pos - 1), b = v.var_type == 1 ? v.pos : v.pos + v.ref_len - 1; // cr_add: start clamped at 0, st > en dropped
        if (a <= b) vp.push_back({a, b});
    }
    CvOvl var_pos; var_pos.build(vp);
    std::vector<std::pair<long long, long long>> low;
    for (int k = 0; k < n_low; ++k) { const long long a = std::max<long long>(0, low_comp[2 * k]), b = low_comp[2 * k + 1]; if (a <= b) low.push_back({a, b}); }
    std::vector<std::pair<long long, long long>> pre;
    for (int i = 0; i < n_pre; ++i) { const long long a = std::max<long long>(0, pre_regs[i].start), b = pre_regs[i].end; if (a <= b) pre.push_back({a, b}); }
    struct Act { int check; long long vs, ve; };
    std::vector<Act> acts; std::vector<long long> q;
    for (int i = 0; i < ns; ++i) {
        const CvSite &v = sites[i]; const int vc = cate[i];
        if (vc == CV_NON_VAR || vc == CV_STRAND_BIAS) continue;
        const long long qs = v.pos - 1, qe = v.var_type == 1 ? v.pos : v.pos + v.ref_len - 1;
        if (!pre.empty()) {
            bool hit = false;
            for (auto &x : pre) if (x.first < qe && qs < x.second) { hit = true; break; }
            if (hit) { cate[i] = CV_NON_VAR; continue; }
        }
        if (vc == CV_LOW_COV) continue;
        const bool in_reg = v.pos >= reg_beg && v.pos <= reg_end;
        auto add_var_cr = [&](int check) { // cr_add_var_cr (:750-775): grow to the overlapping low-complexity intervals (one query with the variant's own span)
            long long vs = v.pos, ve = v.var_type == 1 ? v.pos : v.pos + v.ref_len - 1;
            const long long ls = vs - 1, le = ve;
            for (auto &x : low) if (x.first < le && ls < x.second) { vs = std::min(vs, x.first + 1); ve = std::max(ve, x.second); }
            acts.push_back({check ? (int)(q.size() / 2) : -1, vs, ve});
            if (check) { q.push_back(vs); q.push_back(ve); }
        };
        if (vc == CV_REP_HET) { if (in_reg) add_var_cr(0); continue; }
        if (var_pos.count(qs, qe) > 1 && in_reg) add_var_cr(1);
        if (vc == CV_LOW_AF) cate[i] = CV_LOW_COV;
    }
    std::vector<int> qc(q.size() + 2, 0);
    const int nq = (int)(q.size() / 2);
    if (nq) { // var_noisy_reads_ratio on the digars in HBM
        DevBuf d_err, d_nerr, d_q, d_qc;
        if (d_err.ensure((n_rec + 1) * sizeof(IvRec)) || d_nerr.ensure((n + 1) * 4ull) || d_q.ensure(q.size() * 8 + 64) || d_qc.ensure(q.size() * 4 + 64)) return -11;
        HIPCHK(hipMemsetAsync(d_nerr.p, 0xff, (n + 1) * 4ull, st));
        HIPCHK(hipMemcpyAsync(d_q.p, q.data(), q.size() * 8, hipMemcpyHostToDevice, st));
        lcd_launch_cv_err_ivs(R, O, m, dg, (IvRec *)d_err.p, (int *)d_nerr.p, st);
        lcd_launch_cv_ratio(R, O, m, (const IvRec *)d_err.p, (const int *)d_nerr.p, (const long long *)d_q.p, nq, (int *)d_qc.p, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(qc.data(), d_qc.p, q.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    std::vector<NIv> nv;
    for (const Act &a : acts) {
        if (a.check >= 0) {
            const int tot = qc[2 * a.check], noisy = qc[2 * a.check + 1];
            const float ratio = tot == 0 ? 0.0f : (float)noisy / (tot + 0.0);
            if (!(ratio >= opt->min_af)) continue;
        }
        niv_add(nv, a.vs - 1, a.ve, 1);
    }
    std::vector<NIv> regs;
    for (int i = 0; i < n_pre; ++i) niv_add(regs, pre_regs[i].start, pre_regs[i].end, pre_regs[i].label);
    if (!nv.empty()) { // cr_merge2(chunk_noisy_regs, noisy_var_cr, -1, ..): both lists in their index order, cr_index, cr_merge
        niv_index(nv);
        for (const NIv &x : nv) regs.push_back(x);
        niv_index(regs);
        niv_merge(regs);
    }
    std::vector<lcd_noisy_iv_t> rin(regs.size() + 1);
    for (size_t i = 0; i < regs.size(); ++i) { rin[i].start = (int64_t)regs[i].x; rin[i].end = regs[i].en; rin[i].label = regs[i].label; rin[i].pad = 0; }
    std::vector<int64_t> vpos(ns + 1); std::vector<int> vrl(ns + 1);
    for (int i = 0; i < ns; ++i) { vpos[i] = sites[i].pos; vrl[i] = sites[i].ref_len; }
    lcd_noisy_iv_t *fin = nullptr;
    const int n_fin = lcd_post_process_noisy_regs(rin.data(), (int)regs.size(), ns, vpos.data(), vrl.data(), cate.data(), opt->noisy_reg_flank_len, &fin);
    // compaction (:1007-1023): candidates not contained in a final noisy region (cr_is_contained: the last region starting at or before the query start)
    std::vector<int> keep;
    for (int i = 0; i < ns; ++i) {
        if (cate[i] & CV_NOT_CAND) continue;
        if (n_fin > 0) {
            const long long qs = sites[i].pos - 1, qe = sites[i].pos + sites[i].ref_len;
            int lo = 0, hi = n_fin;
            while (hi > lo) { const int mid = lo + ((hi - lo) >> 1); if (fin[mid].start <= qs) lo = mid + 1; else hi = mid; }
            if (lo > 0 && fin[lo - 1].start < qe && fin[lo - 1].end >= qe) { cate[i] = CV_NON_VAR; continue; }
        }
        keep.push_back(i);
    }
    const int V = (int)keep.size();
    out->n_regs = n_fin > 0 ? n_fin : 0;
    out->regs = fin ? fin : (lcd_noisy_iv_t *)calloc(1, sizeof(lcd_noisy_iv_t));
    std::vector<CvSite> vars(V + 1); std::vector<int> vcate(V + 1); std::vector<unsigned long long> aoff(V + 1, 0);
    out->n_vars = V;
    out->pos = (int64_t *)malloc((V + 1) * 8ull); out->var_type = (int *)malloc((V + 1) * 4ull); out->ref_len = (int *)malloc((V + 1) * 4ull);
    out->alt_len = (int *)malloc((V + 1) * 4ull); out->cate = (int *)malloc((V + 1) * 4ull); out->total_cov = (int *)malloc((V + 1) * 4ull);
    out->low_qual_cov = (int *)malloc((V + 1) * 4ull); out->alle_covs = (int *)malloc((V + 1) * 8ull); out->strand_alle_covs = (int *)malloc((V + 1) * 16ull);
    out->alt_off = (uint64_t *)malloc((V + 1) * 8ull); out->is_homopolymer_indel = (int *)calloc(V + 1, 4);
    out->alt_ref_base = (uint8_t *)malloc((size_t)V + 1); memset(out->alt_ref_base, 4, (size_t)V + 1);   // unknown (src/collect_var.c:44)
    unsigned long long na = 0;
    for (int k = 0; k < V; ++k) {
        const int i = keep[k]; const CvSite &v = sites[i]; const CvCov &cv = cov[i];
        vars[k] = v; vcate[k] = cate[i];
        out->pos[k] = v.pos; out->var_type[k] = v.var_type; out->ref_len[k] = v.ref_len; out->alt_len[k] = v.alt_len; out->cate[k] = cate[i];
        out->total_cov[k] = cv.total; out->low_qual_cov[k] = cv.low; out->alle_covs[2 * k] = cv.alle[0]; out->alle_covs[2 * k + 1] = cv.alle[1];
        for (int j = 0; j < 4; ++j) out->strand_alle_covs[4 * k + j] = cv.strand[j];
        aoff[k] = na; out->alt_off[k] = na;
        if (v.var_type == 8 || v.var_type == 1) na += (unsigned long long)v.alt_len;
    }
    aoff[V] = na; out->alt_off[V] = na;
    out->alt_pool = (uint8_t *)malloc(na + 1);
    // 3.1 collect_read_var_profile: spans, CSR offsets, alleles; the alt bases of the variants
    DevBuf d_vars, d_vcate, d_aoff, d_pool, d_se, d_poff, d_al, d_qi;
    if (d_vars.ensure((V + 1) * sizeof(CvSite)) || d_vcate.ensure((V + 1) * 4ull) || d_aoff.ensure((V + 1) * 8ull) || d_pool.ensure(na + 64) ||
        d_se.ensure(2ull * (n + 1) * 4) || d_poff.ensure((n + 1) * 8ull)) return -11;
    int *d_start = (int *)d_se.p, *d_end = d_start + (n + 1);
    if (V) {
        HIPCHK(hipMemcpyAsync(d_vars.p, vars.data(), V * sizeof(CvSite), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_vcate.p, vcate.data(), V * 4ull, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_aoff.p, aoff.data(), (V + 1) * 8ull, hipMemcpyHostToDevice, st));
    }
    const CvSite *VV = (const CvSite *)d_vars.p;
    lcd_launch_cv_alt(VV, R, (const unsigned long long *)d_aoff.p, V, (unsigned char *)d_pool.p, st);
    lcd_launch_cv_profile(0, R, O, m, dg, VV, (const int *)d_vcate.p, V, (const IvRec *)d_ivs.p, d_start, d_end, nullptr, nullptr, nullptr, o, st);
    HIPCHK(hipGetLastError());
    std::vector<int> se(2ull * (n + 1));
    if (na) HIPCHK(hipMemcpyAsync(out->alt_pool, d_pool.p, na, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(se.data(), d_se.p, 2ull * (n + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out->n_reads = n;
    out->start_var_idx = (int *)malloc((n + 1) * 4ull); out->end_var_idx = (int *)malloc((n + 1) * 4ull); out->allele_off = (uint64_t *)malloc((n + 1) * 8ull);
    std::vector<char> walked(n + 1, 0);
    for (int r : order) walked[r] = 1;
    uint64_t tot = 0;
    for (int r = 0; r < n; ++r) {
        const int s0 = walked[r] ? se[r] : -1, e0 = walked[r] ? se[(n + 1) + r] : -2;
        out->start_var_idx[r] = s0; out->end_var_idx[r] = e0; out->allele_off[r] = tot;
        if (s0 >= 0) tot += (uint64_t)(e0 - s0 + 1);
    }
    out->allele_off[n] = tot;
    out->alleles = (int *)malloc((tot + 1) * 4); out->alt_qi = (int *)malloc((tot + 1) * 4);
    if (tot) {
        if (d_al.ensure(tot * 4 + 64) || d_qi.ensure(tot * 4 + 64)) return -11;
        HIPCHK(hipMemcpyAsync(d_poff.p, out->allele_off, (n + 1) * 8ull, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_al.p, 0xff, tot * 4, st)); HIPCHK(hipMemsetAsync(d_qi.p, 0xff, tot * 4, st));
        lcd_launch_cv_profile(1, R, O, m, dg, VV, (const int *)d_vcate.p, V, (const IvRec *)d_ivs.p, d_start, d_end, (const unsigned long long *)d_poff.p, (int *)d_al.p,
                              (int *)d_qi.p, o, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out->alleles, d_al.p, tot * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(out->alt_qi, d_qi.p, tot * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // read_var_cr: cr_add(start, end + 1, read) in ordered_read_ids order, cr_index
    std::vector<NIv> rv;
    for (int r : order) if (out->start_var_idx[r] >= 0 && out->end_var_idx[r] >= 0) niv_add(rv, out->start_var_idx[r], out->end_var_idx[r] + 1, r);
    niv_index(rv);
    out->n_cr = (int)rv.size();
    out->cr_read = (int *)malloc((rv.size() + 1) * 4);
    for (size_t i = 0; i < rv.size(); ++i) out->cr_read[i] = rv[i].label;
    return 0;
}
int lcd_chunk_clean_vars(const lcd_chunk_t *c, const lcd_clean_opt_t *opt, const int *ordered_read_ids, const uint8_t *is_rev, const uint8_t *ref_seq, int64_t ref_beg,
                         int64_t ref_end, int64_t reg_beg, int64_t reg_end, const lcd_noisy_iv_t *pre_regs, int n_pre_regs, const int64_t *low_comp, int n_low,
                         lcd_clean_vars_t *out) {
    if (c && c->pending) { if (out) memset(out, 0, sizeof(*out)); return set_err(-4, "lcd_chunk_clean_vars: the chunk was opened and not resolved (lcd_chunk_resolve)"); }
    if (ensure_init()) { if (out) memset(out, 0, sizeof(*out)); return -1; }
    const int rc = clean_vars_one(c, opt, ordered_read_ids, is_rev, ref_seq, ref_beg, ref_end, reg_beg, reg_end, pre_regs, n_pre_regs, low_comp, n_low, out);
    if (rc) lcd_clean_vars_free(out);
    return rc;
}
int lcd_chunk_clean_vars_batch(int n, const lcd_chunk_t *const *chunks, const lcd_clean_opt_t *opt, const int *const *ordered_read_ids, const uint8_t *const *is_rev,
                               const uint8_t *const *ref_seq, const int64_t *ref_beg, const int64_t *ref_end, const int64_t *reg_beg, const int64_t *reg_end,
                               const lcd_noisy_iv_t *const *pre_regs, const int *n_pre_regs, const int64_t *const *low_comp, const int *n_low, lcd_clean_vars_t *outs) {
    if (n <= 0) return 0;
    for (int c = 0; c < n; ++c) if (chunks && chunks[c] && chunks[c]->pending) return set_err(-4, "lcd_chunk_clean_vars: the chunk was opened and not resolved (lcd_chunk_resolve)");
    if (ensure_init()) return -1;
    std::vector<int> rc(n, 0);
    std::vector<std::string> err(n);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int i; (i = next.fetch_add(1)) < n;) {
            rc[i] = lcd_chunk_clean_vars(chunks[i], opt, ordered_read_ids[i], is_rev ? is_rev[i] : nullptr, ref_seq[i], ref_beg[i], ref_end[i], reg_beg[i], reg_end[i],
                                         pre_regs ? pre_regs[i] : nullptr, n_pre_regs ? n_pre_regs[i] : 0, low_comp ? low_comp[i] : nullptr, n_low ? n_low[i] : 0, outs + i);
            if (rc[i]) err[i] = lcd_last_error();
        }
    };
    const int nt = std::max(1, std::min(n, host_team(HostSwitches::from_env())));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (int i = 0; i < n; ++i) if (rc[i]) { for (int j = 0; j < n; ++j) lcd_clean_vars_free(outs + j); return set_err(rc[i], "chunk " + std::to_string(i) + ": " + err[i]); }
    return 0;
}
void lcd_clean_vars_free(lcd_clean_vars_t *v) {
    if (!v) return;
    free(v->pos); free(v->var_type); free(v->ref_len); free(v->alt_len); free(v->cate); free(v->total_cov); free(v->low_qual_cov); free(v->alle_covs);
    free(v->strand_alle_covs); free(v->alt_off); free(v->alt_pool); free(v->is_homopolymer_indel); free(v->regs); free(v->start_var_idx); free(v->end_var_idx);
    free(v->allele_off); free(v->alleles); free(v->alt_qi); free(v->cr_read); free(v->alt_ref_base);
    memset(v, 0, sizeof(*v));
}
int lcd_clean_vars_hap_problem(const lcd_clean_vars_t *v, int is_ont, const int *ordered_read_ids, const uint8_t *is_skipped, int *alle_off, int *allele_off,
                               lcd_hap_problem_t *p) {
    for (int i = 0; i <= v->n_vars; ++i) alle_off[i] = 2 * i;
    for (int r = 0; r <= v->n_reads; ++r) allele_off[r] = (int)v->allele_off[r];
    p->n_reads = v->n_reads; p->n_vars = v->n_vars; p->is_ont = is_ont;
    p->var_pos = v->pos; p->var_type = v->var_type; p->var_cate = v->cate; p->is_homopolymer_indel = v->is_homopolymer_indel; p->total_cov = v->total_cov;
    p->alle_off = alle_off; p->alle_covs = v->alle_covs; p->start_var_idx = v->start_var_idx; p->end_var_idx = v->end_var_idx; p->allele_off = allele_off;
    p->alleles = v->alleles; p->ordered_read_ids = ordered_read_ids; p->is_skipped = is_skipped; p->n_cr = v->n_cr; p->cr_read = v->cr_read;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// merge_var_profile (src/collect_var.c:1298-1387) for every region of a pass: table walk on the host, profile on the device (merge_vars_kernel.hip)
} // extern "C"
namespace {
struct MvVar { int64_t pos; int type, ref_len, alt_len; const uint8_t *alt; int origin /* -1: the chunk's table, else the region */, idx; };
// exact_comp_var_site (:1878): position key, type, ref_len, alt_len, alt bases of X / INS
int mv_cmp(const MvVar &a, const MvVar &b) {
    const int64_t ka = a.type == 8 ? a.pos : a.pos - 1, kb = b.type == 8 ? b.pos : b.pos - 1;
    if (ka != kb) return ka < kb ? -1 : 1;
    if (a.type != b.type) return a.type < b.type ? -1 : 1;
    if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len ? -1 : 1;
    if (a.alt_len != b.alt_len) return a.alt_len < b.alt_len ? -1 : 1;
    if ((a.type == 8 || a.type == 1) && a.alt_len > 0) return memcmp(a.alt, b.alt, (size_t)a.alt_len);
    return 0;
}
struct MvChunk {                       // one chunk of a call between the host walk and the device profile
    std::vector<int> a2m; std::vector<std::vector<int>> b2m; std::vector<char> active;
    uint64_t o_a2m = 0, o_al = 0, o_qi = 0; std::vector<uint64_t> o_b2m, o_prof;
    int read0 = 0;
};
// validation + the fold of two-pointer walks; fills every per-variant array of *out and the maps.  No device call.
int mv_walk(const char *who, const lcd_clean_vars_t *cur, int n_regions, const lcd_region_vars_t *regions, const int *ordered, const uint8_t *is_skipped,
            lcd_clean_vars_t *out, MvChunk &mc) {
    const std::string W(who);
    if (!cur || !out) return set_err(-4, W + ": NULL argument");
    if (n_regions < 0) return set_err(-4, W + ": n_regions < 0");
    if (n_regions > 0 && !regions) return set_err(-4, W + ": no regions");
    const int V = cur->n_vars, R = cur->n_reads;
    if (V < 0 || R < 0) return set_err(-4, W + ": negative n_vars / n_reads");
    if (R > 0 && (!ordered || !is_skipped || !cur->start_var_idx || !cur->end_var_idx || !cur->allele_off)) return set_err(-4, W + ": no ordered_read_ids / is_skipped / profile");
    if (V > 0 && (!cur->pos || !cur->var_type || !cur->ref_len || !cur->alt_len || !cur->cate || !cur->total_cov || !cur->low_qual_cov || !cur->alle_covs ||
                  !cur->strand_alle_covs || !cur->alt_off || !cur->is_homopolymer_indel)) return set_err(-4, W + ": incomplete variant table");
    for (int i = 0; i < V; ++i) {
        const uint64_t nb = cur->alt_off[i + 1] - cur->alt_off[i];
        if (cur->alt_off[i + 1] < cur->alt_off[i] || cur->alt_len[i] < 0 || ((cur->var_type[i] == 8 || cur->var_type[i] == 1) && nb != (uint64_t)cur->alt_len[i]))
            return set_err(-4, W + ": alt_off does not match alt_len at variant " + std::to_string(i));
    }
    mc.active.assign(R + 1, 0);
    for (int i = 0; i < R; ++i) {
        const int r = ordered[i];
        if (r < 0 || r >= R) return set_err(-4, W + ": ordered_read_ids out of range");
        if (!is_skipped[r]) mc.active[r] = 1;
    }
    for (int r = 0; r < R; ++r) {
        const int s = cur->start_var_idx[r], e = cur->end_var_idx[r];
        const uint64_t nc = cur->allele_off[r + 1] - cur->allele_off[r];
        if (cur->allele_off[r + 1] < cur->allele_off[r]) return set_err(-4, W + ": allele_off decreases at read " + std::to_string(r));
        if (s < 0) continue;
        if (e < s || e >= V || nc != (uint64_t)(e - s + 1)) return set_err(-4, W + ": profile span of read " + std::to_string(r) + " outside [0, n_vars) or not matching allele_off");
        if (!cur->alleles || !cur->alt_qi) return set_err(-4, W + ": no profile cells");
    }
    std::vector<int> seen(R + 1, -1);
    for (int k = 0; k < n_regions; ++k) {
        const lcd_region_vars_t &g = regions[k];
        if (g.n_vars <= 0) continue;
        if (!g.vars || g.n_rows < 0 || (g.n_rows > 0 && (!g.row_read_ids || !g.prof_start || !g.prof_end || !g.prof_alleles))) return set_err(-4, W + ": region " + std::to_string(k) + " incomplete");
        for (int j = 0; j < g.n_vars; ++j)
            if (g.vars[j].alt_len < 0 || ((g.vars[j].var_type == 8 || g.vars[j].var_type == 1) && g.vars[j].alt_len > 0 && !g.vars[j].alt_seq))
                return set_err(-4, W + ": region " + std::to_string(k) + " variant " + std::to_string(j) + " has no alt_seq");
        for (int q = 0; q < g.n_rows; ++q) {
            const int r = g.row_read_ids[q];
            if (r < 0 || r >= R) return set_err(-4, W + ": region " + std::to_string(k) + " row " + std::to_string(q) + ": read id outside [0, n_reads)");
            if (seen[r] == k) return set_err(-4, W + ": region " + std::to_string(k) + ": read " + std::to_string(r) + " twice");
            seen[r] = k;
            if (g.prof_start[q] >= 0 && g.prof_end[q] >= g.prof_start[q] && g.prof_end[q] >= g.n_vars)
                return set_err(-4, W + ": region " + std::to_string(k) + " row " + std::to_string(q) + ": span outside [0, n_vars)");
        }
    }
    // the fold
    std::vector<MvVar> tab(V), nxt;
    for (int i = 0; i < V; ++i) tab[i] = {cur->pos[i], cur->var_type[i], cur->ref_len[i], cur->alt_len[i], cur->alt_pool ? cur->alt_pool + cur->alt_off[i] : nullptr, -1, i};
    for (int k = 0; k < n_regions; ++k) {
        const lcd_region_vars_t &g = regions[k];
        if (g.n_vars <= 0) continue;
        nxt.clear(); nxt.reserve(tab.size() + g.n_vars);
        size_t i = 0; int j = 0;
        auto reg_var = [&](int q) { const lcd_noisy_var_t &v = g.vars[q]; return MvVar{v.pos, v.var_type, v.ref_len, v.alt_len, v.alt_seq, k, q}; };
        while (i < tab.size() && j < g.n_vars) {
            const MvVar b = reg_var(j);
            const int c = mv_cmp(tab[i], b);
            if (c < 0) nxt.push_back(tab[i++]);
            else if (c > 0) { nxt.push_back(b); ++j; }
            else { nxt.push_back(tab[i++]); ++j; }   // equal: the table's entry stays, the region's is dropped
        }
        for (; i < tab.size(); ++i) nxt.push_back(tab[i]);
        for (; j < g.n_vars; ++j) nxt.push_back(reg_var(j));
        tab.swap(nxt);
    }
    const int M = (int)tab.size();
    mc.a2m.assign(V + 1, -1); mc.b2m.resize(n_regions);
    for (int k = 0; k < n_regions; ++k) mc.b2m[k].assign(regions[k].n_vars > 0 ? regions[k].n_vars : 0, -1);
    out->n_vars = M;
    out->pos = (int64_t *)malloc((M + 1) * 8ull); out->var_type = (int *)malloc((M + 1) * 4ull); out->ref_len = (int *)malloc((M + 1) * 4ull);
    out->alt_len = (int *)malloc((M + 1) * 4ull); out->cate = (int *)malloc((M + 1) * 4ull); out->total_cov = (int *)malloc((M + 1) * 4ull);
    out->low_qual_cov = (int *)calloc(M + 1, 4); out->alle_covs = (int *)malloc((M + 1) * 8ull); out->strand_alle_covs = (int *)calloc(M + 1, 16);
    out->alt_off = (uint64_t *)malloc((M + 1) * 8ull); out->is_homopolymer_indel = (int *)calloc(M + 1, 4);
    out->alt_ref_base = (uint8_t *)malloc((size_t)M + 1); out->alt_ref_base[M] = 4;
    uint64_t na = 0;
    for (int m = 0; m < M; ++m) { const MvVar &t = tab[m]; if (t.origin < 0) na += cur->alt_off[t.idx + 1] - cur->alt_off[t.idx]; else if (t.type == 8 || t.type == 1) na += (uint64_t)t.alt_len; }
    out->alt_pool = (uint8_t *)malloc(na + 1);
    na = 0;
    for (int m = 0; m < M; ++m) {
        const MvVar &t = tab[m];
        out->pos[m] = t.pos; out->var_type[m] = t.type; out->ref_len[m] = t.ref_len; out->alt_len[m] = t.alt_len; out->alt_off[m] = na;
        if (t.origin < 0) {
            const int i = t.idx; mc.a2m[i] = m;
            out->cate[m] = cur->cate[i]; out->total_cov[m] = cur->total_cov[i]; out->low_qual_cov[m] = cur->low_qual_cov[i];
            out->alle_covs[2 * m] = cur->alle_covs[2 * i]; out->alle_covs[2 * m + 1] = cur->alle_covs[2 * i + 1];
            memcpy(out->strand_alle_covs + 4 * m, cur->strand_alle_covs + 4 * i, 16); out->is_homopolymer_indel[m] = cur->is_homopolymer_indel[i];
            out->alt_ref_base[m] = cur->alt_ref_base ? cur->alt_ref_base[i] : 4;   // (a table without the member: all unknown)
            const uint64_t nb = cur->alt_off[i + 1] - cur->alt_off[i];
            if (nb) memcpy(out->alt_pool + na, cur->alt_pool + cur->alt_off[i], nb);
            na += nb;
        } else {
            const lcd_noisy_var_t &v = regions[t.origin].vars[t.idx]; mc.b2m[t.origin][t.idx] = m;
            out->cate[m] = v.cate; out->total_cov[m] = v.total_cov; out->alle_covs[2 * m] = v.alle_covs[0]; out->alle_covs[2 * m + 1] = v.alle_covs[1];
            out->is_homopolymer_indel[m] = v.is_homopolymer_indel;
            out->alt_ref_base[m] = t.type == 8 ? 0 : (uint8_t)v.alt_ref_base;      // make_cand_vars0 (:1755-1756): an X variant keeps the cleared struct's 0
            if ((t.type == 8 || t.type == 1) && t.alt_len > 0) { memcpy(out->alt_pool + na, v.alt_seq, (size_t)t.alt_len); na += (uint64_t)t.alt_len; }
        }
    }
    out->alt_off[M] = na;
    out->n_regs = cur->n_regs > 0 ? cur->n_regs : 0;
    out->regs = (lcd_noisy_iv_t *)calloc(out->n_regs + 1, sizeof(lcd_noisy_iv_t));
    if (out->n_regs) memcpy(out->regs, cur->regs, out->n_regs * sizeof(lcd_noisy_iv_t));
    out->n_reads = R; out->qual_upload_bytes = 0;
    return 0;
}
} // namespace
extern "C" {
int lcd_merge_region_vars_batch(int n_chunks, const lcd_clean_vars_t *const *cur, const int *n_regions, const lcd_region_vars_t *const *regions,
                                const int *const *ordered_read_ids, const uint8_t *const *is_skipped, lcd_clean_vars_t *outs, int *const *cur_to_merged,
                                int **const *region_to_merged) {
    if (n_chunks <= 0) return n_chunks < 0 ? set_err(-4, "lcd_merge_region_vars_batch: n_chunks < 0") : 0;
    if (!cur || !n_regions || !regions || !ordered_read_ids || !is_skipped || !outs) return set_err(-4, "lcd_merge_region_vars_batch: NULL argument");
    memset(outs, 0, sizeof(lcd_clean_vars_t) * (size_t)n_chunks);
    auto fail = [&](int rc) { const std::string m = g_err; for (int c = 0; c < n_chunks; ++c) lcd_clean_vars_free(outs + c); g_err = m; return rc; };
    std::vector<MvChunk> mcs(n_chunks);
    // 1. host: validation and the table walks of every chunk (nothing is launched on malformed input)
    for (int c = 0; c < n_chunks; ++c) {
        const int rc = mv_walk("lcd_merge_region_vars", cur[c], n_regions[c], regions[c], ordered_read_ids[c], is_skipped[c], outs + c, mcs[c]);
        if (rc) { if (n_chunks > 1) g_err = "chunk " + std::to_string(c) + ": " + g_err; return fail(rc); }
    }
    // 2. one staging block: maps, source cells, the source table, the reads' new start / end (min / max identities) and the flag
    std::vector<uint8_t> hb(16, 0);   // (offset 0 stays unused: MvSrc.alt_qi == 0 means "no alt_qi")
    StagePut put{hb};
    std::vector<MvSrc> srcs;
    int G = 0;
    for (int c = 0; c < n_chunks; ++c) { mcs[c].read0 = G; G += cur[c]->n_reads; }
    std::vector<int> lo(G + 1, 0x7fffffff), hi(G + 1, -1);   // per read: bounds of its merged span (exact for the current profile, the region's extent for a row)
    unsigned long long n_cells = 0;
    for (int c = 0; c < n_chunks; ++c) {
        MvChunk &mc = mcs[c]; const lcd_clean_vars_t &cv = *cur[c];
        const int R = cv.n_reads, V = cv.n_vars; const uint64_t NA = R ? cv.allele_off[R] : 0;
        mc.o_a2m = put(mc.a2m.data(), (size_t)V * 4); mc.o_al = put(cv.alleles, NA * 4); mc.o_qi = put(cv.alt_qi, NA * 4);
        for (int r = 0; r < R; ++r) {
            const int s = cv.start_var_idx[r], e = cv.end_var_idx[r];
            if (!mc.active[r] || s < 0) continue;
            srcs.push_back({mc.o_a2m, mc.o_al + cv.allele_off[r] * 4, mc.o_qi + cv.allele_off[r] * 4, c, mc.read0 + r, s, e - s + 1, n_cells});
            n_cells += (unsigned long long)(e - s + 1);
            lo[mc.read0 + r] = mc.a2m[s]; hi[mc.read0 + r] = mc.a2m[e];
        }
        mc.o_b2m.assign(n_regions[c], 0); mc.o_prof.assign(n_regions[c], 0);
        for (int k = 0; k < n_regions[c]; ++k) {
            const lcd_region_vars_t &g = regions[c][k];
            if (g.n_vars <= 0) continue;
            int mn = 0x7fffffff, mx = -1;
            for (int m : mc.b2m[k]) if (m >= 0) { mn = std::min(mn, m); mx = std::max(mx, m); }
            if (mx < 0 || g.n_rows <= 0) continue;   // every variant dropped: no cell of this region moves
            mc.o_b2m[k] = put(mc.b2m[k].data(), (size_t)g.n_vars * 4); mc.o_prof[k] = put(g.prof_alleles, (size_t)g.n_rows * g.n_vars * 4);
            for (int q = 0; q < g.n_rows; ++q) {
                const int r = g.row_read_ids[q], s = g.prof_start[q], e = g.prof_end[q];
                if (!mc.active[r] || s < 0 || e < s) continue;
                srcs.push_back({mc.o_b2m[k], mc.o_prof[k] + ((uint64_t)q * g.n_vars + s) * 4, 0, c, mc.read0 + r, s, e - s + 1, n_cells});
                n_cells += (unsigned long long)(e - s + 1);
                lo[mc.read0 + r] = std::min(lo[mc.read0 + r], mn); hi[mc.read0 + r] = std::max(hi[mc.read0 + r], mx);
            }
        }
    }
    unsigned long long cap = 0;
    for (int g = 0; g < G; ++g) if (hi[g] >= lo[g]) cap += (unsigned long long)(hi[g] - lo[g] + 1);
    const int S = (int)srcs.size(), NB = (G + 255) / 256;
    std::vector<int> se;                              // downloaded: start[G], end[G]
    std::vector<uint8_t> dl;
    const unsigned long long *off = nullptr; const int *d_al = nullptr, *d_qi = nullptr;
    std::vector<unsigned long long> zero_off(G + 1, 0);
    if (S > 0) {
        if (ensure_init()) return fail(-1);
        const uint64_t o_src = put(nullptr, (size_t)S * sizeof(MvSrc));
        const uint64_t o_start = put(nullptr, (size_t)G * 4), o_end = put(nullptr, (size_t)G * 4), o_flag = put(nullptr, 16);
        for (int g = 0; g < G; ++g) { ((int *)(hb.data() + o_start))[g] = 0x7fffffff; ((int *)(hb.data() + o_end))[g] = -1; }
        const uint64_t up_bytes = lcd_align_up(hb.size(), 16);
        const uint64_t o_off = up_bytes, o_bsum = o_off + lcd_align_up((uint64_t)(G + 1) * 8, 16), o_cells = o_bsum + lcd_align_up((uint64_t)NB * 8 + 16, 16);
        const uint64_t total = o_cells + 2 * cap * 4 + 64;
        StreamGuard st; if (st.create()) return fail(-10);
        DevBuf d; if (d.ensure(total, 63)) return fail(-11);          // the call's one allocation
        const uint64_t B = d.addr();
        for (MvSrc &s : srcs) { s.map += B; s.alleles += B; if (s.alt_qi) s.alt_qi += B; }
        memcpy(hb.data() + o_src, srcs.data(), (size_t)S * sizeof(MvSrc));
#define MVCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(-10, std::string(#x) + ": " + hipGetErrorString(e_)); return fail(-10); } } while (0)
        MVCHK(hipMemcpyAsync(d.p, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
        const MvSrc *SS = (const MvSrc *)(uintptr_t)(B + o_src);
        int *d_start = (int *)(uintptr_t)(B + o_start), *d_end = (int *)(uintptr_t)(B + o_end), *d_flag = (int *)(uintptr_t)(B + o_flag);
        unsigned long long *d_off = (unsigned long long *)(uintptr_t)(B + o_off), *d_bsum = (unsigned long long *)(uintptr_t)(B + o_bsum);
        int *cells = (int *)(uintptr_t)(B + o_cells);
        lcd_launch_mv_span(SS, S, d_start, d_end, st);
        lcd_launch_mv_scan(d_start, d_end, G, d_off, d_bsum, st);
        lcd_launch_mv_fill(cells, 2 * cap, st);
        lcd_launch_mv_scatter(SS, S, n_cells, d_start, d_off, cells, cells + cap, cap, d_flag, st);
        MVCHK(hipGetLastError());
        dl.resize(o_cells + 2 * cap * 4 - o_start);
        MVCHK(hipMemcpyAsync(dl.data(), (const uint8_t *)d.p + o_start, dl.size(), hipMemcpyDeviceToHost, st));
        MVCHK(hipStreamSynchronize(st));
#undef MVCHK
        auto at = [&](uint64_t o) { return dl.data() + (o - o_start); };   // the downloaded copy of device offset o (>= o_start)
        se.assign((const int *)at(o_start), (const int *)at(o_start) + G); se.insert(se.end(), (const int *)at(o_end), (const int *)at(o_end) + G);
        off = (const unsigned long long *)at(o_off); d_al = (const int *)at(o_cells); d_qi = d_al + cap;
        if (*(const int *)at(o_flag) || off[G] > cap) { set_err(-24, "lcd_merge_region_vars: cell capacity exceeded (" + std::to_string(off[G]) + " cells, " + std::to_string(cap) + " allocated)"); return fail(-24); }
    } else {
        se.assign(G, -1); se.insert(se.end(), G, -2); off = zero_off.data();
    }
    // 3. per chunk: spans, CSR, cells, the interval index; the maps
    for (int c = 0; c < n_chunks; ++c) {
        const MvChunk &mc = mcs[c]; lcd_clean_vars_t *out = outs + c; const int R = out->n_reads, g0 = mc.read0;
        out->start_var_idx = (int *)malloc((R + 1) * 4ull); out->end_var_idx = (int *)malloc((R + 1) * 4ull); out->allele_off = (uint64_t *)malloc((R + 1) * 8ull);
        for (int r = 0; r < R; ++r) { out->start_var_idx[r] = se[g0 + r]; out->end_var_idx[r] = se[G + g0 + r]; out->allele_off[r] = off[g0 + r] - off[g0]; }
        const uint64_t tot = off[g0 + R] - off[g0];
        out->allele_off[R] = tot;
        out->alleles = (int *)malloc((tot + 1) * 4); out->alt_qi = (int *)malloc((tot + 1) * 4);
        if (tot) { memcpy(out->alleles, d_al + off[g0], tot * 4); memcpy(out->alt_qi, d_qi + off[g0], tot * 4); }
        std::vector<NIv> rv;   // read_var_cr: cr_add(start, end + 1, read) in ordered_read_ids order, cr_index
        for (int i = 0; i < R; ++i) { const int r = ordered_read_ids[c][i]; if (is_skipped[c][r]) continue; if (out->start_var_idx[r] >= 0 && out->end_var_idx[r] >= 0) niv_add(rv, out->start_var_idx[r], out->end_var_idx[r] + 1, r); }
        niv_index(rv);
        out->n_cr = (int)rv.size();
        out->cr_read = (int *)malloc((rv.size() + 1) * 4);
        for (size_t i = 0; i < rv.size(); ++i) out->cr_read[i] = rv[i].label;
        if (cur_to_merged && cur_to_merged[c] && cur[c]->n_vars > 0) memcpy(cur_to_merged[c], mc.a2m.data(), (size_t)cur[c]->n_vars * 4);
        if (region_to_merged && region_to_merged[c])
            for (int k = 0; k < n_regions[c]; ++k) if (region_to_merged[c][k] && !mc.b2m[k].empty()) memcpy(region_to_merged[c][k], mc.b2m[k].data(), mc.b2m[k].size() * 4);
    }
    return 0;
}
int lcd_merge_region_vars(const lcd_clean_vars_t *cur, int n_regions, const lcd_region_vars_t *regions, const int *ordered_read_ids, const uint8_t *is_skipped,
                          lcd_clean_vars_t *out, int *cur_to_merged, int **region_to_merged) {
    if (!out) return set_err(-4, "lcd_merge_region_vars: NULL argument");
    return lcd_merge_region_vars_batch(1, &cur, &n_regions, &regions, &ordered_read_ids, &is_skipped, out, cur_to_merged ? &cur_to_merged : nullptr,
                                       region_to_merged ? &region_to_merged : nullptr);
}

// ---------------------------------------------------------------------------------------------------
// the noisy-region rounds of collect_var_main (src/collect_var.c:2946-2977) on device-resident chunks: pass plan (plan_kernel.hip), planned regions into a
// batch, K5 state across a merge, and the driver that composes them with lcd_batch_run_many, lcd_merge_region_vars_batch and lcd_assign_hap_batch
void lcd_pass_opt_default(lcd_pass_opt_t *o) { o->max_noisy_reg_len = 50000; o->max_noisy_reg_cov = 1000; o->noisy_reg_flank_len = 10; } // src/call_var_main.h:36-42
void lcd_pass_plan_free(lcd_pass_plan_t *p) {
    if (!p) return;
    free(p->status); free(p->beg); free(p->end); free(p->read_off); free(p->read_ids); free(p->read_beg); free(p->read_end); free(p->cover);
    memset(p, 0, sizeof(*p));
}
int lcd_chunk_plan_pass_batch(int n_chunks, const lcd_chunk_t *const *chunks, const lcd_pass_opt_t *opt, const int *n_regs, const lcd_noisy_iv_t *const *regs,
                              const int *const *done, const int *const *ordered_read_ids, const uint8_t *const *is_skipped, const int64_t *ref_beg,
                              const int64_t *ref_end, lcd_pass_plan_t *outs) {
    const std::string W = "lcd_chunk_plan_pass";
    if (n_chunks <= 0) return n_chunks < 0 ? set_err(-4, W + ": n_chunks < 0") : 0;
    if (!chunks || !opt || !n_regs || !regs || !done || !ordered_read_ids || !is_skipped || !ref_beg || !ref_end || !outs) return set_err(-4, W + ": NULL argument");
    memset(outs, 0, sizeof(lcd_pass_plan_t) * (size_t)n_chunks);
    for (int c = 0; c < n_chunks; ++c) if (chunks[c] && chunks[c]->pending) return set_err(-4, W + ": the chunk was opened and not resolved (lcd_chunk_resolve)");
    // 1. host: validation; nothing touches the device on malformed input
    long long G = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const std::string at = n_chunks > 1 ? "chunk " + std::to_string(c) + ": " : "";
        if (n_regs[c] < 0) return set_err(-4, W + ": " + at + "n_regs < 0");
        if (ref_end[c] < ref_beg[c]) return set_err(-4, W + ": " + at + "ref_end < ref_beg");
        if (n_regs[c] > 0 && (!regs[c] || !done[c])) return set_err(-4, W + ": " + at + "no regs / done");
    }
    for (int c = 0; c < n_chunks; ++c) {
        const std::string at = n_chunks > 1 ? "chunk " + std::to_string(c) + ": " : "";
        if (!chunks[c]) return set_err(-4, W + ": " + at + "NULL chunk");
        if (chunks[c]->device != chunks[0]->device) return set_err(-4, W + ": chunks on different devices");
        const int R = chunks[c]->n_reads;
        if (R > 0 && (!ordered_read_ids[c] || !is_skipped[c])) return set_err(-4, W + ": " + at + "no ordered_read_ids / is_skipped");
        for (int i = 0; i < R; ++i) if (ordered_read_ids[c][i] < 0 || ordered_read_ids[c][i] >= R) return set_err(-4, W + ": " + at + "ordered_read_ids entry outside [0, n_reads)");
        G += n_regs[c];
    }
    if (G > (1ll << 30)) return set_err(-4, W + ": too many regions");
    // 2. the region tables; long and done regions are decided here
    std::vector<PlanReg> pr((size_t)G); std::vector<int> reg0(n_chunks + 1, 0);
    int n_pending = 0;
    for (int c = 0, g = 0; c < n_chunks; ++c) {
        reg0[c] = g;
        for (int i = 0; i < n_regs[c]; ++i, ++g) {
            PlanReg &q = pr[g]; q.chunk = c;
            q.beg = std::max<int64_t>(regs[c][i].start, ref_beg[c]); q.end = std::min<int64_t>(regs[c][i].end, ref_end[c]);   // collect_reg_ref_bseq, src/seq.c:417-418
            q.status = done[c][i] ? LCD_PLAN_DONE_BEFORE : q.end - q.beg + 1 > (long long)opt->max_noisy_reg_len ? LCD_PLAN_SKIP_LONG : LCD_PLAN_SUBMIT;
            n_pending += q.status == LCD_PLAN_SUBMIT;
        }
        reg0[c + 1] = g;
    }
    std::vector<int> st_h((size_t)G); std::vector<unsigned long long> off_h((size_t)G + 1, 0);
    for (long long g = 0; g < G; ++g) st_h[g] = pr[g].status;
    std::vector<uint8_t> pairs;                       // downloaded: SliceOut[P], read ids[P]
    unsigned long long P = 0;
    if (n_pending > 0) {
        if (use_device(chunks[0]->device)) return -1;
        // the chunks' read tables: once per chunk
        for (int c = 0; c < n_chunks; ++c) {
            lcd_chunk_s *ch = const_cast<lcd_chunk_s *>(chunks[c]);
            std::lock_guard<std::mutex> lk(ch->plan_mu);
            if (ch->plan_ready || ch->n_reads <= 0) continue;
            std::vector<PlanRead> tab(ch->n_reads);
            for (int r = 0; r < ch->n_reads; ++r) { PlanRead &x = tab[r]; x.beg = ch->beg[r]; x.end = ch->end[r]; x.digar_off = ch->slot[r]; x.n_digar = ch->n_digar[r]; x.qlen = ch->qlen[r]; x.status = ch->status[r]; x.pad = 0; }
            if (ch->d_plan.ensure(tab.size() * sizeof(PlanRead), 63)) return -11;
            if (hipMemcpy(ch->d_plan.p, tab.data(), tab.size() * sizeof(PlanRead), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); ch->d_plan.release(); return set_err(-10, W + ": read table upload failed"); }
            ch->plan_ready = true;
        }
        // one staged block: chunk table, region table, every chunk's ordered_read_ids and is_skipped; behind it on the device: counts, statuses, offsets
        std::vector<uint8_t> hb;
        StagePut put{hb};
        const uint64_t o_ch = put(nullptr, (size_t)n_chunks * sizeof(PlanChunk)), o_pr = put(pr.data(), (size_t)G * sizeof(PlanReg));
        std::vector<PlanChunk> pc(n_chunks);
        for (int c = 0; c < n_chunks; ++c) {
            const lcd_chunk_s *ch = chunks[c]; const int R = ch->n_reads;
            pc[c].reads = ch->d_plan.addr(); pc[c].digars = ch->d_dig.addr(); pc[c].n_reads = R; pc[c].pad = 0;
            pc[c].order = put(ordered_read_ids[c], (size_t)R * 4); pc[c].skipped = put(is_skipped[c], (size_t)R);
        }
        const uint64_t up_bytes = lcd_align_up(hb.size(), 16);
        const uint64_t o_cnt = up_bytes, o_st = o_cnt + lcd_align_up((uint64_t)G * 4, 16), o_off = o_st + lcd_align_up((uint64_t)G * 4, 16);
        const uint64_t total = o_off + ((uint64_t)G + 1) * 8 + 64;
        StreamGuard st; if (st.create()) return -10;
        DevBuf d; if (d.ensure(total, 63)) return -11;
        const uint64_t B = d.addr();
        for (int c = 0; c < n_chunks; ++c) { pc[c].order += B; pc[c].skipped += B; }
        memcpy(hb.data() + o_ch, pc.data(), (size_t)n_chunks * sizeof(PlanChunk));
        HIPCHK(hipMemcpyAsync(d.p, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
        const PlanChunk *d_ch = (const PlanChunk *)(uintptr_t)(B + o_ch); const PlanReg *d_pr = (const PlanReg *)(uintptr_t)(B + o_pr);
        int *d_cnt = (int *)(uintptr_t)(B + o_cnt), *d_st = (int *)(uintptr_t)(B + o_st); unsigned long long *d_off = (unsigned long long *)(uintptr_t)(B + o_off);
        lcd_launch_plan_count(d_ch, d_pr, (int)G, opt->max_noisy_reg_cov, d_cnt, d_st, st);
        lcd_launch_plan_scan(d_cnt, (int)G, d_off, st);
        HIPCHK(hipGetLastError());
        std::vector<uint8_t> dl(o_off + ((uint64_t)G + 1) * 8 - o_st);
        HIPCHK(hipMemcpyAsync(dl.data(), (const uint8_t *)d.p + o_st, dl.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                                             // (1) the counts size the pair area
        memcpy(st_h.data(), dl.data(), (size_t)G * 4); memcpy(off_h.data(), dl.data() + (o_off - o_st), ((size_t)G + 1) * 8);
        P = off_h[G];
        if (P > 0x7fffffffull) return set_err(-24, W + ": more than 2^31 - 1 (region, read) pairs in one call");
        if (P > 0) {
            DevBuf dp; if (dp.ensure(P * (sizeof(SliceOut) + 8) + 64, 63)) return -11;     // the pair area: slices, read ids, region of the pair
            SliceOut *d_so = (SliceOut *)dp.p; int *d_ids = (int *)((uint8_t *)dp.p + P * sizeof(SliceOut)), *d_preg = d_ids + P;
            lcd_launch_plan_fill(d_ch, d_pr, (int)G, d_st, d_off, d_ids, d_preg, st);
            lcd_launch_plan_slices(d_ch, d_pr, d_ids, d_preg, P, opt->noisy_reg_flank_len, d_so, st);
            HIPCHK(hipGetLastError());
            pairs.resize(P * (sizeof(SliceOut) + 4));
            HIPCHK(hipMemcpyAsync(pairs.data(), dp.p, pairs.size(), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));                                         // (2)
        }
    }
    // 3. per chunk: the malloc()'d plan
    const SliceOut *so = (const SliceOut *)pairs.data(); const int *ids = (const int *)(pairs.data() + P * sizeof(SliceOut));
    for (int c = 0; c < n_chunks; ++c) {
        lcd_pass_plan_t &o = outs[c]; const int n = n_regs[c], g0 = reg0[c];
        const unsigned long long p0 = off_h[g0], np = off_h[g0 + n] - p0;
        o.n_regs = n;
        o.status = (int *)malloc((n + 1) * 4ull); o.beg = (int64_t *)malloc((n + 1) * 8ull); o.end = (int64_t *)malloc((n + 1) * 8ull); o.read_off = (uint64_t *)malloc((n + 1) * 8ull);
        o.read_ids = (int *)malloc((np + 1) * 4); o.read_beg = (int *)malloc((np + 1) * 4); o.read_end = (int *)malloc((np + 1) * 4); o.cover = (int *)malloc((np + 1) * 4);
        for (int i = 0; i < n; ++i) { o.status[i] = st_h[g0 + i]; o.beg[i] = pr[g0 + i].beg; o.end[i] = pr[g0 + i].end; o.read_off[i] = off_h[g0 + i] - p0; }
        o.read_off[n] = np;
        for (unsigned long long k = 0; k < np; ++k) { o.read_ids[k] = ids[p0 + k]; o.read_beg[k] = so[p0 + k].read_beg; o.read_end[k] = so[p0 + k].read_end; o.cover[k] = so[p0 + k].cover; }
    }
    return 0;
}
int lcd_chunk_plan_pass(const lcd_chunk_t *c, const lcd_pass_opt_t *opt, int n_regs, const lcd_noisy_iv_t *regs, const int *done, const int *ordered_read_ids,
                        const uint8_t *is_skipped, int64_t ref_beg, int64_t ref_end, lcd_pass_plan_t *out) {
    if (!out) return set_err(-4, "lcd_chunk_plan_pass: NULL argument");
    return lcd_chunk_plan_pass_batch(1, &c, opt, &n_regs, &regs, &done, &ordered_read_ids, &is_skipped, &ref_beg, &ref_end, out);
}
void lcd_hap_state_free(lcd_hap_state_t *s) {
    if (!s) return;
    free(s->haps); free(s->phase_sets); free(s->n_clean_agree_snps); free(s->n_clean_conflict_snps); free(s->var_phase_set); free(s->hap_to_cons_alle); free(s->hap_to_alle_profile);
    memset(s, 0, sizeof(*s));
}
int lcd_hap_state_init(int R, int V, lcd_hap_state_t *o) {
    if (!o || R < 0 || V < 0) return set_err(-4, "lcd_hap_state_init: bad arguments");
    o->n_reads = R; o->n_vars = V;
    o->haps = (int *)calloc(R + 1, 4); o->phase_sets = (int64_t *)malloc((R + 1) * 8ull); o->n_clean_agree_snps = (int *)calloc(R + 1, 4); o->n_clean_conflict_snps = (int *)calloc(R + 1, 4);
    o->var_phase_set = (int64_t *)malloc((V + 1) * 8ull); o->hap_to_cons_alle = (int *)malloc((3ull * V + 1) * 4); o->hap_to_alle_profile = (int *)calloc(6ull * V + 1, 4);
    for (int r = 0; r < R; ++r) o->phase_sets[r] = -1;
    for (int i = 0; i < V; ++i) o->var_phase_set[i] = -1;
    for (int i = 0; i < 3 * V; ++i) o->hap_to_cons_alle[i] = -1;
    return 0;
}
int lcd_hap_state_carry(const lcd_hap_state_t *old, int M, const int *c2m, lcd_hap_state_t *out) {
    if (!old || !out || old == out || M < 0 || old->n_vars < 0 || old->n_reads < 0 || (old->n_vars > 0 && !c2m)) return set_err(-4, "lcd_hap_state_carry: bad arguments");
    const int V = old->n_vars, R = old->n_reads;
    std::vector<char> taken(M + 1, 0);
    for (int i = 0; i < V; ++i) {
        if (c2m[i] < 0 || c2m[i] >= M) return set_err(-4, "lcd_hap_state_carry: cur_to_merged[" + std::to_string(i) + "] outside [0, merged n_vars)");
        if (taken[c2m[i]]) return set_err(-4, "lcd_hap_state_carry: two variants map to merged variant " + std::to_string(c2m[i]));
        taken[c2m[i]] = 1;
    }
    if (lcd_hap_state_init(R, M, out)) return -4;
    if (R) { memcpy(out->haps, old->haps, R * 4ull); memcpy(out->phase_sets, old->phase_sets, R * 8ull); memcpy(out->n_clean_agree_snps, old->n_clean_agree_snps, R * 4ull); memcpy(out->n_clean_conflict_snps, old->n_clean_conflict_snps, R * 4ull); }
    for (int i = 0; i < V; ++i) {
        const int m = c2m[i];
        out->var_phase_set[m] = old->var_phase_set[i];
        for (int h = 0; h < 3; ++h) {
            out->hap_to_cons_alle[3 * m + h] = old->hap_to_cons_alle[3 * i + h];
            out->hap_to_alle_profile[(size_t)h * 2 * M + 2 * m] = old->hap_to_alle_profile[(size_t)h * 2 * V + 2 * i];
            out->hap_to_alle_profile[(size_t)h * 2 * M + 2 * m + 1] = old->hap_to_alle_profile[(size_t)h * 2 * V + 2 * i + 1];
        }
    }
    return 0;
}
} // extern "C"
namespace {
struct RoundsChunk {               // one chunk of lcd_chunks_noisy_rounds between passes
    lcd_clean_vars_t own_vars; lcd_hap_state_t own_state; bool has_own = false;   // the driver's own current state (else the caller's)
    std::vector<int> order, done, f2f; int n_passes = 0; bool in_loop = false;
};
struct RegionVarsOwned {           // lcd_batch_region_vars' outputs, freed with the object
    lcd_noisy_var_t *vars = nullptr; int n = 0, rows = 0; int *ids = nullptr, *ps = nullptr, *pe = nullptr, *pa = nullptr;
    void release() { for (int i = 0; i < n; ++i) free(vars[i].alt_seq); free(vars); free(ids); free(ps); free(pe); free(pa); vars = nullptr; ids = ps = pe = pa = nullptr; n = rows = 0; }
};
// one entry per (cluster, read) of a region that has just resolved, in update_digars_from_aln_str's order: the rows of lcd_batch_region_vars' row_read_ids
int log_region(lcd_refine_log_t *log, lcd_batch_t *b, int region, const lcd_pass_plan_t &plan, int i, int pass, const RegionVarsOwned &x) {
    const int rows = x.rows;
    std::vector<int> len(rows + 1); std::vector<const uint8_t *> t(rows + 1), q(rows + 1);
    const int n = lcd_batch_region_ref_read_rows(b, region, rows, len.data(), t.data(), q.data());
    if (n < 0) return n;
    if (n != rows) return set_err(-23, "lcd_chunks_noisy_rounds_log: the region's rows and its ref<->read rows differ in number");
    const uint64_t k0 = plan.read_off[i], k1 = plan.read_off[i + 1];
    for (int r = 0; r < rows; ++r) {
        uint64_t k = k0;
        while (k < k1 && plan.read_ids[k] != x.ids[r]) ++k;
        if (k == k1) return set_err(-23, "lcd_chunks_noisy_rounds_log: a cluster read is not in the region's plan");
        const lcd_refine_entry_t e = {x.ids[r], plan.cover[k], plan.read_beg[k], plan.read_end[k], len[r], pass, plan.beg[i], plan.end[i], t[r], q[r]};
        if (int rc = lcd_refine_log_append(log, &e)) return rc;
    }
    return 0;
}
int rounds_core(const std::string &W, int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt, lcd_refine_log_t *const *logs);
}
extern "C" {
int lcd_chunks_noisy_rounds(int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt) {
    return rounds_core("lcd_chunks_noisy_rounds", n_chunks, chunks, opt, pass_opt, nullptr);
}
int lcd_chunks_noisy_rounds_log(int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt, lcd_refine_log_t *const *logs) {
    bool any = false;
    for (int c = 0; logs && c < n_chunks; ++c) any |= logs[c] != nullptr;
    return rounds_core(any ? "lcd_chunks_noisy_rounds_log" : "lcd_chunks_noisy_rounds", n_chunks, chunks, opt, pass_opt, any ? logs : nullptr);
}
}
namespace {
int rounds_core(const std::string &W, int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt, lcd_refine_log_t *const *logs) {
    if (n_chunks <= 0) return n_chunks < 0 ? set_err(-4, W + ": n_chunks < 0") : 0;
    if (!chunks || !opt || !pass_opt) return set_err(-4, W + ": NULL argument");
    if (opt->collect_ref_read_aln_str) return set_err(-2, W + ": somatic / refine mode (collect_ref_read_aln_str) is not supported: the regions of a pass are order-dependent there");
    for (int c = 0; c < n_chunks; ++c) {
        lcd_rounds_chunk_t &x = chunks[c];
        x.done = nullptr; x.first_to_final = nullptr; x.n_passes = 0; x.n_first_vars = 0;
        const std::string at = W + ": chunk " + std::to_string(c) + ": ";
        if (!x.chunk || !x.vars || !x.state || !x.ref_seq) return set_err(-4, at + "NULL member");
        if (x.ref_end < x.ref_beg) return set_err(-4, at + "ref_end < ref_beg");
        if (x.vars->n_reads != x.chunk->n_reads || x.state->n_reads != x.vars->n_reads || x.state->n_vars != x.vars->n_vars) return set_err(-4, at + "chunk, vars and state disagree on n_reads / n_vars");
        if (x.vars->n_regs < 0 || (x.vars->n_regs > 0 && !x.vars->regs)) return set_err(-4, at + "no regs");
        if (x.vars->n_reads > 0 && (!x.ordered_read_ids || !x.is_skipped)) return set_err(-4, at + "no ordered_read_ids / is_skipped");
        if (x.chunk->device != chunks[0].chunk->device) return set_err(-4, W + ": chunks on different devices");
    }
    lcd_opt_t bopt = *opt; bopt.collect_noisy_vars = 2;
    if (logs) bopt.collect_ref_read_aln_str = 1;            // the sink's rows: the only strings that come down
    std::vector<RoundsChunk> rc(n_chunks);
    std::vector<lcd_batch_t *> batches;            // of the current pass
    std::vector<lcd_pass_plan_t> plans;
    auto drop_pass = [&]() { for (lcd_batch_t *b : batches) if (b) lcd_batch_destroy(b); batches.clear(); for (lcd_pass_plan_t &p : plans) lcd_pass_plan_free(&p); plans.clear(); };
    auto fail = [&](int code) {
        const std::string m = g_err; drop_pass();
        for (RoundsChunk &r : rc) if (r.has_own) { lcd_clean_vars_free(&r.own_vars); lcd_hap_state_free(&r.own_state); r.has_own = false; }
        g_err = m; return code;
    };
    auto cur_vars = [&](int c) -> lcd_clean_vars_t * { return rc[c].has_own ? &rc[c].own_vars : chunks[c].vars; };
    auto cur_state = [&](int c) -> lcd_hap_state_t * { return rc[c].has_own ? &rc[c].own_state : chunks[c].state; };
    for (int c = 0; c < n_chunks; ++c) {
        RoundsChunk &r = rc[c]; const lcd_clean_vars_t *v = chunks[c].vars;
        r.order.resize(v->n_regs); r.done.assign(v->n_regs, 0); r.f2f.resize(v->n_vars); std::iota(r.f2f.begin(), r.f2f.end(), 0);
        if (v->n_regs > 0 && lcd_sort_noisy_regs(v->regs, v->n_regs, r.order.data())) return fail(-4);
        r.in_loop = v->n_regs > 0;
    }
    for (;;) {
        std::vector<int> A;
        for (int c = 0; c < n_chunks; ++c) if (rc[c].in_loop) A.push_back(c);
        if (A.empty()) break;
        const int na = (int)A.size();
        // 1. the plan of this pass over the chunks still in the loop
        std::vector<const lcd_chunk_t *> p_ch(na); std::vector<int> p_n(na); std::vector<const lcd_noisy_iv_t *> p_regs(na); std::vector<const int *> p_done(na), p_ord(na);
        std::vector<const uint8_t *> p_skip(na); std::vector<int64_t> p_rb(na), p_re(na);
        for (int a = 0; a < na; ++a) {
            const int c = A[a]; const lcd_clean_vars_t *v = cur_vars(c);
            p_ch[a] = chunks[c].chunk; p_n[a] = v->n_regs; p_regs[a] = v->regs; p_done[a] = rc[c].done.data(); p_ord[a] = chunks[c].ordered_read_ids; p_skip[a] = chunks[c].is_skipped;
            p_rb[a] = chunks[c].ref_beg; p_re[a] = chunks[c].ref_end;
        }
        plans.assign(na, lcd_pass_plan_t());
        int rcode = lcd_chunk_plan_pass_batch(na, p_ch.data(), pass_opt, p_n.data(), p_regs.data(), p_done.data(), p_ord.data(), p_skip.data(), p_rb.data(), p_re.data(), plans.data());
        if (rcode) return fail(rcode);
        // 2. one batch per chunk, one joint run
        batches.assign(na, nullptr);
        std::vector<std::vector<int>> ridx(na);
        std::vector<lcd_batch_t *> run;
        for (int a = 0; a < na; ++a) {
            const int c = A[a];
            ridx[a].assign(plans[a].n_regs + 1, -1);
            bool any = false; for (int i = 0; i < plans[a].n_regs; ++i) any |= plans[a].status[i] == LCD_PLAN_SUBMIT;
            if (!any) continue;
            batches[a] = lcd_batch_create_on(&bopt, chunks[c].chunk->device);
            if (!batches[a]) return fail(-10);
            rcode = lcd_batch_add_planned(batches[a], chunks[c].chunk, &plans[a], cur_state(c)->haps, cur_state(c)->phase_sets, chunks[c].ref_seq, chunks[c].ref_beg, ridx[a].data());
            if (rcode < 0) return fail(rcode);
            if ((rcode = lcd_batch_upload(batches[a]))) return fail(rcode);
            run.push_back(batches[a]);
        }
        if (!run.empty()) {
            if ((rcode = lcd_batch_run_many(run.data(), (int)run.size()))) return fail(rcode);
            for (lcd_batch_t *b : run) if ((rcode = lcd_batch_download(b))) return fail(rcode);
        }
        // 3. the regions' variants in sorted-region order, done[] by the reference's rule
        std::vector<std::vector<RegionVarsOwned>> got(na); std::vector<char> new_var(na, 0), new_done(na, 0);
        auto free_got = [&]() { for (auto &g : got) for (RegionVarsOwned &x : g) x.release(); };
        for (int a = 0; a < na; ++a) {
            const int c = A[a]; RoundsChunk &r = rc[c];
            for (int k = 0; k < plans[a].n_regs; ++k) {
                const int i = r.order[k], st = plans[a].status[i];
                if (st == LCD_PLAN_SKIP_LONG || st == LCD_PLAN_SKIP_DEEP) { r.done[i] = 1; new_done[a] = 1; continue; }   // collect_noisy_vars1 returns 0
                if (st != LCD_PLAN_SUBMIT) continue;
                if (batches[a]->regs[ridx[a][i]].n_cons <= 0) continue;                                                  // returns -1: tried again
                RegionVarsOwned x;
                const int n = lcd_batch_region_vars(batches[a], ridx[a][i], plans[a].beg[i], chunks[c].ref_seq, chunks[c].ref_beg, chunks[c].ref_end - chunks[c].ref_beg + 1, &x.vars,
                                                    &x.rows, &x.ids, &x.ps, &x.pe, &x.pa);
                x.n = n > 0 ? n : 0;
                got[a].push_back(x);
                if (n < 0) { const std::string m = g_err; free_got(); g_err = m; return fail(n); }
                if (logs && logs[c]) {
                    const int lrc = log_region(logs[c], batches[a], ridx[a][i], plans[a], i, r.n_passes, got[a].back());
                    if (lrc) { const std::string m = g_err; free_got(); g_err = m; return fail(lrc); }
                }
                r.done[i] = 1; new_done[a] = 1;
                if (n > 0) new_var[a] = 1;
            }
        }
        // 4. merge + carry + K5 over all germline categories for the chunks that got a variant
        std::vector<int> M; for (int a = 0; a < na; ++a) if (new_var[a]) M.push_back(a);
        if (!M.empty()) {
            const int nm = (int)M.size();
            std::vector<std::vector<lcd_region_vars_t>> rv(nm); std::vector<const lcd_clean_vars_t *> m_cur(nm); std::vector<int> m_n(nm); std::vector<const lcd_region_vars_t *> m_rv(nm);
            std::vector<const int *> m_ord(nm); std::vector<const uint8_t *> m_skip(nm); std::vector<std::vector<int>> c2m(nm); std::vector<int *> m_c2m(nm);
            for (int q = 0; q < nm; ++q) {
                const int a = M[q], c = A[a];
                for (const RegionVarsOwned &x : got[a]) rv[q].push_back(lcd_region_vars_t{x.n, x.vars, x.rows, x.ids, x.ps, x.pe, x.pa});
                m_cur[q] = cur_vars(c); m_n[q] = (int)rv[q].size(); m_rv[q] = rv[q].data(); m_ord[q] = chunks[c].ordered_read_ids; m_skip[q] = chunks[c].is_skipped;
                c2m[q].assign(m_cur[q]->n_vars + 1, -1); m_c2m[q] = c2m[q].data();
            }
            std::vector<lcd_clean_vars_t> merged(nm); std::vector<lcd_hap_state_t> carried(nm, lcd_hap_state_t());
            rcode = lcd_merge_region_vars_batch(nm, m_cur.data(), m_n.data(), m_rv.data(), m_ord.data(), m_skip.data(), merged.data(), m_c2m.data(), nullptr);
            free_got();
            auto drop_new = [&]() { const std::string m = g_err; for (int q = 0; q < nm; ++q) { lcd_clean_vars_free(&merged[q]); lcd_hap_state_free(&carried[q]); } g_err = m; };
            if (rcode) return fail(rcode);   // (the merge freed its outputs)
            std::vector<lcd_hap_problem_t> probs(nm); std::vector<std::vector<int>> alle_off(nm), allele_off(nm); std::vector<int> targets(nm, 0x004 | 0x008 | 0x080 | 0x100 | 0x200); // LONGCALLD_CAND_GERMLINE_VAR_CATE, src/collect_var.h:25
            for (int q = 0; q < nm; ++q) {
                const int c = A[M[q]];
                if ((rcode = lcd_hap_state_carry(cur_state(c), merged[q].n_vars, c2m[q].data(), &carried[q]))) { drop_new(); return fail(rcode); }
                alle_off[q].resize(merged[q].n_vars + 1); allele_off[q].resize(merged[q].n_reads + 1);
                lcd_clean_vars_hap_problem(&merged[q], chunks[c].is_ont, chunks[c].ordered_read_ids, chunks[c].is_skipped, alle_off[q].data(), allele_off[q].data(), &probs[q]);
                lcd_hap_problem_t &p = probs[q]; const lcd_hap_state_t &s = carried[q];
                p.haps = s.haps; p.phase_sets = s.phase_sets; p.n_clean_agree_snps = s.n_clean_agree_snps; p.n_clean_conflict_snps = s.n_clean_conflict_snps;
                p.var_phase_set = s.var_phase_set; p.hap_to_cons_alle = s.hap_to_cons_alle; p.hap_to_alle_profile = s.hap_to_alle_profile;
            }
            if ((rcode = lcd_assign_hap_batch(nm, probs.data(), targets.data()))) { drop_new(); return fail(rcode); }
            for (int q = 0; q < nm; ++q) {
                const int c = A[M[q]]; RoundsChunk &r = rc[c];
                if (r.has_own) { lcd_clean_vars_free(&r.own_vars); lcd_hap_state_free(&r.own_state); }
                r.own_vars = merged[q]; r.own_state = carried[q]; r.has_own = true;
                for (int &f : r.f2f) f = c2m[q][f];
            }
        } else free_got();
        for (int a = 0; a < na; ++a) { RoundsChunk &r = rc[A[a]]; ++r.n_passes; if (!new_done[a]) r.in_loop = false; }
        drop_pass();
    }
    // the caller's structures take the final state
    for (int c = 0; c < n_chunks; ++c) {
        RoundsChunk &r = rc[c]; lcd_rounds_chunk_t &x = chunks[c];
        x.n_first_vars = (int)r.f2f.size(); x.n_passes = r.n_passes;
        x.done = (int *)malloc((r.done.size() + 1) * 4); if (!r.done.empty()) memcpy(x.done, r.done.data(), r.done.size() * 4);
        x.first_to_final = (int *)malloc((r.f2f.size() + 1) * 4); if (!r.f2f.empty()) memcpy(x.first_to_final, r.f2f.data(), r.f2f.size() * 4);
        if (r.has_own) { lcd_clean_vars_free(x.vars); *x.vars = r.own_vars; lcd_hap_state_free(x.state); *x.state = r.own_state; r.has_own = false; }
    }
    return 0;
}
} // namespace
