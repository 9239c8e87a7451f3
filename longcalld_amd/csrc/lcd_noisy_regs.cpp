// lcd_noisy_regs.cpp -- noisy-region intervals: the cgranges-ordered interval helpers (niv_*), pre_ / post_process_noisy_regs, cr_merge, sort_noisy_regs and the
// digar walk of collect_noisy_read_info for (region, read) pairs on host digars.
#include "lcd_host_internal.h"

using namespace lcd_internal;


extern "C" {

// ---- SURVEY 8(f) f2, chunk level: pre_process_noisy_regs (src/collect_var.c:557-638) ----
// cr_index's ordering (src/cgranges.c:13-86, :350-353): kept as added when the keys are non-decreasing, otherwise klib's in-place MSD radix sort
// on the 64-bit key (8 bits per pass from bit 56, buckets of <= 64 entries by insertion sort) -- NOT stable, and windows found in many reads give
// many equal starts, so the tie order of the real thing is reproduced, not approximated
void niv_insertion(NIv *b, NIv *e) {
    for (NIv *i = b + 1; i < e; ++i)
        if (i->x < (i - 1)->x) { NIv t = *i, *j; for (j = i; j > b && t.x < (j - 1)->x; --j) *j = *(j - 1); *j = t; }
}
void niv_radix(NIv *beg, NIv *end, int s) {
    struct Bk { NIv *b, *e; } bk[256];
    for (auto &k : bk) k.b = k.e = beg;
    for (NIv *i = beg; i != end; ++i) ++bk[(i->x >> s) & 255].e;
    for (int k = 1; k < 256; ++k) { bk[k].e += bk[k - 1].e - beg; bk[k].b = bk[k - 1].e; }
    for (Bk *k = bk; k != bk + 256;) {
        if (k->b != k->e) {
            Bk *l = bk + ((k->b->x >> s) & 255);
            if (l != k) { NIv tmp = *k->b, sw; do { sw = tmp; tmp = *l->b; *l->b++ = sw; l = bk + ((tmp.x >> s) & 255); } while (l != k); *k->b++ = tmp; }
            else ++k->b;
        } else ++k;
    }
    bk[0].b = beg; for (int k = 1; k < 256; ++k) bk[k].b = bk[k - 1].e;
    if (s) {
        s = s > 8 ? s - 8 : 0;
        for (auto &k : bk) { if (k.e - k.b > 64) niv_radix(k.b, k.e, s); else if (k.e - k.b > 1) niv_insertion(k.b, k.e); }
    }
}
void niv_index(std::vector<NIv> &v) {
    bool sorted = true; for (size_t i = 1; i < v.size(); ++i) if (v[i - 1].x > v[i].x) { sorted = false; break; }
    if (sorted) return;
    if (v.size() <= 64) niv_insertion(v.data(), v.data() + v.size()); else niv_radix(v.data(), v.data() + v.size(), 56);
}
void niv_add(std::vector<NIv> &v, long long st, long long en, int label) { if (st < 0) st = 0; if (st > en) return; v.push_back({(uint64_t)st, en, label}); } // cr_add :145-149
// cr_merge(cr, -1, ...) (src/cgranges.c:225-300): passes of "merge every later interval that starts within min(label, label') of the running end"
// until the number of intervals stops changing; each pass re-indexes
void niv_merge(std::vector<NIv> &v, const int fixed_win) { // fixed_win >= 0: cr_merge(cr, fixed_win, ..): that window instead of the smaller label
    size_t cur = v.size();
    for (;;) {
        std::vector<NIv> out; std::vector<char> merged(v.size(), 0);
        for (size_t j = 0; j < v.size(); ++j) {
            if (merged[j]) continue;
            uint64_t ms = v[j].x; long long me = v[j].en; int ml = v[j].label;
            for (size_t k = j + 1; k < v.size(); ++k) {
                if (merged[k]) continue;
                const int win = fixed_win >= 0 ? fixed_win : (ml < v[k].label ? ml : v[k].label);
                if ((uint64_t)(me + win) >= v[k].x) { ml = std::max(ml, v[k].label); ms = std::min(ms, v[k].x); me = std::max(me, v[k].en); merged[k] = 1; }
            }
            niv_add(out, (long long)ms, me, ml);
        }
        niv_index(out);
        v.swap(out);
        if (v.size() == cur) break;
        cur = v.size();
    }
}

// collect_noisy_read_info's digar walk (src/align.c:1392-1456) for many (region, read) pairs in one launch, on digars as lcd_digar_batch returns them: which
// query interval of each read lies over its region and how the read covers the region's ends.  The per-region form of the same walk is the host loop of
// lcd_batch_add_region_from_chunk; this is the chunk-level form of SURVEY f2 (all regions of a chunk against all their reads: tens of thousands of pairs).
int lcd_region_read_slices_batch(int n_pairs, const int *pair_read, const int64_t *pair_reg_beg, const int64_t *pair_reg_end, int n_reads,
                                 const uint64_t *digar_off, const lcd_digar_t *digars, const int *qlen, int noisy_reg_flank_len,
                                 int *read_beg, int *read_end, int *cover) {
    static_assert(sizeof(lcd_digar_t) == sizeof(DigarRec), "lcd_digar_t is DigarRec");
    if (ensure_init()) return -1;
    if (n_pairs <= 0) return 0;
    if (n_reads <= 0) return set_err(-4, "lcd_region_read_slices_batch: no reads");
    std::vector<SliceJob> jobs(n_pairs);
    for (int i = 0; i < n_pairs; ++i) {
        const int r = pair_read[i];
        if (r < 0 || r >= n_reads) return set_err(-4, "lcd_region_read_slices_batch: read index out of range");
        SliceJob &j = jobs[i]; j.digar_off = digar_off[r]; j.n_digar = (int)(digar_off[r + 1] - digar_off[r]); j.qlen = qlen[r]; j.reg_beg = pair_reg_beg[i]; j.reg_end = pair_reg_end[i];
    }
    const uint64_t nd = digar_off[n_reads];
    StreamGuard st; if (st.create()) return -10;
    DevBuf d_dig, d_jobs, d_outs;
    if (d_dig.ensure((nd + 1) * sizeof(DigarRec)) || d_jobs.ensure(n_pairs * sizeof(SliceJob)) || d_outs.ensure(n_pairs * sizeof(SliceOut))) return -11;
    if (nd) { HIPCHK(hipMemcpyAsync(d_dig.p, digars, nd * sizeof(DigarRec), hipMemcpyHostToDevice, st)); g_copy_bytes[1] += nd * sizeof(DigarRec); }
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), n_pairs * sizeof(SliceJob), hipMemcpyHostToDevice, st));
    lcd_launch_slices((const SliceJob *)d_jobs.p, (SliceOut *)d_outs.p, (const DigarRec *)d_dig.p, noisy_reg_flank_len, n_pairs, st);
    HIPCHK(hipGetLastError());
    std::vector<SliceOut> outs(n_pairs);
    HIPCHK(hipMemcpyAsync(outs.data(), d_outs.p, n_pairs * sizeof(SliceOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n_pairs; ++i) { read_beg[i] = outs[i].read_beg; read_end[i] = outs[i].read_end; cover[i] = outs[i].cover; }
    return 0;
}

int lcd_pre_process_noisy_regs(const lcd_noisy_iv_t *chunk_noisy, int n_noisy, const int64_t *low_comp, int n_low, int n_reads, const int64_t *read_beg,
                               const int64_t *read_end, const uint64_t *read_iv_off, const lcd_noisy_iv_t *read_ivs, int min_alt_dp, float min_af,
                               lcd_noisy_iv_t **regs_out) {
    *regs_out = nullptr;
    if (ensure_init()) return -1;
    if (n_noisy <= 0) return 0;
    std::vector<NIv> v;
    for (int i = 0; i < n_noisy; ++i) niv_add(v, chunk_noisy[i].start, chunk_noisy[i].end, chunk_noisy[i].label);
    pre_regs_merge(v, low_comp, n_low);
    const int nr = (int)v.size();
    if (nr == 0) return 0;
    // read support on the device
    StreamGuard st; if (st.create()) return -10;
    std::vector<IvRec> regs(nr);
    for (int i = 0; i < nr; ++i) { regs[i].st = (long long)v[i].x; regs[i].en = v[i].en; regs[i].label = v[i].label; regs[i].pad = 0; }
    const uint64_t niv = n_reads > 0 ? read_iv_off[n_reads] : 0;
    DevBuf d_regs, d_rb, d_re, d_off, d_iv, d_cnt;
    if (d_regs.ensure(nr * sizeof(IvRec)) || d_rb.ensure((n_reads + 1) * 8) || d_re.ensure((n_reads + 1) * 8) || d_off.ensure((n_reads + 2) * 8) || d_iv.ensure((niv + 1) * sizeof(IvRec)) ||
        d_cnt.ensure(2ull * nr * 4 + 64)) return -11;
    HIPCHK(hipMemcpyAsync(d_regs.p, regs.data(), nr * sizeof(IvRec), hipMemcpyHostToDevice, st));
    if (n_reads > 0) {
        HIPCHK(hipMemcpyAsync(d_rb.p, read_beg, n_reads * 8, hipMemcpyHostToDevice, st)); HIPCHK(hipMemcpyAsync(d_re.p, read_end, n_reads * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off.p, read_iv_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, st));
        if (niv) HIPCHK(hipMemcpyAsync(d_iv.p, read_ivs, niv * sizeof(IvRec), hipMemcpyHostToDevice, st));
    }
    lcd_launch_region_support((const IvRec *)d_regs.p, nr, (const long long *)d_rb.p, (const long long *)d_re.p, (const unsigned long long *)d_off.p, (const IvRec *)d_iv.p, n_reads,
                              (int *)d_cnt.p, (int *)d_cnt.p + nr, st);
    HIPCHK(hipGetLastError());
    std::vector<int> cnt(2 * (size_t)nr);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, 2ull * nr * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    lcd_noisy_iv_t *out = (lcd_noisy_iv_t *)malloc((nr + 1) * sizeof(lcd_noisy_iv_t));
    int n_out = 0;
    for (int i = 0; i < nr; ++i) {
        const int tot = cnt[i], nz = cnt[nr + i];
        if (nz < min_alt_dp || (float)nz / tot < min_af) continue; // (:609-610; 0 / 0 compares false, the first test already dropped it)
        out[n_out].start = (long long)v[i].x; out[n_out].end = v[i].en; out[n_out].label = v[i].label; out[n_out].pad = 0; ++n_out;
    }
    *regs_out = out;
    return n_out;
}

// cr_merge (src/cgranges.c:289-300; cr_cluster0 :225-268) of n labelled intervals: cr_add (negative starts clamped to 0, st > en dropped), cr_index, then passes of
// "from every interval not yet merged, swallow every later one that starts within the window of the running end" until the count stops changing.  Window:
// fixed_merge_win if >= 0 (src/collect_var.c:657 uses 0), else the smaller of the two labels (the dynamic window and its label minimum are not used by the
// reference's code: src/cgranges.c:248-254).  Host code, as in the reference.  *out malloc()'d, index order; returns the number of merged intervals.
int lcd_cr_merge(const lcd_noisy_iv_t *iv, int n, int fixed_merge_win, lcd_noisy_iv_t **out) {
    std::vector<NIv> v;
    for (int i = 0; i < n; ++i) niv_add(v, iv[i].start, iv[i].end, iv[i].label);
    niv_index(v);
    niv_merge(v, fixed_merge_win);
    lcd_noisy_iv_t *o = (lcd_noisy_iv_t *)calloc(v.size() + 1, sizeof(lcd_noisy_iv_t));
    for (size_t i = 0; i < v.size(); ++i) { o[i].start = (int64_t)v[i].x; o[i].end = v[i].en; o[i].label = v[i].label; }
    *out = o;
    return (int)v.size();
}

// post_process_noisy_regs (src/collect_var.c:640-660) -- host glue, see include/lcd_hotpath.h
int lcd_post_process_noisy_regs(const lcd_noisy_iv_t *regs, int n_regs, int n_vars, const int64_t *var_pos, const int *var_ref_len, const int *var_cate,
                                int flank, lcd_noisy_iv_t **regs_out) {
    *regs_out = nullptr;
    if (n_regs <= 0) return 0;
    const int NOT_CAND = 0x800 | 0x001 | 0x002; // LONGCALLD_NOT_CAND_VAR_CATE
    std::vector<NIv> v;
    for (int i = 0; i < n_regs; ++i) niv_add(v, regs[i].start, regs[i].end, regs[i].label);
    niv_index(v);
    const int n = (int)v.size();
    std::vector<int> maxl(n, -1), minr(n, -1);
    auto cand = [&](int vi) { return !(var_cate[vi] & NOT_CAND); };
    for (int ri = 0, vi = 0; ri < n && vi < n_vars;) { // (:488-503) last candidate left of each region, first one right of it
        if (!cand(vi)) { ++vi; continue; }
        const long long vs = var_pos[vi], ve = var_pos[vi] + var_ref_len[vi] - 1, rs = (long long)v[ri].x + 1, re = v[ri].en;
        if (vs > re) { if (minr[ri] == -1) minr[ri] = vi; ++ri; }
        else if (ve < rs) { maxl[ri] = vi; ++vi; }
        else ++vi;
    }
    std::vector<NIv> w;
    for (int ri = 0; ri < n; ++ri) { // (:505-533)
        if (maxl[ri] == -1) maxl[ri] = std::min(n_vars - 1, 0);
        if (minr[ri] == -1) minr[ri] = std::max(0, n_vars - 1);
        long long cs = (long long)v[ri].x + 1 - flank, ce = v[ri].en + flank;
        for (int vi = maxl[ri]; vi >= 0; --vi) {
            if (!cand(vi)) continue;
            const long long vs = var_pos[vi], ve = var_pos[vi] + var_ref_len[vi] - 1;
            if (ve < cs - 1) break;
            if (vs - flank < cs) cs = vs - flank;
        }
        for (int vi = minr[ri]; vi < n_vars; ++vi) {
            if (!cand(vi)) continue;
            const long long vs = var_pos[vi], ve = var_pos[vi] + var_ref_len[vi] - 1;
            if (vs > ce + 1) break;
            if (ve + flank > ce) ce = ve + flank;
        }
        niv_add(w, cs, ce, v[ri].label); // (the reference stores the 1-based start as the interval start here, :648)
    }
    niv_index(w);
    // cr_merge(cr, 0, -1, -1): fixed window 0 -- join while the running end reaches the next start (src/cgranges.c:225-300)
    size_t cur = w.size();
    for (;;) {
        std::vector<NIv> out; std::vector<char> merged(w.size(), 0);
        for (size_t j = 0; j < w.size(); ++j) {
            if (merged[j]) continue;
            uint64_t ms = w[j].x; long long me = w[j].en; int ml = w[j].label;
            for (size_t k = j + 1; k < w.size(); ++k) {
                if (merged[k]) continue;
                if ((uint64_t)me >= w[k].x) { ml = std::max(ml, w[k].label); ms = std::min(ms, w[k].x); me = std::max(me, w[k].en); merged[k] = 1; }
            }
            niv_add(out, (long long)ms, me, ml);
        }
        niv_index(out); w.swap(out);
        if (w.size() == cur) break;
        cur = w.size();
    }
    lcd_noisy_iv_t *o = (lcd_noisy_iv_t *)malloc((w.size() + 1) * sizeof(lcd_noisy_iv_t));
    for (size_t i = 0; i < w.size(); ++i) { o[i].start = (long long)w[i].x; o[i].end = w[i].en; o[i].label = w[i].label; o[i].pad = 0; }
    *regs_out = o;
    return (int)w.size();
}

// sort_noisy_regs (src/collect_var.c:2745-2769): exchange sort by label, then by end - start, with that function's swap sequence (not stable)
int lcd_sort_noisy_regs(const lcd_noisy_iv_t *regs, int n, int *order_out) {
    if (n < 0 || (n > 0 && (!regs || !order_out))) return set_err(-4, "lcd_sort_noisy_regs: bad arguments");
    for (int i = 0; i < n; ++i) order_out[i] = i;
    auto after = [&](int a, int b) { // region a belongs behind region b
        if (regs[a].label != regs[b].label) return regs[a].label > regs[b].label;
        return (int)(regs[a].end - regs[a].start) > (int)(regs[b].end - regs[b].start);
    };
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (after(order_out[i], order_out[j])) std::swap(order_out[i], order_out[j]);
    return 0;
}

} // extern "C"

// the host part of pre_process_noisy_regs in front of the read support (src/collect_var.c:559-568): cr_index, the extension to the overlapping low-complexity
// intervals, cr_merge twice.  v: the chunk's windows in cr_add order.  Shared by lcd_pre_process_noisy_regs and lcd_chunks_first_round.
namespace lcd_internal {
void pre_regs_merge(std::vector<NIv> &v, const int64_t *low_comp, int n_low) {
    niv_index(v);
    if (n_low > 0) { // cr_extend_noisy_regs_with_low_comp / low_comp_cr_start_end (:466-478, :538-551): grow to every overlapping low-complexity interval
        std::vector<NIv> w;
        for (const NIv &a : v) {
            const long long start = (long long)a.x + 1, end = a.en; long long ns = start, ne = end;
            for (int k = 0; k < n_low; ++k) {
                long long ls = low_comp[2 * k] < 0 ? 0 : low_comp[2 * k], le = low_comp[2 * k + 1];
                if (ls > le) continue;
                if (ls < end && start - 1 < le) { if (ls + 1 < ns) ns = ls + 1; if (le > ne) ne = le; }
            }
            niv_add(w, ns - 1, ne, a.label);
        }
        niv_index(w); v.swap(w);
    }
    niv_merge(v); niv_merge(v); // (:552 and :568)
}
} // namespace lcd_internal
