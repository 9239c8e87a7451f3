// lcd_first_round.cpp -- the head of collect_var_main (src/collect_var.c:2897-2945) for a pipeline step's device chunks: read order, is_skipped, low-complexity
// intervals, pre_process_noisy_regs from the chunk handles (read support of all chunks' regions in one launch), the clean-region variants and the first K5 call.
// Ends where lcd_chunks_noisy_rounds (lcd_chunk_vars.cpp) starts.
#include "lcd_host_internal.h"

using namespace lcd_internal;

extern "C" {

void lcd_first_round_free(lcd_first_chunk_t *x) {
    if (!x) return;
    free(x->order); free(x->is_skipped); free(x->low_comp); free(x->pre_regs);
    if (x->vars) { lcd_clean_vars_free(x->vars); free(x->vars); }
    if (x->state) { lcd_hap_state_free(x->state); free(x->state); }
    x->n_reads = x->n_low = x->n_pre_regs = 0; x->order = nullptr; x->is_skipped = nullptr; x->low_comp = nullptr; x->pre_regs = nullptr; x->vars = nullptr; x->state = nullptr;
}

int lcd_chunks_first_round(int n, lcd_first_chunk_t *ch, const lcd_clean_opt_t *opt) {
    const std::string W = "lcd_chunks_first_round";
    if (n <= 0) return n < 0 ? set_err(-4, W + ": n_chunks < 0") : 0;
    if (!ch || !opt) return set_err(-4, W + ": NULL argument");
    for (int c = 0; c < n; ++c) { lcd_first_chunk_t &x = ch[c]; x.n_reads = x.n_low = x.n_pre_regs = 0; x.order = nullptr; x.is_skipped = nullptr; x.low_comp = nullptr; x.pre_regs = nullptr; x.vars = nullptr; x.state = nullptr; }
    if (opt->out_somatic) return set_err(-2, W + ": somatic mode (out_somatic) is not supported");
    // 0. everything that can be checked without the device
    for (int c = 0; c < n; ++c) {
        const lcd_first_chunk_t &x = ch[c];
        const std::string at = W + ": chunk " + std::to_string(c) + ": ";
        if (!x.chunk || !x.ref_seq) return set_err(-4, at + "NULL chunk / ref_seq");
        if (x.chunk->pending) return set_err(-4, at + "the chunk was opened and not resolved (lcd_chunk_resolve)");
        if (x.ref_end < x.ref_beg) return set_err(-4, at + "ref_end < ref_beg");
        if (x.reg_beg < 1 || x.reg_end < x.reg_beg || x.reg_end - x.reg_beg > (1ll << 28)) return set_err(-4, at + "region [reg_beg, reg_end] out of range");
        if (x.chunk->device != ch[0].chunk->device) return set_err(-4, W + ": chunks on different devices");
        const int R = x.chunk->n_reads;
        if (x.ordered_read_ids) {
            std::vector<char> seen(R + 1, 0);
            for (int i = 0; i < R; ++i) {
                const int r = x.ordered_read_ids[i];
                if (r < 0 || r >= R) return set_err(-4, at + "ordered_read_ids out of range");
                if (seen[r]) return set_err(-4, at + "ordered_read_ids names read " + std::to_string(r) + " twice");
                seen[r] = 1;
            }
        } else if (R > 0) {
            const lcd_bam_reads_t *m = x.meta;
            if (!x.chunk->from_bam || !m || m->n_reads != R || !m->pos0 || !m->end_pos || !m->name_off || !m->name_pool)
                return set_err(-4, at + "no ordered_read_ids: the order needs a chunk made from a BAM and its meta (pos0, end_pos, names)");
        }
        if (x.meta && x.meta->n_reads != R) return set_err(-4, at + "meta and chunk disagree on n_reads");
    }
    if (use_device(ch[0].chunk->device)) return -1;
    auto fail = [&](int code) { const std::string m = g_err; for (int c = 0; c < n; ++c) lcd_first_round_free(ch + c); g_err = m; return code; };
    // 1. chunk->ordered_read_ids (sort_chunk_reads) and chunk->is_skipped
    std::vector<std::vector<uint8_t>> rev(n);
    for (int c = 0; c < n; ++c) {
        lcd_first_chunk_t &x = ch[c]; const lcd_chunk_s *k = x.chunk; const int R = k->n_reads;
        x.n_reads = R;
        x.order = (int *)malloc(((size_t)R + 1) * sizeof(int)); x.is_skipped = (uint8_t *)calloc((size_t)R + 1, 1);
        if (!x.order || !x.is_skipped) return fail(set_err(-11, W + ": out of memory"));
        if (x.ordered_read_ids) { if (R) memcpy(x.order, x.ordered_read_ids, (size_t)R * sizeof(int)); }
        else if (R > 0) {
            std::vector<int> nm(R);
            int rc = lcd_chunk_read_nm(k, nm.data());
            if (rc < 0) return fail(rc);
            rc = lcd_sort_chunk_reads(R, x.meta->pos0, x.meta->end_pos, nm.data(), x.meta->name_off, x.meta->name_pool, x.order);
            if (rc < 0) return fail(rc);
        }
        for (int r = 0; r < R; ++r) x.is_skipped[r] = k->status[r] != 0;
        if (!x.is_rev && x.meta && x.meta->flag) { rev[c].resize((size_t)R + 1); for (int r = 0; r < R; ++r) rev[c][r] = (x.meta->flag[r] & 16) != 0; }
    }
    // 2. chunk->low_comp_cr: sdust over the region's window of every chunk, one launch
    {
        std::vector<const uint8_t *> seqs(n); std::vector<int64_t> lens(n), wbeg(n); std::vector<int64_t *> iv(n, nullptr); std::vector<int> cnt(n, 0);
        for (int c = 0; c < n; ++c) {
            const lcd_first_chunk_t &x = ch[c];
            wbeg[c] = std::max(x.reg_beg, x.ref_beg); const int64_t wend = std::min(x.reg_end, x.ref_end);
            lens[c] = wend >= wbeg[c] ? wend - wbeg[c] + 1 : 0; seqs[c] = x.ref_seq + (lens[c] > 0 ? wbeg[c] - x.ref_beg : 0);
        }
        const int rc = lcd_sdust_batch(n, seqs.data(), lens.data(), 5, 20, iv.data(), cnt.data());   // LONGCALLD_SDUST_T / _W (src/call_var_main.h:82-83)
        if (rc < 0) { for (int64_t *p : iv) free(p); return fail(rc); }
        for (int c = 0; c < n; ++c) {
            lcd_first_chunk_t &x = ch[c];
            x.n_low = cnt[c]; x.low_comp = iv[c] ? iv[c] : (int64_t *)calloc(2, sizeof(int64_t));
            for (int i = 0; i < 2 * cnt[c]; ++i) x.low_comp[i] += wbeg[c] - 1;   // cr_add(reg_beg + start - 1, reg_beg + finish - 1) (src/bam_utils.c:1579)
        }
    }
    // 3. pre_process_noisy_regs: host merge per chunk, then the read support of all chunks' regions in one launch
    {
        std::vector<std::vector<NIv>> merged(n);
        std::vector<uint8_t> hb; StagePut put{hb};
        std::vector<SupChunk> sc(n); std::vector<SupReg> sr; std::vector<int> first(n + 1, 0);
        for (int c = 0; c < n; ++c) {
            const lcd_first_chunk_t &x = ch[c]; const lcd_chunk_s *k = x.chunk; const int R = k->n_reads;
            std::vector<NIv> &v = merged[c];
            std::vector<long long> rb, re; std::vector<unsigned long long> off(1, 0); std::vector<IvRec> ivs;
            for (int i = 0; i < R; ++i) {
                const int r = x.order[i];
                if (x.is_skipped[r]) continue;
                rb.push_back(k->beg[r]); re.push_back(k->end[r]);
                for (uint64_t q = k->iv_off[r]; q < k->iv_off[r + 1]; ++q) {
                    const lcd_noisy_iv_t &w = k->ivs[q];
                    IvRec t; t.st = w.start; t.en = w.end; t.label = w.label; t.pad = 0; ivs.push_back(t);
                    if (k->iv_in_chunk[q]) niv_add(v, w.start, w.end, w.label);
                }
                off.push_back(ivs.size());
            }
            if (!v.empty()) pre_regs_merge(v, x.low_comp, x.n_low);
            first[c] = (int)sr.size();
            for (const NIv &a : v) { SupReg g; g.st = (long long)a.x; g.en = a.en; g.chunk = c; g.pad = 0; sr.push_back(g); }
            SupChunk &s = sc[c]; s.n_reads = (int)rb.size(); s.pad = 0;
            s.read_beg = put(rb.data(), rb.size() * 8); s.read_end = put(re.data(), re.size() * 8); s.iv_off = put(off.data(), off.size() * 8); s.ivs = put(ivs.data(), ivs.size() * sizeof(IvRec));
        }
        first[n] = (int)sr.size();
        const int nr = (int)sr.size();
        std::vector<int> cntv(2 * (size_t)nr + 1, 0);
        if (nr > 0) {
            const uint64_t o_sc = put(sc.data(), (size_t)n * sizeof(SupChunk)), o_sr = put(sr.data(), (size_t)nr * sizeof(SupReg));
            StreamGuard st; if (st.create()) return fail(-10);
            DevBuf d_in, d_cnt;
            if (d_in.ensure(hb.size() + 64) || d_cnt.ensure(2ull * nr * 4 + 64)) return fail(-11);
            SupChunk *hsc = (SupChunk *)(hb.data() + o_sc);
            for (int c = 0; c < n; ++c) { hsc[c].read_beg += d_in.addr(); hsc[c].read_end += d_in.addr(); hsc[c].iv_off += d_in.addr(); hsc[c].ivs += d_in.addr(); }
#define FRCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { (void)hipGetLastError(); return fail(set_err(-10, std::string(#x) + ": " + hipGetErrorString(e_))); } } while (0)
            FRCHK(hipMemcpyAsync(d_in.p, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
            lcd_launch_region_support_batch((const SupChunk *)((const uint8_t *)d_in.p + o_sc), (const SupReg *)((const uint8_t *)d_in.p + o_sr), nr, (int *)d_cnt.p, (int *)d_cnt.p + nr, st);
            FRCHK(hipGetLastError());
            FRCHK(hipMemcpyAsync(cntv.data(), d_cnt.p, 2ull * nr * 4, hipMemcpyDeviceToHost, st));
            FRCHK(hipStreamSynchronize(st));
#undef FRCHK
        }
        for (int c = 0; c < n; ++c) {
            lcd_first_chunk_t &x = ch[c]; const std::vector<NIv> &v = merged[c];
            x.pre_regs = (lcd_noisy_iv_t *)calloc(v.size() + 1, sizeof(lcd_noisy_iv_t));
            if (!x.pre_regs) return fail(set_err(-11, W + ": out of memory"));
            int m = 0;
            for (size_t i = 0; i < v.size(); ++i) {
                const int tot = cntv[first[c] + i], nz = cntv[nr + first[c] + i];
                if (nz < opt->min_alt_dp || (float)nz / tot < (float)opt->min_af) continue;   // (:609-610; 0 / 0 compares false, the first test already dropped it)
                x.pre_regs[m].start = (long long)v[i].x; x.pre_regs[m].end = v[i].en; x.pre_regs[m].label = v[i].label; x.pre_regs[m].pad = 0; ++m;
            }
            x.n_pre_regs = m;
        }
    }
    // 4. the clean-region variants of all chunks
    {
        std::vector<const lcd_chunk_t *> cs(n); std::vector<const int *> ord(n); std::vector<const uint8_t *> rv(n), refs(n); std::vector<int64_t> rb(n), re(n), gb(n), ge(n);
        std::vector<const lcd_noisy_iv_t *> pre(n); std::vector<int> npre(n), nlow(n); std::vector<const int64_t *> low(n);
        std::vector<lcd_clean_vars_t> outs(n);
        for (int c = 0; c < n; ++c) {
            const lcd_first_chunk_t &x = ch[c];
            cs[c] = x.chunk; ord[c] = x.order; rv[c] = x.is_rev ? x.is_rev : rev[c].empty() ? nullptr : rev[c].data(); refs[c] = x.ref_seq; rb[c] = x.ref_beg; re[c] = x.ref_end;
            gb[c] = x.reg_beg; ge[c] = x.reg_end; pre[c] = x.pre_regs; npre[c] = x.n_pre_regs; low[c] = x.low_comp; nlow[c] = x.n_low;
            memset(&outs[c], 0, sizeof(lcd_clean_vars_t));
        }
        const int rc = lcd_chunk_clean_vars_batch(n, cs.data(), opt, ord.data(), rv.data(), refs.data(), rb.data(), re.data(), gb.data(), ge.data(), pre.data(), npre.data(), low.data(),
                                                  nlow.data(), outs.data());
        if (rc) return fail(rc);   // (the batch freed its outputs)
        for (int c = 0; c < n; ++c) {
            ch[c].vars = (lcd_clean_vars_t *)malloc(sizeof(lcd_clean_vars_t));
            if (!ch[c].vars) { for (int q = c; q < n; ++q) lcd_clean_vars_free(&outs[q]); return fail(set_err(-11, W + ": out of memory")); }
            *ch[c].vars = outs[c];
        }
    }
    // 5. K5's state; one K5 launch over the clean categories for the chunks that have a variant (src/collect_var.c:2934-2944)
    std::vector<int> K;
    for (int c = 0; c < n; ++c) {
        lcd_first_chunk_t &x = ch[c];
        x.state = (lcd_hap_state_t *)calloc(1, sizeof(lcd_hap_state_t));
        if (!x.state) return fail(set_err(-11, W + ": out of memory"));
        const int rc = lcd_hap_state_init(x.vars->n_reads, x.vars->n_vars, x.state);
        if (rc) return fail(rc);
        if (x.vars->n_vars > 0) K.push_back(c);
    }
    if (!K.empty()) {
        const int nk = (int)K.size();
        std::vector<lcd_hap_problem_t> probs(nk); std::vector<std::vector<int>> alle_off(nk), allele_off(nk);
        std::vector<int> targets(nk, 0x004 | 0x008 | 0x080);   // LONGCALLD_CLEAN_HET_SNP | LONGCALLD_CLEAN_HET_INDEL | LONGCALLD_CLEAN_HOM_VAR (src/collect_var.h)
        for (int q = 0; q < nk; ++q) {
            lcd_first_chunk_t &x = ch[K[q]];
            memset(&probs[q], 0, sizeof(lcd_hap_problem_t));
            alle_off[q].resize(x.vars->n_vars + 1); allele_off[q].resize(x.vars->n_reads + 1);
            lcd_clean_vars_hap_problem(x.vars, x.is_ont, x.order, x.is_skipped, alle_off[q].data(), allele_off[q].data(), &probs[q]);
            lcd_hap_problem_t &p = probs[q]; const lcd_hap_state_t &s = *x.state;
            p.haps = s.haps; p.phase_sets = s.phase_sets; p.n_clean_agree_snps = s.n_clean_agree_snps; p.n_clean_conflict_snps = s.n_clean_conflict_snps;
            p.var_phase_set = s.var_phase_set; p.hap_to_cons_alle = s.hap_to_cons_alle; p.hap_to_alle_profile = s.hap_to_alle_profile;
        }
        const int rc = lcd_assign_hap_batch(nk, probs.data(), targets.data());
        if (rc) return fail(rc);
    }
    return 0;
}

} // extern "C"
