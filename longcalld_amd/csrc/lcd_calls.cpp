// lcd_calls.cpp -- the per-call entry points of liblcd_hotpath.so: sdust, the K5 phasing batch and the one-pair mirrors of src/align.h.  Each call brings its
// own stream and buffers; the alignment mirrors go through lcd_edlib_batch / lcd_wfa_batch and the region-batch ABI of lcd_host.cpp.
#include "lcd_host_internal.h"

using namespace lcd_internal;

extern "C" {

// ---- sdust on the device (sdust_kernel.hip): segments on lanes, each reports what the automaton saves at its steps, the host chains the lists with sdust's merge rule ----
// lcd_sdust_batch: the references of MANY chunks in one launch.  A lane's automaton is serial and latency-bound (21 ms for one 500 kb chunk against 9 ms
// for the reference's sdust() on one core), but the chip holds ~60 000 lanes: the chunk workers' references of one pipeline step go in together.
int lcd_sdust_batch(int n_seqs, const uint8_t *const *seqs, const int64_t *lens, int T, int W, int64_t **intervals_out, int *n_out) {
    for (int q = 0; q < n_seqs; ++q) { intervals_out[q] = nullptr; n_out[q] = 0; }
    if (ensure_init()) return -1;
    if (n_seqs <= 0) return 0;
    if (W > 64 || W < 4) return set_err(-4, "lcd_sdust: W must be in [4, 64]");
    // segment length: the automaton is serial inside a segment (plus ~3W bases of lead-in), so short segments = more lanes, less latency
    const int seg = W <= 32 ? 128 : 256, cap = seg + 8;
    auto code = [](uint8_t c) { return c < 4 ? (int)c : (c == 'A' || c == 'a') ? 0 : (c == 'C' || c == 'c') ? 1 : (c == 'G' || c == 'g') ? 2 : (c == 'T' || c == 't') ? 3 : 4; };
    std::vector<SdSeg> segs; std::vector<size_t> first(n_seqs + 1, 0);
    uint64_t pool_bytes = 0;
    for (int q = 0; q < n_seqs; ++q) {
        first[q] = segs.size();
        if (lens[q] <= 0) continue;
        if (lens[q] > 2000000000ll) return set_err(-4, "lcd_sdust: sequences below 2 Gb");
        const int len = (int)lens[q], n_seg = (len + seg - 1) / seg;
        const uint8_t *seq = seqs[q];
        // where each segment's automaton starts: W + 4 triplet words before (segment start - 2W); a word ends at i when i-2..i are all A/C/G/T
        // (why that is enough: the header of sdust_kernel.hip; tests/sdust_model.py lane_starts is the same count)
        std::vector<int> ring(W + 4, -1); size_t rn = 0; // ring of the last W+4 word-end positions
        int l = 0, next = 0;
        std::vector<int> from(n_seg, 0);
        for (int i = 0; i < len && next < n_seg; ++i) {
            while (next < n_seg && std::max(0, next * seg - 2 * W) == i) { from[next] = rn >= ring.size() ? std::max(0, ring[rn % ring.size()] - 2) : 0; ++next; }
            if (code(seq[i]) < 4) { if (++l >= 3) { ring[rn % ring.size()] = i; ++rn; } } else l = 0;
        }
        for (int k = 0; k < n_seg; ++k) { SdSeg sg; sg.seq_off = pool_bytes; sg.len = len; sg.a = k * seg; sg.from = from[k]; sg.pad = 0; segs.push_back(sg); }
        pool_bytes += lcd_align_up((uint64_t)len + 16, 16);
    }
    first[n_seqs] = segs.size();
    const size_t n_seg = segs.size();
    if (n_seg == 0) return 0;
    // (grow-only buffers and one stream kept across calls: five hipMalloc / hipFree pairs cost more than the kernel)
    static std::mutex mu; std::lock_guard<std::mutex> lk(mu);
    static hipStream_t st[LCD_MAX_DEV] = {};
    static DevBuf d_seq[LCD_MAX_DEV], d_segs[LCD_MAX_DEV], d_n[LCD_MAX_DEV], d_out[LCD_MAX_DEV], d_p[LCD_MAX_DEV];
    const int dv = cur_device();
    if (!st[dv]) HIPCHK(hipStreamCreateWithFlags(&st[dv], hipStreamNonBlocking));
    const int pcap = W * W + 8;
    if (d_seq[dv].ensure(pool_bytes + 64) || d_segs[dv].ensure(n_seg * sizeof(SdSeg)) || d_n[dv].ensure(n_seg * 4) || d_out[dv].ensure(n_seg * (size_t)cap * 8) ||
        d_p[dv].ensure(n_seg * (size_t)pcap * 16)) return -11;
    { uint64_t o = 0; for (int q = 0; q < n_seqs; ++q) if (lens[q] > 0) { HIPCHK(hipMemcpyAsync((uint8_t *)d_seq[dv].p + o, seqs[q], (size_t)lens[q], hipMemcpyHostToDevice, st[dv])); o += lcd_align_up((uint64_t)lens[q] + 16, 16); } }
    HIPCHK(hipMemcpyAsync(d_segs[dv].p, segs.data(), n_seg * sizeof(SdSeg), hipMemcpyHostToDevice, st[dv]));
    lcd_launch_sdust((const unsigned char *)d_seq[dv].p, (const SdSeg *)d_segs[dv].p, T, W, seg, (int)n_seg, cap, (int *)d_n[dv].p, (int2 *)d_out[dv].p, (int4 *)d_p[dv].p, pcap, st[dv]);
    HIPCHK(hipGetLastError());
    std::vector<int> n(n_seg); std::vector<int> raw(n_seg * (size_t)cap * 2);
    HIPCHK(hipMemcpyAsync(n.data(), d_n[dv].p, n_seg * 4, hipMemcpyDeviceToHost, st[dv]));
    HIPCHK(hipMemcpyAsync(raw.data(), d_out[dv].p, n_seg * (size_t)cap * 8, hipMemcpyDeviceToHost, st[dv]));
    HIPCHK(hipStreamSynchronize(st[dv]));
    for (int q = 0; q < n_seqs; ++q) {
        std::vector<int64_t> res; // save_masked_regions' merge (src/sdust.c:93-98) over the lanes' lists in lane order = the order of the automaton's saves
        for (size_t s = first[q]; s < first[q + 1]; ++s) {
            if (n[s] < 0 || n[s] > cap) return set_err(-24, "lcd_sdust: per-segment capacity exceeded (sequence " + std::to_string(q) + ", segment " + std::to_string(s - first[q]) + ": " + std::to_string(n[s]) + ")");
            for (int k = 0; k < n[s]; ++k) {
                const int64_t ps = raw[(s * cap + k) * 2], pf = raw[(s * cap + k) * 2 + 1];
                if (!res.empty() && ps <= res.back()) { if (pf > res.back()) res.back() = pf; }
                else { res.push_back(ps); res.push_back(pf); }
            }
        }
        int64_t *out = (int64_t *)malloc((res.size() + 2) * sizeof(int64_t));
        memcpy(out, res.data(), res.size() * sizeof(int64_t));
        intervals_out[q] = out; n_out[q] = (int)(res.size() / 2);
    }
    return 0;
}
int lcd_sdust(const uint8_t *seq, int64_t len, int T, int W, int64_t **intervals_out) {
    int n = 0;
    const int rc = lcd_sdust_batch(1, &seq, &len, T, W, intervals_out, &n);
    return rc ? rc : n;
}

// ---------------------------------------------------------------------------------------------------
// K5
int lcd_assign_hap_batch(int n, lcd_hap_problem_t *probs, const int *targets) {
    if (ensure_init()) return -1;
    if (n <= 0) return 0;
    StreamGuard st; if (st.create()) return -10;
    std::vector<uint8_t> hb; // host staging; offsets become device addresses
    StagePut put{hb};
    struct Off { uint64_t var_pos, var_type, var_cate, is_hp, total_cov, alle_off, alle_covs, start_var, end_var, allele_off, alleles, ordered, cr_read, is_skipped,
                 haps, phase_sets, agree, conflict, var_ps, cons, prof, valid, vii, het, is_het, n_agree, n_conflict, cur_cons, flags; };
    std::vector<Off> offs(n);
    for (int i = 0; i < n; ++i) {
        const lcd_hap_problem_t &p = probs[i]; Off &o = offs[i];
        const int R = p.n_reads, V = p.n_vars, TA = V ? p.alle_off[V] : 0, NA = R ? p.allele_off[R] : 0;
        o.var_pos = put(p.var_pos, (size_t)V * 8); o.var_type = put(p.var_type, (size_t)V * 4); o.var_cate = put(p.var_cate, (size_t)V * 4);
        o.is_hp = put(p.is_homopolymer_indel, (size_t)V * 4); o.total_cov = put(p.total_cov, (size_t)V * 4);
        o.alle_off = put(p.alle_off, (size_t)(V + 1) * 4); o.alle_covs = put(p.alle_covs, (size_t)TA * 4);
        o.start_var = put(p.start_var_idx, (size_t)R * 4); o.end_var = put(p.end_var_idx, (size_t)R * 4);
        o.allele_off = put(p.allele_off, (size_t)(R + 1) * 4); o.alleles = put(p.alleles, (size_t)NA * 4);
        o.ordered = put(p.ordered_read_ids, (size_t)R * 4); o.cr_read = put(p.cr_read, (size_t)p.n_cr * 4); o.is_skipped = put(p.is_skipped, (size_t)R);
        o.haps = put(p.haps, (size_t)R * 4); o.phase_sets = put(p.phase_sets, (size_t)R * 8);
        o.agree = put(p.n_clean_agree_snps, (size_t)R * 4); o.conflict = put(p.n_clean_conflict_snps, (size_t)R * 4);
        o.var_ps = put(p.var_phase_set, (size_t)V * 8); o.cons = put(p.hap_to_cons_alle, (size_t)V * 3 * 4); o.prof = put(p.hap_to_alle_profile, (size_t)TA * 3 * 4);
        o.valid = put(nullptr, (size_t)V * 4); o.vii = put(nullptr, (size_t)V * 4); o.het = put(nullptr, (size_t)V * 4); o.is_het = put(nullptr, (size_t)V * 4);
        o.n_agree = put(nullptr, (size_t)V * 4); o.n_conflict = put(nullptr, (size_t)V * 4); o.cur_cons = put(nullptr, (size_t)V * 2 * 4); o.flags = put(nullptr, 64);
    }
    DevBuf d_buf, d_probs;
    if (d_buf.ensure(hb.size() + 64) || d_probs.ensure(n * sizeof(HapProb))) return -11;
    HIPCHK(hipMemcpyAsync(d_buf.p, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
    std::vector<HapProb> hp(n);
    const uint64_t B = d_buf.addr();
    for (int i = 0; i < n; ++i) {
        const lcd_hap_problem_t &p = probs[i]; const Off &o = offs[i]; HapProb &q = hp[i];
        q.n_reads = p.n_reads; q.n_vars = p.n_vars; q.is_ont = p.is_ont; q.n_cr = p.n_cr; q.total_alle = p.n_vars ? p.alle_off[p.n_vars] : 0; q.target = targets[i];
#define DP(T, f) (T)(uintptr_t)(B + o.f)
        q.var_pos = DP(const long long *, var_pos); q.var_type = DP(const int *, var_type); q.var_cate = DP(const int *, var_cate); q.is_hp = DP(const int *, is_hp);
        q.total_cov = DP(const int *, total_cov); q.alle_off = DP(const int *, alle_off); q.alle_covs = DP(const int *, alle_covs);
        q.start_var = DP(const int *, start_var); q.end_var = DP(const int *, end_var); q.allele_off = DP(const int *, allele_off); q.alleles = DP(const int *, alleles);
        q.ordered = DP(const int *, ordered); q.cr_read = DP(const int *, cr_read); q.is_skipped = DP(const uint8_t *, is_skipped);
        q.haps = DP(int *, haps); q.phase_sets = DP(long long *, phase_sets); q.n_agree_snps = DP(int *, agree); q.n_conflict_snps = DP(int *, conflict);
        q.var_ps = DP(long long *, var_ps); q.cons = DP(int *, cons); q.prof = DP(int *, prof);
        q.valid = DP(int *, valid); q.vii = DP(int *, vii); q.het = DP(int *, het); q.is_het = DP(int *, is_het); q.n_agree = DP(int *, n_agree); q.n_conflict = DP(int *, n_conflict);
        q.cur_cons = DP(int *, cur_cons); q.flags = DP(int *, flags);
#undef DP
    }
    HIPCHK(hipMemcpyAsync(d_probs.p, hp.data(), n * sizeof(HapProb), hipMemcpyHostToDevice, st));
    lcd_launch_hap((const HapProb *)d_probs.p, n, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hb.data(), d_buf.p, hb.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        lcd_hap_problem_t &p = probs[i]; const Off &o = offs[i];
        const int R = p.n_reads, V = p.n_vars, TA = V ? p.alle_off[V] : 0;
        memcpy(p.haps, hb.data() + o.haps, (size_t)R * 4); memcpy(p.phase_sets, hb.data() + o.phase_sets, (size_t)R * 8);
        memcpy(p.n_clean_agree_snps, hb.data() + o.agree, (size_t)R * 4); memcpy(p.n_clean_conflict_snps, hb.data() + o.conflict, (size_t)R * 4);
        memcpy(p.var_phase_set, hb.data() + o.var_ps, (size_t)V * 8); memcpy(p.hap_to_cons_alle, hb.data() + o.cons, (size_t)V * 3 * 4);
        memcpy(p.hap_to_alle_profile, hb.data() + o.prof, (size_t)TA * 3 * 4);
    }
    return 0;
}
int lcd_assign_hap_germline(lcd_hap_problem_t *p, int target_var_cate) { return lcd_assign_hap_batch(1, p, &target_var_cate); }

// ---------------------------------------------------------------------------------------------------
// per-call mirrors of src/align.h
int lcd_wfa_end2end_aln(uint8_t *pattern, int plen, uint8_t *text, int tlen, int gap_aln, int b, int q, int e, int q2, int e2, int heuristic,
                        int affine_gap, uint32_t **cigar_buf, int *cigar_length, uint8_t **pattern_alg, uint8_t **text_alg, int *alg_length) {
    if (heuristic != 0 || affine_gap != 1) return set_err(-2, "only heuristic=NONE, affine_gap=2P (the germline-live WFA configuration) is implemented");
    std::vector<uint8_t> pool((size_t)plen + tlen + 32, 4);
    if (plen) memcpy(pool.data(), pattern, plen);
    const uint64_t toff = lcd_align_up(plen, 16);
    pool.resize(toff + tlen + 16, 4);
    if (tlen) memcpy(pool.data() + toff, text, tlen);
    const uint64_t po = 0; const int want = ((cigar_buf && cigar_length) ? 1 : 0) | ((pattern_alg && text_alg) ? 2 : 0);
    const int maxl = plen + tlen + 1;
    std::vector<uint32_t> cig(maxl); std::vector<uint8_t> rows(2 * (size_t)maxl);
    int score = 0, nc = 0, al = 0;
    int rc = lcd_wfa_batch(1, pool.data(), pool.size(), &po, &plen, &toff, &tlen, &gap_aln, b, q, e, q2, e2, want, &score, cig.data(), maxl, &nc, rows.data(), maxl, &al);
    if (rc) return rc;
    if (want & 1) { *cigar_buf = (uint32_t *)malloc((nc > 0 ? nc : 1) * sizeof(uint32_t)); memcpy(*cigar_buf, cig.data(), (size_t)nc * 4); *cigar_length = nc; }
    if (want & 2) {
        uint8_t *mem = (uint8_t *)calloc(2 * (size_t)maxl, 1); // src/align.c:288-291
        memcpy(mem, rows.data(), al); memcpy(mem + maxl, rows.data() + maxl, al);
        *pattern_alg = mem; *text_alg = mem + maxl; *alg_length = al;
    }
    return 0;
}

// end2end_aln (src/align.c:610-628): target given as letters, mapped with nst_nt4_table (src/seq.c:14-31: ACGT / acgt -> 0..3, '-' -> 5, else 4;
// the bytes 0..3 map to themselves), then the 2-piece WFA with opt's penalties; returns the CIGAR length, *cigar_buf malloc()'d
int lcd_end2end_aln(const lcd_opt_t *opt, char *tseq, int tlen, uint8_t *qseq, int qlen, uint32_t **cigar_buf) {
    if (qlen <= 0 || tlen <= 0) return 0;
    std::vector<uint8_t> t2((size_t)tlen);
    for (int i = 0; i < tlen; ++i) {
        const uint8_t c = (uint8_t)tseq[i];
        t2[i] = c < 4 ? c : (c == 'A' || c == 'a') ? 0 : (c == 'C' || c == 'c') ? 1 : (c == 'G' || c == 'g') ? 2 : (c == 'T' || c == 't') ? 3 : c == '-' ? 5 : 4;
    }
    int cigar_len = 0;
    const int rc = lcd_wfa_end2end_aln(t2.data(), tlen, qseq, qlen, opt->gap_aln, opt->mismatch, opt->gap_open1, opt->gap_ext1, opt->gap_open2, opt->gap_ext2, 0, 1,
                                       cigar_buf, &cigar_len, nullptr, nullptr, nullptr);
    return rc < 0 ? rc : cigar_len;
}
// wfa_collect_diff_ins_seq (src/align.c:463-494): align large vs small, return the longest run of large-only columns (first one on ties)
int lcd_wfa_collect_diff_ins_seq(const lcd_opt_t *opt, uint8_t *large_seq, int large_len, uint8_t *small_seq, int small_len, uint8_t **diff_seq) {
    uint8_t *la = nullptr, *sa = nullptr; int aln_len = 0;
    const int rc = lcd_wfa_end2end_aln(large_seq, large_len, small_seq, small_len, opt->gap_aln, opt->mismatch, opt->gap_open1, opt->gap_ext1, opt->gap_open2, opt->gap_ext2, 0, 1,
                                       nullptr, nullptr, &la, &sa, &aln_len);
    if (rc < 0) return rc;
    int best_len = 0, best_pos = -1;
    for (int i = 0; i < aln_len; ++i) {
        if (sa[i] == 5 && la[i] != 5) {
            int j = i; while (j < aln_len && sa[j] == 5 && la[j] != 5) ++j;
            if (j - i > best_len) { best_len = j - i; best_pos = i; }
            i = j - 1;
        }
    }
    if (best_len > 0) { *diff_seq = (uint8_t *)malloc((size_t)best_len); memcpy(*diff_seq, la + best_pos, (size_t)best_len); }
    free(la);
    return best_len;
}
// The two exports of src/align.h that the germline path never reaches (edlib_infix_aln is only called from somatic-mode code,
// wfa_heuristic_aln has no caller at all): present so that a longcallD built against this library links, and loud when reached
// edlib_infix_aln (src/align.c:256-275): edlib's HW mode with the path -- a somatic-mode (-s) call in longcallD, implemented and pinned to the reference's own edlib
// (tests/golden/edlib_golden.json, hw_cases).  Returns the edit distance, -1 on error; *n_eq / *n_xid from the path as edlibAlignmentToXID counts them.
int lcd_edlib_infix_aln(uint8_t *target, int tlen, uint8_t *query, int qlen, int *n_eq, int *n_xid) {
    std::vector<uint8_t> pool((size_t)lcd_align_up(qlen, 16) + tlen + 32, 4);
    if (qlen) memcpy(pool.data(), query, qlen);
    const uint64_t qo = 0, to = lcd_align_up(qlen, 16);
    if (tlen) memcpy(pool.data() + to, target, tlen);
    int d, x, a, c, s0, e0;
    if (lcd_edlib_batch_hw(1, pool.data(), pool.size(), &qo, &qlen, &to, &tlen, &d, &x, &a, &c, &s0, &e0)) { if (n_eq) *n_eq = -1; if (n_xid) *n_xid = -1; return -1; }
    if (n_eq && n_xid) { *n_eq = a; *n_xid = c; }
    return d;
}
// The export of src/align.h that has no caller at all in longcallD: present so that a longcallD built against this library links, and loud when reached
int lcd_wfa_heuristic_aln(uint8_t *, int, uint8_t *, int, int, int, int, int, int, int, int *n_eq, int *n_xid) {
    if (n_eq) *n_eq = -1; if (n_xid) *n_xid = -1;
    fprintf(stderr, "liblcd_hotpath: wfa_heuristic_aln (x-drop WFA, src/align.c:332) has no caller in longcallD and is not implemented\n");
    return set_err(-2, "wfa_heuristic_aln (x-drop heuristic) is not implemented");
}

static int ed1(uint8_t *target, int tlen, uint8_t *query, int qlen, int *dist, int *xg, int *neq, int *nxid) {
    std::vector<uint8_t> pool((size_t)lcd_align_up(qlen, 16) + tlen + 32, 4);
    if (qlen) memcpy(pool.data(), query, qlen);
    const uint64_t qo = 0, to = lcd_align_up(qlen, 16);
    if (tlen) memcpy(pool.data() + to, target, tlen);
    return lcd_edlib_batch(1, pool.data(), pool.size(), &qo, &qlen, &to, &tlen, dist, xg, neq, nxid);
}
int lcd_edlib_end2end_aln(uint8_t *target, int tlen, uint8_t *query, int qlen, int *n_eq, int *n_xid) {
    int d, x, a, c; if (ed1(target, tlen, query, qlen, &d, &x, &a, &c)) return -1;
    if (n_eq && n_xid) { *n_eq = a; *n_xid = c; }
    return d;
}
int lcd_edlib_xgaps(uint8_t *target, int tlen, uint8_t *query, int qlen) { int d, x, a, c; if (ed1(target, tlen, query, qlen, &d, &x, &a, &c)) return -1; return x; }
int lcd_edlib_edit_distance(uint8_t *target, int tlen, uint8_t *query, int qlen) { int d, x, a, c; if (ed1(target, tlen, query, qlen, &d, &x, &a, &c)) return -1; return d; }

int lcd_collect_noisy_reg_aln_strs(const lcd_opt_t *opt, const lcd_read_view_t *chunk_reads, int64_t noisy_reg_beg, int64_t noisy_reg_end, int noisy_reg_i,
                                   int n, int *noisy_reads, const uint8_t *ref_seq, int ref_seq_len, int *clu_n_seqs, int **clu_read_ids, lcd_aln_str_t **aln_strs) {
    (void)noisy_reg_i;
    if (n <= 0) return 0;
    lcd_batch_t *b = lcd_batch_create(opt);
    if (!b) return -1;
    int rc = lcd_batch_add_region_from_chunk(b, chunk_reads, noisy_reg_beg, noisy_reg_end, n, noisy_reads, ref_seq, ref_seq_len);
    if (rc < 0) { lcd_batch_destroy(b); return rc; }
    if ((rc = lcd_batch_upload(b)) || (rc = lcd_batch_run(b)) || (rc = lcd_batch_download(b))) { lcd_batch_destroy(b); return rc; }
    lcd_batch_region_sorted_ids(b, 0, noisy_reads);
    int nc = lcd_batch_region_result(b, 0, clu_n_seqs, clu_read_ids, aln_strs);
    lcd_batch_destroy(b);
    return nc;
}

} // extern "C"
