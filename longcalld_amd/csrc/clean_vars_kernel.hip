// clean_vars_kernel.hip -- the first round of collect_var_main (src/collect_var.c:2897-2980, steps 1.2 - 3.1) on a device-resident chunk (lcd_chunk_t):
// the chunk's digars, 4-bit bases and qualities are read where lcd_chunk_create[_from_bam] left them in HBM.
//   sites     collect_all_cand_var_sites (:1209-1253): per read its collectible digars (is_collectible_var_digar :1152), compacted by a prefix sum
//             over the reads; sorted by comp_var_site_for_sort (= exact_comp_var_site :1878) as a counting sort on the site's position key
//             (pos for X, pos - 1 otherwise; 64 keys per bucket) followed by a rank sort inside each bucket (the order is total, ties only between identical records,
//             which are ranked by input order); deduplicated against the LAST KEPT record with exact_comp_var_site_ins (:1901), one lane per bucket
//   pile-up   update_cand_vars_from_digar (src/bam_utils.c:287-327): one lane per read, integer atomics on the coverage counters
//   classify  classify_var_cate (:413-435) with var_is_homopolymer / var_is_repeat_region (:306-405) on the chunk's reference, except the ONT
//             strand-bias test (host, double precision, src/collect_var.c:270)
//   ratios    var_noisy_reads_ratio (:717-747): the per-read error intervals of build_var_noisy_reads_ratio_cache (:662-715), then one lane per query
//   profile   update_read_vs_all_var_profile_from_digar (src/bam_utils.c:446-549, germline branch): one lane per read, twice (spans, then alleles)
// Every lane reads only inside its read's digars / bases / qualities (query offsets checked against qlen) and the reference inside [ref_beg, ref_end].
#include <hip/hip_runtime.h>
#include "lcd_types.h"
#include "lcd_kernels.h"

namespace {
constexpr int CV_T = 256;
constexpr int CV_BSHIFT = 6; // a sort bucket holds 64 consecutive position keys: bounded histogram and scan, small buckets for the rank sort
constexpr int CDIFF = 8, CINS = 1, CDEL = 2, CEQUAL = 7;
constexpr int LOW_COV_VAR = 0x001, LOW_AF_VAR = 0x400, CLEAN_HET_SNP = 0x004, CLEAN_HET_INDEL = 0x008, REP_HET_VAR = 0x010, CLEAN_HOM_VAR = 0x080, NON_VAR = 0x800;

__device__ __forceinline__ int cv_base(const CvRead &r, int i) { // seq_nt16_int[bam_seqi(bseq, i)]; past the record: N
    if (i < 0 || i >= r.qlen) return 4;
    const unsigned b = ((const unsigned char *)r.seq)[i >> 1];
    const unsigned c = (b >> ((~i & 1) << 2)) & 0xf;
    return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 8 ? 3 : 4;
}
__device__ __forceinline__ int cv_alt_cmp(const CvSite &a, const CvSite &b, const CvRead *reads, int len) { // memcmp over alt_seq codes 0-4
    const CvRead ra = reads[a.read], rb = reads[b.read];
    for (int k = 0; k < len; ++k) { const int x = cv_base(ra, a.qi + k), y = cv_base(rb, b.qi + k); if (x != y) return x - y; }
    return 0;
}
__device__ __forceinline__ long long cv_key(const CvSite &s) { return s.var_type == CDIFF ? s.pos : s.pos - 1; }
__device__ __forceinline__ CvSite cv_site(int read, const DigarRec &d) { // make_var_site_from_digar (src/collect_var.c:1113)
    CvSite s; s.pos = d.pos; s.var_type = d.type; s.ref_len = 1; s.alt_len = d.len; s.read = read; s.qi = d.qi; s.pad = 0;
    if (d.type == CINS) s.ref_len = 0;
    else if (d.type == CDEL) { s.ref_len = d.len; s.alt_len = 0; }
    return s;
}
__device__ int cv_exact(const CvSite &a, const CvSite &b, const CvRead *reads) { // exact_comp_var_site
    const long long p1 = cv_key(a), p2 = cv_key(b);
    if (p1 != p2) return p1 < p2 ? -1 : 1;
    if (a.var_type != b.var_type) return a.var_type < b.var_type ? -1 : 1;
    if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len ? -1 : 1;
    if (a.alt_len != b.alt_len) return a.alt_len < b.alt_len ? -1 : 1;
    if (a.var_type == CDIFF || a.var_type == CINS) return cv_alt_cmp(a, b, reads, a.alt_len);
    return 0;
}
__device__ int cv_exact_ins(const CvSite &a, const CvSite &b, const CvRead *reads, int min_sv_len) { // exact_comp_var_site_ins
    const long long p1 = cv_key(a), p2 = cv_key(b);
    if (p1 != p2) return p1 < p2 ? -1 : 1;
    if (a.var_type != b.var_type) return a.var_type < b.var_type ? -1 : 1;
    if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len ? -1 : 1;
    if (a.var_type == CDIFF || (a.var_type == CINS && a.alt_len < min_sv_len)) {
        if (a.alt_len != b.alt_len) return a.alt_len < b.alt_len ? -1 : 1;
        return cv_alt_cmp(a, b, reads, a.alt_len);
    }
    if (a.var_type == CINS) {
        const int mn = min(a.alt_len, b.alt_len), mx = max(a.alt_len, b.alt_len);
        if (mn >= mx * 0.8) return 0;
        return a.alt_len - b.alt_len;
    }
    return 0;
}
__device__ __forceinline__ int cv_ovlp(const CvSite &a, const CvSite &b) { // ovlp_var_site (src/collect_var.c:79)
    const int b1 = (int)a.pos, e1 = (int)(a.pos + a.ref_len), b2 = (int)b.pos, e2 = (int)(b.pos + b.ref_len);
    if (a.ref_len == 0 && b.ref_len == 0) return b1 == b2;
    if (a.ref_len == 0) return b1 > b2 && e1 < e2;
    if (b.ref_len == 0) return b2 > b1 && e2 < e1;
    return !(b1 >= e2 || b2 >= e1);
}
__device__ __forceinline__ int cv_collectible(const DigarRec &d, long long reg_beg, long long reg_end) {
    if (d.pos < reg_beg || d.pos > reg_end || d.is_low_qual) return 0;
    return d.type == CDIFF || d.type == CINS || d.type == CDEL;
}
__device__ int cv_start(const CvSite *v, int n, long long start) { // get_var_site_start / get_var_start (src/bam_utils.c:202-226)
    const long long target = start > 0 ? start - 1 : start;
    int left = 0, right = n;
    while (left < right) { const int mid = left + (right - left) / 2; if (cv_key(v[mid]) < target) left = mid + 1; else right = mid; }
    while (left < n && v[left].pos < start) left++;
    return left;
}
__device__ int cv_ave_qual(const CvRead &r, const DigarRec &d) { // get_digar_ave_qual (src/bam_utils.c:258)
    if (d.is_low_qual || d.qi < 0) return 0;
    int qs, qe;
    if (d.type == CDEL) { if (d.qi == 0) qs = qe = 0; else { qs = d.qi - 1; qe = d.qi; } }
    else { qs = d.qi; qe = d.qi + d.len - 1; }
    const unsigned char *q = (const unsigned char *)r.qual;
    int s = 0;
    for (int i = qs; i <= qe; ++i) s += (i < r.qlen) ? q[i] : 0;
    return s / (qe - qs + 1);
}
__device__ __forceinline__ int cv_nt4(unsigned char c) {
    if (c <= 4) return c;
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
__device__ __forceinline__ int cv_ref(const unsigned char *ref, const CvOpt &o, long long pos) { return (pos < o.ref_beg || pos > o.ref_end) ? 4 : cv_nt4(ref[pos - o.ref_beg]); }
__device__ int cv_homopolymer(const CvSite &v, const unsigned char *ref, const CvOpt &o) { // var_is_homopolymer (src/collect_var.c:306)
    long long sp, ep;
    if (v.var_type == CDIFF) { sp = v.pos - 1; ep = v.pos + 1; }
    else if (v.var_type == CINS) { if (v.alt_len > o.max_xgaps) return 0; sp = v.pos - 1; ep = v.pos; }
    else { if (v.ref_len > o.max_xgaps) return 0; sp = v.pos + v.ref_len - 1; ep = v.pos; }
    int hp = 1, rb[6];
    for (int i = 0; i < 6; ++i) rb[i] = cv_ref(ref, o, ep + i);
    for (int u = 1; u <= 6; ++u) {
        hp = 1;
        for (int i = 1; i < 3 && hp; ++i) for (int j = 0; j < u; ++j) if (cv_ref(ref, o, ep + i * u + j) != rb[j]) { hp = 0; break; }
        if (hp) break;
    }
    if (hp) return 1;
    for (int i = 0; i < 6; ++i) rb[i] = cv_ref(ref, o, sp - i);
    for (int u = 1; u <= 6; ++u) {
        hp = 1;
        for (int i = 1; i < 3 && hp; ++i) for (int j = 0; j < u; ++j) if (cv_ref(ref, o, sp - i * u - j) != rb[j]) { hp = 0; break; }
        if (hp) break;
    }
    return hp;
}
__device__ int cv_repeat(const CvSite &v, const CvRead *reads, const unsigned char *ref, const CvOpt &o) { // var_is_repeat_region (src/collect_var.c:361)
    const long long pos = v.pos;
    if (v.var_type == CDEL) {
        const int dl = v.ref_len; if (dl > o.max_xgaps) return 0;
        const int len = dl * 3;
        if (pos < o.ref_beg || pos + dl + len >= o.ref_end) return 0;
        for (int i = 0; i < len; ++i) if (cv_ref(ref, o, pos + i) != cv_ref(ref, o, pos + dl + i)) return 0;
        return 1;
    }
    const int il = v.alt_len; if (il > o.max_xgaps) return 0;
    const int len = il * 3;
    if (pos < o.ref_beg || pos + len >= o.ref_end) return 0;
    const CvRead r = reads[v.read];
    for (int k = 0; k < len; ++k) { // alt = alt_seq, then the first il reference bases repeated (the copy loop of :388-389)
        const int a = k < il ? cv_base(r, v.qi + k) : cv_ref(ref, o, pos + (k % il));
        if (cv_ref(ref, o, pos + k) != a) return 0;
    }
    return 1;
}
} // namespace

__global__ void __launch_bounds__(CV_T) cv_count_kernel(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long rb, long long re, int *cnt) {
    const int k = blockIdx.x * CV_T + threadIdx.x;
    if (k >= n) return;
    const CvRead r = reads[order[k]];
    int c = 0;
    for (int j = 0; j < r.n_digar; ++j) c += cv_collectible(dg[r.dig + j], rb, re);
    cnt[k] = c;
}
__global__ void __launch_bounds__(CV_T) cv_emit_kernel(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long rb, long long re, const int *off,
                                                       CvSite *sites, int *hist, long long key0) {
    const int k = blockIdx.x * CV_T + threadIdx.x;
    if (k >= n) return;
    const int rid = order[k];
    const CvRead r = reads[rid];
    int w = off[k];
    for (int j = 0; j < r.n_digar; ++j) {
        const DigarRec d = dg[r.dig + j];
        if (!cv_collectible(d, rb, re)) continue;
        const CvSite s = cv_site(rid, d);
        sites[w++] = s;
        atomicAdd(hist + ((cv_key(s) - key0) >> CV_BSHIFT), 1);
    }
}
__global__ void __launch_bounds__(1024) cv_scan_kernel(int *a, int n, int *total) {
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024, b = t * per, e = min(n, b + per);
    int s = 0;
    for (int i = b; i < e; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) { const int v = t >= o ? part[t - o] : 0; __syncthreads(); part[t] += v; __syncthreads(); }
    int run = t ? part[t - 1] : 0;
    for (int i = b; i < e; ++i) { const int x = a[i]; a[i] = run; run += x; }
    if (t == 1023) *total = part[1023];
}
__global__ void __launch_bounds__(CV_T) cv_scatter_kernel(const CvSite *sites, int n, const int *bstart, int *fill, int *tmp, long long key0) {
    const int i = blockIdx.x * CV_T + threadIdx.x;
    if (i >= n) return;
    const long long b = (cv_key(sites[i]) - key0) >> CV_BSHIFT;
    tmp[bstart[b] + atomicAdd(fill + b, 1)] = i;
}
// rank inside the bucket: records that sort before this one, ties (identical records) by input order -- independent of the scatter's atomic order
__global__ void __launch_bounds__(CV_T) cv_rank_kernel(const CvSite *sites, int n, const CvRead *reads, const int *bstart, const int *tmp, int *sorted, long long key0) {
    const int p = blockIdx.x * CV_T + threadIdx.x;
    if (p >= n) return;
    const int i = tmp[p];
    const CvSite si = sites[i];
    const long long b = (cv_key(si) - key0) >> CV_BSHIFT;
    const int b0 = bstart[b], b1 = bstart[b + 1];
    int rank = 0;
    for (int q = b0; q < b1; ++q) {
        const int j = tmp[q];
        if (j == i) continue;
        const int c = cv_exact(sites[j], si, reads);
        rank += (c < 0 || (c == 0 && j < i));
    }
    sorted[b0 + rank] = i;
}
__global__ void __launch_bounds__(CV_T) cv_dedup_kernel(const CvSite *sites, const CvRead *reads, const int *bstart, const int *sorted, int n_buckets, int *keep, int min_sv_len) {
    const int b = blockIdx.x * CV_T + threadIdx.x;
    if (b >= n_buckets) return;
    const int b0 = bstart[b], b1 = bstart[b + 1];
    int last = -1;
    for (int p = b0; p < b1; ++p) {
        const int k = last < 0 || cv_exact_ins(sites[sorted[last]], sites[sorted[p]], reads, min_sv_len) != 0;
        keep[p] = k;
        if (k) last = p;
    }
}
__global__ void __launch_bounds__(CV_T) cv_compact_kernel(const CvSite *sites, const int *sorted, const int *keep, const int *kidx, int n, CvSite *out) {
    const int p = blockIdx.x * CV_T + threadIdx.x;
    if (p >= n || !keep[p]) return;
    out[kidx[p]] = sites[sorted[p]];
}
__global__ void __launch_bounds__(CV_T) cv_pileup_kernel(const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *sites, int ns, CvCov *cov, CvOpt o) {
    const int k = blockIdx.x * CV_T + threadIdx.x;
    if (k >= n) return;
    const int rid = order[k];
    const CvRead r = reads[rid];
    const DigarRec *d = dg + r.dig;
    int si = cv_start(sites, ns, r.beg), di = 0;
    auto add = [&](int s, int low, int a) {
        if (low) { atomicAdd(&cov[s].low, 1); return; }
        atomicAdd(&cov[s].total, 1); atomicAdd(&cov[s].alle[a], 1); atomicAdd(&cov[s].strand[2 * r.strand + a], 1);
    };
    while (si < ns && di < r.n_digar) {
        const DigarRec dd = d[di];
        if (dd.type == CEQUAL) { di++; continue; }
        const CvSite ds = cv_site(rid, dd);
        const int aq = cv_ave_qual(r, dd);
        const int ret = cv_exact_ins(sites[si], ds, reads, o.min_sv_len);
        if (ret < 0) { add(si, 0, 0); si++; }
        else if (ret == 0) { add(si, dd.is_low_qual || aq < o.min_bq, 1); si++; }
        else di++;
    }
    for (; si < ns; ++si) { if (sites[si].pos > r.end) break; add(si, 0, 0); }
}
__global__ void __launch_bounds__(CV_T) cv_classify_kernel(const CvSite *sites, const CvRead *reads, const CvCov *cov, int ns, const unsigned char *ref, CvOpt o, int *cate) {
    const int i = blockIdx.x * CV_T + threadIdx.x;
    if (i >= ns) return;
    const CvCov c = cov[i];
    const CvSite v = sites[i];
    int r;
    if (c.total + c.low < o.min_dp) r = LOW_COV_VAR;
    else {
        const int alt_dp = c.alle[1];
        const double af = (double)alt_dp / c.total;
        if (alt_dp < o.min_alt_dp) r = LOW_COV_VAR;
        else if (af < o.min_af) r = LOW_AF_VAR;          // (the ONT strand-bias test sits between these two; the host applies it)
        else if (af > o.max_af) r = CLEAN_HOM_VAR;
        else if ((v.var_type == CINS || v.var_type == CDEL) && (cv_homopolymer(v, ref, o) || cv_repeat(v, reads, ref, o))) r = REP_HET_VAR;
        else r = v.var_type == CDIFF ? CLEAN_HET_SNP : CLEAN_HET_INDEL;
    }
    cate[i] = r;
}
// build_var_noisy_reads_ratio_cache: each read's X / I / D digars (low-quality ones too) merged into intervals (start, end]; n_err = -1: not in the coverage list
__global__ void __launch_bounds__(CV_T) cv_err_kernel(const CvRead *reads, const int *order, int n, const DigarRec *dg, IvRec *err, int *n_err) {
    const int k = blockIdx.x * CV_T + threadIdx.x;
    if (k >= n) return;
    const int rid = order[k];
    const CvRead r = reads[rid];
    if (r.n_digar <= 0 || r.beg > r.end) { n_err[rid] = -1; return; }
    IvRec *o = err + r.dig;
    int m = 0, has = 0;
    long long ns = -1, ne = -1;
    for (int j = 0; j < r.n_digar; ++j) {
        const DigarRec d = dg[r.dig + j];
        if (d.type != CDIFF && d.type != CINS && d.type != CDEL) continue;
        const long long cs = d.pos - 1, ce = d.pos + ((d.type == CDIFF || d.type == CDEL) ? d.len - 1 : 0);
        if (!has) { ns = cs; ne = ce; has = 1; continue; }
        if (cs < ne) { if (ce > ne) ne = ce; continue; }
        o[m].st = ns; o[m].en = ne; o[m].label = rid; o[m].pad = 0; ++m;
        ns = cs; ne = ce;
    }
    if (has) { o[m].st = ns; o[m].en = ne; o[m].label = rid; o[m].pad = 0; ++m; }
    n_err[rid] = m;
}
// var_noisy_reads_ratio(var_start, var_end): reads spanning (var_start - 1, var_end] and, of all reads, those with an error interval overlapping it
__global__ void __launch_bounds__(CV_T) cv_ratio_kernel(const CvRead *reads, const int *order, int n, const IvRec *err, const int *n_err, const long long *q, int nq, int *counts) {
    const int t = blockIdx.x * CV_T + threadIdx.x;
    if (t >= nq) return;
    const long long qs = (int)(q[2 * t] - 1), qe = (int)q[2 * t + 1];
    int total = 0, noisy = 0;
    for (int k = 0; k < n; ++k) {
        const int rid = order[k];
        const int m = n_err[rid];
        if (m < 0) continue;
        const CvRead r = reads[rid];
        if ((int)(r.beg - 1) < qe && qs < (int)r.end) total++;
        const IvRec *e = err + r.dig;
        for (int j = 0; j < m; ++j) {
            if ((int)e[j].st >= qe) break;
            if (qs < (int)e[j].en) { noisy++; break; }
        }
    }
    counts[2 * t] = total; counts[2 * t + 1] = noisy;
}
__global__ void __launch_bounds__(CV_T) cv_profile_kernel(int pass, const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *vars, const int *cate, int nv,
                                                          const IvRec *ivs, int *start, int *end, const unsigned long long *aoff, int *alleles, int *alt_qi, CvOpt o) {
    const int k = blockIdx.x * CV_T + threadIdx.x;
    if (k >= n) return;
    const int rid = order[k];
    const CvRead r = reads[rid];
    const DigarRec *d = dg + r.dig;
    int s0 = -1, e0 = -2;
    const int cap = pass ? (start[rid] >= 0 ? end[rid] - start[rid] + 1 : 0) : 0;
    auto set = [&](int vi, int a, int qi) { // update_read_var_profile_with_allele
        if (s0 == -1) s0 = vi;
        e0 = vi;
        const int x = vi - s0;
        if (pass && x < cap) { alleles[aoff[rid] + x] = a; alt_qi[aoff[rid] + x] = qi; }
    };
    int vi = cv_start(vars, nv, r.beg), di = 0;
    while (vi < nv && di < r.n_digar) {
        if (cate[vi] == NON_VAR) { vi++; continue; }
        const DigarRec dd = d[di];
        if (dd.type == CEQUAL) { di++; continue; }
        const CvSite ds = cv_site(rid, dd);
        const CvSite v = vars[vi];
        const int aq = cv_ave_qual(r, dd), is_ovlp = cv_ovlp(v, ds), ret = cv_exact(v, ds, reads);
        if (is_ovlp == 0) {
            if (ret < 0) { set(vi, 0, -1); vi++; }
            else if (ret > 0) di++;
            else { vi++; di++; }
        } else {
            if (ret == 0) set(vi, aq < o.min_bq ? -2 : 1, dd.qi);
            else set(vi, -1, -1);
            vi++;
        }
    }
    for (; vi < nv; ++vi) {
        const long long p = vars[vi].pos;
        if (p > r.end) break;
        int in = 0; // is_in_noisy_reg: the read's own noisy windows, overlap with [p, p + 1)
        for (int j = 0; j < r.n_iv; ++j) if (ivs[r.iv + j].st < p + 1 && p < ivs[r.iv + j].en) { in = 1; break; }
        if (in) continue;
        set(vi, 0, -1);
    }
    if (!pass) { start[rid] = s0; end[rid] = e0; }
}
__global__ void __launch_bounds__(CV_T) cv_alt_kernel(const CvSite *vars, const CvRead *reads, const unsigned long long *alt_off, int nv, unsigned char *pool) {
    const int i = blockIdx.x * CV_T + threadIdx.x;
    if (i >= nv) return;
    const CvSite v = vars[i];
    if (v.var_type != CDIFF && v.var_type != CINS) return;
    const CvRead r = reads[v.read];
    for (int k = 0; k < v.alt_len; ++k) pool[alt_off[i] + k] = (unsigned char)cv_base(r, v.qi + k);
}

static inline int cv_blocks(long long n) { return (int)((n + CV_T - 1) / CV_T); }
void lcd_launch_cv_count(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long rb, long long re, int *cnt, hipStream_t st) {
    if (n > 0) cv_count_kernel<<<cv_blocks(n), CV_T, 0, st>>>(reads, order, n, dg, rb, re, cnt);
}
void lcd_launch_cv_emit(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long rb, long long re, const int *off, CvSite *sites, int *hist, long long key0,
                        hipStream_t st) {
    if (n > 0) cv_emit_kernel<<<cv_blocks(n), CV_T, 0, st>>>(reads, order, n, dg, rb, re, off, sites, hist, key0);
}
int lcd_launch_cv_scan(int *a, int n, int *total, hipStream_t st) {
    cv_scan_kernel<<<1, 1024, 0, st>>>(a, n, total);
    return 0;
}
void lcd_launch_cv_sort(const CvSite *sites, int ns, const CvRead *reads, const int *bstart, int *fill, int *tmp, int *sorted, long long key0, int nb, int *keep, int min_sv_len,
                        hipStream_t st) {
    if (ns <= 0) return;
    cv_scatter_kernel<<<cv_blocks(ns), CV_T, 0, st>>>(sites, ns, bstart, fill, tmp, key0);
    cv_rank_kernel<<<cv_blocks(ns), CV_T, 0, st>>>(sites, ns, reads, bstart, tmp, sorted, key0);
    cv_dedup_kernel<<<cv_blocks(nb), CV_T, 0, st>>>(sites, reads, bstart, sorted, nb, keep, min_sv_len);
}
void lcd_launch_cv_compact(const CvSite *sites, const int *sorted, const int *keep, const int *kidx, int n, CvSite *out, hipStream_t st) {
    if (n > 0) cv_compact_kernel<<<cv_blocks(n), CV_T, 0, st>>>(sites, sorted, keep, kidx, n, out);
}
void lcd_launch_cv_pileup(const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *sites, int ns, CvCov *cov, CvOpt opt, hipStream_t st) {
    if (n > 0 && ns > 0) cv_pileup_kernel<<<cv_blocks(n), CV_T, 0, st>>>(reads, order, n, dg, sites, ns, cov, opt);
}
void lcd_launch_cv_classify(const CvSite *sites, const CvRead *reads, const CvCov *cov, int ns, const unsigned char *ref, CvOpt opt, int *cate, hipStream_t st) {
    if (ns > 0) cv_classify_kernel<<<cv_blocks(ns), CV_T, 0, st>>>(sites, reads, cov, ns, ref, opt, cate);
}
void lcd_launch_cv_err_ivs(const CvRead *reads, const int *order, int n, const DigarRec *dg, IvRec *err, int *n_err, hipStream_t st) {
    if (n > 0) cv_err_kernel<<<cv_blocks(n), CV_T, 0, st>>>(reads, order, n, dg, err, n_err);
}
void lcd_launch_cv_ratio(const CvRead *reads, const int *order, int n, const IvRec *err, const int *n_err, const long long *q, int nq, int *counts, hipStream_t st) {
    if (nq > 0) cv_ratio_kernel<<<cv_blocks(nq), CV_T, 0, st>>>(reads, order, n, err, n_err, q, nq, counts);
}
void lcd_launch_cv_profile(int pass, const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *vars, const int *cate, int nv, const IvRec *ivs,
                           int *start, int *end, const unsigned long long *aoff, int *alleles, int *alt_qi, CvOpt opt, hipStream_t st) {
    if (n > 0) cv_profile_kernel<<<cv_blocks(n), CV_T, 0, st>>>(pass, reads, order, n, dg, vars, cate, nv, ivs, start, end, aoff, alleles, alt_qi, opt);
}
void lcd_launch_cv_alt(const CvSite *vars, const CvRead *reads, const unsigned long long *alt_off, int nv, unsigned char *pool, hipStream_t st) {
    if (nv > 0) cv_alt_kernel<<<cv_blocks(nv), CV_T, 0, st>>>(vars, reads, alt_off, nv, pool);
}
