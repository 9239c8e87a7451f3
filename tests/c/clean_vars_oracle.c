/* tests/c/clean_vars_oracle.c -- TEST INFRASTRUCTURE (CPU restatement; never linked into the product).
 *
 * The first round of collect_var_main (src/collect_var.c:2897-2980, steps 1.2 - 3.1) on one chunk whose digars are already made:
 * candidate sites, pile-up, classification + extra noisy regions, read x variant profile.  Restates, function by function:
 *   is_collectible_var_digar, comp_var_site_for_sort        src/collect_var.c:1152-1163
 *   collect_all_cand_var_sites                              src/collect_var.c:1209-1253
 *   make_var_site_from_digar                                src/collect_var.c:1113-1121
 *   exact_comp_var_site, exact_comp_var_site_ins            src/collect_var.c:1878-1926
 *   ovlp_var_site, comp_ovlp_var_site                       src/collect_var.c:79-96, :1147-1150
 *   collect_cand_vars / init_cand_vars_based_on_sites       src/collect_var.c:238-247, :20-50
 *   get_var_site_start, get_var_start                       src/bam_utils.c:202-226
 *   get_digar_ave_qual                                      src/bam_utils.c:258-280
 *   update_var_site_with_allele                             src/bam_utils.c:238-246
 *   update_cand_vars_from_digar                             src/bam_utils.c:287-327
 *   var_is_strand_bias                                      src/collect_var.c:270-285
 *   fisher_exact_test, log_hypergeometric, fast_lgamma      src/math_utils.c:13-18, :101-168
 *   var_is_homopolymer, var_is_repeat_region                src/collect_var.c:306-405
 *   classify_var_cate                                       src/collect_var.c:413-435
 *   build_var_noisy_reads_ratio_cache, var_noisy_reads_ratio src/collect_var.c:662-747
 *   cr_add_var_cr                                           src/collect_var.c:750-775
 *   classify_cand_vars (germline: out_somatic == 0)         src/collect_var.c:902-1040
 *   cr_add / cr_index order / cr_cluster0 / cr_merge / cr_merge2 / cr_overlap / cr_is_contained   src/cgranges.c:145-160, 13-86, 225-334, 449-527
 *   collect_noisy_reg_start_end, post_process_noisy_regs    src/collect_var.c:481-536, :640-660
 *   update_read_var_profile_with_allele                     src/bam_utils.c:248-255
 *   update_read_vs_all_var_profile_from_digar (germline)    src/bam_utils.c:446-549
 *   is_in_noisy_reg                                         src/bam_utils.h:136-141
 *   collect_read_var_profile (read_var_cr)                  src/collect_var.c:1389-1420
 * Reference positions outside [ref_beg, ref_end] read as N (code 4) in var_is_homopolymer, which has no bounds check of its own.
 * Output layout == lcd_clean_vars_t (include/lcd_hotpath.h).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define CDIFF 8
#define CINS 1
#define CDEL 2
#define CEQUAL 7
#define NON_VAR 0x800
#define LOW_COV_VAR 0x001
#define STRAND_BIAS_VAR 0x002
#define LOW_AF_VAR 0x400
#define CLEAN_HET_SNP 0x004
#define CLEAN_HET_INDEL 0x008
#define REP_HET_VAR 0x010
#define CLEAN_HOM_VAR 0x080
#define NOT_CAND_VAR_CATE (NON_VAR | LOW_COV_VAR | STRAND_BIAS_VAR)

typedef struct { int64_t pos; int type, len, qi, is_low_qual; } cvo_digar_t;   /* == lcd_digar_t */
typedef struct { int64_t start, end; int label, pad; } cvo_iv_t;              /* == lcd_noisy_iv_t */
typedef struct {
    int min_dp, min_alt_dp, min_bq, min_sv_len, noisy_reg_max_xgaps, noisy_reg_flank_len, noisy_reg_merge_dis, is_ont, out_somatic;
    double min_af, max_af; float strand_bias_pval;
} cvo_opt_t;                                                                   /* == lcd_clean_opt_t */
typedef struct {
    int n_vars;
    int64_t *pos; int *var_type, *ref_len, *alt_len, *cate;
    int *total_cov, *low_qual_cov, *alle_covs, *strand_alle_covs;
    uint64_t *alt_off; uint8_t *alt_pool;
    int *is_homopolymer_indel;
    int n_regs; cvo_iv_t *regs;
    int n_reads; int *start_var_idx, *end_var_idx;
    uint64_t *allele_off; int *alleles, *alt_qi;
    int n_cr; int *cr_read;
    uint64_t qual_upload_bytes;
} cvo_clean_vars_t;                                                            /* == lcd_clean_vars_t */

static const uint8_t seq_nt16_int[16] = {4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4};
static int nt4(uint8_t c) { /* codes 0-4 as they are; letters through nst_nt4_table */
    if (c <= 4) return c;
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}

/* ---- the chunk as the walks see it ---- */
typedef struct {
    const cvo_opt_t *opt;
    int n_reads; const int *ordered, *status; const int64_t *beg, *end;
    const uint64_t *doff; const cvo_digar_t *dg;
    const uint8_t *seq_pool; const uint64_t *seq_off; const uint8_t *qual_pool; const uint64_t *qual_off; const int *qlen;
    const uint64_t *iv_off; const cvo_iv_t *ivs; const uint8_t *is_rev;
    const uint8_t *ref; int64_t ref_beg, ref_end, reg_beg, reg_end;
} chunk_t;

/* var_site_t: the alt bases stay in the read they came from (read r, query offset qi); alt_seq codes = seq_nt16_int[bam_seqi()] */
typedef struct { int64_t pos; int var_type, ref_len, alt_len, read, qi; } site_t;
static int alt_base(const chunk_t *c, const site_t *s, int k) {
    const uint8_t *b = c->seq_pool + c->seq_off[s->read]; int i = s->qi + k;
    if (i < 0 || i >= c->qlen[s->read]) return 4; /* (past the record: N, as on the device) */
    return seq_nt16_int[(b[i >> 1] >> ((~i & 1) << 2)) & 0xf];
}
static int alt_memcmp(const chunk_t *c, const site_t *a, const site_t *b, int len) {
    for (int k = 0; k < len; ++k) { int x = alt_base(c, a, k), y = alt_base(c, b, k); if (x != y) return x - y; }
    return 0;
}
static site_t site_of_digar(int read, const cvo_digar_t *d) { /* make_var_site_from_digar */
    site_t s; s.pos = d->pos; s.var_type = d->type; s.ref_len = 1; s.alt_len = d->len; s.read = read; s.qi = d->qi;
    if (d->type == CINS) s.ref_len = 0;
    else if (d->type == CDEL) { s.ref_len = d->len; s.alt_len = 0; }
    return s;
}
static int exact_comp(const chunk_t *c, const site_t *v1, const site_t *v2) {
    int64_t p1 = v1->var_type == CDIFF ? v1->pos : v1->pos - 1, p2 = v2->var_type == CDIFF ? v2->pos : v2->pos - 1;
    if (p1 < p2) return -1; if (p1 > p2) return 1;
    if (v1->var_type < v2->var_type) return -1; if (v1->var_type > v2->var_type) return 1;
    if (v1->ref_len < v2->ref_len) return -1; if (v1->ref_len > v2->ref_len) return 1;
    if (v1->alt_len < v2->alt_len) return -1; if (v1->alt_len > v2->alt_len) return 1;
    if (v1->var_type == CDIFF || v1->var_type == CINS) return alt_memcmp(c, v1, v2, v1->alt_len);
    return 0;
}
static int exact_comp_ins(const chunk_t *c, const site_t *v1, const site_t *v2) {
    int64_t p1 = v1->var_type == CDIFF ? v1->pos : v1->pos - 1, p2 = v2->var_type == CDIFF ? v2->pos : v2->pos - 1;
    if (p1 < p2) return -1; if (p1 > p2) return 1;
    if (v1->var_type < v2->var_type) return -1; if (v1->var_type > v2->var_type) return 1;
    if (v1->ref_len < v2->ref_len) return -1; if (v1->ref_len > v2->ref_len) return 1;
    if (v1->var_type == CDIFF) {
        if (v1->alt_len < v2->alt_len) return -1; if (v1->alt_len > v2->alt_len) return 1;
        return alt_memcmp(c, v1, v2, v1->alt_len);
    } else if (v1->var_type == CINS) {
        if (v1->alt_len < c->opt->min_sv_len) {
            if (v1->alt_len < v2->alt_len) return -1; if (v1->alt_len > v2->alt_len) return 1;
            return alt_memcmp(c, v1, v2, v1->alt_len);
        } else {
            int mn = v1->alt_len < v2->alt_len ? v1->alt_len : v2->alt_len, mx = v1->alt_len > v2->alt_len ? v1->alt_len : v2->alt_len;
            if (mn >= mx * 0.8) return 0;
            return v1->alt_len - v2->alt_len;
        }
    }
    return 0;
}
static int ovlp_site(const site_t *v1, const site_t *v2) {
    int b1 = (int)v1->pos, e1 = (int)(v1->pos + v1->ref_len), b2 = (int)v2->pos, e2 = (int)(v2->pos + v2->ref_len);
    if (v1->ref_len == 0 && v2->ref_len == 0) return b1 == b2;
    if (v1->ref_len == 0) return b1 > b2 && e1 < e2;
    if (v2->ref_len == 0) return b2 > b1 && e2 < e1;
    return !(b1 >= e2 || b2 >= e1);
}
static __thread const chunk_t *g_sort_chunk; /* (qsort has no context argument: one per calling thread) */
static int cmp_sort(const void *a, const void *b) { return exact_comp(g_sort_chunk, (const site_t *)a, (const site_t *)b); }

static int is_collectible(const cvo_digar_t *d, int64_t reg_beg, int64_t reg_end) {
    if (reg_beg != -1 && d->pos < reg_beg) return 0;
    if (reg_end != -1 && d->pos > reg_end) return 0;
    if (d->is_low_qual) return 0;
    return d->type == CDIFF || d->type == CINS || d->type == CDEL;
}
static int skipped(const chunk_t *c, int r) { return c->status[r] == -1; }

/* collect_all_cand_var_sites: qsort by exact_comp_var_site -- a total order on (pos', type, ref_len, alt_len, alt bases), so records that compare equal are
 * identical and which of them qsort puts first changes nothing -- then keep the first of every run equal to the LAST KEPT under exact_comp_var_site_ins */
static int collect_sites(const chunk_t *c, site_t **out) {
    int n = 0, m = 0;
    for (int i = 0; i < c->n_reads; ++i) {
        int r = c->ordered[i]; if (skipped(c, r)) continue;
        for (uint64_t j = c->doff[r]; j < c->doff[r + 1]; ++j) if (is_collectible(c->dg + j, c->reg_beg, c->reg_end)) m++;
    }
    *out = NULL;
    if (m == 0) return 0;
    site_t *s = (site_t *)malloc((size_t)m * sizeof(site_t));
    for (int i = 0; i < c->n_reads; ++i) {
        int r = c->ordered[i]; if (skipped(c, r)) continue;
        for (uint64_t j = c->doff[r]; j < c->doff[r + 1]; ++j) if (is_collectible(c->dg + j, c->reg_beg, c->reg_end)) s[n++] = site_of_digar(r, c->dg + j);
    }
    g_sort_chunk = c;
    qsort(s, (size_t)n, sizeof(site_t), cmp_sort);
    int w = 1;
    for (int i = 1; i < n; ++i) {
        if (exact_comp_ins(c, s + w - 1, s + i) == 0) continue;
        s[w++] = s[i];
    }
    *out = s;
    return w;
}

static int site_start(const site_t *v, int n, int64_t start) { /* get_var_site_start / get_var_start */
    int64_t target = start > 0 ? start - 1 : start;
    int left = 0, right = n;
    while (left < right) {
        int mid = left + (right - left) / 2;
        int64_t mp = v[mid].var_type == CDIFF ? v[mid].pos : v[mid].pos - 1;
        if (mp < target) left = mid + 1; else right = mid;
    }
    while (left < n && v[left].pos < start) left++;
    return left;
}
static int ave_qual(const chunk_t *c, int r, const cvo_digar_t *d) { /* get_digar_ave_qual */
    if (d->is_low_qual) return 0;
    if (d->qi < 0) return 0;
    int qs, qe;
    if (d->type == CDEL) { if (d->qi == 0) qs = qe = 0; else { qs = d->qi - 1; qe = d->qi; } }
    else { qs = d->qi; qe = d->qi + d->len - 1; }
    const uint8_t *q = c->qual_pool + c->qual_off[r];
    int s = 0, n = qe - qs + 1;
    for (int i = qs; i <= qe; ++i) s += (i < c->qlen[r]) ? q[i] : 0; /* (past the record: 0) */
    return s / n;
}

typedef struct { int total, low, alle[2], strand[2][2]; } cov_t;
static void update_allele(cov_t *v, int is_low_qual, int strand, int a) {
    if (is_low_qual) { v->low++; return; }
    v->total++; v->alle[a]++; v->strand[strand][a]++;
}
static void pileup_read(const chunk_t *c, int r, int n, const site_t *sites, cov_t *cov) { /* update_cand_vars_from_digar */
    const cvo_digar_t *d = c->dg + c->doff[r]; int nd = (int)(c->doff[r + 1] - c->doff[r]);
    int strand = c->is_rev ? (c->is_rev[r] != 0) : 0;
    int si = site_start(sites, n, c->beg[r]), di = 0;
    while (si < n && di < nd) {
        if (d[di].type == CEQUAL) { di++; continue; }
        site_t ds = site_of_digar(r, d + di);
        int aq = ave_qual(c, r, d + di);
        int ret = exact_comp_ins(c, sites + si, &ds);
        if (ret < 0) { update_allele(cov + si, 0, strand, 0); si++; }
        else if (ret == 0) { update_allele(cov + si, d[di].is_low_qual || aq < c->opt->min_bq, strand, 1); si++; }
        else di++;
    }
    for (; si < n; ++si) { if (sites[si].pos > c->end[r]) break; update_allele(cov + si, 0, strand, 0); }
}

/* ---- fisher_exact_test (src/math_utils.c:119-168): fast_lgamma is lgamma (its cache holds lgamma(i)) ---- */
static double log_hyper(int a, int b, int cc, int d) {
    const int n1 = a + b, n2 = cc + d, m1 = a + cc, m2 = b + d, N = n1 + n2;
    if (n1 > n2) return log_hyper(cc, d, a, b);
    if (m1 > m2) return log_hyper(b, a, d, cc);
    return lgamma(n1 + 1) + lgamma(n2 + 1) + lgamma(m1 + 1) + lgamma(m2 + 1) - (lgamma(a + 1) + lgamma(b + 1) + lgamma(cc + 1) + lgamma(d + 1) + lgamma(N + 1));
}
double cvo_fisher_exact_test(int a, int b, int cc, int d) {
    double p_obs = exp(log_hyper(a, b, cc, d)), total = 0.0;
    int min_a = (0 > (a + cc) - (a + b + cc + d)) ? 0 : (a + cc) - (b + d);
    int max_a = (a + b) < (a + cc) ? (a + b) : (a + cc);
    int mode_a = (int)((a + b) * (a + cc) / (double)(a + b + cc + d));
    for (int delta = 0; delta <= max_a - min_a; delta++) {
        int ca = mode_a + delta;
        if (ca <= max_a) {
            int cb = (a + b) - ca, c2 = (a + cc) - ca, cd = (b + d) - cb;
            if (cb >= 0 && c2 >= 0 && cd >= 0) { double p = exp(log_hyper(ca, cb, c2, cd)); if (p <= p_obs + DBL_EPSILON) total += p; }
        }
        if (delta > 0) {
            ca = mode_a - delta;
            if (ca >= min_a) {
                int cb = (a + b) - ca, c2 = (a + cc) - ca, cd = (b + d) - cb;
                if (cb >= 0 && c2 >= 0 && cd >= 0) { double p = exp(log_hyper(ca, cb, c2, cd)); if (p <= p_obs + DBL_EPSILON) total += p; }
            }
        }
    }
    return total;
}
static int strand_bias(const cov_t *v, const cvo_opt_t *opt) { /* var_is_strand_bias */
    int f = v->strand[0][1], r = v->strand[1][1], e = (f + r) / 2;
    if (e == 0) return 0;
    float p = (float)cvo_fisher_exact_test(f, r, e, e);
    return p < opt->strand_bias_pval;
}
static int refc(const chunk_t *c, int64_t pos) { /* ref_seq[pos - ref_beg] through nst_nt4_table; outside the chunk's reference: N */
    if (pos < c->ref_beg || pos > c->ref_end) return 4;
    return nt4(c->ref[pos - c->ref_beg]);
}
static int is_homopolymer(const chunk_t *c, const site_t *v) {
    int64_t sp, ep; int xid = c->opt->noisy_reg_max_xgaps;
    if (v->var_type == CDIFF) { sp = v->pos - 1; ep = v->pos + 1; }
    else if (v->var_type == CINS) { if (v->alt_len > xid) return 0; sp = v->pos - 1; ep = v->pos; }
    else { if (v->ref_len > xid) return 0; sp = v->pos + v->ref_len - 1; ep = v->pos; }
    int hp = 1, rb[6];
    for (int i = 0; i < 6; ++i) rb[i] = refc(c, ep + i);
    for (int u = 1; u <= 6; ++u) {
        hp = 1;
        for (int i = 1; i < 3 && hp; ++i) for (int j = 0; j < u; ++j) if (refc(c, ep + i * u + j) != rb[j]) { hp = 0; break; }
        if (hp) break;
    }
    if (hp) return hp;
    for (int i = 0; i < 6; ++i) rb[i] = refc(c, sp - i);
    for (int u = 1; u <= 6; ++u) {
        hp = 1;
        for (int i = 1; i < 3 && hp; ++i) for (int j = 0; j < u; ++j) if (refc(c, sp - i * u - j) != rb[j]) { hp = 0; break; }
        if (hp) break;
    }
    return hp;
}
static int is_repeat(const chunk_t *c, const site_t *v) {
    int64_t pos = v->pos; int xid = c->opt->noisy_reg_max_xgaps;
    if (v->var_type == CDEL) {
        int dl = v->ref_len; if (dl > xid) return 0;
        int len = dl * 3;
        if (pos < c->ref_beg || pos + dl + len >= c->ref_end) return 0;
        for (int i = 0; i < len; ++i) if (refc(c, pos + i) != refc(c, pos + dl + i)) return 0;
        return 1;
    } else {
        int il = v->alt_len; if (il > xid) return 0;
        int len = il * 3;
        if (pos < c->ref_beg || pos + len >= c->ref_end) return 0;
        /* alt_bseq: the reference window, shifted copy (alt[j] = alt[j - il] for j >= il, i.e. the first il bases repeated), then alt_seq in front */
        for (int k = 0; k < len; ++k) {
            int a = k < il ? alt_base(c, v, k) : refc(c, pos + (k % il));
            if (refc(c, pos + k) != a) return 0;
        }
        return 1;
    }
}
static int classify(const chunk_t *c, const site_t *v, const cov_t *cv) { /* classify_var_cate */
    const cvo_opt_t *o = c->opt;
    if (cv->total + cv->low < o->min_dp) return LOW_COV_VAR;
    int alt_dp = cv->alle[1]; double alt_af = (double)alt_dp / cv->total;
    if (alt_dp < o->min_alt_dp) return LOW_COV_VAR;
    if (o->is_ont && strand_bias(cv, o)) return STRAND_BIAS_VAR;
    if (alt_af < o->min_af) return LOW_AF_VAR;
    if (alt_af > o->max_af) return CLEAN_HOM_VAR;
    if ((v->var_type == CINS || v->var_type == CDEL) && (is_homopolymer(c, v) || is_repeat(c, v))) return REP_HET_VAR;
    return v->var_type == CDIFF ? CLEAN_HET_SNP : CLEAN_HET_INDEL;
}

/* ---- cgranges: list of intervals + cr_index's order ---- */
typedef struct { uint64_t x; int64_t en; int label; } iv_t;
typedef struct { iv_t *a; int n, m; } cr_t;
static void cr_add(cr_t *cr, int64_t st, int64_t en, int label) {
    if (st < 0) st = 0;
    if (st > en) return;
    if (cr->n == cr->m) { cr->m = cr->m ? cr->m * 2 : 16; cr->a = (iv_t *)realloc(cr->a, (size_t)cr->m * sizeof(iv_t)); }
    cr->a[cr->n].x = (uint64_t)st; cr->a[cr->n].en = en; cr->a[cr->n].label = label; cr->n++;
}
static void rs_insertsort(iv_t *beg, iv_t *end) {
    for (iv_t *i = beg + 1; i < end; ++i)
        if (i->x < (i - 1)->x) { iv_t *j, tmp = *i; for (j = i; j > beg && tmp.x < (j - 1)->x; --j) *j = *(j - 1); *j = tmp; }
}
static void rs_sort(iv_t *beg, iv_t *end, int n_bits, int s) {
    typedef struct { iv_t *b, *e; } bucket_t;
    int size = 1 << n_bits, m = size - 1;
    bucket_t b[256], *k, *be = b + size;
    for (k = b; k != be; ++k) k->b = k->e = beg;
    for (iv_t *i = beg; i != end; ++i) ++b[i->x >> s & m].e;
    for (k = b + 1; k != be; ++k) k->e += (k - 1)->e - beg, k->b = (k - 1)->e;
    for (k = b; k != be;) {
        if (k->b != k->e) {
            bucket_t *l;
            if ((l = b + (k->b->x >> s & m)) != k) {
                iv_t tmp = *k->b, swap;
                do { swap = tmp; tmp = *l->b; *l->b++ = swap; l = b + (tmp.x >> s & m); } while (l != k);
                *k->b++ = tmp;
            } else ++k->b;
        } else ++k;
    }
    for (b->b = beg, k = b + 1; k != be; ++k) k->b = (k - 1)->e;
    if (s) {
        s = s > n_bits ? s - n_bits : 0;
        for (k = b; k != be; ++k)
            if (k->e - k->b > 64) rs_sort(k->b, k->e, n_bits, s);
            else if (k->e - k->b > 1) rs_insertsort(k->b, k->e);
    }
}
static void cr_index(cr_t *cr) {
    int sorted = 1;
    for (int i = 1; i < cr->n; ++i) if (cr->a[i - 1].x > cr->a[i].x) { sorted = 0; break; }
    if (sorted) return;
    if (cr->n <= 64) rs_insertsort(cr->a, cr->a + cr->n); else rs_sort(cr->a, cr->a + cr->n, 8, 7 * 8);
}
static int64_t cr_overlap_n(const cr_t *cr, int64_t st, int64_t en) {
    int64_t n = 0;
    for (int i = 0; i < cr->n; ++i) if ((int64_t)cr->a[i].x < en && st < cr->a[i].en) n++;
    return n;
}
static int cr_is_contained(const cr_t *cr, int64_t st, int64_t en) { /* cr_max_start_int + the scan from there */
    int left = 0, right = cr->n;
    while (right > left) { int mid = left + ((right - left) >> 1); if ((int64_t)cr->a[mid].x <= st) left = mid + 1; else right = mid; }
    if (left == 0) return 0;
    int n = 0;
    for (int i = left - 1; i < cr->n; ++i) {
        if ((int64_t)cr->a[i].x >= en) break;
        if ((int64_t)cr->a[i].x <= st && cr->a[i].en >= en) n++;
    }
    return n;
}
static void cr_merge(cr_t *cr, int fixed_win) { /* cr_merge: cr_cluster0 passes until the count stops changing */
    int cur = cr->n;
    for (;;) {
        cr_t out = {0, 0, 0};
        char *merged = (char *)calloc((size_t)cr->n + 1, 1);
        for (int j = 0; j < cr->n; ++j) {
            if (merged[j]) continue;
            uint64_t ms = cr->a[j].x; int64_t me = cr->a[j].en; int ml = cr->a[j].label;
            for (int k = j + 1; k < cr->n; ++k) {
                if (merged[k]) continue;
                int win = fixed_win >= 0 ? fixed_win : (ml < cr->a[k].label ? ml : cr->a[k].label);
                if ((uint64_t)(me + win) >= cr->a[k].x) {
                    ml = ml > cr->a[k].label ? ml : cr->a[k].label;
                    ms = ms < cr->a[k].x ? ms : cr->a[k].x;
                    me = me > cr->a[k].en ? me : cr->a[k].en;
                    merged[k] = 1;
                }
            }
            cr_add(&out, (int64_t)ms, me, ml);
        }
        free(merged); free(cr->a);
        cr_index(&out);
        *cr = out;
        if (cr->n == cur) break;
        cur = cr->n;
    }
}
/* cr_merge2(cr1, cr2, fixed_win, ..): cr1's intervals then cr2's, each list in its index order; cr_index; cr_merge */
int cvo_cr_merge2(const cvo_iv_t *a, int na, const cvo_iv_t *b, int nb, int fixed_win, cvo_iv_t **out) {
    cr_t m = {0, 0, 0};
    for (int i = 0; i < na; ++i) cr_add(&m, a[i].start, a[i].end, a[i].label);
    for (int i = 0; i < nb; ++i) cr_add(&m, b[i].start, b[i].end, b[i].label);
    cr_index(&m);
    cr_merge(&m, fixed_win);
    cvo_iv_t *o = (cvo_iv_t *)calloc((size_t)m.n + 1, sizeof(cvo_iv_t));
    for (int i = 0; i < m.n; ++i) { o[i].start = (int64_t)m.a[i].x; o[i].end = m.a[i].en; o[i].label = m.a[i].label; }
    free(m.a);
    *out = o;
    return m.n;
}

/* ---- var_noisy_reads_ratio with its per-chunk cache ---- */
typedef struct { cr_t cov, err; } noisy_cache_t;
static void build_noisy_cache(const chunk_t *c, noisy_cache_t *nc) {
    memset(nc, 0, sizeof(*nc));
    for (int i = 0; i < c->n_reads; ++i) {
        int r = c->ordered[i]; const cvo_digar_t *d = c->dg + c->doff[r]; int nd = (int)(c->doff[r + 1] - c->doff[r]);
        if (skipped(c, r)) continue;
        if (nd <= 0) continue;
        if (c->beg[r] > c->end[r]) continue;
        cr_add(&nc->cov, (int32_t)(c->beg[r] - 1), (int32_t)c->end[r], r);
        int has = 0; int64_t ns = -1, ne = -1;
        for (int j = 0; j < nd; ++j) {
            if (d[j].type != CDIFF && d[j].type != CINS && d[j].type != CDEL) continue;
            int64_t cs = d[j].pos - 1, ce = d[j].pos;
            if (d[j].type == CDIFF || d[j].type == CDEL) ce += d[j].len - 1;
            if (!has) { ns = cs; ne = ce; has = 1; continue; }
            if (cs < ne) { if (ce > ne) ne = ce; continue; }
            cr_add(&nc->err, (int32_t)ns, (int32_t)ne, r);
            ns = cs; ne = ce;
        }
        if (has) cr_add(&nc->err, (int32_t)ns, (int32_t)ne, r);
    }
    cr_index(&nc->cov); cr_index(&nc->err);
}
static float noisy_reads_ratio(const chunk_t *c, const noisy_cache_t *nc, int64_t vs, int64_t ve) {
    int total = (int)cr_overlap_n(&nc->cov, (int32_t)(vs - 1), (int32_t)ve), noisy = 0;
    if (total > 0) {
        char *mark = (char *)calloc((size_t)c->n_reads + 1, 1);
        for (int i = 0; i < nc->err.n; ++i) {
            const iv_t *a = nc->err.a + i;
            if (!((int64_t)a->x < (int32_t)ve && (int32_t)(vs - 1) < a->en)) continue;
            if (mark[a->label]) continue;
            mark[a->label] = 1; noisy++;
        }
        free(mark);
    }
    if (total == 0) return 0.0;
    return (float)noisy / (total + 0.0);
}
static void add_var_cr(const chunk_t *c, const noisy_cache_t *nc, cr_t *var_cr, const cr_t *low, const site_t *v, int check) { /* cr_add_var_cr */
    int64_t vs = v->pos, ve = v->var_type == CINS ? v->pos : v->pos + v->ref_len - 1;
    const int64_t qs = vs - 1, qe = ve; /* one cr_overlap query with the variant's own span */
    for (int j = 0; j < low->n; ++j) {
        const iv_t *a = low->a + j;
        if (!((int64_t)a->x < qe && qs < a->en)) continue;
        int64_t s = (int64_t)a->x + 1, e = a->en;
        if (s < vs) vs = s;
        if (e > ve) ve = e;
    }
    if (check == 0 || noisy_reads_ratio(c, nc, vs, ve) >= c->opt->min_af) cr_add(var_cr, vs - 1, ve, 1);
}

/* ---- post_process_noisy_regs ---- */
static void post_process(const cvo_opt_t *o, cr_t *regs, int n, const site_t *v, const int *cate) {
    int nr = regs->n, flank = o->noisy_reg_flank_len;
    int *ml = (int *)malloc(((size_t)nr + 1) * sizeof(int)), *mr = (int *)malloc(((size_t)nr + 1) * sizeof(int));
    for (int i = 0; i < nr; ++i) ml[i] = mr[i] = -1;
    for (int ri = 0, vi = 0; ri < nr && vi < n;) {
        if (cate[vi] & NOT_CAND_VAR_CATE) { vi++; continue; }
        int32_t vs = (int32_t)v[vi].pos, ve = (int32_t)(v[vi].pos + v[vi].ref_len - 1);
        int32_t rs = (int32_t)regs->a[ri].x + 1, re = (int32_t)regs->a[ri].en;
        if (vs > re) { if (mr[ri] == -1) mr[ri] = vi; ri++; }
        else if (ve < rs) { ml[ri] = vi; vi++; }
        else vi++;
    }
    cr_t w = {0, 0, 0};
    for (int ri = 0; ri < nr; ++ri) {
        if (ml[ri] == -1) ml[ri] = n - 1 < 0 ? n - 1 : 0;
        if (mr[ri] == -1) mr[ri] = n - 1 > 0 ? n - 1 : 0;
        int32_t cs = (int32_t)regs->a[ri].x + 1 - flank, ce = (int32_t)regs->a[ri].en + flank;
        for (int vi = ml[ri]; vi >= 0; --vi) {
            if (cate[vi] & NOT_CAND_VAR_CATE) continue;
            int32_t vs = (int32_t)v[vi].pos, ve = (int32_t)(v[vi].pos + v[vi].ref_len - 1);
            if (ve < cs - 1) break;
            else if (vs - flank < cs) cs = vs - flank;
        }
        for (int vi = mr[ri]; vi < n; ++vi) {
            if (cate[vi] & NOT_CAND_VAR_CATE) continue;
            int32_t vs = (int32_t)v[vi].pos, ve = (int32_t)(v[vi].pos + v[vi].ref_len - 1);
            if (vs > ce + 1) break;
            else if (ve + flank > ce) ce = ve + flank;
        }
        cr_add(&w, cs, ce, regs->a[ri].label);
    }
    free(ml); free(mr);
    cr_index(&w);
    cr_merge(&w, 0);
    free(regs->a);
    *regs = w;
}

/* ---- update_read_vs_all_var_profile_from_digar, germline branch ---- */
typedef struct { int start, end, *alleles, *alt_qi, cap; } prof_t;
static void prof_set(prof_t *p, int var_i, int allele, int alt_qi) { /* update_read_var_profile_with_allele */
    if (p->start == -1) p->start = var_i;
    p->end = var_i;
    int k = var_i - p->start;
    if (k >= p->cap) {
        int nc = p->cap ? p->cap * 2 : 16; while (nc <= k) nc *= 2;
        p->alleles = (int *)realloc(p->alleles, (size_t)nc * sizeof(int)); p->alt_qi = (int *)realloc(p->alt_qi, (size_t)nc * sizeof(int));
        for (int i = p->cap; i < nc; ++i) p->alleles[i] = p->alt_qi[i] = -1;
        p->cap = nc;
    }
    p->alleles[k] = allele; p->alt_qi[k] = alt_qi;
}
static int in_noisy_reg(const chunk_t *c, int r, int64_t pos) {
    for (uint64_t k = c->iv_off[r]; k < c->iv_off[r + 1]; ++k) if (c->ivs[k].start < pos + 1 && pos < c->ivs[k].end) return 1;
    return 0;
}
static void profile_read(const chunk_t *c, int r, int n, const site_t *v, const int *cate, prof_t *p) {
    const cvo_digar_t *d = c->dg + c->doff[r]; int nd = (int)(c->doff[r + 1] - c->doff[r]);
    int vi = site_start(v, n, c->beg[r]), di = 0;
    while (vi < n && di < nd) {
        if (cate[vi] == NON_VAR) { vi++; continue; }
        if (d[di].type == CEQUAL) { di++; continue; }
        site_t ds = site_of_digar(r, d + di);
        int aq = ave_qual(c, r, d + di), rqi = d[di].qi, is_ovlp = ovlp_site(v + vi, &ds), ret = exact_comp(c, v + vi, &ds);
        if (is_ovlp == 0) {
            if (ret < 0) { prof_set(p, vi, 0, -1); vi++; }
            else if (ret > 0) di++;
            else { vi++; di++; }
        } else {
            if (ret == 0) { prof_set(p, vi, aq < c->opt->min_bq ? -2 : 1, rqi); vi++; }
            else { prof_set(p, vi, -1, -1); vi++; }
        }
    }
    for (; vi < n; ++vi) {
        if (v[vi].pos > c->end[r]) break;
        if (in_noisy_reg(c, r, v[vi].pos)) continue;
        prof_set(p, vi, 0, -1);
    }
}

int cvo_clean_vars(const cvo_opt_t *opt, int n_reads, const int *ordered, const int *status, const int64_t *beg, const int64_t *end,
                   const uint64_t *digar_off, const cvo_digar_t *digars, const uint8_t *seq_pool, const uint64_t *seq_off,
                   const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint64_t *iv_off, const cvo_iv_t *ivs, const uint8_t *is_rev,
                   const uint8_t *ref_seq, int64_t ref_beg, int64_t ref_end, int64_t reg_beg, int64_t reg_end,
                   const cvo_iv_t *pre_regs, int n_pre, const int64_t *low_comp, int n_low, cvo_clean_vars_t *out) {
    memset(out, 0, sizeof(*out));
    if (opt->out_somatic) return -2;
    chunk_t c = {opt, n_reads, ordered, status, beg, end, digar_off, digars, seq_pool, seq_off, qual_pool, qual_off, qlen, iv_off, ivs, is_rev,
                 ref_seq, ref_beg, ref_end, reg_beg, reg_end};
    /* 1.2 + 1.3 */
    site_t *s = NULL;
    const int n = collect_sites(&c, &s);
    cov_t *cov = (cov_t *)calloc((size_t)n + 1, sizeof(cov_t));
    for (int i = 0; i < n_reads; ++i) { int r = ordered[i]; if (!skipped(&c, r)) pileup_read(&c, r, n, s, cov); }
    /* 2.2 / 2.3: classify_cand_vars */
    int *cate = (int *)malloc(((size_t)n + 1) * sizeof(int));
    cr_t var_pos = {0, 0, 0}, noisy_var = {0, 0, 0}, low = {0, 0, 0}, regs = {0, 0, 0};
    for (int k = 0; k < n_low; ++k) cr_add(&low, low_comp[2 * k], low_comp[2 * k + 1], 0);
    cr_index(&low);
    for (int i = 0; i < n_pre; ++i) cr_add(&regs, pre_regs[i].start, pre_regs[i].end, pre_regs[i].label);
    for (int i = 0; i < n; ++i) {
        cate[i] = classify(&c, s + i, cov + i);
        if (cate[i] == LOW_COV_VAR) continue;
        if (opt->is_ont && cate[i] == STRAND_BIAS_VAR) continue;
        if (s[i].var_type == CINS) cr_add(&var_pos, s[i].pos - 1, s[i].pos, 1);
        else cr_add(&var_pos, s[i].pos - 1, s[i].pos + s[i].ref_len - 1, 1);
    }
    cr_index(&var_pos);
    noisy_cache_t nc; int have_cache = 0;
    for (int i = 0; i < n; ++i) {
        const site_t *v = s + i; int vc = cate[i];
        if (vc == NON_VAR || vc == STRAND_BIAS_VAR) continue;
        if (regs.n > 0) {
            int64_t on = v->var_type == CINS ? cr_overlap_n(&regs, v->pos - 1, v->pos) : cr_overlap_n(&regs, v->pos - 1, v->pos + v->ref_len - 1);
            if (on > 0) { cate[i] = NON_VAR; continue; }
        }
        if (vc == LOW_COV_VAR) continue;
        if (vc == REP_HET_VAR) {
            if (v->pos >= reg_beg && v->pos <= reg_end) add_var_cr(&c, NULL, &noisy_var, &low, v, 0);
            continue;
        }
        int64_t pn = v->var_type == CINS ? cr_overlap_n(&var_pos, v->pos - 1, v->pos) : cr_overlap_n(&var_pos, v->pos - 1, v->pos + v->ref_len - 1);
        if (pn > 1 && v->pos >= reg_beg && v->pos <= reg_end) {
            if (!have_cache) { build_noisy_cache(&c, &nc); have_cache = 1; }
            add_var_cr(&c, &nc, &noisy_var, &low, v, 1);
        }
        if (vc == LOW_AF_VAR) cate[i] = LOW_COV_VAR;
    }
    if (noisy_var.n > 0) {
        cr_index(&noisy_var);
        cr_t m = {0, 0, 0};
        for (int i = 0; i < regs.n; ++i) cr_add(&m, (int64_t)regs.a[i].x, regs.a[i].en, regs.a[i].label);
        for (int i = 0; i < noisy_var.n; ++i) cr_add(&m, (int64_t)noisy_var.a[i].x, noisy_var.a[i].en, noisy_var.a[i].label);
        cr_index(&m);
        cr_merge(&m, -1);
        free(regs.a); regs = m;
    }
    post_process(opt, &regs, n, s, cate);
    /* compaction (:1007-1023) */
    int nv = 0;
    int *keep = (int *)malloc(((size_t)n + 1) * sizeof(int));
    for (int i = 0; i < n; ++i) {
        if (cate[i] & NOT_CAND_VAR_CATE) continue;
        if (regs.n > 0 && cr_is_contained(&regs, s[i].pos - 1, s[i].pos + s[i].ref_len) > 0) { cate[i] = NON_VAR; continue; }
        keep[nv++] = i;
    }
    site_t *vs = (site_t *)malloc(((size_t)nv + 1) * sizeof(site_t));
    int *vcate = (int *)malloc(((size_t)nv + 1) * sizeof(int));
    out->n_vars = nv;
    out->pos = (int64_t *)malloc(((size_t)nv + 1) * 8);
    out->var_type = (int *)malloc(((size_t)nv + 1) * 4); out->ref_len = (int *)malloc(((size_t)nv + 1) * 4); out->alt_len = (int *)malloc(((size_t)nv + 1) * 4);
    out->cate = (int *)malloc(((size_t)nv + 1) * 4); out->total_cov = (int *)malloc(((size_t)nv + 1) * 4); out->low_qual_cov = (int *)malloc(((size_t)nv + 1) * 4);
    out->alle_covs = (int *)malloc(((size_t)nv + 1) * 8); out->strand_alle_covs = (int *)malloc(((size_t)nv + 1) * 16);
    out->alt_off = (uint64_t *)malloc(((size_t)nv + 1) * 8); out->is_homopolymer_indel = (int *)malloc(((size_t)nv + 1) * 4);
    uint64_t na = 0;
    for (int k = 0; k < nv; ++k) na += (s[keep[k]].var_type == CDIFF || s[keep[k]].var_type == CINS) ? (uint64_t)s[keep[k]].alt_len : 0;
    out->alt_pool = (uint8_t *)malloc(na + 1);
    na = 0;
    for (int k = 0; k < nv; ++k) {
        const int i = keep[k]; const site_t *v = s + i;
        vs[k] = *v; vcate[k] = cate[i];
        out->pos[k] = v->pos; out->var_type[k] = v->var_type; out->ref_len[k] = v->ref_len; out->alt_len[k] = v->alt_len; out->cate[k] = cate[i];
        out->total_cov[k] = cov[i].total; out->low_qual_cov[k] = cov[i].low; out->alle_covs[2 * k] = cov[i].alle[0]; out->alle_covs[2 * k + 1] = cov[i].alle[1];
        out->strand_alle_covs[4 * k] = cov[i].strand[0][0]; out->strand_alle_covs[4 * k + 1] = cov[i].strand[0][1];
        out->strand_alle_covs[4 * k + 2] = cov[i].strand[1][0]; out->strand_alle_covs[4 * k + 3] = cov[i].strand[1][1];
        out->alt_off[k] = na;
        if (v->var_type == CDIFF || v->var_type == CINS) for (int j = 0; j < v->alt_len; ++j) out->alt_pool[na++] = (uint8_t)alt_base(&c, v, j);
        /* var_is_homopolymer_indel (src/collect_var.c:1720) is what lcd_hap_problem_t reads: the noisy-region pass sets it; clean variants keep 0 */
        out->is_homopolymer_indel[k] = 0;
    }
    out->alt_off[nv] = na;
    out->n_regs = regs.n;
    out->regs = (cvo_iv_t *)calloc((size_t)regs.n + 1, sizeof(cvo_iv_t));
    for (int i = 0; i < regs.n; ++i) { out->regs[i].start = (int64_t)regs.a[i].x; out->regs[i].end = regs.a[i].en; out->regs[i].label = regs.a[i].label; }
    /* 3.1: collect_read_var_profile */
    out->n_reads = n_reads;
    out->start_var_idx = (int *)malloc(((size_t)n_reads + 1) * 4); out->end_var_idx = (int *)malloc(((size_t)n_reads + 1) * 4);
    out->allele_off = (uint64_t *)malloc(((size_t)n_reads + 1) * 8);
    prof_t *pr = (prof_t *)calloc((size_t)n_reads + 1, sizeof(prof_t));
    for (int r = 0; r < n_reads; ++r) { pr[r].start = -1; pr[r].end = -2; }
    cr_t rv = {0, 0, 0};
    for (int i = 0; i < n_reads; ++i) {
        int r = ordered[i]; if (skipped(&c, r)) continue;
        profile_read(&c, r, nv, vs, vcate, pr + r);
        if (pr[r].start < 0 || pr[r].end < 0) continue;
        cr_add(&rv, pr[r].start, pr[r].end + 1, r);
    }
    cr_index(&rv);
    uint64_t tot = 0;
    for (int r = 0; r < n_reads; ++r) { out->allele_off[r] = tot; if (pr[r].start >= 0) tot += (uint64_t)(pr[r].end - pr[r].start + 1); }
    out->allele_off[n_reads] = tot;
    out->alleles = (int *)malloc((tot + 1) * 4); out->alt_qi = (int *)malloc((tot + 1) * 4);
    for (int r = 0; r < n_reads; ++r) {
        out->start_var_idx[r] = pr[r].start; out->end_var_idx[r] = pr[r].end;
        if (pr[r].start >= 0) {
            memcpy(out->alleles + out->allele_off[r], pr[r].alleles, (size_t)(pr[r].end - pr[r].start + 1) * 4);
            memcpy(out->alt_qi + out->allele_off[r], pr[r].alt_qi, (size_t)(pr[r].end - pr[r].start + 1) * 4);
        }
        free(pr[r].alleles); free(pr[r].alt_qi);
    }
    out->n_cr = rv.n;
    out->cr_read = (int *)malloc(((size_t)rv.n + 1) * 4);
    for (int i = 0; i < rv.n; ++i) out->cr_read[i] = rv.a[i].label;
    free(pr); free(rv.a); free(vs); free(vcate); free(keep); free(s); free(cov); free(cate);
    free(var_pos.a); free(noisy_var.a); free(low.a); free(regs.a);
    if (have_cache) { free(nc.cov.a); free(nc.err.a); }
    return 0;
}

void cvo_clean_vars_free(cvo_clean_vars_t *v) {
    free(v->pos); free(v->var_type); free(v->ref_len); free(v->alt_len); free(v->cate); free(v->total_cov); free(v->low_qual_cov); free(v->alle_covs);
    free(v->strand_alle_covs); free(v->alt_off); free(v->alt_pool); free(v->is_homopolymer_indel); free(v->regs); free(v->start_var_idx); free(v->end_var_idx);
    free(v->allele_off); free(v->alleles); free(v->alt_qi); free(v->cr_read);
    memset(v, 0, sizeof(*v));
}
