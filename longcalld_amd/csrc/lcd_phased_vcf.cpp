// lcd_phased_vcf.cpp -- lcd_phased_vcf_read: the heterozygous phased sites of one sample of a VCF as per-contig tables for lcd_chunk_haplotag (the rules:
// include/lcd_hotpath.h; the same rules in Python: tests/haplotag_common.py).  Host only.  No HIP call or header in this file: a stand-alone program compiles it
// with the host compiler and its sanitizers (tests/c/haplotag_vcf_sanitize.cpp).  Errors: NULL, with the code and a message in lcd_phased_vcf_errno / _error.
#include <zlib.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/lcd_hotpath.h"
#include "lcd_phased_vcf.h"

namespace {
thread_local int g_code = 0;
thread_local std::string g_msg;
lcd_phased_vcf_t *fail(int code, const std::string &m) { g_code = code; g_msg = m; return nullptr; }

struct Span { const char *p; size_t n; bool is(const char *s) const { return strlen(s) == n && !memcmp(p, s, n); } };
// the fields of [p, p + n) between `sep`
void split(const char *p, size_t n, char sep, std::vector<Span> &out) {
    out.clear();
    size_t a = 0;
    for (size_t i = 0; i <= n; ++i) if (i == n || p[i] == sep) { out.push_back(Span{p + a, i - a}); a = i + 1; }
}
// all digits, 1 ... 18 of them
bool number(const Span &s, int64_t *v) {
    if (s.n < 1 || s.n > 18) return false;
    int64_t x = 0;
    for (size_t i = 0; i < s.n; ++i) { if (s.p[i] < '0' || s.p[i] > '9') return false; x = x * 10 + (s.p[i] - '0'); }
    *v = x;
    return true;
}
int nt16(char c) { return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : c == 'T' ? 8 : 15; }
bool plain(const Span &s, std::string &up) {
    if (!s.n) return false;
    up.assign(s.p, s.n);
    for (char &c : up) {
        if (c >= 'a' && c <= 'z') c = (char)(c - 32);
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N') return false;
    }
    return true;
}
struct Site { int64_t pos, ps; int kind, hap, len, ref_code, alt_code; std::string ins; };
} // namespace

extern "C" {

void lcd_hapvcf_opt_default(lcd_hapvcf_opt_t *o) { if (o) { memset(o, 0, sizeof(*o)); o->max_indel = 50; } }
int lcd_phased_vcf_errno(void) { return g_code; }
const char *lcd_phased_vcf_error(void) { return g_msg.c_str(); }

lcd_phased_vcf_t *lcd_phased_vcf_read(const char *path, const char *sample, int n_contigs, const char *const *names, const lcd_hapvcf_opt_t *opt_in, lcd_hapvcf_stats_t *stats) {
    const std::string W = "lcd_phased_vcf_read";
    g_code = 0; g_msg.clear();
    lcd_hapvcf_stats_t S; memset(&S, 0, sizeof(S));
    if (stats) *stats = S;
    lcd_hapvcf_opt_t opt; lcd_hapvcf_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    if (!path || n_contigs < 0 || (n_contigs > 0 && !names)) return fail(-4, W + ": NULL argument");
    for (int i = 0; i < n_contigs; ++i) if (!names[i]) return fail(-4, W + ": NULL contig name");
    if (opt.max_indel < 1) return fail(-4, W + ": max_indel must be at least 1");
    gzFile f = gzopen(path, "r");
    if (!f) return fail(-30, W + ": cannot open " + path);
    std::vector<char> buf;
    {
        std::vector<char> tmp(1 << 16); int got;
        while ((got = gzread(f, tmp.data(), (unsigned)tmp.size())) > 0) buf.insert(buf.end(), tmp.begin(), tmp.begin() + got);
        int zerr = Z_OK; (void)gzerror(f, &zerr);
        gzclose(f);
        if (got < 0 || (zerr != Z_OK && zerr != Z_STREAM_END)) return fail(-30, W + ": read error on " + path + " (a compressed member cut short?)");
    }
    std::vector<std::vector<Site>> sites((size_t)n_contigs);
    std::vector<Span> col, fmt, smp, gt, alts;
    std::string R, A;
    int n_head = 0, sample_col = -1;
    int64_t line_no = 0;
    for (size_t at = 0; at < buf.size();) {
        const char *nl = (const char *)memchr(buf.data() + at, '\n', buf.size() - at);
        const char *p = buf.data() + at;
        size_t n = nl ? (size_t)(nl - p) : buf.size() - at;
        at += n + 1; ++line_no;
        if (n && p[n - 1] == '\r') --n;
        if (!n) continue;
        const std::string L = std::to_string(line_no);
        if (p[0] == '#') {
            if (n >= 6 && !memcmp(p, "#CHROM", 6) && (n == 6 || p[6] == '\t')) {
                split(p, n, '\t', col);
                n_head = (int)col.size();
                if (n_head < 10) return fail(-4, W + ": the #CHROM line (line " + L + ") has no sample column");
                sample_col = 9;
                if (sample) {
                    sample_col = -1;
                    for (int c = 9; c < n_head && sample_col < 0; ++c) if (col[c].is(sample)) sample_col = c;
                    if (sample_col < 0) return fail(-4, W + ": no sample " + sample + " in the #CHROM line");
                }
            }
            continue;
        }
        if (sample_col < 0) return fail(-4, W + ": line " + L + ": a data line in front of the #CHROM line");
        split(p, n, '\t', col);
        if ((int)col.size() < n_head) return fail(-4, W + ": line " + L + " has " + std::to_string(col.size()) + " columns, the #CHROM line " + std::to_string(n_head));
        int64_t pos = 0;
        if (!number(col[1], &pos) || pos < 1) return fail(-4, W + ": line " + L + ": POS is not a positive integer");
        ++S.n_lines;
        int tid = -1;
        for (int c = 0; c < n_contigs && tid < 0; ++c) if (col[0].is(names[c])) tid = c;
        if (tid < 0) { ++S.n_unknown_contig; continue; }
        if (!col[6].is("PASS") && !col[6].is(".")) { ++S.n_filtered; continue; }
        split(col[8].p, col[8].n, ':', fmt);
        split(col[sample_col].p, col[sample_col].n, ':', smp);
        if (!fmt[0].is("GT")) { ++S.n_other_gt; continue; }
        if (memchr(smp[0].p, '/', smp[0].n)) { ++S.n_unphased; continue; }
        split(smp[0].p, smp[0].n, '|', gt);
        int64_t a = 0, b = 0;
        if (gt.size() != 2 || !number(gt[0], &a) || !number(gt[1], &b)) { ++S.n_other_gt; continue; }
        if (a == b) { ++S.n_hom; continue; }
        split(col[4].p, col[4].n, ',', alts);
        if (std::max(a, b) > (int64_t)alts.size()) { ++S.n_other_gt; continue; }
        if ((a == 0) == (b == 0)) { ++S.n_both_alt; continue; }
        const Span alt = alts[(size_t)(a ? a : b) - 1];
        if (!plain(col[3], R) || !plain(alt, A)) { ++S.n_symbolic; continue; }
        while (R.size() > 1 && A.size() > 1 && R.back() == A.back()) { R.pop_back(); A.pop_back(); }
        size_t k = 0;
        while (R.size() - k > 1 && A.size() - k > 1 && R[k] == A[k]) ++k;
        R.erase(0, k); A.erase(0, k); pos += (int64_t)k;
        Site s; s.pos = pos; s.ps = 0; s.hap = a ? 1 : 2; s.len = 1; s.ref_code = s.alt_code = 0;
        if (R.size() == 1 && A.size() == 1 && R[0] != A[0]) { s.kind = 0; s.ref_code = nt16(R[0]); s.alt_code = nt16(A[0]); }
        else if (R.size() == 1 && A.size() > 1 && R[0] == A[0]) { s.kind = 1; s.ins = A.substr(1); }
        else if (A.size() == 1 && R.size() > 1 && R[0] == A[0]) { s.kind = 2; }
        else { ++S.n_complex; continue; }
        if (s.kind) {
            const size_t ln = (s.kind == 1 ? A.size() : R.size()) - 1;
            if (ln > (size_t)opt.max_indel) { ++S.n_long_indel; continue; }
            if (opt.snvs_only) { ++S.n_indel_off; continue; }
            s.len = (int)ln;
        }
        for (size_t c = 1; c < fmt.size() && c < smp.size(); ++c)
            if (fmt[c].is("PS")) { int64_t v = 0; if (number(smp[c], &v) && v > 0) s.ps = v; break; }
        ++S.n_sites; ++(s.kind == 0 ? S.n_snv : s.kind == 1 ? S.n_ins : S.n_del);
        sites[(size_t)tid].push_back(std::move(s));
    }
    if (sample_col < 0) return fail(-4, W + ": no #CHROM line in " + path);
    std::unique_ptr<lcd_phased_vcf_s> v(new lcd_phased_vcf_s());
    v->contigs.resize((size_t)n_contigs);
    for (int c = 0; c < n_contigs; ++c) {
        v->names.push_back(names[c]);
        std::vector<Site> &in = sites[(size_t)c];
        lcd_hapvcf_contig &t = v->contigs[(size_t)c];
        std::vector<size_t> order(in.size());
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return in[x].pos < in[y].pos; });
        std::unordered_map<int64_t, int> seen;
        int64_t wide = 0;                                           // the value of the contig-wide set: the POS of its first site in table order
        for (size_t i : order) if (!in[i].ps) { wide = in[i].pos; break; }
        for (size_t i : order) {
            const Site &s = in[i];
            const int64_t ps = s.ps ? s.ps : wide;
            const auto ins = seen.emplace(ps, (int)t.ps_value.size());                                            // (sets are told apart by value)
            if (ins.second) t.ps_value.push_back(ps);
            const int idx = ins.first->second;
            t.pos.push_back(s.pos); t.kind.push_back((uint8_t)s.kind); t.hap_of_alt.push_back((uint8_t)s.hap); t.len.push_back(s.len);
            t.ref_code.push_back((uint8_t)s.ref_code); t.alt_code.push_back((uint8_t)s.alt_code); t.ps_idx.push_back(idx);
            t.ins_off.push_back(s.kind == 1 ? (int64_t)t.pool.size() : 0);
            for (char ch : s.ins) t.pool.push_back((uint8_t)nt16(ch));
            t.max_footprint = std::max(t.max_footprint, s.kind == 0 ? 1 : s.kind == 1 ? 2 : s.len + 1);
        }
        S.n_phase_sets += (int64_t)t.ps_value.size();
    }
    if (stats) *stats = S;
    return v.release();
}

#define LCD_VCF_CONTIG(v, c, bad) if (!(v) || (c) < 0 || (size_t)(c) >= (v)->contigs.size()) return (bad); const lcd_hapvcf_contig &t = (v)->contigs[(size_t)(c)]
int lcd_phased_vcf_n_contigs(const lcd_phased_vcf_t *v) { return v ? (int)v->contigs.size() : 0; }
int64_t lcd_phased_vcf_n_sites(const lcd_phased_vcf_t *v, int c) { LCD_VCF_CONTIG(v, c, -4); return (int64_t)t.pos.size(); }
int lcd_phased_vcf_n_phase_sets(const lcd_phased_vcf_t *v, int c) { LCD_VCF_CONTIG(v, c, -4); return (int)t.ps_value.size(); }
int64_t lcd_phased_vcf_pool_size(const lcd_phased_vcf_t *v, int c) { LCD_VCF_CONTIG(v, c, -4); return (int64_t)t.pool.size(); }
int lcd_phased_vcf_max_footprint(const lcd_phased_vcf_t *v, int c) { LCD_VCF_CONTIG(v, c, -4); return t.max_footprint; }
int lcd_phased_vcf_sites_to_host(const lcd_phased_vcf_t *v, int c, int64_t *pos, uint8_t *kind, uint8_t *hap_of_alt, int *len, uint8_t *ref_code, uint8_t *alt_code,
                                 int64_t *ins_off, int *ps_idx, int64_t *ps_value, uint8_t *pool) {
    LCD_VCF_CONTIG(v, c, -4);
    const size_t n = t.pos.size();
    if (n) {
        if (pos) memcpy(pos, t.pos.data(), n * 8);
        if (kind) memcpy(kind, t.kind.data(), n);
        if (hap_of_alt) memcpy(hap_of_alt, t.hap_of_alt.data(), n);
        if (len) memcpy(len, t.len.data(), n * sizeof(int));
        if (ref_code) memcpy(ref_code, t.ref_code.data(), n);
        if (alt_code) memcpy(alt_code, t.alt_code.data(), n);
        if (ins_off) memcpy(ins_off, t.ins_off.data(), n * 8);
        if (ps_idx) memcpy(ps_idx, t.ps_idx.data(), n * sizeof(int));
    }
    if (ps_value && !t.ps_value.empty()) memcpy(ps_value, t.ps_value.data(), t.ps_value.size() * 8);
    if (pool && !t.pool.empty()) memcpy(pool, t.pool.data(), t.pool.size());
    return 0;
}
#undef LCD_VCF_CONTIG
void lcd_phased_vcf_free(lcd_phased_vcf_t *v) {
    if (!v) return;
    if (v->dev && v->dev_free) v->dev_free(v->dev);
    delete v;
}

} // extern "C"
