// lcd_mods_format.cpp -- the host-only side of the methylation table (lcd_chunk_mod_pileup, lcd_mods.cpp): the options' defaults and their check, the strand
// combination of a chunk's rows and the table's text.  No HIP call or header in this file: a stand-alone program compiles it with the host compiler and its
// sanitizers (tests/c/mods_sanitize.cpp).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/lcd_hotpath.h"

extern "C" {

void lcd_mods_opt_default(lcd_mods_opt_t *o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->code = 'm'; o->threshold = 204; o->ref_beg = 1; o->ref_end = 0;
}
int lcd_mods_opt_check(const lcd_mods_opt_t *o) {
    if (!o) return -4;
    if (o->code != 'm' && o->code != 'h') return -4;
    if (o->threshold < 128 || o->threshold > 255) return -4;
    return 0;
}
// rows by (pos, strand): a '-' row at p joins the '+' row at p - 1, which -- when it exists -- is the row in front of it
int lcd_mods_combine_rows(int n, int64_t *pos, char *strand, uint32_t *counts) {
    if (n < 0 || (n > 0 && (!pos || !strand || !counts))) return -4;
    for (int i = 0; i < n; ++i) if (strand[i] != '+' && strand[i] != '-') return -4;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t key = strand[i] == '+' ? pos[i] : pos[i] - 1;
        if (m > 0 && pos[m - 1] == key) { for (int z = 0; z < 9; ++z) counts[9 * (size_t)(m - 1) + z] += counts[9 * (size_t)i + z]; continue; }
        pos[m] = key; strand[m] = '.';
        if (m != i) memmove(counts + 9 * (size_t)m, counts + 9 * (size_t)i, 9 * sizeof(uint32_t));
        ++m;
    }
    return m;
}
int lcd_mods_format(int n, const int64_t *pos, const char *strand, const uint32_t *counts, const char *chrom, int code, int with_header, char **text) {
    if (text) *text = nullptr;
    if (!text || !chrom || n < 0 || (n > 0 && (!pos || !strand || !counts)) || (code != 'm' && code != 'h')) return -4;
    for (int i = 0; i < n; ++i) if (strand[i] != '+' && strand[i] != '-' && strand[i] != '.') return -4;
    std::string s;
    if (with_header) s += "#chrom\tstart\tend\tcode\tstrand\tn_all\tmod_all\tn_h1\tmod_h1\tn_h2\tmod_h2\tn_filtered\n";
    char buf[256];
    for (int i = 0; i < n; ++i) {
        const uint32_t *c = counts + 9 * (size_t)i;
        uint64_t nh[3], mod = 0, all = 0, filt = 0;
        for (int h = 0; h < 3; ++h) { nh[h] = (uint64_t)c[3 * h] + c[3 * h + 1]; all += nh[h]; mod += c[3 * h]; filt += c[3 * h + 2]; }
        s += chrom;
        snprintf(buf, sizeof(buf), "\t%lld\t%lld\t%c\t%c\t%llu\t%llu\t%llu\t%u\t%llu\t%u\t%llu\n", (long long)pos[i] - 1, (long long)pos[i] + (strand[i] == '.' ? 1 : 0), (char)code,
                 strand[i], (unsigned long long)all, (unsigned long long)mod, (unsigned long long)nh[1], c[3], (unsigned long long)nh[2], c[6], (unsigned long long)filt);
        s += buf;
    }
    char *out = (char *)malloc(s.size() + 1);
    if (!out) return -11;
    memcpy(out, s.c_str(), s.size() + 1);
    *text = out;
    return 0;
}

} // extern "C"
