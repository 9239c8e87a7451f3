// lcd_depth_format.cpp -- the host-only side of the depth track (lcd_chunk_depth, lcd_depth.cpp): the options' defaults and their check, the window rule and the
// track's text.  No HIP call or header in this file: a stand-alone program compiles it with the host compiler and its sanitizers (tests/c/depth_sanitize.cpp).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/lcd_hotpath.h"
#include "lcd_types.h"

extern "C" {

void lcd_depth_opt_default(lcd_depth_opt_t *o) {
    if (o) memset(o, 0, sizeof(*o));
}
int lcd_depth_opt_check(const lcd_depth_opt_t *o) {
    if (!o) return -4;
    if (o->window < 0 || o->window > (1 << 30)) return -4;
    return 0;
}
int lcd_depth_tile(void) { return LCD_DEPTH_TILE; }

// window k is [kW + 1, (k + 1)W]: the rows, which tile a span in order, cut at the window bounds; one output row per window that meets the span
int lcd_depth_windows(int n, const int64_t *beg, const int64_t *end, const uint32_t *depth, int window, int64_t **wbeg, int64_t **wend, uint64_t **wsum) {
    if (wbeg) *wbeg = nullptr;
    if (wend) *wend = nullptr;
    if (wsum) *wsum = nullptr;
    if (!wbeg || !wend || !wsum || window < 1 || n < 0 || (n > 0 && (!beg || !end || !depth))) return -4;
    for (int i = 0; i < n; ++i) if (beg[i] < 1 || end[i] < beg[i] || (i > 0 && beg[i] != end[i - 1] + 1)) return -4;
    const int64_t W = window;
    std::vector<int64_t> b, e; std::vector<uint64_t> s;
    try {
        for (int i = 0; i < n; ++i) {
            for (int64_t p = beg[i]; p <= end[i];) {
                const int64_t k = (p - 1) / W, last = (k + 1) * W, q = end[i] < last ? end[i] : last;      // [p, q]: the row inside window k
                if (b.empty() || (b.back() - 1) / W != k) { b.push_back(p); e.push_back(q); s.insert(s.end(), 3, 0); }
                e.back() = q;
                for (int h = 0; h < 3; ++h) s[s.size() - 3 + h] += (uint64_t)depth[3 * (size_t)i + h] * (uint64_t)(q - p + 1);
                p = q + 1;
            }
        }
    } catch (const std::bad_alloc &) { return -11; }
    const size_t m = b.size();
    if (m > (size_t)INT32_MAX) return -11;
    int64_t *ob = (int64_t *)malloc((m + 1) * 8), *oe = (int64_t *)malloc((m + 1) * 8); uint64_t *os = (uint64_t *)malloc((m + 1) * 24);
    if (!ob || !oe || !os) { free(ob); free(oe); free(os); return -11; }
    if (m) { memcpy(ob, b.data(), m * 8); memcpy(oe, e.data(), m * 8); memcpy(os, s.data(), m * 24); }
    *wbeg = ob; *wend = oe; *wsum = os;
    return (int)m;
}

int lcd_depth_format(int n, const int64_t *beg, const int64_t *end, const uint32_t *depth, const uint64_t *wsum, const char *chrom, int with_header, char **text) {
    if (text) *text = nullptr;
    if (!text || !chrom || n < 0 || (n > 0 && (!beg || !end || (!depth && !wsum)))) return -4;
    for (int i = 0; i < n; ++i) if (beg[i] < 1 || end[i] < beg[i]) return -4;
    std::string s;
    if (with_header) s += wsum ? "#chrom\tstart\tend\tbases_all\tbases_h1\tbases_h2\tbases_unassigned\n" : "#chrom\tstart\tend\tdepth_all\tdepth_h1\tdepth_h2\tdepth_unassigned\n";
    char buf[256];
    for (int i = 0; i < n; ++i) {
        uint64_t v[3];
        for (int h = 0; h < 3; ++h) v[h] = wsum ? wsum[3 * (size_t)i + h] : (uint64_t)depth[3 * (size_t)i + h];
        s += chrom;
        snprintf(buf, sizeof(buf), "\t%lld\t%lld\t%llu\t%llu\t%llu\t%llu\n", (long long)beg[i] - 1, (long long)end[i], (unsigned long long)(v[0] + v[1] + v[2]), (unsigned long long)v[1],
                 (unsigned long long)v[2], (unsigned long long)v[0]);
        s += buf;
    }
    char *out = (char *)malloc(s.size() + 1);
    if (!out) return -11;
    memcpy(out, s.c_str(), s.size() + 1);
    *text = out;
    return 0;
}

} // extern "C"
