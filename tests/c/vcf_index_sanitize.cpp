// TEST ONLY: the finisher of the VCF indexes (longcalld_amd/csrc/lcd_index_host.cpp, a translation unit without a HIP call) under AddressSanitizer + UBSan.  A
// stand-alone program: it is compiled together with that file by the host compiler and compares lcd_tbx_from_records with a second, naive implementation written
// here from the rules of include/lcd_hotpath.h ("VCF indexes"): bins by walking up from the leaf, loffset by a scan over every line, maps instead of sorted runs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "lcd_hotpath.h"

namespace {
int n_checks = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); exit(1); } ++n_checks; } while (0)

struct Rec { int tid; int64_t beg, end; uint64_t vbeg, vend; };
void p32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
void p64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// the bin of [beg, end) at `depth`: start at the leaf of beg and go to the parent until the bin holds end - 1
uint32_t naive_bin(int64_t beg, int64_t end, int depth, int64_t *lo, int64_t *hi) {
    int lv = depth; int64_t idx = beg >> 14;
    while (lv > 0 && ((end - 1) >> (14 + 3 * (depth - lv))) != idx) { --lv; idx >>= 3; }
    uint32_t first = 0; for (int l = 0; l < lv; ++l) first += 1u << (3 * l);
    *lo = idx << (14 + 3 * (depth - lv)); *hi = (idx + 1) << (14 + 3 * (depth - lv));
    return first + (uint32_t)idx;
}

std::vector<uint8_t> naive(int format, const std::vector<std::string> &names, int64_t max_clen, const std::vector<Rec> &recs) {
    const bool csi = format == LCD_VIDX_CSI;
    int depth = 5;
    if (csi) {
        int64_t want = max_clen;
        if (!want) for (const Rec &r : recs) want = std::max(want, r.end);
        while ((1ll << (14 + 3 * depth)) < want) ++depth;
    }
    std::vector<uint8_t> aux, out;
    p32(aux, 2); p32(aux, 1); p32(aux, 2); p32(aux, 0); p32(aux, '#'); p32(aux, 0);
    uint32_t l_nm = 0; for (const std::string &s : names) l_nm += (uint32_t)s.size() + 1;
    p32(aux, l_nm);
    for (const std::string &s : names) { for (char c : s) aux.push_back((uint8_t)c); aux.push_back(0); }
    if (csi) { out = {'C', 'S', 'I', 1}; p32(out, 14); p32(out, (uint32_t)depth); p32(out, (uint32_t)aux.size()); out.insert(out.end(), aux.begin(), aux.end()); p32(out, (uint32_t)names.size()); }
    else { out = {'T', 'B', 'I', 1}; p32(out, (uint32_t)names.size()); out.insert(out.end(), aux.begin(), aux.end()); }
    for (int t = 0; t < (int)names.size(); ++t) {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; std::map<uint32_t, uint64_t> loff; std::map<int64_t, uint64_t> lin;
        uint64_t n = 0, first = 0, last = 0; uint32_t run_bin = 0; bool in_run = false;
        size_t t0 = 0; while (t0 < recs.size() && recs[t0].tid != t) ++t0;          // (a contig's lines are consecutive)
        for (size_t i = 0; i < recs.size(); ++i) {
            const Rec &r = recs[i];
            if (r.tid != t) { in_run = false; continue; }
            int64_t lo, hi;
            const uint32_t b = naive_bin(r.beg, r.end, depth, &lo, &hi);
            auto &ch = bins[b];
            if (in_run && run_bin == b) ch.back().second = r.vend;
            else if (!ch.empty() && (ch.back().second >> 16) >= (r.vbeg >> 16)) ch.back().second = r.vend;
            else ch.emplace_back(r.vbeg, r.vend);
            in_run = true; run_bin = b;
            if (!n++) first = r.vbeg;
            last = r.vend;
            for (int64_t w = r.beg >> 14; w <= (r.end - 1) >> 14; ++w) { auto it = lin.find(w); if (it == lin.end() || r.vbeg < it->second) lin[w] = r.vbeg; }
            if (csi && !loff.count(b)) {                 // every line of the contig that overlaps the bin's interval
                uint64_t m = ~0ull;
                for (size_t k = t0; k < recs.size() && recs[k].tid == t; ++k) if (recs[k].beg < hi && recs[k].end > lo) m = std::min(m, recs[k].vbeg);
                loff[b] = m;
            }
        }
        if (!n) { p32(out, 0); if (!csi) p32(out, 0); continue; }
        p32(out, (uint32_t)bins.size() + 1);
        for (auto &kv : bins) {
            p32(out, kv.first); if (csi) p64(out, loff[kv.first]);
            p32(out, (uint32_t)kv.second.size());
            for (auto &c : kv.second) { p64(out, c.first); p64(out, c.second); }
        }
        p32(out, csi ? (uint32_t)((((1ull << (3 * depth + 3)) - 1) / 7) + 1) : 37450u); if (csi) p64(out, 0);
        p32(out, 2); p64(out, first); p64(out, last); p64(out, n); p64(out, 0);
        if (!csi) {
            const int64_t n_intv = lin.rbegin()->first + 1;
            p32(out, (uint32_t)n_intv);
            uint64_t prev = 0;
            for (int64_t w = 0; w < n_intv; ++w) { auto it = lin.find(w); if (it != lin.end()) prev = it->second; p64(out, prev); }
        }
    }
    p64(out, 0);
    return out;
}

int ours(int format, const std::vector<std::string> &names, int64_t max_clen, const std::vector<Rec> &recs, std::vector<uint8_t> &got) {
    std::vector<const char *> nm; for (const std::string &s : names) nm.push_back(s.c_str());
    std::vector<int> tid; std::vector<int64_t> beg, end; std::vector<uint64_t> vb, ve;
    for (const Rec &r : recs) { tid.push_back(r.tid); beg.push_back(r.beg); end.push_back(r.end); vb.push_back(r.vbeg); ve.push_back(r.vend); }
    uint8_t *bytes = nullptr; size_t n = 0;
    const int rc = lcd_tbx_from_records(format, (int)nm.size(), nm.data(), max_clen, (int64_t)recs.size(), tid.data(), beg.data(), end.data(), vb.data(), ve.data(), &bytes, &n);
    got.assign(bytes, bytes + (bytes ? n : 0));
    free(bytes);
    return rc;
}
void same(int format, const std::vector<std::string> &names, int64_t max_clen, const std::vector<Rec> &recs) {
    std::vector<uint8_t> got;
    CHECK(ours(format, names, max_clen, recs, got) == 0);
    CHECK(got == naive(format, names, max_clen, recs));
}
uint64_t rnd(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
} // namespace

int main() {
    std::vector<uint8_t> got;
    for (int fmt : {LCD_VIDX_TBI, LCD_VIDX_CSI}) {
        same(fmt, {}, 0, {});                                                       // zero records, zero contigs
        same(fmt, {"c1", "empty"}, 0, {});                                          // zero records
        same(fmt, {"c1"}, 0, {{0, 5, 6, 100ull << 16, (100ull << 16) | 40}});       // one record
        same(fmt, {"c1"}, 0, {{0, (1ll << 29) - 1, 1ll << 29, 7ull << 16, 9ull << 16}});                 // an end of exactly 2^29
        same(fmt, {"a", "b"}, 0, {{0, 0, 1ll << 29, 1ull << 16, 2ull << 16}, {1, 3, 4, 2ull << 16, 3ull << 16}});   // bin 0
    }
    const std::vector<Rec> over = {{0, 10, 11, 1ull << 16, 2ull << 16}, {0, 1ll << 29, (1ll << 29) + 1, 2ull << 16, 3ull << 16}};   // an end of 2^29 + 1
    CHECK(ours(LCD_VIDX_TBI, {"c"}, 0, over, got) == LCD_ERR_VIDX_CSI && got.empty());
    same(LCD_VIDX_CSI, {"c"}, 0, over);
    CHECK(ours(LCD_VIDX_CSI, {"c"}, 0, over, got) == 0 && got[8] == 6);                                     // depth 6 from the largest end
    CHECK(ours(LCD_VIDX_CSI, {"c"}, 1000, over, got) == LCD_ERR_VIDX_CSI);                                  // a header's depth that does not hold it
    {   // depth-6 bins at every level, from a header length of 4 Gb
        std::vector<Rec> r; uint64_t v = 1;
        for (int lv = 0; lv <= 5; ++lv) { const int64_t b = (1ll << (14 + 3 * lv)) - 3 + (lv == 0 ? 100 : 0); r.push_back({0, b, b + 8, v << 16, (v + 1) << 16}); ++v; }
        r.push_back({0, (1ll << 31) - 3, (1ll << 31) + 5, 0, 0});                    // over a border of the level under the root: bin 0
        std::sort(r.begin(), r.end(), [](const Rec &x, const Rec &y) { return x.beg < y.beg; });
        for (size_t i = 0; i < r.size(); ++i) { r[i].vbeg = (i + 1) << 16; r[i].vend = (i + 2) << 16; }
        same(LCD_VIDX_CSI, {"big"}, 4000000000ll, r);
        CHECK(ours(LCD_VIDX_CSI, {"big"}, 4000000000ll, r, got) == 0 && got[8] == 6);
    }
    CHECK(ours(LCD_VIDX_TBI, {"c"}, 0, {{0, 9, 10, 1, 2}, {0, 8, 9, 2, 3}}, got) == LCD_ERR_VIDX_ORDER);
    CHECK(ours(LCD_VIDX_TBI, {"c", "d"}, 0, {{1, 9, 10, 1, 2}, {0, 8, 9, 2, 3}}, got) == LCD_ERR_VIDX_ORDER);
    CHECK(ours(LCD_VIDX_TBI, {"c"}, 0, {{0, 9, 9, 1, 2}}, got) == -4 && ours(7, {"c"}, 0, {}, got) == -4);
    for (int fmt : {LCD_VIDX_TBI, LCD_VIDX_CSI}) {   // 10^5 seeded records on 7 contigs: dense runs, long intervals, members of 1 ... 60 000 bytes
        uint64_t s = 0x9e3779b97f4a7c15ull + (uint64_t)fmt; std::vector<Rec> r; std::vector<std::string> names;
        uint64_t coff = 0, in = 0;
        for (int t = 0; t < 7; ++t) {
            names.push_back("ctg" + std::to_string(t));
            if (t == 3) continue;                                                   // a contig without lines
            int64_t pos = 0;
            const int n = 100000 / 6;
            for (int i = 0; i < n; ++i) {
                pos += (int64_t)(rnd(s) % (t == 0 ? 30 : 20000));
                const int64_t len = rnd(s) % 50 == 0 ? (int64_t)(rnd(s) % 300000) + 1 : (int64_t)(rnd(s) % 40) + 1;
                const uint64_t vb = (coff << 16) | in;
                in += 40 + rnd(s) % 200;
                while (in >= 65280 || rnd(s) % 400 == 0) { coff += 1 + rnd(s) % 60000; in = in >= 65280 ? in - 65280 : 0; }
                r.push_back({t, pos, pos + len, vb, (coff << 16) | in});
            }
        }
        same(fmt, names, fmt == LCD_VIDX_CSI ? 400000000 : 0, r);
    }
    printf("%d checks ok\n", n_checks);
    return 0;
}
