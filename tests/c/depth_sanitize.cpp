// The host-only side of the depth track (longcalld_amd/csrc/lcd_depth_format.cpp: options, window rule, text) under the host compiler's sanitizers.
// argv[1]: a file of tables: a line "T <window>" starts a table, the lines "beg end d0 d1 d2" behind it are its rows (written by tests/test_depth_sanitized.py from
// the case table, seeded chunks and rows near the 64-bit limits).  Per table the per-base text, "--windows--" and the windows' text are printed, "--table--"
// between tables, for the test to compare.  Prints "<n> checks ok" as its last line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lcd_hotpath.h"

static int n_checks = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); return 1; } ++n_checks; } while (0)

struct Table { int window; std::vector<int64_t> beg, end; std::vector<uint32_t> dep; };

static int one(const Table &t) {
    const int n = (int)t.beg.size();
    // exact-size heap copies: a read or write past any array is an error here
    std::vector<int64_t> beg(t.beg), end(t.end); std::vector<uint32_t> dep(t.dep);
    char *text = nullptr;
    CHECK(lcd_depth_format(n, beg.data(), end.data(), dep.data(), nullptr, "chrS", 1, &text) == 0 && text);
    printf("%s", text);
    { int lines = 0; for (const char *q = text; *q; ++q) lines += *q == '\n'; CHECK(lines == n + 1); }
    free(text); text = nullptr;
    int64_t *wb = nullptr, *we = nullptr; uint64_t *ws = nullptr;
    const int m = lcd_depth_windows(n, beg.data(), end.data(), dep.data(), t.window, &wb, &we, &ws);
    CHECK(m >= (n > 0) && wb && we && ws);
    // the windows tile the rows' span, each inside one window, and keep the sum of depth x positions (modulo 2^64, as the rule adds them)
    uint64_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) for (int h = 0; h < 3; ++h) a[h] += (uint64_t)dep[3 * (size_t)i + h] * (uint64_t)(end[i] - beg[i] + 1);
    for (int k = 0; k < m; ++k) {
        for (int h = 0; h < 3; ++h) b[h] += ws[3 * (size_t)k + h];
        CHECK(wb[k] <= we[k] && (wb[k] - 1) / t.window == (we[k] - 1) / t.window);
        if (k) CHECK(wb[k] == we[k - 1] + 1 && (wb[k] - 1) % t.window == 0);
    }
    if (n) CHECK(wb[0] == beg[0] && we[m - 1] == end[n - 1]);
    CHECK(a[0] == b[0] && a[1] == b[1] && a[2] == b[2]);
    std::vector<int64_t> wb1(wb, wb + m), we1(we, we + m); std::vector<uint64_t> ws1(ws, ws + 3 * (size_t)m);
    free(wb); free(we); free(ws);
    CHECK(lcd_depth_format(m, wb1.data(), we1.data(), nullptr, ws1.data(), "chrS", 1, &text) == 0 && text);
    printf("--windows--\n%s", text);
    free(text);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<Table> tables;
    char line[256];
    while (fgets(line, sizeof(line), f)) {
        long long b, e; unsigned d[3]; int w;
        if (sscanf(line, "T %d", &w) == 1) { tables.emplace_back(); tables.back().window = w; }
        else if (sscanf(line, "%lld %lld %u %u %u", &b, &e, &d[0], &d[1], &d[2]) == 5 && !tables.empty()) {
            Table &t = tables.back(); t.beg.push_back(b); t.end.push_back(e); for (int h = 0; h < 3; ++h) t.dep.push_back(d[h]);
        }
    }
    fclose(f);
    CHECK(tables.size() > 20);
    for (size_t k = 0; k < tables.size(); ++k) { if (k) printf("--table--\n"); if (one(tables[k])) return 1; }
    printf("--end--\n");
    lcd_depth_opt_t o; o.skip_dels = 3; o.window = 9; lcd_depth_opt_default(&o);
    CHECK(!o.skip_dels && !o.window && !o.reserved[0] && !o.reserved[1] && lcd_depth_opt_check(&o) == 0);
    lcd_depth_opt_default(nullptr);
    o.window = 1 << 30; CHECK(lcd_depth_opt_check(&o) == 0); o.window = (1 << 30) + 1; CHECK(lcd_depth_opt_check(&o) == -4); o.window = -1; CHECK(lcd_depth_opt_check(&o) == -4);
    CHECK(lcd_depth_opt_check(nullptr) == -4 && lcd_depth_tile() > 0);
    char *text = nullptr; int64_t *wb = nullptr, *we = nullptr; uint64_t *ws = nullptr;
    int64_t b1[2] = {5, 11}, e1[2] = {10, 20}; uint32_t d1[6] = {1, 2, 3, 4, 5, 6};
    CHECK(lcd_depth_format(0, nullptr, nullptr, nullptr, nullptr, "c", 0, &text) == 0 && text && !text[0]); free(text); text = nullptr;
    CHECK(lcd_depth_format(0, nullptr, nullptr, nullptr, nullptr, "c", 1, &text) == 0 && text && text[0] == '#'); free(text); text = nullptr;
    CHECK(lcd_depth_format(2, nullptr, e1, d1, nullptr, "c", 0, &text) == -4 && !text);
    CHECK(lcd_depth_format(2, b1, e1, nullptr, nullptr, "c", 0, &text) == -4 && lcd_depth_format(2, b1, e1, d1, nullptr, nullptr, 0, &text) == -4);
    CHECK(lcd_depth_format(2, b1, e1, d1, nullptr, "c", 0, nullptr) == -4 && lcd_depth_format(-1, b1, e1, d1, nullptr, "c", 0, &text) == -4);
    { int64_t b0[1] = {0}, e0[1] = {3}; CHECK(lcd_depth_format(1, b0, e0, d1, nullptr, "c", 0, &text) == -4); }
    { int64_t b0[1] = {7}, e0[1] = {6}; CHECK(lcd_depth_format(1, b0, e0, d1, nullptr, "c", 0, &text) == -4); }
    CHECK(lcd_depth_windows(2, b1, e1, d1, 0, &wb, &we, &ws) == -4 && !wb && !we && !ws);
    CHECK(lcd_depth_windows(2, b1, e1, d1, 4, nullptr, &we, &ws) == -4 && lcd_depth_windows(2, nullptr, e1, d1, 4, &wb, &we, &ws) == -4);
    { int64_t b2[2] = {5, 12}; CHECK(lcd_depth_windows(2, b2, e1, d1, 4, &wb, &we, &ws) == -4); }       // a gap between the rows
    { int64_t b2[2] = {5, 10}; CHECK(lcd_depth_windows(2, b2, e1, d1, 4, &wb, &we, &ws) == -4); }       // rows that overlap
    CHECK(lcd_depth_windows(0, nullptr, nullptr, nullptr, 4, &wb, &we, &ws) == 0 && wb && we && ws); free(wb); free(we); free(ws);
    {   // the widest line: sums near 2^63, the last position an int64 holds, a long contig name
        int64_t bb[1] = {INT64_MAX - 5}, be[1] = {INT64_MAX}; uint64_t s[3] = {(1ull << 63) - 1, 1ull << 62, 5};
        const std::string name(300, 'c');
        CHECK(lcd_depth_format(1, bb, be, nullptr, s, name.c_str(), 0, &text) == 0 && text);
        CHECK(strstr(text, "\t9223372036854775801\t9223372036854775807\t13835058055282163716\t4611686018427387904\t5\t9223372036854775807\n") != nullptr);
        free(text); text = nullptr;
        // one row of the widest depth over 2^31 positions: 2^63 - 2^31 per haplotype, in one window and in two
        int64_t rb[1] = {1}, re[1] = {1ll << 31}; uint32_t rd[3] = {0xffffffffu, 0xffffffffu, 1};
        CHECK(lcd_depth_windows(1, rb, re, rd, 1 << 30, &wb, &we, &ws) == 2 && ws[0] == 0xffffffffull << 30 && ws[3] == ws[0] && ws[5] == 1ull << 30 && wb[1] == (1ll << 30) + 1);
        free(wb); free(we); free(ws);
    }
    printf("%d checks ok\n", n_checks);
    return 0;
}
