// The host-only side of the per-haplotype read sets (longcalld_amd/csrc/lcd_split_format.cpp: options, paths, prefix sums) under the host compiler's sanitizers.
// argv[1]: a file of tables: a line "T" starts a table, the lines "stream fq_len list_len" behind it are its rows (written by tests/test_split_sanitized.py from
// the case table's measure rows, seeded rows and lengths near the 64-bit limit).  Per table one line "fq_off list_off" per row and a line "= t0 t1 t2 t3" are
// printed, "--table--" between tables, for the test to compare; behind "--end--" the paths of some prefixes.  Prints "<n> checks ok" as its last line.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lcd_hotpath.h"

static int n_checks = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); return 1; } ++n_checks; } while (0)

struct Table { std::vector<int> stream; std::vector<uint64_t> fq, ls; };

static int one(const Table &t) {
    const int n = (int)t.stream.size();
    // exact-size heap copies: a read or write past any array is an error here
    std::vector<int> stream(t.stream); std::vector<uint64_t> fq(t.fq), ls(t.ls), fo((size_t)n), lo((size_t)n);
    uint64_t tot[4] = {9, 9, 9, 9};
    CHECK(lcd_split_offsets(n, stream.data(), fq.data(), ls.data(), fo.data(), lo.data(), tot) == 0);
    uint64_t sum[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        printf("%" PRIu64 " %" PRIu64 "\n", fo[i], lo[i]);
        if (stream[i] < 0) continue;
        CHECK(fo[i] == sum[stream[i]] && lo[i] == sum[3]);                       // exclusive prefix sums per stream
        sum[stream[i]] += fq[i]; sum[3] += ls[i];
    }
    CHECK(sum[0] == tot[0] && sum[1] == tot[1] && sum[2] == tot[2] && sum[3] == tot[3]);
    printf("= %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot[0], tot[1], tot[2], tot[3]);
    if (n) {     // a stream outside -1 ... 2 and a NULL array are refused, and the totals read as zero
        std::vector<int> bad(stream); bad[n - 1] = 3;
        CHECK(lcd_split_offsets(n, bad.data(), fq.data(), ls.data(), fo.data(), lo.data(), tot) == -4 && !tot[0] && !tot[1] && !tot[2] && !tot[3]);
        bad[n - 1] = -2;
        CHECK(lcd_split_offsets(n, bad.data(), fq.data(), ls.data(), fo.data(), lo.data(), tot) == -4);
        CHECK(lcd_split_offsets(n, stream.data(), nullptr, ls.data(), fo.data(), lo.data(), tot) == -4);
        CHECK(lcd_split_offsets(n, stream.data(), fq.data(), ls.data(), fo.data(), lo.data(), nullptr) == -4);
    }
    return 0;
}

static int paths() {
    char *p[3] = {(char *)1, (char *)1, (char *)1};
    const std::string longp(5000, 'q');
    for (const std::string &pre : {std::string("p"), std::string("dir.with.dots/x"), longp}) {
        for (int gz = 0; gz < 2; ++gz) {
            CHECK(lcd_split_paths(pre.c_str(), gz, 0, nullptr, p) == 0 && p[0] && p[1] && p[2]);
            for (int s = 0; s < 3; ++s) { if (pre.size() < 100) printf("%s\n", p[s]); CHECK(strlen(p[s]) == pre.size() + (s ? 3 : 5) + (gz ? 9 : 6)); free(p[s]); }
        }
    }
    const char *other[5] = {"a.vcf", nullptr, "-", "", "p.h1.fastq"};
    CHECK(lcd_split_paths("p", 1, 5, other, p) == 0);                            // (p.h1.fastq.gz is another file)
    for (char *q : p) free(q);
    CHECK(lcd_split_paths("p", 0, 5, other, p) == -4 && !p[0] && !p[1] && !p[2]);
    CHECK(lcd_split_paths("p", 0, 4, other, p) == 0);
    for (char *q : p) free(q);
    const char *twice[3] = {"x", "y", "x"}, *dash[2] = {"-", "-"};
    CHECK(lcd_split_paths("p", 0, 3, twice, p) == -4 && lcd_split_paths(nullptr, 0, 3, twice, nullptr) == -4 && lcd_split_paths(nullptr, 0, 2, twice, nullptr) == 0);
    CHECK(lcd_split_paths(nullptr, 0, 2, dash, nullptr) == 0);
    CHECK(lcd_split_paths("", 0, 0, nullptr, p) == -4 && lcd_split_paths("-", 1, 0, nullptr, p) == -4 && lcd_split_paths("p", 0, -1, nullptr, p) == -4);
    CHECK(lcd_split_paths("p", 0, 1, nullptr, p) == -4 && lcd_split_paths("p", 0, 0, nullptr, nullptr) == -4);
    lcd_split_opt_t o; memset(&o, 0x7f, sizeof(o));
    CHECK(lcd_split_opt_check(&o) == -4);
    lcd_split_opt_default(&o); lcd_split_opt_default(nullptr);
    CHECK(lcd_split_opt_check(&o) == 0 && !o.comment && !o.list && !o.reserved[0] && !o.reserved[1] && lcd_split_opt_check(nullptr) == -4);
    o.comment = 1; o.list = 1; CHECK(lcd_split_opt_check(&o) == 0);
    o.list = 2; CHECK(lcd_split_opt_check(&o) == -4);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: split_sanitize tables.txt\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<Table> tables;
    char line[256];
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == 'T') { tables.emplace_back(); continue; }
        int s; uint64_t a, b;
        if (sscanf(line, "%d %" SCNu64 " %" SCNu64, &s, &a, &b) != 3 || tables.empty()) { fprintf(stderr, "bad line: %s", line); fclose(f); return 2; }
        tables.back().stream.push_back(s); tables.back().fq.push_back(a); tables.back().ls.push_back(b);
    }
    fclose(f);
    for (size_t k = 0; k < tables.size(); ++k) {
        if (k) printf("--table--\n");
        if (one(tables[k])) return 1;
    }
    // lengths that overflow 64 bits are refused, not wrapped
    { int st[2] = {1, 1}; uint64_t fq[2] = {UINT64_MAX - 3, 4}, ls[2] = {0, 0}, fo[2], lo[2], tot[4]; CHECK(lcd_split_offsets(2, st, fq, ls, fo, lo, tot) == -4); fq[1] = 3; CHECK(lcd_split_offsets(2, st, fq, ls, fo, lo, tot) == 0 && tot[1] == UINT64_MAX); }
    { uint64_t tot[4]; CHECK(lcd_split_offsets(0, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == 0 && lcd_split_offsets(-1, nullptr, nullptr, nullptr, nullptr, nullptr, tot) == -4); }
    printf("--end--\n");
    if (paths()) return 1;
    printf("%d checks ok\n", n_checks);
    return 0;
}
