// The host-only side of the methylation table (longcalld_amd/csrc/lcd_mods_format.cpp: options, strand combination, text) under the host compiler's sanitizers.
// argv[1]: a file of rows "pos strand c0 ... c8" (the case table's rows, written by tests/test_mods_sanitized.py); the text and the combined rows are printed for
// the test to compare.  Prints "<n> checks ok" as its last line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "lcd_hotpath.h"

static int n_checks = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); return 1; } ++n_checks; } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<int64_t> pos; std::vector<char> strand; std::vector<uint32_t> cnt;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long p; char s; unsigned c[9];
    while (fscanf(f, "%lld %c %u %u %u %u %u %u %u %u %u", &p, &s, &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &c[6], &c[7], &c[8]) == 11) {
        pos.push_back(p); strand.push_back(s); for (int z = 0; z < 9; ++z) cnt.push_back(c[z]);
    }
    fclose(f);
    const int n = (int)pos.size();
    CHECK(n > 50);
    lcd_mods_opt_t o; lcd_mods_opt_default(&o);
    CHECK(o.code == 'm' && o.threshold == 204 && !o.combine_strands && !o.ref_seq && lcd_mods_opt_check(&o) == 0);
    lcd_mods_opt_default(nullptr);
    o.threshold = 127; CHECK(lcd_mods_opt_check(&o) == -4); o.threshold = 255; CHECK(lcd_mods_opt_check(&o) == 0); o.code = 'x'; CHECK(lcd_mods_opt_check(&o) == -4);
    CHECK(lcd_mods_opt_check(nullptr) == -4);
    char *text = nullptr;
    // exact-size heap copies: a read or write past any array is an error here
    std::vector<int64_t> pos1(pos); std::vector<char> strand1(strand); std::vector<uint32_t> cnt1(cnt);
    CHECK(lcd_mods_format(n, pos1.data(), strand1.data(), cnt1.data(), "chrS", 'm', 1, &text) == 0 && text);
    printf("%s", text);
    { int lines = 0; for (const char *q = text; *q; ++q) lines += *q == '\n'; CHECK(lines == n + 1); }
    free(text); text = nullptr;
    CHECK(lcd_mods_format(0, nullptr, nullptr, nullptr, "c", 'h', 0, &text) == 0 && text && !text[0]); free(text); text = nullptr;
    CHECK(lcd_mods_format(0, nullptr, nullptr, nullptr, "c", 'h', 1, &text) == 0 && text && text[0] == '#'); free(text); text = nullptr;
    CHECK(lcd_mods_format(1, nullptr, strand1.data(), cnt1.data(), "c", 'm', 0, &text) == -4 && !text);
    CHECK(lcd_mods_format(1, pos1.data(), strand1.data(), cnt1.data(), nullptr, 'm', 0, &text) == -4);
    CHECK(lcd_mods_format(1, pos1.data(), strand1.data(), cnt1.data(), "c", 'q', 0, &text) == -4);
    CHECK(lcd_mods_format(1, pos1.data(), strand1.data(), cnt1.data(), "c", 'm', 0, nullptr) == -4);
    CHECK(lcd_mods_format(-1, pos1.data(), strand1.data(), cnt1.data(), "c", 'm', 0, &text) == -4);
    { char badc = 'x'; CHECK(lcd_mods_format(1, pos1.data(), &badc, cnt1.data(), "c", 'm', 0, &text) == -4); }
    {   // the widest line: every number at its maximum, a long contig name
        int64_t bp = INT64_MAX - 1; char bs = '.'; uint32_t bc[9]; for (int z = 0; z < 9; ++z) bc[z] = 0xffffffffu;
        const std::string name(300, 'c');
        CHECK(lcd_mods_format(1, &bp, &bs, bc, name.c_str(), 'h', 0, &text) == 0 && text);
        CHECK(strstr(text, "\t25769803770\t12884901885\t8589934590\t4294967295\t8589934590\t4294967295\t12884901885\n") != nullptr);
        free(text); text = nullptr;
    }
    const int m = lcd_mods_combine_rows(n, pos1.data(), strand1.data(), cnt1.data());
    CHECK(m > 0 && m <= n);
    unsigned long long before = 0, after = 0;
    for (uint32_t v : cnt) before += v;
    for (int k = 0; k < 9 * m; ++k) after += cnt1[k];
    CHECK(before == after);
    for (int k = 0; k < m; ++k) { CHECK(strand1[k] == '.'); if (k) CHECK(pos1[k] > pos1[k - 1]); }
    CHECK(lcd_mods_format(m, pos1.data(), strand1.data(), cnt1.data(), "chrS", 'm', 0, &text) == 0 && text);
    printf("--combined--\n%s", text);
    free(text); text = nullptr;
    CHECK(lcd_mods_combine_rows(0, nullptr, nullptr, nullptr) == 0 && lcd_mods_combine_rows(2, nullptr, nullptr, nullptr) == -4);
    CHECK(lcd_mods_combine_rows(m, pos1.data(), strand1.data(), cnt1.data()) == -4);           // (combined rows are not combined again: their strand is '.')
    { int64_t a[1] = {5}; char b[1] = {'-'}; uint32_t d[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0}; CHECK(lcd_mods_combine_rows(1, a, b, d) == 1 && a[0] == 4 && b[0] == '.'); }
    printf("--end--\n%d checks ok\n", n_checks);
    return 0;
}
