// TEST ONLY, host code: lcd_refine_log_* (longcalld_amd/csrc/lcd_refine_log.cpp) with lcd_update_digars_from_msa1 (lcd_emit.cpp) -- translation units without a HIP
// call -- built by the host compiler with -fsanitize=address,undefined and run over refine logs a test wrote to a file: tests/test_refine_log_sanitized.py dumps the
// logs and digars of its chunks and compares the final lists this program prints with the oracle's.
// file (little-endian int64 words): n_reads, then per read [qlen, n_digar, n_digar x (pos, type, len, qi, is_low_qual)], then n_entries, then per entry
// [read_id, cover, read_beg, read_end, reg_beg, reg_end, pass, aln_len] followed by aln_len target bytes and aln_len query bytes.
// output: "rejected <n>", then per touched read "<read> <n_digar>" and its digars, one per line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lcd_hotpath.h"

static bool rd(FILE *f, int64_t &v) { return fread(&v, 8, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <dump file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n_reads = 0, v = 0;
    if (!rd(f, n_reads) || n_reads < 0) return 2;
    std::vector<uint64_t> off(1, 0); std::vector<lcd_digar_t> dg; std::vector<int> qlen;
    for (int64_t r = 0; r < n_reads; ++r) {
        int64_t q = 0, n = 0;
        if (!rd(f, q) || !rd(f, n)) return 2;
        qlen.push_back((int)q);
        for (int64_t k = 0; k < n; ++k) {
            int64_t x[5];
            for (int j = 0; j < 5; ++j) if (!rd(f, x[j])) return 2;
            lcd_digar_t d; d.pos = x[0]; d.type = (int)x[1]; d.len = (int)x[2]; d.qi = (int)x[3]; d.is_low_qual = (int)x[4];
            dg.push_back(d);
        }
        off.push_back(dg.size());
    }
    lcd_refine_log_t *log = lcd_refine_log_create();
    if (!log) return 3;
    int64_t n_entries = 0;
    if (!rd(f, n_entries)) return 2;
    for (int64_t i = 0; i < n_entries; ++i) {
        int64_t h[8];
        for (int j = 0; j < 8; ++j) if (!rd(f, h[j])) return 2;
        std::vector<uint8_t> t((size_t)h[7] + 1), q((size_t)h[7] + 1);
        if (h[7] && (fread(t.data(), 1, (size_t)h[7], f) != (size_t)h[7] || fread(q.data(), 1, (size_t)h[7], f) != (size_t)h[7])) return 2;
        lcd_refine_entry_t e = {(int)h[0], (int)h[1], (int)h[2], (int)h[3], (int)h[7], (int)h[6], h[4], h[5], t.data(), q.data()};
        if (lcd_refine_log_append(log, &e)) return 4;
    }
    fclose(f);
    if (lcd_refine_log_n_entries(log) != n_entries) return 5;
    for (int64_t i = 0; i < n_entries; ++i) { lcd_refine_entry_t e; if (lcd_refine_log_entry(log, i, &e) || e.aln_len < 0) return 5; }
    lcd_refine_entry_t none;
    if (lcd_refine_log_entry(log, n_entries, &none) != -4 || lcd_refine_log_append(log, nullptr) != -4) return 5;      // the refusals read nothing
    int n_touched = 0; int *ids = nullptr; uint64_t *toff = nullptr; lcd_digar_t *tdg = nullptr; int64_t rej = 0;
    if (lcd_refine_log_apply(log, (int)n_reads, off.data(), dg.data(), qlen.data(), &n_touched, &ids, &toff, &tdg, &rej)) return 6;
    printf("rejected %lld\n", (long long)rej);
    for (int t = 0; t < n_touched; ++t) {
        printf("%d %llu\n", ids[t], (unsigned long long)(toff[t + 1] - toff[t]));
        for (uint64_t k = toff[t]; k < toff[t + 1]; ++k) printf("%lld %d %d %d %d\n", (long long)tdg[k].pos, tdg[k].type, tdg[k].len, tdg[k].qi, tdg[k].is_low_qual);
    }
    free(ids); free(toff); free(tdg);
    if (n_reads > 0) {      // a log that names a read outside the chunk is refused before anything is read
        int nt = 0; int *a = nullptr; uint64_t *b = nullptr; lcd_digar_t *c = nullptr;
        lcd_refine_log_t *bad = lcd_refine_log_create();
        uint8_t z = 0;
        lcd_refine_entry_t e = {(int)n_reads, 12, 0, 0, 1, 0, 1, 1, &z, &z};
        if (lcd_refine_log_append(bad, &e) || lcd_refine_log_apply(bad, (int)n_reads, off.data(), dg.data(), qlen.data(), &nt, &a, &b, &c, nullptr) != -4 || a || b || c) return 7;
        lcd_refine_log_free(bad);
    }
    lcd_refine_log_free(log);
    return 0;
}
