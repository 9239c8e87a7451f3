// TEST ONLY, host code: the TE file reader (lcd_te_lib_from_fasta) and the formatter with read names (lcd_format_vcf_fields, lcd_alt_read_names) of
// longcalld_amd/csrc/lcd_emit.cpp -- a translation unit without a HIP call -- on their corner cases, built together with that file by the host compiler with
// -fsanitize=address,undefined: the empty file, a file without a final newline, CRLF, a lone header, FASTQ with a short quality string, a gzip file, a missing file;
// names of 1 and of 250 bytes, a line of more than 64 KB, alt_read_i outside the chunk's reads, AD[1] above the stored indices.  Prints "<checks> checks ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>
#include "lcd_hotpath.h"

static int n_checks = 0;
#define CHECK(x) do { ++n_checks; if (!(x)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static std::string put(const std::string &dir, const char *name, const std::string &bytes, bool gz = false) {
    const std::string p = dir + "/" + name;
    if (gz) { gzFile f = gzopen(p.c_str(), "wb"); gzwrite(f, bytes.data(), (unsigned)bytes.size()); gzclose(f); }
    else { FILE *f = fopen(p.c_str(), "wb"); fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); }
    return p;
}

struct Lib { lcd_te_lib_t *lib = nullptr; char **names = nullptr; int *lens = nullptr; int n = 0, rc = 0;
             explicit Lib(const std::string &p, int k = 0) { rc = lcd_te_lib_from_fasta(p.c_str(), k, &lib, &names, &lens, &n); }
             ~Lib() { lcd_te_lib_from_fasta_free(lib, names, lens, n); } };

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::string te;
    unsigned x = 12345;
    for (int i = 0; i < 300; ++i) { x = x * 1103515245u + 12345u; te += "ACGT"[(x >> 16) & 3]; }
    // ---- the reader ----
    { Lib l(put(dir, "empty.fa", "")); CHECK(l.rc == 0 && l.n == 0 && lcd_te_lib_n_seqs(l.lib) == 0); int rev = 7; CHECK(lcd_check_te_seq(l.lib, (const uint8_t *)te.data(), 120, &rev) == -1); }
    { Lib l(put(dir, "header_only.fa", ">")); CHECK(l.rc == 0 && l.n == 0); }
    { Lib l(put(dir, "name_only.fa", ">lonely")); CHECK(l.rc == 0 && l.n == 1 && !strcmp(l.names[0], "lonely") && l.lens[0] == 0); }
    { Lib l(put(dir, "no_newline.fa", ">a d\n" + te.substr(0, 100) + "\n" + te.substr(100))); CHECK(l.rc == 0 && l.n == 1 && l.lens[0] == 300 && !strcmp(l.names[0], "a"));
      int rev = 7; CHECK(lcd_check_te_seq(l.lib, (const uint8_t *)te.data() + 30, 150, &rev) == 0 && rev == 0); }
    { Lib l(put(dir, "crlf.fa", ">a\r\n" + te.substr(0, 150) + "\r\n" + te.substr(150) + "\r\n>hollow\r\n\r\n>b x\r\n\r\nAC\r\n")); CHECK(l.rc == 0 && l.n == 3 && l.lens[0] == 300 && l.lens[1] == 1 && l.lens[2] == 3); }   // (kseq keeps the lone \r of a one-byte sequence, src/kseq.h:140)
    { Lib l(put(dir, "short_qual.fq", "@q\n" + te + "\n+\nIIII\n")); CHECK(l.rc == 0 && l.n == 0); }
    { Lib l(put(dir, "plus_at_end.fq", "@q\nACGT\n+")); CHECK(l.rc == 0 && l.n == 0); }
    { Lib l(put(dir, "te.fa.gz", ">z\n" + te + "\n>y\n" + te.substr(10, 200) + "\n", true), 11); CHECK(l.rc == 0 && l.n == 2 && l.lens[1] == 200); }
    { Lib l(dir + "/no/such/file.fa"); CHECK(l.rc == -30 && !l.lib && !l.names && l.n == 0); }
    { Lib l(put(dir, "k.fa", ">a\nACGT\n"), 16); CHECK(l.rc == -4 && !l.lib); }
    // ---- the formatter ----
    lcd_call_opt_t opt; lcd_call_opt_default(&opt);
    const int n_reads = 400;
    std::vector<uint64_t> off; std::string pool;
    for (int i = 0; i < n_reads; ++i) { off.push_back(pool.size()); pool += i == 0 ? std::string("r") : i == 1 ? std::string(250, 'n') : "movie" + std::to_string(i) + "/" + std::string(190, 'z') + "/ccs"; pool += '\0'; }
    std::vector<int> all(n_reads); for (int i = 0; i < n_reads; ++i) all[i] = n_reads - 1 - i;
    uint8_t ref[1] = {0}, alt[1] = {2};
    lcd_var1_t v; memset(&v, 0, sizeof(v));
    v.pos = 10; v.type = 8; v.ref_len = 1; v.n_alt_allele = 1; v.alt_len[0] = 1; v.ref_bases = ref; v.alt_bases[0] = alt; v.GT[0] = 1; v.GT[1] = 1; v.DP = n_reads; v.AD[1] = n_reads;
    v.QUAL = 60; v.GQ = 60; v.is_clean = 1; v.n_alt_reads = n_reads; v.alt_read_i = all.data(); v.te_seq_i = -1; v.tsd_pos1 = v.tsd_pos2 = -1;
    char *text = nullptr; int mei = -1;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_ALL, n_reads, off.data(), pool.data(), &text, &mei) == 1 && text && strlen(text) > 65536 && mei == 0);
    { const std::string t = text; CHECK(t.size() > 252 && t.substr(t.size() - 253) == std::string(250, 'n') + ",r\n"); }
    free(text); text = nullptr;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_SV, n_reads, off.data(), pool.data(), &text, nullptr) == 1 && text && !strstr(text, "ALTREADS"));
    free(text); text = nullptr;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_NONE, 0, nullptr, nullptr, &text, nullptr) == 1 && text);
    free(text); text = nullptr;
    all[17] = n_reads;                                      // one past the chunk's reads
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_ALL, n_reads, off.data(), pool.data(), &text, nullptr) == -4 && !text);
    all[17] = -1;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_ALL, n_reads, off.data(), pool.data(), &text, nullptr) == -4 && !text);
    all[17] = 17; v.n_alt_reads = 5;                        // AD[1] above the stored indices
    char *one = nullptr;
    CHECK(lcd_alt_read_names(&v, n_reads, off.data(), pool.data(), &one) == -4 && !one);
    v.n_alt_reads = n_reads; v.AD[1] = 2;
    CHECK(lcd_alt_read_names(&v, n_reads, off.data(), pool.data(), &one) == 0 && one && std::string(one).find(',') != std::string::npos);
    free(one); one = nullptr;
    v.AD[1] = 0; opt.min_alt_dp = 0;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_ALL, 0, nullptr, nullptr, &text, nullptr) == 1 && text && strstr(text, ":.\n"));
    free(text); text = nullptr;
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, 3, n_reads, off.data(), pool.data(), &text, nullptr) == -4);
    CHECK(lcd_format_vcf_fields(&opt, "chr1", &v, 1, nullptr, LCD_RNAMES_ALL, n_reads, nullptr, nullptr, &text, nullptr) == -4);
    printf("%d checks ok\n", n_checks);
    return 0;
}
