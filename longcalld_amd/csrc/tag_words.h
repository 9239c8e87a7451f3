// tag_words.h -- the host side of the cs / MD digar sources: the tag strings are O(events) long, so they are parsed on the host into EQX-shaped operation words
// that lcd_digar_kernel reads like a CIGAR.  Plain C++ without HIP: lcd_chunk.cpp includes it, and tests/c/tag_words_fuzz.cpp builds it alone under the host
// sanitizers.  `cs` / `md0` are NUL-terminated; nothing is read behind the NUL.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace lcd_tag_words __attribute__((visibility("hidden"))) {
inline bool is_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }
inline uint32_t opw(long long len, int op) { return ((uint32_t)len << 4) | (uint32_t)op; }
// collect_digar_from_cs_tag, src/bam_utils.c:876-976: clips from the first / last CIGAR operation, everything else from the cs string
inline bool cs_to_words(const uint32_t *cig, int n_cigar, const char *cs, std::vector<uint32_t> &w) {
    if (n_cigar <= 0 || !cs) return false;
    if ((cig[0] & 0xf) == 4 || (cig[0] & 0xf) == 5) w.push_back(cig[0]);
    while (*cs) {
        if (*cs == ':') { char *e; const long len = strtol(cs + 1, &e, 10); if (e == cs + 1 || len < 0) return false; cs = e; w.push_back(opw(len, 7)); }
        else if (*cs == '=' || *cs == '+' || *cs == '-') { const int op = *cs == '=' ? 7 : *cs == '+' ? 1 : 2; ++cs; long len = 0; while (is_alpha(*cs)) { ++len; ++cs; } w.push_back(opw(len, op)); }
        else if (*cs == '*') { if (!cs[1] || !cs[2]) return false; w.push_back(opw(1, 8)); cs += 3; }
        else if (*cs == '~') { ++cs; while (is_alpha(*cs) || is_digit(*cs)) ++cs; }   // intron: stepped over without moving pos (:951-953)
        else return false;                                                             // the reference exits (:955)
    }
    const uint32_t last = cig[n_cigar - 1];
    if ((last & 0xf) == 4 || (last & 0xf) == 5) w.push_back(last);
    return true;
}
// collect_digar_from_MD_tag, src/bam_utils.c:1035-1134: 'M' operations split by the MD string ('=' runs that may continue over an insertion into the
// next 'M', one 'X' per letter), deletions step over "^LETTERS", a "0" after either is skipped
inline bool md_to_words(const uint32_t *cig, int n_cigar, const char *md0, std::vector<uint32_t> &w) {
    if (!md0) return false;
    const char *md = md0, *md_end = md0 + strlen(md0); long md_i = 0;
    auto at = [&](long k) -> char { const char *q = md + k; return (q >= md0 && q < md_end) ? *q : '\0'; };
    long last_eq = 0;
    for (int i = 0; i < n_cigar; ++i) {
        const int op = cig[i] & 0xf; const long len = cig[i] >> 4;
        if (op == 0) {
            long m = len;
            while (1) {
                if (last_eq > 0) {
                    if (last_eq >= m) { w.push_back(opw(m, 7)); last_eq -= m; m = 0; }
                    else { w.push_back(opw(last_eq, 7)); m -= last_eq; md_i = 0; last_eq = 0; }
                } else if (is_digit(at(md_i))) {
                    char *e; long eq = strtol(md + md_i, &e, 10); md = e;
                    bool emit = true;
                    if (eq > m) { last_eq = eq - m; eq = m; }
                    else if (eq == 0) { md_i = 0; emit = false; }
                    if (emit) { w.push_back(opw(eq, 7)); m -= eq; md_i = 0; }
                    else continue;
                } else if (is_alpha(at(md_i))) {
                    w.push_back(opw(1, 8)); m -= 1;
                    if (at(md_i + 1) == '\0' || at(md_i + 1) != '0') md_i++; else md_i += 2;
                } else return false;                                                   // "MD and CIGAR do not match": the reference exits (:1088)
                if (m <= 0) break;
            }
        } else if (op == 2) {
            w.push_back(cig[i]);
            md_i++;
            while (at(md_i) && is_alpha(at(md_i))) md_i++;
            if (at(md_i) == '0') md_i++;
        } else if (op == 1 || op == 4 || op == 5 || op == 3) w.push_back(cig[i]);
        else if (op == 7 || op == 8) return false;                                     // '=' / 'X' next to an MD tag: the reference exits (:1134)
    }
    return true;
}
} // namespace lcd_tag_words
