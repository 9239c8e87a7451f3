// lcd_split_format.cpp -- the host-only side of the per-haplotype read sets (lcd_chunk_split_reads, lcd_split.cpp): the options' defaults and their check, the
// three FASTQ paths of a prefix with the test that no output of a run names another's file, and the prefix sums that place every record's entry and line.
// No HIP call or header in this file: a stand-alone program compiles it with the host compiler and its sanitizers (tests/c/split_sanitize.cpp).
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/lcd_hotpath.h"

extern "C" {

void lcd_split_opt_default(lcd_split_opt_t *o) {
    if (o) memset(o, 0, sizeof(*o));
}
int lcd_split_opt_check(const lcd_split_opt_t *o) {
    if (!o) return -4;
    if ((o->comment != 0 && o->comment != 1) || (o->list != 0 && o->list != 1)) return -4;
    return 0;
}

// paths[s]: the file of stream s (0 none, 1, 2).  prefix NULL: no FASTQ files, only the others are compared (paths may then be NULL)
int lcd_split_paths(const char *prefix, int gz, int n_other, const char *const *other, char *paths[3]) {
    if (paths) paths[0] = paths[1] = paths[2] = nullptr;
    if (n_other < 0 || (n_other > 0 && !other) || (prefix && !paths)) return -4;
    if (prefix && (!prefix[0] || !strcmp(prefix, "-"))) return -4;
    std::vector<std::string> all;
    try {
        if (prefix) for (const char *s : {".none", ".h1", ".h2"}) all.push_back(std::string(prefix) + s + (gz ? ".fastq.gz" : ".fastq"));
        for (int k = 0; k < n_other; ++k) if (other[k]) all.push_back(other[k]);
    } catch (const std::bad_alloc &) { return -11; }
    for (size_t a = 0; a < all.size(); ++a) {
        if (a >= (prefix ? 3u : 0u) && (all[a].empty() || all[a] == "-")) continue;        // (the other outputs have their own rules for stdout; it is no file)
        for (size_t b = a + 1; b < all.size(); ++b) if (all[a] == all[b]) return -4;
    }
    if (!prefix) return 0;
    for (int s = 0; s < 3; ++s) {
        paths[s] = (char *)malloc(all[s].size() + 1);
        if (!paths[s]) { for (int t = 0; t < s; ++t) { free(paths[t]); paths[t] = nullptr; } return -11; }
        memcpy(paths[s], all[s].c_str(), all[s].size() + 1);
    }
    return 0;
}

int lcd_split_offsets(int n, const int *stream, const uint64_t *fq_len, const uint64_t *list_len, uint64_t *fq_off, uint64_t *list_off, uint64_t totals[4]) {
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
    if (n < 0 || !totals || (n > 0 && (!stream || !fq_len || !list_len || !fq_off || !list_off))) return -4;
    for (int i = 0; i < n; ++i) if (stream[i] < -1 || stream[i] > 2) return -4;
    for (int i = 0; i < n; ++i) {
        const int s = stream[i];
        fq_off[i] = s < 0 ? 0 : totals[s]; list_off[i] = totals[3];
        if (s < 0) continue;
        if (fq_len[i] > UINT64_MAX - totals[s] || list_len[i] > UINT64_MAX - totals[3]) return -4;      // (lengths that cannot be a measure pass's)
        totals[s] += fq_len[i]; totals[3] += list_len[i];
    }
    return 0;
}

} // extern "C"
