// lcd_refine_log.cpp -- the refine log of a chunk (what update_digars_from_aln_str, src/align.c:1745-1756, would have applied while the chunk was called) and its
// application to a host copy of the chunk's digars.  No HIP call or header in this file: a stand-alone program compiles it, with lcd_emit.cpp
// (lcd_update_digars_from_msa1), by the host compiler and its sanitizers (tests/c/refine_log_sanitize.cpp).
#include <climits>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include "../../include/lcd_hotpath.h"

// defined in lcd_bai.cpp (sets lcd_last_error's string); absent from a stand-alone program
extern "C" __attribute__((weak)) void lcd_index_set_last_error(const char *m);
namespace {
int set_err(int code, const std::string &m) { if (lcd_index_set_last_error) lcd_index_set_last_error(m.c_str()); return code; }
}

struct lcd_refine_log_s {
    struct Entry { int read_id, cover, read_beg, read_end, aln_len, pass; int64_t reg_beg, reg_end; size_t rows; };   // rows: offset of the target row; the query row follows it
    std::vector<Entry> e; std::vector<uint8_t> pool;
};

extern "C" {

lcd_refine_log_t *lcd_refine_log_create(void) { return new (std::nothrow) lcd_refine_log_s(); }
void lcd_refine_log_free(lcd_refine_log_t *log) { delete log; }
int64_t lcd_refine_log_n_entries(const lcd_refine_log_t *log) { return log ? (int64_t)log->e.size() : 0; }
int64_t lcd_refine_log_row_bytes(const lcd_refine_log_t *log) { return log ? (int64_t)log->pool.size() : 0; }
int lcd_refine_log_append(lcd_refine_log_t *log, const lcd_refine_entry_t *x) {
    if (!log || !x || x->aln_len < 0 || (x->aln_len > 0 && (!x->target || !x->query))) return set_err(-4, "lcd_refine_log_append: NULL argument or negative aln_len");
    lcd_refine_log_s::Entry n = {x->read_id, x->cover, x->read_beg, x->read_end, x->aln_len, x->pass, x->reg_beg, x->reg_end, log->pool.size()};
    log->pool.insert(log->pool.end(), x->target, x->target + x->aln_len);
    log->pool.insert(log->pool.end(), x->query, x->query + x->aln_len);
    log->e.push_back(n);
    return 0;
}
int lcd_refine_log_entry(const lcd_refine_log_t *log, int64_t i, lcd_refine_entry_t *out) {
    if (!log || !out || i < 0 || i >= (int64_t)log->e.size()) return set_err(-4, "lcd_refine_log_entry: no such entry");
    const lcd_refine_log_s::Entry &n = log->e[(size_t)i];
    out->read_id = n.read_id; out->cover = n.cover; out->read_beg = n.read_beg; out->read_end = n.read_end; out->aln_len = n.aln_len; out->pass = n.pass;
    out->reg_beg = n.reg_beg; out->reg_end = n.reg_end; out->target = log->pool.data() + n.rows; out->query = out->target + n.aln_len;
    return 0;
}

int lcd_refine_log_apply(const lcd_refine_log_t *log, int n_reads, const uint64_t *digar_off, const lcd_digar_t *digars, const int *qlen, int *n_touched,
                         int **touched_reads, uint64_t **touched_off, lcd_digar_t **touched_digars, int64_t *n_rejected) {
    const std::string W = "lcd_refine_log_apply";
    if (n_touched) *n_touched = 0;
    if (touched_reads) *touched_reads = nullptr;
    if (touched_off) *touched_off = nullptr;
    if (touched_digars) *touched_digars = nullptr;
    if (n_rejected) *n_rejected = 0;
    if (!log || n_reads < 0 || !n_touched || !touched_reads || !touched_off || !touched_digars || (n_reads > 0 && (!digar_off || !qlen))) return set_err(-4, W + ": NULL argument");
    // the running copy: a read's own list until an entry replaces it.  Entries of one read are applied front to back: the cut of the list decides the cs text
    std::vector<std::vector<lcd_digar_t>> cur(n_reads); std::vector<char> own(n_reads, 0);
    int64_t rejected = 0;
    for (const lcd_refine_log_s::Entry &n : log->e) {
        const int r = n.read_id;
        if (r < 0 || r >= n_reads) return set_err(-4, W + ": an entry names a read outside [0, n_reads)");
        if (!own[r]) {
            if (digar_off[r + 1] < digar_off[r] || digar_off[r + 1] - digar_off[r] > (uint64_t)INT32_MAX || (digar_off[r + 1] > digar_off[r] && !digars)) return set_err(-4, W + ": digar_off falls");
            cur[r].assign(digars + digar_off[r], digars + digar_off[r + 1]); own[r] = 1;
        }
        lcd_digar_t *out = nullptr; int n_out = 0;
        const uint8_t *t = log->pool.data() + n.rows;
        const int rc = lcd_update_digars_from_msa1(cur[r].data(), (int)cur[r].size(), qlen[r], n.aln_len, t, t + n.aln_len, n.cover, n.reg_beg, n.reg_end, n.read_beg, n.read_end, &out, &n_out);
        if (rc < 0) { free(out); return rc; }
        if (rc == 0) cur[r].assign(out, out + n_out);        // 1: double_check_digar rejected the result, the read keeps its list; 2: the read covers neither end
        else if (rc == 1) ++rejected;
        free(out);
    }
    int m = 0; uint64_t tot = 0;
    for (int r = 0; r < n_reads; ++r) if (own[r]) { ++m; tot += cur[r].size(); }
    int *ids = (int *)malloc(((size_t)m + 1) * sizeof(int)); uint64_t *off = (uint64_t *)malloc(((size_t)m + 1) * sizeof(uint64_t));
    lcd_digar_t *dg = (lcd_digar_t *)malloc((tot + 1) * sizeof(lcd_digar_t));
    if (!ids || !off || !dg) { free(ids); free(off); free(dg); return set_err(-11, W + ": out of memory"); }
    uint64_t w = 0; int k = 0;
    for (int r = 0; r < n_reads; ++r) if (own[r]) { ids[k] = r; off[k] = w; if (!cur[r].empty()) memcpy(dg + w, cur[r].data(), cur[r].size() * sizeof(lcd_digar_t)); w += cur[r].size(); ++k; }
    off[m] = w;
    *n_touched = m; *touched_reads = ids; *touched_off = off; *touched_digars = dg;
    if (n_rejected) *n_rejected = rejected;
    return 0;
}

} // extern "C"
