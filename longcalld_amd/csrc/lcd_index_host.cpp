// lcd_index_host.cpp -- the host half of the index writers, WITHOUT a HIP call or header, so that a stand-alone program can compile this file with the host compiler
// and its sanitizers:
//   * the finisher of the .bai builder: accumulated chunk list, window arrays and counters -> the bytes of SAM specification 5.2 (rules 6-9 of include/lcd_hotpath.h);
//   * lcd_bai_from_records: rules 2-9 on a record table -- what bai_kernel.hip computes per record, as a plain loop -- then the same finisher;
//   * lcd_fai_build: the .fai of a FASTA file (htslib's fai_build is not in the reference checkout; the reference's FASTA loader builds a missing .fai through it).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../../include/lcd_hotpath.h"
#include "lcd_bai_internal.h"

// defined in lcd_bai.cpp (sets lcd_last_error's string); absent from a stand-alone program
extern "C" __attribute__((weak)) void lcd_index_set_last_error(const char *m);

namespace lcd_bai {
namespace { thread_local std::string g_index_err; }
int index_err(int code, const std::string &m) { g_index_err = m; if (lcd_index_set_last_error) lcd_index_set_last_error(m.c_str()); return code; }
const char *index_host_error() { return g_index_err.c_str(); }

namespace {
void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
void put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
} // namespace

void serialize(const Accum &a, std::vector<uint8_t> &out) {
    out.clear();
    out.push_back('B'); out.push_back('A'); out.push_back('I'); out.push_back(1);
    put32(out, (uint32_t)a.n_ref);
    // the runs by (refid, bin), file order kept inside a bin
    std::vector<uint32_t> ord(a.chunks.size());
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
        const Chunk &p = a.chunks[x], &q = a.chunks[y];
        return p.refid != q.refid ? p.refid < q.refid : p.bin < q.bin;
    });
    size_t k = 0;
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    for (int t = 0; t < a.n_ref; ++t) {
        const Contig &c = a.ctg[(size_t)t];
        while (k < ord.size() && a.chunks[ord[k]].refid < t) ++k;
        if (c.n_mapped + c.n_unmapped == 0) { put32(out, 0); put32(out, 0); continue; }
        const size_t at_nbin = out.size(); put32(out, 0);
        uint32_t n_bin = 0;
        while (k < ord.size() && a.chunks[ord[k]].refid == t) {
            const uint32_t bin = a.chunks[ord[k]].bin;
            ch.clear();
            for (; k < ord.size() && a.chunks[ord[k]].refid == t && a.chunks[ord[k]].bin == bin; ++k) {
                const Chunk &x = a.chunks[ord[k]];
                if (!ch.empty() && (ch.back().second >> 16) >= (x.vbeg >> 16)) ch.back().second = std::max(ch.back().second, x.vend);   // rule 6: no member twice for one bin
                else ch.emplace_back(x.vbeg, x.vend);
            }
            put32(out, bin); put32(out, (uint32_t)ch.size());
            for (auto &p : ch) { put64(out, p.first); put64(out, p.second); }
            ++n_bin;
        }
        put32(out, 37450); put32(out, 2);
        put64(out, c.first_vbeg); put64(out, c.last_vend); put64(out, (uint64_t)c.n_mapped); put64(out, (uint64_t)c.n_unmapped);
        ++n_bin;
        for (int b = 0; b < 4; ++b) out[at_nbin + (size_t)b] = (uint8_t)(n_bin >> (8 * b));
        size_t n_intv = c.win.size();
        while (n_intv > 0 && c.win[n_intv - 1] == ~0ull) --n_intv;
        put32(out, (uint32_t)n_intv);
        uint64_t prev = 0;
        for (size_t w = 0; w < n_intv; ++w) { if (c.win[w] != ~0ull) prev = c.win[w]; put64(out, prev); }
    }
    put64(out, a.n_no_coor);
}

// rules 6-10 of the section "VCF indexes": the uncompressed bytes of a .tbi or a .csi
int serialize_tbx(const VAccum &v, std::vector<uint8_t> &out) {
    const std::string W = "lcd_vcf_index";
    const Accum &a = v.a;
    const bool csi = v.format == LCD_VIDX_CSI;
    int depth = 5;
    if (!csi) {
        if (v.max_end > (1ll << 29)) return index_err(LCD_ERR_VIDX_CSI, W + ": a line ends behind 2^29 (" + std::to_string((long long)v.max_end) + "): TBI cannot hold it, ask for CSI");
    } else {
        const int64_t want = v.max_contig_len > 0 ? v.max_contig_len : v.max_end;
        while (depth < VIDX_MAX_DEPTH && (1ll << (14 + 3 * depth)) < want) ++depth;
        if (v.max_end > (1ll << (14 + 3 * depth)))
            return index_err(LCD_ERR_VIDX_CSI, W + ": a line ends at " + std::to_string((long long)v.max_end) + ", behind what a CSI of depth " + std::to_string(depth) + " (from the header's contig lengths) holds");
    }
    out.clear();
    std::vector<uint8_t> aux;
    put32(aux, 2); put32(aux, 1); put32(aux, 2); put32(aux, 0); put32(aux, (uint32_t)'#'); put32(aux, 0);
    size_t l_nm = 0;
    for (const std::string &s : v.names) l_nm += s.size() + 1;
    put32(aux, (uint32_t)l_nm);
    for (const std::string &s : v.names) { aux.insert(aux.end(), s.begin(), s.end()); aux.push_back(0); }
    if (csi) {
        out.push_back('C'); out.push_back('S'); out.push_back('I'); out.push_back(1);
        put32(out, 14); put32(out, (uint32_t)depth); put32(out, (uint32_t)aux.size());
        out.insert(out.end(), aux.begin(), aux.end());
        put32(out, (uint32_t)a.n_ref);
    } else {
        out.push_back('T'); out.push_back('B'); out.push_back('I'); out.push_back(1);
        put32(out, (uint32_t)a.n_ref);
        out.insert(out.end(), aux.begin(), aux.end());
    }
    const uint32_t pseudo = (uint32_t)((((1ull << (3 * depth + 3)) - 1) / 7) + 1);
    // the runs by (tid, bin number at this depth), file order kept inside a bin
    std::vector<uint32_t> ord(a.chunks.size()), bin(a.chunks.size());
    for (size_t i = 0; i < ord.size(); ++i) { ord[i] = (uint32_t)i; bin[i] = vidx_bin(a.chunks[i].bin, depth); }
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return a.chunks[x].refid != a.chunks[y].refid ? a.chunks[x].refid < a.chunks[y].refid : bin[x] < bin[y]; });
    size_t k = 0;
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    std::vector<uint64_t> nxt;                  // CSI: per window the value of the first set window at or behind it
    for (int t = 0; t < a.n_ref; ++t) {
        const Contig &c = a.ctg[(size_t)t];
        while (k < ord.size() && a.chunks[ord[k]].refid < t) ++k;
        if (c.n_mapped == 0) { put32(out, 0); if (!csi) put32(out, 0); continue; }
        if (csi) {
            nxt.assign(c.win.size() + 1, ~0ull);
            for (size_t w = c.win.size(); w-- > 0;) nxt[w] = c.win[w] != ~0ull ? c.win[w] : nxt[w + 1];
        }
        const size_t at_nbin = out.size(); put32(out, 0);
        uint32_t n_bin = 0;
        while (k < ord.size() && a.chunks[ord[k]].refid == t) {
            const uint32_t b = bin[ord[k]], key = a.chunks[ord[k]].bin;
            ch.clear();
            for (; k < ord.size() && a.chunks[ord[k]].refid == t && bin[ord[k]] == b; ++k) {
                const Chunk &x = a.chunks[ord[k]];
                if (!ch.empty() && (ch.back().second >> 16) >= (x.vbeg >> 16)) ch.back().second = std::max(ch.back().second, x.vend);
                else ch.emplace_back(x.vbeg, x.vend);
            }
            put32(out, b);
            if (csi) {                          // rule 9: the first set 16 kb window inside the bin's span
                const uint64_t w0 = (uint64_t)(key & 0xfffffffu) << (3 * (key >> 28));
                put64(out, w0 < nxt.size() ? nxt[(size_t)w0] : ~0ull);
            }
            put32(out, (uint32_t)ch.size());
            for (auto &p : ch) { put64(out, p.first); put64(out, p.second); }
            ++n_bin;
        }
        put32(out, pseudo);
        if (csi) put64(out, 0);
        put32(out, 2);
        put64(out, c.first_vbeg); put64(out, c.last_vend); put64(out, (uint64_t)c.n_mapped); put64(out, 0);
        ++n_bin;
        for (int b = 0; b < 4; ++b) out[at_nbin + (size_t)b] = (uint8_t)(n_bin >> (8 * b));
        if (!csi) {
            size_t n_intv = c.win.size();
            while (n_intv > 0 && c.win[n_intv - 1] == ~0ull) --n_intv;
            put32(out, (uint32_t)n_intv);
            uint64_t prev = 0;
            for (size_t w = 0; w < n_intv; ++w) { if (c.win[w] != ~0ull) prev = c.win[w]; put64(out, prev); }
        }
    }
    put64(out, 0);
    return 0;
}
} // namespace lcd_bai

using namespace lcd_bai;

extern "C" int lcd_tbx_from_records(int format, int n_ref, const char *const *names, int64_t max_contig_len, int64_t n_rec, const int *tid, const int64_t *beg, const int64_t *end,
                                    const uint64_t *vbeg, const uint64_t *vend, uint8_t **bytes, size_t *n) {
    const std::string W = "lcd_tbx_from_records";
    if (bytes) *bytes = nullptr;
    if (n) *n = 0;
    if (!bytes || !n || n_ref < 0 || n_rec < 0 || (n_ref > 0 && !names) || (n_rec > 0 && (!tid || !beg || !end || !vbeg || !vend)) || (format != LCD_VIDX_TBI && format != LCD_VIDX_CSI) ||
        max_contig_len < 0) return index_err(-4, W + ": NULL argument, negative count or unknown format");
    VAccum v; v.format = format; v.max_contig_len = max_contig_len; v.a.n_ref = n_ref; v.a.ctg.resize((size_t)n_ref);
    for (int t = 0; t < n_ref; ++t) { if (!names[t] || !names[t][0]) return index_err(-4, W + ": empty contig name"); v.names.emplace_back(names[t]); }
    int p_tid = -1; int64_t p_beg = -1; uint32_t p_key = 0;
    for (int64_t i = 0; i < n_rec; ++i) {
        const std::string R = W + ": data line " + std::to_string((long long)i);
        if (tid[i] < 0 || tid[i] >= n_ref || beg[i] < 0) return index_err(-4, R + " names a contig outside the table, or has a negative position");
        if (tid[i] < p_tid) return index_err(LCD_ERR_VIDX_ORDER, R + ": contig " + v.names[(size_t)tid[i]] + " reappears after another contig");
        if (tid[i] == p_tid && beg[i] < p_beg) return index_err(LCD_ERR_VIDX_ORDER, R + " lies in front of the line before it: the file is not sorted by position");
        if (end[i] <= beg[i]) return index_err(-4, R + " has an empty interval");
        if (end[i] > (1ll << (14 + 3 * VIDX_MAX_DEPTH)) || (format == LCD_VIDX_TBI && end[i] > (1ll << 29)))
            return index_err(LCD_ERR_VIDX_CSI, R + " ends behind 2^" + (format == LCD_VIDX_TBI ? "29: TBI cannot hold it, ask for CSI" : "38: no CSI this library writes holds it"));
        const uint32_t key = vidx_key(beg[i], end[i]);
        Contig &c = v.a.ctg[(size_t)tid[i]];
        if (tid[i] != p_tid || key != p_key) v.a.chunks.push_back(Chunk{tid[i], key, vbeg[i], vend[i]});
        else v.a.chunks.back().vend = vend[i];
        ++c.n_mapped;
        c.first_vbeg = std::min(c.first_vbeg, vbeg[i]); c.last_vend = std::max(c.last_vend, vend[i]);
        const size_t w1 = (size_t)((end[i] - 1) >> 14);
        if (c.win.size() <= w1) c.win.resize(w1 + 1, ~0ull);
        for (size_t w = (size_t)(beg[i] >> 14); w <= w1; ++w) c.win[w] = std::min(c.win[w], vbeg[i]);
        v.max_end = std::max(v.max_end, end[i]);
        p_tid = tid[i]; p_beg = beg[i]; p_key = key;
    }
    std::vector<uint8_t> out;
    if (int rc = serialize_tbx(v, out)) return rc;
    *bytes = (uint8_t *)malloc(out.size() + 1);
    if (!*bytes) return index_err(-4, W + ": out of memory");
    memcpy(*bytes, out.data(), out.size());
    *n = out.size();
    return 0;
}

extern "C" int lcd_bai_from_records(int n_ref, int64_t n_rec, const int *refid, const int64_t *beg, const int64_t *end, const int *flag, const uint64_t *vbeg, const uint64_t *vend,
                                    uint8_t **bytes, size_t *n) {
    const std::string W = "lcd_bai_from_records";
    if (bytes) *bytes = nullptr;
    if (n) *n = 0;
    if (!bytes || !n || n_ref < 0 || n_rec < 0 || (n_rec > 0 && (!refid || !beg || !end || !flag || !vbeg || !vend))) return index_err(-4, W + ": NULL argument or negative count");
    Accum a; a.n_ref = n_ref; a.ctg.resize((size_t)n_ref);
    bool seen_no_coor = false; int p_ref = -1; int64_t p_pos = -1; uint32_t p_bin = 0; bool have_prev = false;
    for (int64_t i = 0; i < n_rec; ++i) {
        if (refid[i] < 0 || beg[i] < 0) { ++a.n_no_coor; seen_no_coor = true; continue; }
        if (refid[i] >= n_ref) return index_err(-4, W + ": record " + std::to_string(i) + " names a contig outside the table");
        if (seen_no_coor) return index_err(LCD_ERR_BAI_ORDER, W + ": record " + std::to_string(i) + " has a coordinate and follows a record without one: the file is not sorted");
        if (have_prev && (refid[i] < p_ref || (refid[i] == p_ref && beg[i] < p_pos)))
            return index_err(LCD_ERR_BAI_ORDER, W + ": record " + std::to_string(i) + " lies in front of the record before it: the file is not sorted by coordinate");
        if (end[i] <= beg[i]) return index_err(-4, W + ": record " + std::to_string(i) + " has an empty interval");
        if (end[i] > (1ll << 29)) return index_err(LCD_ERR_BAI_CSI, W + ": record " + std::to_string(i) + " ends behind 2^29: only BAI is supported, not CSI");
        const uint32_t bin = reg2bin(beg[i], end[i]);
        Contig &c = a.ctg[(size_t)refid[i]];
        if (!have_prev || refid[i] != p_ref || bin != p_bin) a.chunks.push_back(Chunk{refid[i], bin, vbeg[i], vend[i]});
        else a.chunks.back().vend = vend[i];
        ++((flag[i] & 4) ? c.n_unmapped : c.n_mapped);
        c.first_vbeg = std::min(c.first_vbeg, vbeg[i]); c.last_vend = std::max(c.last_vend, vend[i]);
        const size_t w1 = (size_t)((end[i] - 1) >> 14);
        if (c.win.size() <= w1) c.win.resize(w1 + 1, ~0ull);
        for (size_t w = (size_t)(beg[i] >> 14); w <= w1; ++w) c.win[w] = std::min(c.win[w], vbeg[i]);
        have_prev = true; p_ref = refid[i]; p_pos = beg[i]; p_bin = bin;
    }
    std::vector<uint8_t> out;
    serialize(a, out);
    *bytes = (uint8_t *)malloc(out.size() + 1);
    if (!*bytes) return index_err(-4, W + ": out of memory");
    memcpy(*bytes, out.data(), out.size());
    *n = out.size();
    return 0;
}

extern "C" int lcd_fai_build(const char *fasta_path, const char *out_path) {
    const std::string W = "lcd_fai_build";
    if (!fasta_path) return index_err(-4, W + ": NULL argument");
    const std::string dst = out_path ? std::string(out_path) : std::string(fasta_path) + ".fai";
    FILE *f = fopen(fasta_path, "rb");
    if (!f) return index_err(-30, W + ": cannot open " + fasta_path);
    struct Seq { std::string name; long long len = 0, off = 0, lb = 0, lw = 0; };
    std::vector<Seq> seqs; std::set<std::string> names;
    // one line at a time: `bases` bytes in front of the line end, `width` bytes with it
    std::vector<unsigned char> buf(1 << 20);
    size_t have = 0, at = 0; long long file_off = 0;
    bool in_seq = false, first_line = false, closed = false;    // closed: a shorter (or blank) line was seen: no further line may belong to this sequence
    std::string line_head;                                      // the first bytes of a header line (the name)
    long long bases = 0, line_start = 0; bool is_header = false, cr = false, any = false;
    int rc = 0;
    auto end_line = [&](bool with_nl) {
        long long b = bases;
        if (with_nl && cr) --b;                                 // \r\n
        const long long width = bases + (with_nl ? 1 : 0);
        if (is_header) {
            size_t e = 0;
            while (e < line_head.size() && line_head[e] != ' ' && line_head[e] != '\t' && line_head[e] != '\r' && line_head[e] != '\n' && line_head[e] != '\v' && line_head[e] != '\f') ++e;
            const std::string nm = line_head.substr(0, e);
            if (nm.empty()) { rc = index_err(LCD_ERR_FAI_FORMAT, W + ": a sequence without a name at offset " + std::to_string(line_start) + " of " + fasta_path); return; }
            if (!names.insert(nm).second) { rc = index_err(LCD_ERR_FAI_FORMAT, W + ": duplicate sequence name " + nm + " in " + fasta_path); return; }
            Seq s; s.name = nm; s.off = line_start + width;
            seqs.push_back(s); in_seq = true; first_line = true; closed = false;
            return;
        }
        if (!in_seq) return;
        Seq &s = seqs.back();
        if (b == 0) { closed = true; return; }                   // a blank line: accepted as the end of the sequence (and at the end of the file)
        if (closed) { rc = index_err(LCD_ERR_FAI_FORMAT, W + ": sequence " + s.name + " has lines of different length (" + fasta_path + ", offset " + std::to_string(line_start) + ")"); return; }
        if (first_line) { s.lb = b; s.lw = with_nl ? width : b + 1; first_line = false; }   // (PROJECT RULE: a line without its newline counts one byte for it)
        else if (b > s.lb) { rc = index_err(LCD_ERR_FAI_FORMAT, W + ": sequence " + s.name + " has lines of different length (" + fasta_path + ", offset " + std::to_string(line_start) + ")"); return; }
        if (b < s.lb || (with_nl && width != s.lw)) closed = true;   // a shorter line (or one with another line end) can only be the last
        s.len += b;
    };
    bool line_open = false;
    for (;;) {
        if (at == have) { have = fread(buf.data(), 1, buf.size(), f); at = 0; if (have == 0) break; }
        if (!any) {
            any = true;
            if (have >= 2 && buf[0] == 31 && buf[1] == 139) { fclose(f); return index_err(LCD_ERR_FAI_FORMAT, W + ": " + fasta_path + " is compressed: only a plain FASTA file can be indexed"); }
            if (buf[0] != '>') { fclose(f); return index_err(LCD_ERR_FAI_FORMAT, W + ": " + fasta_path + " does not start with '>'"); }
        }
        const unsigned char c = buf[at++];
        if (!line_open) { line_open = true; line_start = file_off; bases = 0; cr = false; is_header = c == '>'; line_head.clear(); }
        ++file_off;
        if (c == '\n') { end_line(true); line_open = false; if (rc) break; continue; }
        if (is_header && bases > 0 && line_head.size() < 4096) line_head.push_back((char)c);
        cr = c == '\r';
        ++bases;
    }
    if (!rc && line_open) end_line(false);
    const bool rerr = ferror(f) != 0;
    fclose(f);
    if (rc) return rc;
    if (rerr) return index_err(-30, W + ": read error on " + fasta_path);
    if (!any) return index_err(LCD_ERR_FAI_FORMAT, W + ": " + fasta_path + " does not start with '>' (the file is empty)");
    std::string text;
    for (const Seq &s : seqs) text += s.name + "\t" + std::to_string(s.len) + "\t" + std::to_string(s.off) + "\t" + std::to_string(s.lb) + "\t" + std::to_string(s.lw) + "\n";
    FILE *o = fopen(dst.c_str(), "wb");
    if (!o) return index_err(-30, W + ": cannot open " + dst + " for writing");
    const bool ok = fwrite(text.data(), 1, text.size(), o) == text.size();
    if (fclose(o) != 0 || !ok) { remove(dst.c_str()); return index_err(-30, W + ": short write on " + dst); }
    return (int)seqs.size();
}
