// lcd_vcf_index.cpp -- the .tbi / .csi builder on the device side: lcd_vcf_index_builder_* runs vcf_index_kernel.hip over VCF text in HBM and accumulates what the
// finisher (lcd_index_host.cpp: serialize_tbx) serialises; lcd_vcf_index_build streams a .vcf.gz of any size through it, slab by slab, as lcd_bai_build does for a
// BAM.  The rules of the index content are written out in include/lcd_hotpath.h ("VCF indexes").
#include <map>
#include <new>
#include <unordered_map>
#include "lcd_host_internal.h"
#include "lcd_bai_internal.h"

using namespace lcd_internal;

struct lcd_vcf_index_builder_s {
    int device = 0; bool broken = false, finished = false;
    bool take_tail = false;             // the whole-file driver's last slab: a last line without '\n' is a line
    lcd_bai::VAccum acc;
    std::unordered_map<std::string, int> tid_of;
    struct Win { DevBuf buf; uint32_t n = 0; };
    std::map<int, std::unique_ptr<Win>> win;        // per contig its window array (all-ones = unset), grown when a later line ends behind it
    DevBuf d_bcnt, d_boff, d_lstart, d_rank, d_dline, d_lines, d_heads, d_ent, d_mem, d_runs, d_rwin, d_rnwin, d_err, d_chunks, d_cname, d_mclen, d_noffs, d_names;
    StreamGuard st;
    // the data line in front of the next stream
    int c_have = 0, c_tid = -1; long long c_beg = 0; std::string c_name; bool c_run = false;   // c_run: the last chunk of acc.chunks may still grow
    int64_t n_lines = 0, n_data = 0;
    double ms_lines = 0, ms_entry = 0, ms_finish = 0;
    std::vector<uint8_t> bytes; int64_t bytes_file = 0;
};

namespace {
#define BCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { (void)hipGetLastError(); b->broken = true; return set_err(-10, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)
int vfail(lcd_vcf_index_builder_s *b, int rc) { b->broken = true; return rc; }

int err_of_word(lcd_vcf_index_builder_s *b, unsigned long long w, const std::string &name) {
    const long long line = (long long)(w >> 4); const int code = (int)(w & 15);
    const std::string R = "lcd_vcf_index_builder_add_stream: data line " + std::to_string(line);
    b->broken = true;
    switch (code) {
        case 1: return set_err(LCD_ERR_VIDX_ORDER, R + " lies in front of the line before it: the file is not sorted by position");
        case 2: return set_err(LCD_ERR_VCF_LINE, R + " has fewer than 8 columns, an empty CHROM, or a POS that is not a non-negative decimal number");
        case 3: return set_err(LCD_ERR_VIDX_CSI, R + (b->acc.format == LCD_VIDX_TBI ? " ends behind 2^29: TBI cannot hold it, ask for CSI" : " ends behind 2^38: no CSI this library writes holds it"));
        case 6: return set_err(LCD_ERR_VIDX_ORDER, R + ": contig " + name + " reappears after another contig: the file is not sorted");
        default: return set_err(-24, R + ": no window array for its contig");
    }
}
} // namespace

extern "C" {

lcd_vcf_index_builder_t *lcd_vcf_index_builder_create(int format) {
    const std::string W = "lcd_vcf_index_builder_create";
    if (format != LCD_VIDX_TBI && format != LCD_VIDX_CSI) { set_err(-4, W + ": format must be LCD_VIDX_TBI or LCD_VIDX_CSI"); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<lcd_vcf_index_builder_s> b(new lcd_vcf_index_builder_s());
    b->device = cur_device(); b->acc.format = format;
    if (b->st.create()) return nullptr;
    if (b->d_err.ensure(8, 31) || b->d_mclen.ensure(8, 31)) return nullptr;
    const unsigned long long all = ~0ull;
    if (hipMemcpy(b->d_err.p, &all, 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(b->d_mclen.p, 0, 8) != hipSuccess) { (void)hipGetLastError(); set_err(-10, W + ": HIP call failed"); return nullptr; }
    return b.release();
}

int lcd_vcf_index_builder_add_stream(lcd_vcf_index_builder_t *b, uint64_t dev_ptr, size_t n_bytes, size_t first, size_t n_members, const lcd_bai_member_t *members, uint64_t end_coff,
                                     size_t *next_out) {
    const std::string W = "lcd_vcf_index_builder_add_stream";
    if (next_out) *next_out = first;
    if (!b || b->broken || b->finished) return set_err(-4, W + ": no builder, or one that has failed or is finished");
    if ((n_bytes && !dev_ptr) || first > n_bytes || (n_members && !members) || n_bytes >= ((size_t)1 << 40)) return set_err(-4, W + ": NULL argument, or first_line_offset behind the stream");
    for (size_t k = 0; k < n_members; ++k) {
        if (members[k].ulen > 65536 || members[k].uoff + members[k].ulen > n_bytes || (k && members[k].uoff != members[k - 1].uoff + members[k - 1].ulen))
            return set_err(-4, W + ": member " + std::to_string(k) + " of the table does not follow the one before it, or lies outside the stream");
    }
    if (first >= n_bytes) return 0;
    if (use_device(b->device)) return vfail(b, -1);
    hipStream_t st = b->st;
    static_assert(sizeof(lcd_bai_member_t) == sizeof(BaiMember), "member table layout");
    double t0 = now_ms();
    VIdxJob j; memset(&j, 0, sizeof(j));
    j.stream = dev_ptr; j.n_bytes = n_bytes; j.first = first; j.end_coff = end_coff; j.n_members = (int)n_members; j.line0 = b->n_data;
    j.cap = b->acc.format == LCD_VIDX_TBI ? (1ll << 29) : (1ll << (14 + 3 * lcd_bai::VIDX_MAX_DEPTH));
    j.err = b->d_err.addr(); j.max_clen = b->d_mclen.addr();
    if (n_members) {
        if (b->d_mem.ensure(n_members * sizeof(BaiMember))) return vfail(b, -1);
        BCHK(hipMemcpyAsync(b->d_mem.p, members, n_members * sizeof(BaiMember), hipMemcpyHostToDevice, st));
    }
    j.members = b->d_mem.addr();
    // ---- the line table
    const size_t nlb = (n_bytes - first + 4095) / 4096;
    if (nlb > (size_t)1 << 30) return set_err(-4, W + ": stream too long");
    j.n_blocks = (int)nlb;
    if (b->d_bcnt.ensure(nlb * 4) || b->d_boff.ensure((nlb + 1) * 4)) return vfail(b, -1);
    j.block_cnt = b->d_bcnt.addr(); j.block_off = b->d_boff.addr();
    lcd_launch_vidx_nl_count(j, st);
    lcd_launch_vidx_scan(j, (int)nlb, st);
    BCHK(hipGetLastError());
    int n_nl = 0;
    BCHK(hipMemcpyAsync(&n_nl, (const int *)b->d_boff.p + nlb, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (n_nl < 0 || (size_t)n_nl > n_bytes - first) { b->broken = true; return set_err(-24, W + ": inconsistent line count"); }
    if (b->d_lstart.ensure(((size_t)n_nl + 2) * 8)) return vfail(b, -1);
    j.lstart = b->d_lstart.addr();
    lcd_launch_vidx_nl_compact(j, st);
    BCHK(hipGetLastError());
    uint64_t last_start = first;
    BCHK(hipMemcpyAsync(&last_start, (const uint64_t *)b->d_lstart.p + n_nl, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (last_start < first || last_start > n_bytes) { b->broken = true; return set_err(-24, W + ": inconsistent line table"); }
    size_t n_lines = (size_t)n_nl; uint64_t next = last_start;
    if (b->take_tail && last_start < n_bytes) {      // the file's last line has no '\n': it ends at the stream's end
        const uint64_t stop = (uint64_t)n_bytes + 1;
        ++n_lines; next = n_bytes;
        BCHK(hipMemcpy((uint64_t *)b->d_lstart.p + n_lines, &stop, 8, hipMemcpyHostToDevice));
    }
    b->ms_lines += now_ms() - t0;
    if (next_out) *next_out = (size_t)next;
    if (n_lines == 0) return 0;
    // ---- data lines, their fields, the contig runs
    t0 = now_ms();
    j.n_lines = (int)n_lines;
    const size_t lb = (n_lines + 255) / 256;
    if (b->d_bcnt.ensure(lb * 4) || b->d_boff.ensure((lb + 1) * 4) || b->d_rank.ensure(n_lines * 4)) return vfail(b, -1);
    j.block_cnt = b->d_bcnt.addr(); j.block_off = b->d_boff.addr(); j.rank = b->d_rank.addr();
    lcd_launch_vidx_flag(j, st);
    lcd_launch_vidx_scan(j, (int)lb, st);
    BCHK(hipGetLastError());
    int n_data = 0;
    BCHK(hipMemcpyAsync(&n_data, (const int *)b->d_boff.p + lb, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (n_data < 0 || (size_t)n_data > n_lines) { b->broken = true; return set_err(-24, W + ": inconsistent data line count"); }
    j.n_data = n_data;
    if (b->d_dline.ensure((size_t)n_data * 4 + 4) || b->d_lines.ensure(((size_t)n_data + 1) * sizeof(VIdxLine)) || b->d_cname.ensure(b->c_name.size() + 8)) return vfail(b, -1);
    j.dline = b->d_dline.addr(); j.lines = b->d_lines.addr(); j.carry_name = b->d_cname.addr();
    j.c_have = b->c_have; j.c_beg = b->c_beg; j.c_name_len = (int)b->c_name.size();
    if (!b->c_name.empty()) BCHK(hipMemcpyAsync(b->d_cname.p, b->c_name.data(), b->c_name.size(), hipMemcpyHostToDevice, st));
    lcd_launch_vidx_rank(j, st);
    lcd_launch_vidx_parse(j, st);
    BCHK(hipGetLastError());
    b->n_lines += (int64_t)n_lines;
    if (n_data == 0) { BCHK(hipStreamSynchronize(st)); b->ms_lines += now_ms() - t0; return 0; }
    const size_t db = ((size_t)n_data + 255) / 256;
    lcd_launch_vidx_head_count(j, st);
    lcd_launch_vidx_scan(j, (int)db, st);
    BCHK(hipGetLastError());
    int n_heads = 0;
    BCHK(hipMemcpyAsync(&n_heads, (const int *)b->d_boff.p + db, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (n_heads < 0 || n_heads > n_data) { b->broken = true; return set_err(-24, W + ": inconsistent contig run count"); }
    j.n_heads = n_heads;
    const size_t n_runs = (size_t)n_heads + 1;
    std::vector<VIdxRun> runs(n_runs);
    for (VIdxRun &r : runs) { r.n_lines = 0; r.first_vbeg = ~0ull; r.last_vend = 0; r.max_end = 0; }
    if (b->d_heads.ensure(n_runs * sizeof(VIdxHead)) || b->d_runs.ensure(n_runs * sizeof(VIdxRun)) || b->d_rwin.ensure(n_runs * 8) || b->d_rnwin.ensure(n_runs * 4) || b->d_noffs.ensure(n_runs * 8))
        return vfail(b, -1);
    j.heads = b->d_heads.addr(); j.runs = b->d_runs.addr(); j.run_win = b->d_rwin.addr(); j.run_nwin = b->d_rnwin.addr(); j.name_offs = b->d_noffs.addr();
    BCHK(hipMemcpyAsync(b->d_runs.p, runs.data(), n_runs * sizeof(VIdxRun), hipMemcpyHostToDevice, st));
    lcd_launch_vidx_head(j, st);
    BCHK(hipGetLastError());
    std::vector<VIdxHead> heads((size_t)n_heads);
    if (n_heads) BCHK(hipMemcpyAsync(heads.data(), b->d_heads.p, (size_t)n_heads * sizeof(VIdxHead), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(runs.data(), b->d_runs.p, n_runs * sizeof(VIdxRun), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    // only the run heads' names come to the host: tids in order of first appearance; a name seen before is an order error
    std::vector<uint64_t> noffs(n_runs, 0);
    for (int k = 0; k < n_heads; ++k) {
        if (heads[(size_t)k].a + heads[(size_t)k].name_len > n_bytes || heads[(size_t)k].line < 0 || heads[(size_t)k].line >= n_data) { b->broken = true; return set_err(-24, W + ": inconsistent contig run head"); }
        noffs[(size_t)k + 1] = noffs[(size_t)k] + heads[(size_t)k].name_len;
    }
    std::vector<char> nbuf((size_t)noffs[(size_t)n_heads] + 1);
    if (n_heads) {
        if (b->d_names.ensure(nbuf.size() + 8)) return vfail(b, -1);
        j.names = b->d_names.addr();
        BCHK(hipMemcpyAsync(b->d_noffs.p, noffs.data(), n_runs * 8, hipMemcpyHostToDevice, st));
        lcd_launch_vidx_names(j, st);
        BCHK(hipGetLastError());
        if (nbuf.size() > 1) BCHK(hipMemcpyAsync(nbuf.data(), b->d_names.p, nbuf.size() - 1, hipMemcpyDeviceToHost, st));
        BCHK(hipStreamSynchronize(st));
    }
    unsigned long long host_err = ~0ull; std::string host_err_name;
    std::vector<int> run_tid(n_runs, -1);
    run_tid[0] = b->c_have ? b->c_tid : -1;
    for (int k = 0; k < n_heads; ++k) {
        const std::string nm(nbuf.data() + noffs[(size_t)k], (size_t)heads[(size_t)k].name_len);
        if (nm.empty()) continue;                      // (a refused line: the error word names it)
        auto it = b->tid_of.find(nm);
        if (it != b->tid_of.end()) {
            const unsigned long long w = ((unsigned long long)(b->n_data + heads[(size_t)k].line) << 4) | 6u;
            if (w < host_err) { host_err = w; host_err_name = nm; }
            run_tid[(size_t)k + 1] = it->second;
        } else {
            const int t = (int)b->acc.names.size();
            b->tid_of.emplace(nm, t); b->acc.names.push_back(nm); b->acc.a.ctg.emplace_back();
            run_tid[(size_t)k + 1] = t;
        }
    }
    b->acc.a.n_ref = (int)b->acc.names.size();
    // the window arrays: sized from the runs' largest ends
    std::vector<uint64_t> rwin(n_runs, 0); std::vector<uint32_t> rnwin(n_runs, 0);
    for (size_t r = 0; r < n_runs; ++r) {
        const int t = run_tid[r];
        if (t < 0 || runs[r].max_end == 0) continue;
        if (runs[r].max_end > (unsigned long long)j.cap) { b->broken = true; return set_err(-24, W + ": inconsistent largest end"); }
        const uint32_t need = (uint32_t)(((runs[r].max_end - 1) >> 14) + 1);
        std::unique_ptr<lcd_vcf_index_builder_s::Win> &w = b->win[t];
        if (!w) w.reset(new lcd_vcf_index_builder_s::Win());
        if (need > w->n) {
            const uint32_t nn = std::max(need, std::min<uint32_t>(w->n * 2, (uint32_t)((j.cap >> 14) + 1)));
            DevBuf nb;
            if (nb.ensure((size_t)nn * 8, 31)) return vfail(b, -1);
            BCHK(hipMemsetAsync(nb.p, 0xff, (size_t)nn * 8, st));
            if (w->n) BCHK(hipMemcpyAsync(nb.p, w->buf.p, (size_t)w->n * 8, hipMemcpyDeviceToDevice, st));
            BCHK(hipStreamSynchronize(st));
            w->buf.release();
            std::swap(w->buf.p, nb.p); std::swap(w->buf.cap, nb.cap); std::swap(w->buf.dev, nb.dev);
            w->n = nn;
        }
        rwin[r] = w->buf.addr(); rnwin[r] = w->n;
    }
    BCHK(hipMemcpyAsync(b->d_rwin.p, rwin.data(), n_runs * 8, hipMemcpyHostToDevice, st));
    BCHK(hipMemcpyAsync(b->d_rnwin.p, rnwin.data(), n_runs * 4, hipMemcpyHostToDevice, st));
    b->ms_lines += now_ms() - t0;
    // ---- entries and chunks
    t0 = now_ms();
    if (b->d_ent.ensure((size_t)n_data * sizeof(BaiEntry)) || b->d_chunks.ensure((size_t)n_data * sizeof(BaiChunk))) return vfail(b, -1);
    j.entries = b->d_ent.addr(); j.chunks = b->d_chunks.addr();
    lcd_launch_vidx_entry(j, st);
    lcd_launch_vidx_scan(j, (int)db, st);
    lcd_launch_vidx_compact(j, st);
    BCHK(hipGetLastError());
    unsigned long long errw = ~0ull; int n_chunks = 0; VIdxLine last;
    BCHK(hipMemcpyAsync(&errw, b->d_err.p, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&n_chunks, (const int *)b->d_boff.p + db, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&last, (const VIdxLine *)b->d_lines.p + (n_data - 1), sizeof(last), hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(runs.data(), b->d_runs.p, n_runs * sizeof(VIdxRun), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (std::min(errw, host_err) != ~0ull) return err_of_word(b, std::min(errw, host_err), host_err_name);
    if (n_chunks < 0 || n_chunks > n_data || last.run < 0 || (size_t)last.run >= n_runs || run_tid[(size_t)last.run] < 0) { b->broken = true; return set_err(-24, W + ": inconsistent chunk count"); }
    std::vector<BaiChunk> ch((size_t)n_chunks);
    if (n_chunks) BCHK(hipMemcpy(ch.data(), b->d_chunks.p, (size_t)n_chunks * sizeof(BaiChunk), hipMemcpyDeviceToHost));
    for (int k = 0; k < n_chunks; ++k) {
        const BaiChunk &c = ch[(size_t)k];
        if (c.refid < 0 || (size_t)c.refid >= n_runs || run_tid[(size_t)c.refid] < 0) { b->broken = true; return set_err(-24, W + ": inconsistent chunk"); }
        const int t = run_tid[(size_t)c.refid];
        std::vector<lcd_bai::Chunk> &all = b->acc.a.chunks;
        if (k == 0 && b->c_run && !all.empty() && all.back().refid == t && all.back().bin == c.bin) all.back().vend = c.vend;     // the run goes on across the stream border
        else all.push_back(lcd_bai::Chunk{t, c.bin, c.vbeg, c.vend});
    }
    for (size_t r = 0; r < n_runs; ++r) {
        if (!runs[r].n_lines) continue;
        lcd_bai::Contig &c = b->acc.a.ctg[(size_t)run_tid[r]];
        c.n_mapped += (int64_t)runs[r].n_lines; c.first_vbeg = std::min<uint64_t>(c.first_vbeg, runs[r].first_vbeg); c.last_vend = std::max<uint64_t>(c.last_vend, runs[r].last_vend);
        b->acc.max_end = std::max<int64_t>(b->acc.max_end, (int64_t)runs[r].max_end);
    }
    b->c_have = 1; b->c_tid = run_tid[(size_t)last.run]; b->c_beg = last.beg; b->c_name = b->acc.names[(size_t)b->c_tid]; b->c_run = true;
    b->n_data += n_data;
    b->ms_entry += now_ms() - t0;
    return 0;
}

int lcd_vcf_index_builder_finish(lcd_vcf_index_builder_t *b, const char *out_path) {
    const std::string W = "lcd_vcf_index_builder_finish";
    if (!b || b->broken || b->finished) return set_err(-4, W + ": no builder, or one that has failed or is finished");
    if (use_device(b->device)) return vfail(b, -1);
    const double t0 = now_ms();
    BCHK(hipStreamSynchronize(b->st));
    unsigned long long mclen = 0;
    BCHK(hipMemcpy(&mclen, b->d_mclen.p, 8, hipMemcpyDeviceToHost));
    b->acc.max_contig_len = (int64_t)std::min<unsigned long long>(mclen, 1ull << 62);
    for (size_t t = 0; t < b->acc.a.ctg.size(); ++t) {
        lcd_bai::Contig &c = b->acc.a.ctg[t];
        auto it = b->win.find((int)t);
        if (it != b->win.end() && c.n_mapped > 0 && it->second->n) {
            c.win.resize(it->second->n);
            BCHK(hipMemcpy(c.win.data(), it->second->buf.p, (size_t)it->second->n * 8, hipMemcpyDeviceToHost));
        }
    }
    if (int rc = lcd_bai::serialize_tbx(b->acc, b->bytes)) return vfail(b, rc);
    if (out_path) {
        lcd_deflated_t *d = lcd_bgzf_deflate_dev(b->bytes.data(), b->bytes.size(), 0, 1);
        if (!d) return vfail(b, -30);
        const size_t sz = lcd_deflated_size(d);
        std::vector<uint8_t> buf(sz + 1);
        const int rc = lcd_deflated_to_host(d, 0, sz, buf.data());
        lcd_deflated_free(d);
        if (rc) return vfail(b, rc);
        FILE *f = fopen(out_path, "wb");
        if (!f) return vfail(b, set_err(-30, W + ": cannot open " + out_path + " for writing"));
        const bool ok = fwrite(buf.data(), 1, sz, f) == sz;
        if (fclose(f) != 0 || !ok) { remove(out_path); return vfail(b, set_err(-30, W + ": short write on " + out_path)); }
        b->bytes_file = (int64_t)sz;
    }
    b->finished = true;
    b->ms_finish += now_ms() - t0;
    return 0;
}
int lcd_vcf_index_builder_bytes(const lcd_vcf_index_builder_t *b, const uint8_t **bytes, size_t *n) {
    if (!b || !b->finished || !bytes || !n) return set_err(-4, "lcd_vcf_index_builder_bytes: the builder is not finished");
    *bytes = b->bytes.data(); *n = b->bytes.size();
    return 0;
}
void lcd_vcf_index_builder_destroy(lcd_vcf_index_builder_t *b) {
    if (!b) return;
    const std::string m = g_err;
    (void)use_device(b->device);
    if (b->st.s) (void)hipStreamSynchronize(b->st.s);
    delete b;
    g_err = m;
}
#undef BCHK

} // extern "C"

// what the builder has counted, for the writer and the whole-file driver
void lcd_vcf_index_builder_counts(const lcd_vcf_index_builder_t *b, lcd_vcf_index_stats_t *S) {
    S->n_lines = b->n_lines; S->n_data_lines = b->n_data; S->n_meta_lines = b->n_lines - b->n_data; S->n_contigs = (int64_t)b->acc.names.size();
    S->n_chunks = (int64_t)b->acc.a.chunks.size(); S->bytes_index = (int64_t)b->bytes.size(); S->bytes_file = b->bytes_file;
    S->depth = b->finished ? (b->acc.format == LCD_VIDX_CSI && b->bytes.size() >= 12 ? (int)b->bytes[8] : 5) : 0;
    S->ms_lines = b->ms_lines; S->ms_entry = b->ms_entry; S->ms_finish = b->ms_finish;
}

// ---- the whole-file driver ----
namespace {
using Member = lcd_bai::BgzfMember;

int vcf_index_build_impl(const char *path, const char *out_path_in, const lcd_vcf_index_opt_t *opt, lcd_vcf_index_stats_t *stats) {
    const std::string W = "lcd_vcf_index_build";
    lcd_vcf_index_stats_t S; memset(&S, 0, sizeof(S));
    if (stats) *stats = S;
    if (!path) return set_err(-4, W + ": NULL argument");
    if (opt && opt->slab_members < 0) return set_err(-4, W + ": negative slab_members");
    const int format = opt ? opt->format : LCD_VIDX_TBI;
    if (format != LCD_VIDX_TBI && format != LCD_VIDX_CSI) return set_err(-4, W + ": format must be LCD_VIDX_TBI or LCD_VIDX_CSI");
    const std::string out_path = out_path_in ? std::string(out_path_in) : std::string(path) + (format == LCD_VIDX_CSI ? ".csi" : ".tbi");
    const double t_wall = now_ms();
    const size_t slab_members = opt && opt->slab_members ? (size_t)opt->slab_members : 4096;
    const int verify = opt ? opt->verify_crc : 0;
    FILE *f = fopen(path, "rb");
    if (!f) return set_err(-30, W + ": cannot open " + path);
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    fseek(f, 0, SEEK_END); const uint64_t fsize = (uint64_t)std::max<long>(ftell(f), 0);
    {   // BGZF, or which of the two other things
        uint8_t h[18] = {0};
        fseek(f, 0, SEEK_SET);
        const size_t got = fread(h, 1, 18, f);
        if (got < 2 || h[0] != 31 || h[1] != 139) return set_err(-33, W + ": " + path + " is plain text (or empty), not BGZF: compress it with -O z / bgzip first");
        if (got < 18 || h[2] != 8 || !(h[3] & 4) || h[12] != 'B' || h[13] != 'C') return set_err(-33, W + ": " + path + " is plain gzip, not BGZF: a gzip stream has no block offsets to index");
    }
    std::unique_ptr<uint8_t[]> buf; size_t buf_cap = 0, buf_len = 0; uint64_t buf_base = 0;
    const size_t PIECE = (size_t)16 << 20;
    auto buf_seek = [&](uint64_t co) {
        if (co >= buf_base && co <= buf_base + buf_len) { const size_t d = (size_t)(co - buf_base); if (d && buf_len > d) memmove(buf.get(), buf.get() + d, buf_len - d); buf_len -= d; }
        else buf_len = 0;
        buf_base = co;
    };
    auto buf_more = [&]() -> int {
        const uint64_t at = buf_base + buf_len;
        if (at >= fsize) return 0;
        const size_t nb = (size_t)std::min<uint64_t>(PIECE, fsize - at);
        if (buf_len + nb > buf_cap) {
            const size_t cap = std::max(buf_len + nb, buf_cap + (buf_cap >> 1));
            std::unique_ptr<uint8_t[]> nbuf(new uint8_t[cap]);
            if (buf_len) memcpy(nbuf.get(), buf.get(), buf_len);
            buf.swap(nbuf); buf_cap = cap;
        }
        if (fseek(f, (long)at, SEEK_SET) != 0 || fread(buf.get() + buf_len, 1, nb, f) != nb) return set_err(-30, W + ": short read on " + path);
        buf_len += nb;
        return 0;
    };
    auto read_slab = [&](uint64_t co, size_t want, std::vector<Member> &ms, size_t *used) -> int {
        buf_seek(co);
        for (;;) {
            const bool at_eof = buf_base + buf_len >= fsize;
            if (int rc = lcd_bai::parse_members(buf.get(), buf_len, co, want, at_eof, ms, used, W)) return rc;
            if (ms.size() >= want || at_eof) return 0;
            if (int rc = buf_more()) return rc;
        }
    };
    std::unique_ptr<lcd_vcf_index_builder_s, void (*)(lcd_vcf_index_builder_t *)> b(lcd_vcf_index_builder_create(format), lcd_vcf_index_builder_destroy);
    if (!b) return -1;
    uint64_t co = 0, first = 0;
    size_t want = slab_members;
    std::vector<Member> ms; std::vector<lcd_bai_member_t> tab;
    while (co < fsize) {
        double t0 = now_ms();
        size_t used = 0;
        if (int rc = read_slab(co, want, ms, &used)) return rc;
        S.ms_read += now_ms() - t0;
        if (ms.empty()) return set_err(-31, W + ": no whole BGZF member at file offset " + std::to_string(co));
        const uint64_t end_coff = co + used;
        const bool last_slab = end_coff >= fsize;
        tab.resize(ms.size());
        uint64_t u = 0;
        for (size_t k = 0; k < ms.size(); ++k) { tab[k].uoff = u; tab[k].coff = ms[k].coff; tab[k].ulen = ms[k].ulen; tab[k].pad = 0; u += ms[k].ulen; }
        size_t next = first;
        S.n_slabs += 1; S.n_members += (int64_t)ms.size(); S.bytes_in += (int64_t)used; S.bytes_inflated += (int64_t)u;
        if (u > 0) {
            t0 = now_ms();
            lcd_inflated_t *inf = lcd_bgzf_inflate_dev(buf.get(), used, verify);
            if (!inf) return set_err(-32, W + ": " + lcd_io_last_error());
            S.ms_inflate += now_ms() - t0;
            if (lcd_inflated_size(inf) != u) { lcd_inflated_free(inf); return set_err(-24, W + ": inflated size differs from the members' ISIZE"); }
            b->take_tail = last_slab;
            const int rc = first <= u ? lcd_vcf_index_builder_add_stream(b.get(), lcd_inflated_dev_ptr(inf), (size_t)u, (size_t)first, tab.size(), tab.data(), end_coff, &next)
                                      : set_err(-24, W + ": inconsistent slab start");
            lcd_inflated_free(inf);
            if (rc) return rc;
        }
        if (next >= u || last_slab) { co = end_coff; first = 0; want = slab_members; continue; }       // every line of the slab is complete
        // the next slab starts at the member that holds the first unfinished line -- behind a payload that ends exactly there, at the member that follows it
        size_t k = 0;
        while (k < tab.size() && tab[k].uoff + tab[k].ulen <= next) ++k;
        if (k >= tab.size()) return set_err(-24, W + ": inconsistent line offset");
        while (next == tab[k].uoff && k > 0 && tab[k - 1].ulen == 0) --k;
        if (k == 0 || tab[k].coff == co) {                                       // no member was finished: one line larger than the slab grows it for this step
            if (want > ((size_t)1 << 22)) return set_err(-33, W + ": data line " + std::to_string(b->n_data) + " is longer than 2^38 bytes");
            want *= 2;
        } else want = slab_members;
        first = next - tab[k].uoff; co = tab[k].coff;
    }
    if (int rc = lcd_vcf_index_builder_finish(b.get(), out_path.c_str())) { remove(out_path.c_str()); return rc; }
    lcd_vcf_index_builder_counts(b.get(), &S);
    S.wrote = 1;
    S.ms_wall = now_ms() - t_wall;
    if (stats) *stats = S;
    return 0;
}
} // namespace

extern "C" int lcd_vcf_index_build(const char *vcf_gz_path, const char *out_path, const lcd_vcf_index_opt_t *opt, lcd_vcf_index_stats_t *stats) {
    try { return vcf_index_build_impl(vcf_gz_path, out_path, opt, stats); }
    catch (const std::bad_alloc &) { return set_err(-11, "lcd_vcf_index_build: out of host memory"); }
    catch (const std::exception &e) { return set_err(-11, std::string("lcd_vcf_index_build: ") + e.what()); }
}
