// lcd_bai.cpp -- the .bai builder on the device side: lcd_bai_builder_* runs the record walk, the CIGAR statistics and bai_kernel.hip over a stream of BAM records
// in HBM and accumulates what the finisher (lcd_index_host.cpp) serialises; lcd_bai_build streams a file of any size through it, slab by slab.  The rules of the
// index content are written out in include/lcd_hotpath.h.
#include <climits>
#include <map>
#include <new>
#include "lcd_host_internal.h"
#include "lcd_bai_internal.h"

using namespace lcd_internal;

extern "C" __attribute__((visibility("hidden"))) void lcd_index_set_last_error(const char *m) { g_err = m ? m : ""; }

struct lcd_bai_builder_s {
    int device = 0; bool broken = false, finished = false;
    lcd_bai::Accum acc; std::vector<int64_t> lens; std::vector<uint32_t> n_win;
    // device: per contig the window array's address (0 until its first record) and length, the counters, the error word, the batch buffers;
    // d_mm: the batch's smallest / largest contig (two ints) and behind them one presence byte per contig
    std::map<int, std::unique_ptr<DevBuf>> win;
    DevBuf d_wintab, d_nwin, d_ctg, d_err, d_desc, d_wj, d_wo, d_sj, d_so, d_ent, d_mem, d_bcnt, d_boff, d_chunks, d_mm;
    std::vector<uint64_t> h_wintab;
    StreamGuard st;
    // the record in front of the next batch
    int c_have = 0, c_refid = -1, c_pos = -1, c_nocoor = 0; bool c_run = false;   // c_run: the last chunk of acc.chunks may still grow
    int64_t n_records = 0;
    double ms_walk = 0, ms_stat = 0, ms_entry = 0, ms_finish = 0;
    std::vector<uint8_t> bytes;
};

namespace {
const int BATCH = 1 << 18;          // records per walk / entry launch (10 MB of descriptors)

int builder_fail(lcd_bai_builder_s *b, int rc) { b->broken = true; return rc; }
#define BCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { (void)hipGetLastError(); b->broken = true; return set_err(-10, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)

int err_of_word(lcd_bai_builder_s *b, unsigned long long w) {
    const long long rec = (long long)(w >> 4); const int code = (int)(w & 15);
    const std::string R = "lcd_bai_builder_add_stream: record " + std::to_string(rec);
    b->broken = true;
    switch (code) {
        case 1: return set_err(LCD_ERR_BAI_ORDER, R + " lies in front of the record before it: the file is not sorted by coordinate");
        case 2: return set_err(LCD_ERR_BAI_ORDER, R + " has a coordinate and follows a record without one: the file is not sorted");
        case 3: return set_err(LCD_ERR_BAI_CSI, R + " ends behind 2^29: only BAI is supported, not CSI");
        case 4: return set_err(LCD_ERR_BAI_CONTIG, R + " names a contig outside the header's table");
        default: return set_err(LCD_ERR_BAI_CONTIG, R + " ends behind the last 16 kb window of its contig");
    }
}
} // namespace

extern "C" {

lcd_bai_builder_t *lcd_bai_builder_create(int n_ref, const int64_t *ref_lens) {
    const std::string W = "lcd_bai_builder_create";
    if (n_ref < 0 || (n_ref > 0 && !ref_lens)) { set_err(-4, W + ": NULL argument or negative count"); return nullptr; }
    if (ensure_init()) return nullptr;
    std::unique_ptr<lcd_bai_builder_s> b(new lcd_bai_builder_s());
    b->device = cur_device();
    b->acc.n_ref = n_ref; b->acc.ctg.resize((size_t)n_ref); b->lens.assign(ref_lens, ref_lens + n_ref);
    b->n_win.resize((size_t)n_ref + 1, 0); b->h_wintab.assign((size_t)n_ref + 1, 0);
    for (int t = 0; t < n_ref; ++t) {
        if (ref_lens[t] < 0) { set_err(-4, W + ": negative contig length"); return nullptr; }
        b->n_win[(size_t)t] = (uint32_t)std::min<int64_t>((ref_lens[t] >> 14) + 1, (1ll << 29 >> 14) + 1);
    }
    if (b->st.create()) return nullptr;
    const size_t nr = (size_t)n_ref + 1;
    if (b->d_wintab.ensure(nr * 8, 31) || b->d_nwin.ensure(nr * 4, 31) || b->d_ctg.ensure(nr * sizeof(BaiCtg), 31) || b->d_err.ensure(8, 31) || b->d_mm.ensure(8 + nr, 31)) return nullptr;
    std::vector<BaiCtg> z(nr); for (BaiCtg &c : z) { c.n_mapped = c.n_unmapped = 0; c.first_vbeg = ~0ull; c.last_vend = 0; }
    const unsigned long long all = ~0ull;
    if (hipMemcpy(b->d_ctg.p, z.data(), nr * sizeof(BaiCtg), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(b->d_nwin.p, b->n_win.data(), nr * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b->d_wintab.p, 0, nr * 8) != hipSuccess || hipMemset(b->d_mm.p, 0, 8 + nr) != hipSuccess || hipMemcpy(b->d_err.p, &all, 8, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); set_err(-10, W + ": HIP call failed"); return nullptr;
    }
    return b.release();
}

int lcd_bai_builder_add_stream(lcd_bai_builder_t *b, uint64_t dev_ptr, size_t n_bytes, size_t first, size_t n_members, const lcd_bai_member_t *members, uint64_t end_coff,
                               size_t *next_out) {
    const std::string W = "lcd_bai_builder_add_stream";
    if (next_out) *next_out = first;
    if (!b || b->broken || b->finished) return set_err(-4, W + ": no builder, or one that has failed or is finished");
    if ((n_bytes && !dev_ptr) || first > n_bytes || (n_members && !members)) return set_err(-4, W + ": NULL argument, or first_record_offset behind the stream");
    for (size_t k = 0; k < n_members; ++k) {
        if (members[k].ulen > 65536 || members[k].uoff + members[k].ulen > n_bytes || (k && members[k].uoff != members[k - 1].uoff + members[k - 1].ulen))
            return set_err(-4, W + ": member " + std::to_string(k) + " of the table does not follow the one before it, or lies outside the stream");
    }
    if (use_device(b->device)) return builder_fail(b, -1);
    hipStream_t st = b->st;
    static_assert(sizeof(lcd_bai_member_t) == sizeof(BaiMember), "member table layout");
    if (n_members) {
        if (b->d_mem.ensure(n_members * sizeof(BaiMember))) return builder_fail(b, -1);
        BCHK(hipMemcpyAsync(b->d_mem.p, members, n_members * sizeof(BaiMember), hipMemcpyHostToDevice, st));
    }
    uint64_t o = first;
    while (o < n_bytes) {
        const size_t cap = (size_t)std::min<uint64_t>((uint64_t)BATCH, (n_bytes - o) / 36 + 1);
        const size_t nb = (cap + 255) / 256;
        if (b->d_desc.ensure(cap * sizeof(BamRecDesc)) || b->d_wj.ensure(sizeof(BamWalkJob), 31) || b->d_wo.ensure(sizeof(BamWalkOut), 31) || b->d_sj.ensure(cap * sizeof(BamStatJob)) ||
            b->d_so.ensure(cap * sizeof(BamStatOut)) || b->d_ent.ensure(cap * sizeof(BaiEntry)) || b->d_bcnt.ensure(nb * 4) || b->d_boff.ensure((nb + 1) * 4) ||
            b->d_chunks.ensure(cap * sizeof(BaiChunk))) return builder_fail(b, -1);
        double t0 = now_ms();
        BamWalkJob wj; wj.stream = dev_ptr; wj.ubeg = o; wj.uend = n_bytes; wj.usize = n_bytes; wj.descs = b->d_desc.addr(); wj.reg_end = LLONG_MAX; wj.tid = INT_MIN; wj.cap = (int)cap;
        BamWalkOut wo;
        BCHK(hipMemcpyAsync(b->d_wj.p, &wj, sizeof(wj), hipMemcpyHostToDevice, st));
        lcd_launch_bam_walk((const BamWalkJob *)b->d_wj.p, (BamWalkOut *)b->d_wo.p, 1, st);
        BCHK(hipGetLastError());
        BCHK(hipMemcpyAsync(&wo, b->d_wo.p, sizeof(wo), hipMemcpyDeviceToHost, st));
        BCHK(hipStreamSynchronize(st));
        b->ms_walk += now_ms() - t0;            // (the job's upload, the launch, the result's download and the synchronisation: not the kernel alone)
        if (wo.status == 2) { b->broken = true; return set_err(-33, W + ": malformed BAM record " + std::to_string(b->n_records + wo.n) + " (a field runs past the record)"); }
        if (wo.n < 0 || (size_t)wo.n > cap || wo.next < o || wo.next > n_bytes) { b->broken = true; return set_err(-24, W + ": inconsistent record walk"); }
        const int n = wo.n;
        if (n > 0) {
            t0 = now_ms();
            BaiJob j; memset(&j, 0, sizeof(j));
            j.descs = b->d_desc.addr(); j.stats = b->d_so.addr(); j.statjobs = b->d_sj.addr(); j.members = b->d_mem.addr(); j.entries = b->d_ent.addr(); j.win = b->d_wintab.addr();
            j.n_win = b->d_nwin.addr(); j.ctg = b->d_ctg.addr(); j.err = b->d_err.addr(); j.block_cnt = b->d_bcnt.addr(); j.block_off = b->d_boff.addr(); j.chunks = b->d_chunks.addr();
            j.minmax = b->d_mm.addr(); j.stream = dev_ptr; j.end_coff = end_coff; j.rec0 = b->n_records; j.n = n; j.n_members = (int)n_members; j.n_ref = b->acc.n_ref;
            j.c_have = b->c_have; j.c_refid = b->c_refid; j.c_pos = b->c_pos; j.c_nocoor = b->c_nocoor;
            int mm[2] = {INT_MAX, -1};
            BCHK(hipMemcpyAsync(b->d_mm.p, mm, 8, hipMemcpyHostToDevice, st));
            lcd_launch_bai_prep(j, st);
            BCHK(hipGetLastError());
            lcd_launch_bam_stat((const BamStatJob *)b->d_sj.p, (BamStatOut *)b->d_so.p, n, st);
            BCHK(hipGetLastError());
            BCHK(hipMemcpyAsync(mm, b->d_mm.p, 8, hipMemcpyDeviceToHost, st));
            BCHK(hipStreamSynchronize(st));
            // the window arrays of the contigs that have a record in this batch (the prep kernel's presence bytes between the smallest and the largest contig):
            // all-ones, allocated when a contig's first record arrives
            const int t_lo = std::max(mm[0], 0), t_hi = std::min(mm[1], b->acc.n_ref - 1);
            std::vector<uint8_t> present(t_hi >= t_lo ? (size_t)(t_hi - t_lo + 1) : 0);
            if (!present.empty()) BCHK(hipMemcpy(present.data(), (const uint8_t *)b->d_mm.p + 8 + t_lo, present.size(), hipMemcpyDeviceToHost));
            b->ms_stat += now_ms() - t0;
            t0 = now_ms();
            bool tab_changed = false;
            for (int t = t_lo; t <= t_hi; ++t) {
                if (!present[(size_t)(t - t_lo)] || b->h_wintab[(size_t)t]) continue;
                std::unique_ptr<DevBuf> w(new DevBuf());
                const size_t bytes = (size_t)b->n_win[(size_t)t] * 8;
                if (w->ensure(bytes, 31)) return builder_fail(b, -1);
                BCHK(hipMemsetAsync(w->p, 0xff, bytes, st));
                b->h_wintab[(size_t)t] = w->addr(); b->win[t] = std::move(w); tab_changed = true;
            }
            if (tab_changed) BCHK(hipMemcpyAsync(b->d_wintab.p, b->h_wintab.data(), b->h_wintab.size() * 8, hipMemcpyHostToDevice, st));
            lcd_launch_bai_entry(j, st);
            BCHK(hipGetLastError());
            lcd_launch_bai_compact(j, st);
            BCHK(hipGetLastError());
            const int nblk = (n + 255) / 256;
            unsigned long long errw = ~0ull; int n_chunks = 0; BamRecDesc last; BaiEntry last_e;
            BCHK(hipMemcpyAsync(&errw, b->d_err.p, 8, hipMemcpyDeviceToHost, st));
            BCHK(hipMemcpyAsync(&n_chunks, (const int *)b->d_boff.p + nblk, 4, hipMemcpyDeviceToHost, st));
            BCHK(hipMemcpyAsync(&last, (const BamRecDesc *)b->d_desc.p + (n - 1), sizeof(last), hipMemcpyDeviceToHost, st));
            BCHK(hipMemcpyAsync(&last_e, (const BaiEntry *)b->d_ent.p + (n - 1), sizeof(last_e), hipMemcpyDeviceToHost, st));
            BCHK(hipStreamSynchronize(st));
            if (errw != ~0ull) return err_of_word(b, errw);
            if (n_chunks < 0 || n_chunks > n) { b->broken = true; return set_err(-24, W + ": inconsistent chunk count"); }
            std::vector<BaiChunk> ch((size_t)n_chunks);
            if (n_chunks) BCHK(hipMemcpy(ch.data(), b->d_chunks.p, (size_t)n_chunks * sizeof(BaiChunk), hipMemcpyDeviceToHost));
            for (int k = 0; k < n_chunks; ++k) {
                const BaiChunk &c = ch[(size_t)k];
                if (k == 0 && b->c_run && !b->acc.chunks.empty() && b->acc.chunks.back().refid == c.refid && b->acc.chunks.back().bin == c.bin) b->acc.chunks.back().vend = c.vend;   // the run goes on across the batch border
                else b->acc.chunks.push_back(lcd_bai::Chunk{c.refid, c.bin, c.vbeg, c.vend});
            }
            b->c_have = 1; b->c_refid = last.refid; b->c_pos = last.pos;
            if (last_e.cls == 0) { b->c_nocoor = 1; b->c_run = false; } else b->c_run = true;
            b->n_records += n;
            b->ms_entry += now_ms() - t0;
        }
        o = wo.next;
        if (wo.status != 3) break;               // 0: the stream is done; 1: a record that is not complete inside it
    }
    if (o < n_bytes && o + 4 <= n_bytes) {   // a record that is not complete inside the stream: a block_size that no record can have is refused here, not waited for
        int32_t bs = 0;
        BCHK(hipMemcpy(&bs, (const uint8_t *)(uintptr_t)dev_ptr + o, 4, hipMemcpyDeviceToHost));
        if (bs < 32) { b->broken = true; return set_err(-33, W + ": malformed BAM record " + std::to_string(b->n_records) + " (block_size " + std::to_string(bs) + ")"); }
    }
    if (next_out) *next_out = (size_t)o;
    return 0;
}

int lcd_bai_builder_finish(lcd_bai_builder_t *b, const char *out_path) {
    const std::string W = "lcd_bai_builder_finish";
    if (!b || b->broken || b->finished) return set_err(-4, W + ": no builder, or one that has failed or is finished");
    if (use_device(b->device)) return builder_fail(b, -1);
    const double t0 = now_ms();
    const size_t nr = (size_t)b->acc.n_ref;
    std::vector<BaiCtg> ctg(nr + 1);
    BCHK(hipStreamSynchronize(b->st));
    BCHK(hipMemcpy(ctg.data(), b->d_ctg.p, (nr + 1) * sizeof(BaiCtg), hipMemcpyDeviceToHost));
    int64_t indexed = 0;
    for (size_t t = 0; t < nr; ++t) {
        lcd_bai::Contig &c = b->acc.ctg[t];
        c.n_mapped = (int64_t)ctg[t].n_mapped; c.n_unmapped = (int64_t)ctg[t].n_unmapped; c.first_vbeg = ctg[t].first_vbeg; c.last_vend = ctg[t].last_vend;
        indexed += c.n_mapped + c.n_unmapped;
        auto it = b->win.find((int)t);
        if (it != b->win.end() && c.n_mapped + c.n_unmapped > 0) {
            c.win.resize(b->n_win[t]);
            BCHK(hipMemcpy(c.win.data(), it->second->p, (size_t)b->n_win[t] * 8, hipMemcpyDeviceToHost));
        }
    }
    b->acc.n_no_coor = (uint64_t)(b->n_records - indexed);
    lcd_bai::serialize(b->acc, b->bytes);
    b->finished = true;
    if (out_path) {
        FILE *f = fopen(out_path, "wb");
        if (!f) return set_err(-30, W + ": cannot open " + out_path + " for writing");
        const bool ok = fwrite(b->bytes.data(), 1, b->bytes.size(), f) == b->bytes.size();
        if (fclose(f) != 0 || !ok) { remove(out_path); return set_err(-30, W + ": short write on " + out_path); }
    }
    b->ms_finish += now_ms() - t0;
    return 0;
}
int lcd_bai_builder_bytes(const lcd_bai_builder_t *b, const uint8_t **bytes, size_t *n) {
    if (!b || !b->finished || !bytes || !n) return set_err(-4, "lcd_bai_builder_bytes: the builder is not finished");
    *bytes = b->bytes.data(); *n = b->bytes.size();
    return 0;
}
void lcd_bai_builder_destroy(lcd_bai_builder_t *b) {
    if (!b) return;
    const std::string m = g_err;
    (void)use_device(b->device);
    if (b->st.s) (void)hipStreamSynchronize(b->st.s);
    delete b;
    g_err = m;
}
#undef BCHK

} // extern "C"

// ---- the whole-file driver ----
using Member = lcd_bai::BgzfMember;
// the BGZF members inside buf (file offset base): whole members only, at most `want`; 0 or < 0.  *used: the bytes they take
int lcd_bai::parse_members(const uint8_t *f, size_t n, uint64_t base, size_t want, bool at_eof, std::vector<Member> &out, size_t *used, const std::string &W) {
    size_t o = 0;
    out.clear();
    while (out.size() < want && o < n) {
        if (o + 18 > n) { if (at_eof) return set_err(-31, W + ": truncated BGZF member at the end of the file"); break; }
        if (f[o] != 31 || f[o + 1] != 139 || f[o + 2] != 8 || !(f[o + 3] & 4)) return set_err(-31, W + ": not a BGZF block at file offset " + std::to_string(base + o));
        const unsigned xlen = f[o + 10] | (f[o + 11] << 8);
        if (o + 12 + (size_t)xlen > n) { if (at_eof) return set_err(-31, W + ": truncated BGZF member at the end of the file"); break; }
        unsigned bsize = 0; bool found = false;
        for (size_t x = o + 12; x + 4 <= o + 12 + xlen;) {
            const unsigned slen = f[x + 2] | (f[x + 3] << 8);
            if (f[x] == 'B' && f[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) { bsize = f[x + 4] | (f[x + 5] << 8); found = true; }
            x += 4 + slen;
        }
        if (!found || (size_t)bsize + 1 < 12 + (size_t)xlen + 8) return set_err(-31, W + ": BGZF block without BSIZE at file offset " + std::to_string(base + o));
        const size_t end = o + bsize + 1;
        if (end > n) { if (at_eof) return set_err(-31, W + ": truncated BGZF member at the end of the file"); break; }
        const uint32_t isize = f[end - 4] | (f[end - 3] << 8) | (f[end - 2] << 16) | ((uint32_t)f[end - 1] << 24);
        if (isize > 65536) return set_err(-31, W + ": malformed BGZF block at file offset " + std::to_string(base + o));
        out.push_back(Member{base + o, bsize + 1, isize});
        o = end;
    }
    *used = o;
    return 0;
}

namespace {
const uint64_t MAX_RECORD = (1ull << 31) + 4;       // block_size is a signed 32-bit field
int bai_build_impl(const char *bam_path, const char *out_path, const lcd_bai_opt_t *opt, lcd_bai_stats_t *stats) {
    const std::string W = "lcd_bai_build";
    lcd_bai_stats_t S; memset(&S, 0, sizeof(S));
    if (stats) *stats = S;
    if (!bam_path || !out_path) return set_err(-4, W + ": NULL argument");
    if (opt && opt->slab_members < 0) return set_err(-4, W + ": negative slab_members");
    const double t_wall = now_ms();
    const size_t slab_members = opt && opt->slab_members ? (size_t)opt->slab_members : 4096;
    const int verify = opt ? opt->verify_crc : 0;
    // the header by parsing: its length in the inflated stream, the reference table
    std::vector<uint8_t> hdr;
    if (lcd_io_bam_header(bam_path, hdr)) return set_err(std::string(lcd_io_last_error()).find("cannot open") != std::string::npos ? -30 : -33, W + ": " + lcd_io_last_error());
    std::vector<int64_t> lens;
    {
        int32_t l_text = 0, n_ref = 0; memcpy(&l_text, hdr.data() + 4, 4);
        size_t o = 8 + (size_t)l_text; memcpy(&n_ref, hdr.data() + o, 4); o += 4;
        for (int i = 0; i < n_ref; ++i) { int32_t ln = 0, tl = 0; memcpy(&ln, hdr.data() + o, 4); o += 4 + (size_t)ln; memcpy(&tl, hdr.data() + o, 4); o += 4; lens.push_back(tl); }
    }
    const uint64_t H = hdr.size();
    FILE *f = fopen(bam_path, "rb");
    if (!f) return set_err(-30, W + ": cannot open " + bam_path);
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    fseek(f, 0, SEEK_END); const uint64_t fsize = (uint64_t)std::max<long>(ftell(f), 0);
    // the read buffer: bytes [buf_base, buf_base + buf_len) of the file in uninitialised storage that only grows; a slab is read in pieces until it holds the members
    // it wants, and the bytes behind a slab's last member stay for the next one
    std::unique_ptr<uint8_t[]> buf; size_t buf_cap = 0, buf_len = 0; uint64_t buf_base = 0;
    const size_t PIECE = (size_t)16 << 20;
    auto buf_seek = [&](uint64_t co) {                              // make buf start at file offset co, keeping what is already there
        if (co >= buf_base && co <= buf_base + buf_len) { const size_t d = (size_t)(co - buf_base); if (d && buf_len > d) memmove(buf.get(), buf.get() + d, buf_len - d); buf_len -= d; }
        else buf_len = 0;
        buf_base = co;
    };
    auto buf_reserve = [&](size_t want_cap) {                       // (storage is not touched until it is read into)
        if (want_cap <= buf_cap) return;
        std::unique_ptr<uint8_t[]> nbuf(new uint8_t[want_cap]);
        if (buf_len) memcpy(nbuf.get(), buf.get(), buf_len);
        buf.swap(nbuf); buf_cap = want_cap;
    };
    auto buf_more = [&]() -> int {                                  // one more piece behind what is there
        const uint64_t at = buf_base + buf_len;
        if (at >= fsize) return 0;
        const size_t nb = (size_t)std::min<uint64_t>(PIECE, fsize - at);
        if (buf_len + nb > buf_cap) {
            const size_t cap = std::max(buf_len + nb, buf_cap + (buf_cap >> 1));
            std::unique_ptr<uint8_t[]> nbuf(new uint8_t[cap]);
            if (buf_len) memcpy(nbuf.get(), buf.get(), buf_len);
            buf.swap(nbuf); buf_cap = cap;
        }
        if (fseek(f, (long)at, SEEK_SET) != 0 || fread(buf.get() + buf_len, 1, nb, f) != nb) return set_err(-30, W + ": short read on " + bam_path);
        buf_len += nb;
        return 0;
    };
    // the members of the slab that starts at co: up to `want` whole ones
    auto read_slab = [&](uint64_t co, size_t want, std::vector<Member> &ms, size_t *used) -> int {
        buf_seek(co);
        buf_reserve((size_t)std::min<uint64_t>(fsize - co, (uint64_t)std::min<size_t>(want, (size_t)1 << 20) * 65536 + PIECE));   // at most what `want` members can take
        for (;;) {
            const bool at_eof = buf_base + buf_len >= fsize;
            if (int rc = parse_members(buf.get(), buf_len, co, want, at_eof, ms, used, W)) return rc;
            if (ms.size() >= want || at_eof) return 0;
            if (int rc = buf_more()) return rc;
        }
    };
    // where the records begin: behind the last non-empty member that ends at or in front of inflated offset H
    uint64_t co = 0, first = H;
    {
        uint64_t scan = 0, cum = 0; std::vector<Member> ms; bool done = false;
        while (!done && scan < fsize) {
            size_t used = 0;
            if (int rc = read_slab(scan, 64, ms, &used)) return rc;
            if (ms.empty()) break;
            for (const Member &m : ms) {
                if (cum + m.ulen > H) { done = true; break; }
                cum += m.ulen;
                if (m.ulen) { co = m.coff + m.bsize; first = H - cum; }
            }
            scan += used;
        }
    }
    std::unique_ptr<lcd_bai_builder_s, void (*)(lcd_bai_builder_t *)> b(lcd_bai_builder_create((int)lens.size(), lens.data()), lcd_bai_builder_destroy);
    if (!b) return -1;
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
            const int rc = first <= u ? lcd_bai_builder_add_stream(b.get(), lcd_inflated_dev_ptr(inf), (size_t)u, (size_t)first, tab.size(), tab.data(), end_coff, &next)
                                      : set_err(-33, W + ": truncated BAM header");
            lcd_inflated_free(inf);
            if (rc) return rc;
        } else if (first > 0) return set_err(-33, W + ": truncated BAM header");
        if (next >= u) { co = end_coff; first = 0; want = slab_members; continue; }       // every record of the slab is complete
        if (last_slab) return set_err(-33, W + ": truncated BAM record at the end of the file (record " + std::to_string(b->n_records) + ")");
        // the next slab starts at the member that holds the first unfinished record -- behind a payload that ends exactly there, at the member that follows it
        size_t k = 0;
        while (k < tab.size() && tab[k].uoff + tab[k].ulen <= next) ++k;        // the member that holds byte `next`
        while (next == tab[k].uoff && k > 0 && tab[k - 1].ulen == 0) --k;        // (rule 5: empty members in front of it follow the payload that ends there)
        if (k == 0 || tab[k].coff == co) {                                       // no member was finished: one record larger than the slab grows it for this step
            if (u - next > MAX_RECORD) return set_err(-33, W + ": BAM record " + std::to_string(b->n_records) + " is longer than a record can be");   // (the growth ends at one maximal record)
            want *= 2;
        } else want = slab_members;
        first = next - tab[k].uoff; co = tab[k].coff;
    }
    if (int rc = lcd_bai_builder_finish(b.get(), out_path)) return rc;
    S.n_records = b->n_records; S.n_no_coor = (int64_t)b->acc.n_no_coor; S.n_chunks = (int64_t)b->acc.chunks.size(); S.bytes_index = (int64_t)b->bytes.size();
    for (const lcd_bai::Contig &c : b->acc.ctg) { S.n_mapped += c.n_mapped; S.n_unmapped += c.n_unmapped; }
    S.n_indexed = S.n_mapped + S.n_unmapped;
    S.ms_walk = b->ms_walk; S.ms_stat = b->ms_stat; S.ms_entry = b->ms_entry; S.ms_finish = b->ms_finish; S.ms_wall = now_ms() - t_wall;
    if (stats) *stats = S;
    return 0;
}
} // namespace

extern "C" int lcd_bai_build(const char *bam_path, const char *out_path, const lcd_bai_opt_t *opt, lcd_bai_stats_t *stats) {
    try { return bai_build_impl(bam_path, out_path, opt, stats); }
    catch (const std::bad_alloc &) { return set_err(-11, "lcd_bai_build: out of host memory"); }
    catch (const std::exception &e) { return set_err(-11, std::string("lcd_bai_build: ") + e.what()); }
}
