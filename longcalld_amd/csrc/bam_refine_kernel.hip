// bam_refine_kernel.hip -- refine_bam1 + update_bam1_tags (src/bam_utils.c:1718-1942) and the HP / PS rewrite behind them (:1955-2006) on the records where the
// inflate left them in HBM, from each read's FINAL digar list.  One wavefront per record in both kernels; lanes stride the digar list 64 at a time, runs and totals
// go through ballot / prefix scans inside the wavefront and carry from one round of 64 digars to the next:
//   lcd_bam_refine_measure_kernel  the merged CIGAR words (longcalld_push_cigar, :112; hard clip as first / last word -> soft clip) into the job's word arena and
//                                  compared with the record's own words as they are made; new pos, reference length, bin, NM; the lengths of the MD / cs texts
//                                  (get_md_from_digar :1739, get_cs_from_digar :1773); the texts themselves generated ONCE MORE byte by byte against the record's
//                                  first MD:Z / cs:Z value (no text is stored); per field keep / delete / append; the record's new length;
//   lcd_bam_refine_emit_kernel     after the host's prefix sum: core fields with block_size / pos / bin / n_cigar patched, name, the new words, bases, qualities and
//                                  the auxiliary fields without the deleted ones (wave_copy), then NM:i, MD:Z, cs:Z (generated in place), HP:i, PS:i.
// A record that is not refined (filtered; no digars; digar2qlen != l_seq or fields that do not fit the record; first position < 1; more than 65 535 operations;
// a CIGAR that lives in a CG tag) gets exactly what lcd_bam_tag_emit_kernel gives it.  The rules where the reference exits or htslib would decide are in
// include/lcd_hotpath.h (lcd_chunk_refine_records).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "bam_aux_hop.h"

namespace {
using lcd_wave::ld32u;
using lcd_aux::aux2i;

__device__ __forceinline__ int scan_add(int v, const int lane) { // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ int scan_max(int v, const int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v = max(v, t); }
    return v;
}
__device__ __forceinline__ int wave_sum(int v, const int lane) { return __shfl(scan_add(v, lane), 63); }
__device__ __forceinline__ int ndigits(unsigned v) { int n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
__device__ __forceinline__ uint32_t reg2bin(long long beg, long long end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// the fixed part of a record: every value is the same on all lanes
struct RecView { const uint8_t *src, *cig, *seq, *aux, *end; unsigned lname, nc; int lseq, pos; bool layout_ok; };
__device__ __forceinline__ RecView rec_view(const BamRefineJob &j) {
    RecView v;
    v.src = (const uint8_t *)(uintptr_t)j.src; v.end = v.src + j.len;
    const uint8_t *r = v.src + 4;
    v.pos = (int)ld32u(r + 4);
    v.lname = ld32u(r + 8) & 0xff; v.nc = ld32u(r + 12) & 0xffff; v.lseq = (int)ld32u(r + 16);
    v.cig = r + 32 + v.lname; v.seq = v.cig + 4ull * v.nc;
    v.aux = v.seq + (unsigned long long)(((long long)v.lseq + 1) / 2) + (unsigned long long)(long long)v.lseq;
    v.layout_ok = v.lseq >= 0 && v.aux <= v.end;
    return v;
}
// the FIRST field of a name: [beg, end) from src, its type and the first four bytes of its value
struct Field { unsigned beg, end, val; uint8_t ty; bool have; };
#define LCD_FIELD_HIT(F, A, B) if (t0 == (A) && t1 == (B) && !(F).have) { (F).have = true; (F).ty = ty; (F).val = ld32u(aux); (F).beg = (unsigned)(fld - v.src); (F).end = (F).beg + 3u + (unsigned)sz; }
__device__ __forceinline__ void aux_walk(const RecView &v, Field &nm, Field &md, Field &cs, Field &hp, Field &ps, Field &cg) {
    const Field none = {0u, 0u, 0u, 0, false};
    nm = md = cs = hp = ps = cg = none;
    if (!v.layout_ok) return;
    const uint8_t *aux = v.aux;
    while (aux + 3 <= v.end) {
        const unsigned h = ld32u(aux);
        const uint8_t t0 = (uint8_t)(h & 0xff), t1 = (uint8_t)((h >> 8) & 0xff), ty = (uint8_t)((h >> 16) & 0xff);
        const uint8_t *fld = aux; aux += 3;
        size_t sz = 0;
        if (!lcd_aux::value_size(ty, aux, v.end, &sz)) break;
        LCD_FIELD_HIT(nm, 'N', 'M') else LCD_FIELD_HIT(md, 'M', 'D') else LCD_FIELD_HIT(cs, 'c', 's') else LCD_FIELD_HIT(hp, 'H', 'P') else LCD_FIELD_HIT(ps, 'P', 'S')
        else LCD_FIELD_HIT(cg, 'C', 'G')
        aux += sz;
    }
}
#undef LCD_FIELD_HIT

__device__ __forceinline__ int read_code(const RecView &v, const int q) { // seq_nt16_int of the record's 4-bit base q
    if (q < 0 || q >= v.lseq) return 4;
    const unsigned nib = (v.seq[q >> 1] >> ((q & 1) ? 0 : 4)) & 15u;
    return nib == 1 ? 0 : nib == 2 ? 1 : nib == 4 ? 2 : nib == 8 ? 3 : 4;
}
struct RefWin { const uint8_t *ref; long long beg, end; };
__device__ __forceinline__ int ref_code(const RefWin &w, const long long p) { // the reference's bounds test: beg <= p < end, N elsewhere
    if (p >= w.beg && p < w.end) { const unsigned c = w.ref[p - w.beg]; return c < 4u ? (int)c : 4; }
    return 4;
}

// where the MD / cs bytes of the 64 digars of one round go; the carry runs over the rounds of a read
struct TextCarry { int eq, mark, md, cs; };   // '=' bases so far; that sum at the last X / D digar; MD / cs bytes so far
struct TextLane { int eq_len, md_n, cs_n, md_off, cs_off; };
__device__ __forceinline__ TextLane text_round(const int type, const int len, const int lane, TextCarry &c) {
    const int S = c.eq + scan_add(type == 7 ? len : 0, lane);
    const bool xd = type == 8 || type == 2;
    const int mi = scan_max(xd ? S : 0, lane);            // (S never falls: the latest X / D digar has the largest mark)
    int me = __shfl_up(mi, 1); if (lane == 0) me = 0;
    me = max(me, c.mark);
    TextLane t;
    t.eq_len = S - me;                                    // MD's eq_len when this X / D digar prints it
    t.md_n = xd ? ndigits((unsigned)t.eq_len) + (type == 2 ? 1 : 0) + len : 0;
    t.cs_n = type == 7 ? 1 + ndigits((unsigned)len) : type == 8 ? 3 * len : (type == 1 || type == 2) ? 1 + len : 0;
    const int mdi = scan_add(t.md_n, lane), csi = scan_add(t.cs_n, lane);
    t.md_off = c.md + mdi - t.md_n; t.cs_off = c.cs + csi - t.cs_n;
    c.eq = __shfl(S, 63); c.mark = max(c.mark, __shfl(mi, 63)); c.md += __shfl(mdi, 63); c.cs += __shfl(csi, 63);
    return t;
}
template <class Put> __device__ __forceinline__ void put_dec(Put &put, const unsigned o, unsigned v) {
    const int n = ndigits(v);
    for (int k = n - 1; k >= 0; --k) { put(o + (unsigned)k, (uint8_t)('0' + v % 10u)); v /= 10u; }
}
// the MD and / or cs text of a digar list, byte by byte through put_md(offset, byte) / put_cs(offset, byte): a lane writes the bytes of its own digars
template <class PutMd, class PutCs>
__device__ __forceinline__ void gen_text(const DigarRec *dig, const int n, const RecView &v, const RefWin &w, const int lane, const bool do_md, const bool do_cs,
                                         PutMd put_md, PutCs put_cs) {
    TextCarry c = {0, 0, 0, 0};
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane; const bool valid = k < n;
        DigarRec d; d.pos = 0; d.type = -2; d.len = 0; d.qi = 0; d.is_low_qual = 0;
        if (valid) d = dig[k];
        const TextLane t = text_round(d.type, d.len, lane, c);
        if (do_md && (d.type == 8 || d.type == 2)) {
            unsigned o = (unsigned)t.md_off;
            put_dec(put_md, o, (unsigned)t.eq_len); o += (unsigned)ndigits((unsigned)t.eq_len);
            if (d.type == 2) put_md(o++, (uint8_t)'^');
            for (int x = 0; x < d.len; ++x) put_md(o++, (uint8_t)"ACGTN"[ref_code(w, d.pos + x)]);
        }
        if (do_cs) {
            unsigned o = (unsigned)t.cs_off;
            if (d.type == 7) { put_cs(o, (uint8_t)':'); put_dec(put_cs, o + 1, (unsigned)d.len); }
            else if (d.type == 8)
                for (int x = 0; x < d.len; ++x) { put_cs(o++, (uint8_t)'*'); put_cs(o++, (uint8_t)"acgtn"[ref_code(w, d.pos + x)]); put_cs(o++, (uint8_t)"acgtn"[read_code(v, d.qi + x)]); }
            else if (d.type == 1) { put_cs(o++, (uint8_t)'+'); for (int x = 0; x < d.len; ++x) put_cs(o++, (uint8_t)"acgtn"[read_code(v, d.qi + x)]); }
            else if (d.type == 2) { put_cs(o++, (uint8_t)'-'); for (int x = 0; x < d.len; ++x) put_cs(o++, (uint8_t)"acgtn"[ref_code(w, d.pos + x)]); }
        }
    }
    const int tail = c.eq - c.mark;
    if (do_md && tail > 0 && lane == 0) put_dec(put_md, (unsigned)c.md, (unsigned)tail);
}
} // namespace

__global__ void __launch_bounds__(64) lcd_bam_refine_measure_kernel(const BamRefineJob *jobs, BamRefineOut *outs, const uint8_t *ref, const long long ref_beg,
                                                                    const long long ref_end, const int n_jobs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_jobs) return;
    const BamRefineJob j = jobs[i];
    const RecView v = rec_view(j);
    const RefWin w = {ref, ref_beg, ref_end};
    Field nm, md, cs, hp, ps, cg;
    aux_walk(v, nm, md, cs, hp, ps, cg);
    const DigarRec *dig = (const DigarRec *)(uintptr_t)j.dig;
    uint32_t *words = (uint32_t *)(uintptr_t)j.words;
    const int n = j.n_digar;

    BamRefineOut o;
    o.flags = 0; o.n_ops = v.nc; o.md_len = o.cs_len = 0; o.nm = 0; o.new_pos = v.pos; o.pos_moved = 0; o.new_bin = 0; o.dst = 0;
    unsigned state = LCD_REFINE_FILTERED;
    if (j.kept) {
        if (j.skipped || n <= 0) state = LCD_REFINE_NO_DIGARS;
        else if (!v.layout_ok) state = LCD_REFINE_QLEN;
        else {
            // ---- pass 1: the merged words (compared as they are made), NM, reference length, MD / cs lengths ----
            int carry_t = 0, carry_start = -1, carry_type = -1, runs = 0, nm_l = 0, rl_l = 0;
            bool mism = false;
            TextCarry tc = {0, 0, 0, 0};
            for (int base = 0; base < n; base += 64) {
                const int k = base + lane; const bool valid = k < n;
                int type = -2, len = 0;
                if (valid) { type = dig[k].type; len = dig[k].len; }
                int pt = __shfl_up(type, 1); if (lane == 0) pt = carry_type;
                const bool start = valid && type != pt;
                const unsigned long long bal = __ballot(start);
                const int m = runs + __popcll(bal & ((1ull << lane) - 1ull));          // the run that starts at this digar
                const int ti = carry_t + scan_add(len, lane), te = ti - len;
                const int sm = scan_max(start ? te : -1, lane);
                int pstart = __shfl_up(sm, 1); if (lane == 0) pstart = -1;
                pstart = max(pstart, carry_start);                                   // where the run in front of this digar starts
                if (start && m > 0 && m <= 65535) {                                  // this start closes word m - 1
                    const unsigned op = (m == 1 && pt == 5) ? 4u : (unsigned)pt;
                    const uint32_t wd = ((uint32_t)(te - pstart) << 4) | op;
                    words[m - 1] = wd;
                    if ((unsigned)(m - 1) >= v.nc || ld32u(v.cig + 4ull * (unsigned)(m - 1)) != wd) mism = true;
                }
                if (type == 8 || type == 1 || type == 2) nm_l += len;
                if (type == 0 || type == 2 || type == 3 || type == 7 || type == 8) rl_l += len;
                (void)text_round(type, len, lane, tc);
                const int last = min(63, n - 1 - base);
                carry_t = __shfl(ti, 63); carry_start = max(carry_start, __shfl(sm, 63)); carry_type = __shfl(type, last);
                runs += __popcll(bal);
            }
            if (runs >= 1 && runs <= 65535) {                                        // the last word
                const unsigned op = carry_type == 5 ? 4u : (unsigned)carry_type;
                const uint32_t wd = ((uint32_t)(carry_t - carry_start) << 4) | op;
                if (lane == 0) words[runs - 1] = wd;
                if ((unsigned)(runs - 1) >= v.nc || ld32u(v.cig + 4ull * (unsigned)(runs - 1)) != wd) mism = true;
            }
            const bool identical = (unsigned)runs == v.nc && __ballot(mism) == 0ull;
            const int tail = tc.eq - tc.mark;
            o.n_ops = (uint32_t)runs; o.nm = wave_sum(nm_l, lane);
            o.md_len = (uint32_t)(tc.md + (tail > 0 ? ndigits((unsigned)tail) : 0)); o.cs_len = (uint32_t)tc.cs;
            const int rl = wave_sum(rl_l, lane);
            const DigarRec d0 = dig[0], dl = dig[n - 1];
            const int dq = dl.qi + ((dl.type == 7 || dl.type == 0 || dl.type == 8 || dl.type == 1 || dl.type == 4 || dl.type == 5) ? dl.len : 0);   // digar2qlen
            const bool in_cg = v.nc == 2 && ld32u(v.cig) == (((uint32_t)v.lseq << 4) | 4u) && (ld32u(v.cig + 4) & 15u) == 3u && cg.have && cg.ty == 'B';
            if (dq != v.lseq) state = LCD_REFINE_QLEN;
            else if (d0.pos < 1) state = LCD_REFINE_POS;
            else if (runs > 65535) state = LCD_REFINE_OPS;
            else if (in_cg) state = LCD_REFINE_CG;
            else {
                state = identical ? LCD_REFINE_IDENTICAL : LCD_REFINE_CHANGED;
                o.new_pos = (int)(d0.pos - 1);
                o.pos_moved = o.new_pos != v.pos;
                if (o.pos_moved || !identical) { o.flags |= 64u; o.new_bin = reg2bin((long long)o.new_pos, (long long)o.new_pos + (rl > 0 ? rl : 1)); }
            }
        }
    }
    if (state != LCD_REFINE_CHANGED) o.n_ops = v.nc;
    // ---- the fields: NM / MD / cs only where the CIGAR changed; HP / PS as lcd_bam_tag_measure_kernel decides them ----
    unsigned db[5], de[5], n_del = 0, app = 0;
    if (state == LCD_REFINE_CHANGED) {
        o.flags |= 32u;
        if (nm.have && aux2i(nm.ty, nm.val) != (long long)o.nm) { o.flags |= 1u; db[n_del] = nm.beg; de[n_del] = nm.end; ++n_del; app += 7u; }
        const bool md_z = md.have && md.ty == 'Z', cs_z = cs.have && cs.ty == 'Z';
        if (md_z || cs_z) {
            const uint8_t *old_md = v.src + md.beg + 3, *old_cs = v.src + cs.beg + 3;
            const unsigned old_md_len = md_z ? md.end - md.beg - 4u : 0u, old_cs_len = cs_z ? cs.end - cs.beg - 4u : 0u;
            bool md_diff = false, cs_diff = false;
            gen_text(dig, n, v, w, lane, md_z && old_md_len == o.md_len, cs_z && old_cs_len == o.cs_len,
                     [&](const unsigned at, const uint8_t b) { if (at >= old_md_len || old_md[at] != b) md_diff = true; },
                     [&](const unsigned at, const uint8_t b) { if (at >= old_cs_len || old_cs[at] != b) cs_diff = true; });
            if (md_z && (old_md_len != o.md_len || __ballot(md_diff) != 0ull)) { o.flags |= 2u; db[n_del] = md.beg; de[n_del] = md.end; ++n_del; app += 4u + o.md_len; }
            if (cs_z && (old_cs_len != o.cs_len || __ballot(cs_diff) != 0ull)) { o.flags |= 4u; db[n_del] = cs.beg; de[n_del] = cs.end; ++n_del; app += 4u + o.cs_len; }
        }
    }
    const bool want_hp = j.kept && j.hap != 0, want_ps = j.kept && j.ps > 0;
    const bool keep_hp = want_hp && hp.have && aux2i(hp.ty, hp.val) == (long long)j.hap, keep_ps = want_ps && ps.have && aux2i(ps.ty, ps.val) == j.ps;
    if (want_hp && !keep_hp) { o.flags |= 8u; app += 7u; }
    if (want_ps && !keep_ps) { o.flags |= 16u; app += 7u; }
    if (hp.have && !keep_hp) { db[n_del] = hp.beg; de[n_del] = hp.end; ++n_del; }
    if (ps.have && !keep_ps) { db[n_del] = ps.beg; de[n_del] = ps.end; ++n_del; }
    for (unsigned k = n_del; k < 5; ++k) db[k] = de[k] = j.len;
#pragma unroll
    for (int a = 0; a < 4; ++a)                                                      // five spans, ascending
#pragma unroll
        for (int b = 0; b < 4 - a; ++b)
            if (db[b + 1] < db[b]) { const unsigned t0 = db[b], t1 = de[b]; db[b] = db[b + 1]; de[b] = de[b + 1]; db[b + 1] = t0; de[b + 1] = t1; }
    unsigned gone = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { o.del_beg[k] = db[k]; o.del_end[k] = de[k]; gone += de[k] - db[k]; }
    o.state = state;
    o.new_len = j.len + 4u * o.n_ops - 4u * v.nc - gone + app;
    if (lane == 0) outs[i] = o;
}

__global__ void __launch_bounds__(64) lcd_bam_refine_emit_kernel(const BamRefineJob *jobs, const BamRefineOut *outs, const uint8_t *ref, const long long ref_beg,
                                                                 const long long ref_end, uint8_t *out, const int n_jobs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_jobs) return;
    const BamRefineJob j = jobs[i]; const BamRefineOut o = outs[i];
    const RecView v = rec_view(j);
    const RefWin w = {ref, ref_beg, ref_end};
    uint8_t *dst = out + o.dst;
    // a record whose CIGAR and position stay (filtered, unrefined, identical in place) is copied as lcd_bam_tag_emit_kernel copies it: [4, len) without the deleted
    // fields, whatever its name and CIGAR lengths claim -- nothing is read behind the record
    unsigned at, from;
    if (!(o.flags & 96u)) {
        const unsigned bs = o.new_len - 4u;
        if (lane < 4) dst[lane] = (uint8_t)((bs >> (8 * lane)) & 255u);
        at = 4; from = 4;
    } else {
        // block_size and the 32 core bytes: one byte per lane, the patched words chosen by index
        if (lane < 36) {
            const unsigned wi = (unsigned)lane >> 2;
            unsigned x = ld32u(v.src + 4u * wi);
            if (wi == 0) x = o.new_len - 4u;
            else if (wi == 2 && (o.flags & 64u)) x = (unsigned)o.new_pos;
            else if (wi == 3 && (o.flags & 64u)) x = (x & 0xffffu) | (o.new_bin << 16);
            else if (wi == 4) x = (x & 0xffff0000u) | (o.n_ops & 0xffffu);
            dst[lane] = (uint8_t)((x >> (8 * (lane & 3))) & 255u);
        }
        at = 36;
        lcd_wave::wave_copy(dst + at, v.src + 36, (long long)v.lname, lane); at += v.lname;
        if (o.flags & 32u) lcd_wave::wave_copy(dst + at, (const uint8_t *)(uintptr_t)j.words, 4ll * o.n_ops, lane);
        else lcd_wave::wave_copy(dst + at, v.cig, 4ll * v.nc, lane);
        at += 4u * o.n_ops;
        from = 36u + v.lname + 4u * v.nc;                                      // bases, qualities and the fields that stay
    }
    for (int k = 0; k < 5; ++k) {
        lcd_wave::wave_copy(dst + at, v.src + from, (long long)o.del_beg[k] - (long long)from, lane);
        at += o.del_beg[k] - from; from = o.del_end[k];
    }
    lcd_wave::wave_copy(dst + at, v.src + from, (long long)j.len - (long long)from, lane); at += j.len - from;
    if (o.flags & 1u) { if (lane < 7) dst[at + lane] = lane == 0 ? 'N' : lane == 1 ? 'M' : lane == 2 ? 'i' : (uint8_t)(((unsigned)o.nm >> (8 * (lane - 3))) & 255u); at += 7; }
    if (o.flags & 6u) {
        const bool do_md = (o.flags & 2u) != 0, do_cs = (o.flags & 4u) != 0;
        uint8_t *md_at = dst + at + 3, *cs_at = dst + at + (do_md ? 4u + o.md_len : 0u) + 3;
        if (do_md && lane < 3) md_at[lane - 3] = (uint8_t)"MDZ"[lane];
        if (do_md && lane == 3) md_at[o.md_len] = 0;
        if (do_cs && lane >= 4 && lane < 7) cs_at[lane - 7] = (uint8_t)"csZ"[lane - 4];
        if (do_cs && lane == 7) cs_at[o.cs_len] = 0;
        gen_text((const DigarRec *)(uintptr_t)j.dig, j.n_digar, v, w, lane, do_md, do_cs,
                 [&](const unsigned p, const uint8_t b) { if (p < o.md_len) md_at[p] = b; },
                 [&](const unsigned p, const uint8_t b) { if (p < o.cs_len) cs_at[p] = b; });
        at += (do_md ? 4u + o.md_len : 0u) + (do_cs ? 4u + o.cs_len : 0u);
    }
    if (o.flags & 8u) { if (lane < 7) dst[at + lane] = lane == 0 ? 'H' : lane == 1 ? 'P' : lane == 2 ? 'i' : (uint8_t)(((unsigned)j.hap >> (8 * (lane - 3))) & 255u); at += 7; }
    if (o.flags & 16u) { if (lane < 7) dst[at + lane] = lane == 0 ? 'P' : lane == 1 ? 'S' : lane == 2 ? 'i' : (uint8_t)(((unsigned)(unsigned long long)j.ps >> (8 * (lane - 3))) & 255u); }
}

void lcd_launch_bam_refine_measure(const BamRefineJob *jobs, BamRefineOut *outs, const uint8_t *ref, long long ref_beg, long long ref_end, int n_jobs, hipStream_t st) {
    if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_refine_measure_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs, ref, ref_beg, ref_end, n_jobs);
}
void lcd_launch_bam_refine_emit(const BamRefineJob *jobs, const BamRefineOut *outs, const uint8_t *ref, long long ref_beg, long long ref_end, uint8_t *out, int n_jobs,
                                hipStream_t st) {
    if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_refine_emit_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs, ref, ref_beg, ref_end, out, n_jobs);
}
