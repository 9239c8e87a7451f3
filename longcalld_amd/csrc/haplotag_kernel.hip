// haplotag_kernel.hip -- the kept records of a chunk, where the inflate left them in HBM, against the phased sites of their contig (the rules: include/lcd_hotpath.h,
// lcd_chunk_haplotag; the same rules in Python: tests/haplotag_common.py):
//   lcd_htag_measure_kernel  one wavefront per record: the layout check, the operation words (the record's own, or its CG field's: lcd_aux::cg_ops), the span from a
//                            64-bit wave sum of the reference lengths; lane 0 finds the candidate range by two binary searches;
//   lcd_htag_scan_kernel     ONE wavefront: the exclusive prefix of the candidate counts, 64 records per round;
//   lcd_htag_mark_kernel     one wavefront per record, 64 operations per step with carried 64-bit scans of the reference and query offsets.  Every rule is local
//                            to one operation, so nothing else crosses a step: a match lane sets the base bits of the SNV sites inside its interval, a D / N / I
//                            lane the alt-match or disturbed bit of the sites within max_footprint of it.  32-bit vector atomicOr, four pair bytes per word: the
//                            result does not depend on the order of arrival;
//   lcd_htag_reduce_kernel   one wavefront per record, lanes striding the candidates: the verdict bytes, then one pass per distinct phase set among the votes (in
//                            ps_idx order: wave sums of n1 / n2, wave minima of the first voting candidate and of the next set).
// No LDS, no float arithmetic.  Every site index lies in [lo, lo + n_cand) of the record, a sub-range of the table; every pair index below cand_off[n_jobs].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "bam_aux_hop.h"

namespace {
using lcd_wave::ld32u;

__device__ __forceinline__ unsigned long long scan_add64(unsigned long long v, const int lane) { // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ int wave_sum32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_min32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int t = __shfl_xor(v, d); v = t < v ? t : v; }
    return v;
}
enum { HS_RECORDS, HS_PAIRS, HS_VERDICT, HS_TAGGED = HS_VERDICT + 5, HS_MULTI_PS = HS_TAGGED + 3, HS_CG, HS_BAD, HS_NO_SEQ };
__device__ __forceinline__ void stat_add(const HtagIn &in, const int lane, const int which, const unsigned long long n) {
    if (lane == 0 && n) atomicAdd(in.stats + which, n);
}
// the first index in [a, b) whose position is >= key (b when there is none); bound: a <= b <= n_sites
__device__ __forceinline__ long long lower_pos(const long long *pos, long long a, long long b, const long long key) {
    while (a < b) { const long long m = a + ((b - a) >> 1); if (pos[m] < key) a = m + 1; else b = m; }
    return a;
}
__device__ __forceinline__ long long fp_end(const unsigned kind, const long long pos, const int len) {
    return kind == 0u ? pos : kind == 1u ? pos + 1 : pos + (long long)len;
}
// the verdict of candidate site s of a record with span [beg, end] and the pair byte b
__device__ __forceinline__ int verdict_of(const HtagSites &t, const long long s, const long long beg, const long long end, const unsigned b) {
    const long long pos = t.pos[s]; const unsigned kind = t.meta[s] & 3u;
    const long long fe = fp_end(kind, pos, t.len[s]);
    if (fe < beg || pos > end) return LCD_HTAG_NO_PAIR;
    if (pos < beg || fe > end) return LCD_HTAG_NONE;
    if (b & LCD_HTAG_DIST) return LCD_HTAG_OTHER;
    if (b & LCD_HTAG_ALTM) return LCD_HTAG_ALT;
    if (kind == 0u) return (b & LCD_HTAG_B_OTHER) ? LCD_HTAG_OTHER : (b & LCD_HTAG_B_LOWQ) ? LCD_HTAG_LOWQ : (b & LCD_HTAG_B_ALT) ? LCD_HTAG_ALT : (b & LCD_HTAG_B_REF) ? LCD_HTAG_REF : LCD_HTAG_OTHER;
    return LCD_HTAG_REF;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_htag_measure_kernel(const HtagIn in) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const HtagJob j = in.jobs[i];
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src, *end = src + j.len, *r = src + 4;      // (at least 36 bytes: the host refuses anything shorter)
    const long long pos1 = (long long)(int)ld32u(r + 4) + 1;
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xffu, nc16 = w3 & 0xffffu;
    const long long lseq = (long long)(int)ld32u(r + 16);
    HtagRec o; o.beg = pos1; o.end = pos1 - 1; o.lo = 0; o.ops = 0; o.n_ops = 0; o.n_cand = 0; o.lseq = 0; o.seq_off = 0; o.bad = 0; o.pad = 0;
    stat_add(in, lane, HS_RECORDS, 1);
    // everything the passes read lies inside [src, end): name, operation words, bases and qualities end in front of the auxiliary fields, and lcd_aux::cg_ops
    // keeps inside the record by itself.  A record whose fields run past its end is a bad one
    if (lseq < 0 || lseq > (long long)j.cap || (unsigned long long)(end - src) < 36ull + lname + 4ull * nc16 + (unsigned long long)((lseq + 1) / 2) + (unsigned long long)lseq) {
        o.bad = 1;
        if (lane == 0) in.recs[i] = o;
        stat_add(in, lane, HS_BAD, 1);
        return;
    }
    if (lseq == 0) stat_add(in, lane, HS_NO_SEQ, 1);
    const uint8_t *cig = src + 36 + lname; int nc = (int)nc16;
    if (lcd_aux::cg_ops(r, lname, nc, (int)lseq, (int)j.len - 4, lane, &cig, &nc)) stat_add(in, lane, HS_CG, 1);
    unsigned long long rl = 0;
    for (unsigned k = (unsigned)lane; k < (unsigned)(nc > 0 ? nc : 0); k += 64) {
        const unsigned w = ld32u(cig + 4ull * k);                        // bound: k < the operations' count, whose words lie inside the record
        const unsigned op = w & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) rl += w >> 4;
    }
    rl = __shfl(scan_add64(rl, lane), 63);
    if (lane != 0) return;
    o.end = pos1 + (long long)rl - 1;
    o.ops = (unsigned long long)(uintptr_t)cig; o.n_ops = (unsigned)(nc > 0 ? nc : 0); o.lseq = (int)lseq; o.seq_off = 36u + lname + 4u * nc16;
    if (o.end >= o.beg && in.t.n_sites > 0) {
        const long long a = lower_pos(in.t.pos, 0, in.t.n_sites, o.beg - (long long)(in.t.max_fp - 1));
        const long long b = lower_pos(in.t.pos, a, in.t.n_sites, o.end + 1);
        const long long n = b - a;
        o.lo = a; o.n_cand = (unsigned)(n < 0x7fffffffll ? n : 0x7fffffffll);        // (a record below 2^31 candidates: the host refuses larger tables)
    }
    in.recs[i] = o;
}

__global__ void __launch_bounds__(64) lcd_htag_scan_kernel(const HtagIn in) {
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (int b = 0; b < in.n_jobs; b += 64) {
        const int i = b + lane;
        const unsigned long long v = i < in.n_jobs ? (unsigned long long)in.recs[i].n_cand : 0ull;
        const unsigned long long inc = scan_add64(v, lane);
        if (i < in.n_jobs) in.cand_off[i] = carry + inc - v;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) in.cand_off[in.n_jobs] = carry;
}

__global__ void __launch_bounds__(64) lcd_htag_mark_kernel(const HtagIn in) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const HtagRec rc = in.recs[i];
    if (rc.bad || rc.n_cand == 0u) return;
    const HtagSites &t = in.t;
    const uint8_t *src = (const uint8_t *)(uintptr_t)in.jobs[i].src;
    const uint8_t *cig = (const uint8_t *)(uintptr_t)rc.ops, *seq = src + rc.seq_off, *qual = seq + ((size_t)rc.lseq + 1) / 2;
    const long long lo = rc.lo, hi = rc.lo + (long long)rc.n_cand, lseq = rc.lseq;
    const unsigned long long off = in.cand_off[i];
    // bound: lo <= s < hi, so the pair index is below cand_off[i + 1]
    auto set_bits = [&](const long long s, const unsigned b) {
        const unsigned long long p = off + (unsigned long long)(s - lo);
        atomicOr(in.bits + (p >> 2), b << (8u * (unsigned)(p & 3ull)));
    };
    auto code_at = [&](const long long q) -> unsigned { return (seq[q >> 1] >> ((q & 1) ? 0 : 4)) & 15u; };     // bound: 0 <= q < l_seq
    unsigned long long ref_done = 0, q_done = 0;
    for (unsigned base = 0; base < rc.n_ops; base += 64) {
        const unsigned k = base + (unsigned)lane;
        const unsigned w = k < rc.n_ops ? ld32u(cig + 4ull * k) : 0u;    // bound: k < the operations' count, whose words lie inside the record
        const unsigned op = w & 15u; const long long len = (long long)(w >> 4);
        const bool cr = len != 0 && (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u);
        const bool cq = len != 0 && (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u);
        const unsigned long long rl = cr ? (unsigned long long)len : 0ull, ql = cq ? (unsigned long long)len : 0ull;
        const unsigned long long ri = scan_add64(rl, lane), qi = scan_add64(ql, lane);
        const long long rb = rc.beg + (long long)(ref_done + ri - rl);   // the op's first reference position (an I: the r of its boundary r - 1 | r)
        const long long qb = (long long)(q_done + qi - ql);              // its first base's index
        if (len != 0 && (op == 0u || op == 7u || op == 8u)) {
            const long long re = rb + len - 1;
            for (long long s = lower_pos(t.pos, lo, hi, rb); s < hi; ++s) {
                const long long pos = t.pos[s];
                if (pos > re) break;
                const unsigned m = t.meta[s];
                if ((m & 3u) != 0u) continue;
                const long long q = qb + (pos - rb);
                unsigned b;
                if (q < 0 || q >= lseq) b = LCD_HTAG_B_OTHER;
                else if ((int)qual[q] < in.min_bq) b = LCD_HTAG_B_LOWQ;
                else { const unsigned c = code_at(q); b = c == ((m >> 8) & 15u) ? LCD_HTAG_B_ALT : c == ((m >> 4) & 15u) ? LCD_HTAG_B_REF : LCD_HTAG_B_OTHER; }
                set_bits(s, b);
            }
        } else if (len != 0 && (op == 2u || op == 3u)) {
            const long long re = rb + len - 1;
            for (long long s = lower_pos(t.pos, lo, hi, rb - (long long)(t.max_fp - 1)); s < hi; ++s) {
                const long long pos = t.pos[s];
                if (pos > re) break;
                const unsigned kind = t.meta[s] & 3u; const int sl = t.len[s];
                if (fp_end(kind, pos, sl) < rb) continue;
                set_bits(s, (op == 2u && kind == 2u && pos + 1 == rb && (long long)sl == len) ? LCD_HTAG_ALTM : LCD_HTAG_DIST);
            }
        } else if (len != 0 && op == 1u) {
            for (long long s = lower_pos(t.pos, lo, hi, rb - (long long)(t.max_fp - 1)); s < hi; ++s) {
                const long long pos = t.pos[s];
                if (pos >= rb) break;
                const unsigned kind = t.meta[s] & 3u; const int sl = t.len[s];
                if (fp_end(kind, pos, sl) < rb) continue;
                bool match = kind == 1u && pos + 1 == rb && (long long)sl == len && qb >= 0 && qb + len <= lseq;
                if (match) {
                    const long long io = t.ins_off[s];
                    match = io >= 0 && io + len <= t.pool_size;          // (the table's own invariant; kept as the load's bound)
                    for (long long e = 0; match && e < len; ++e) match = code_at(qb + e) == (unsigned)t.pool[io + e];
                }
                set_bits(s, match ? LCD_HTAG_ALTM : LCD_HTAG_DIST);
            }
        }
        ref_done += __shfl(ri, 63); q_done += __shfl(qi, 63);
    }
}

__global__ void __launch_bounds__(64) lcd_htag_reduce_kernel(const HtagIn in) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const HtagRec rc = in.recs[i];
    const HtagSites &t = in.t;
    const int read = in.jobs[i].read;
    const unsigned long long off = in.cand_off[i];
    const int n = (int)rc.n_cand;                                        // (below 2^31)
    // the vote of candidate k: 0 none, 1 / 2 the haplotype
    auto verdict = [&](const int k) -> int {
        const unsigned long long p = off + (unsigned long long)k;
        return verdict_of(t, rc.lo + k, rc.beg, rc.end, (in.bits[p >> 2] >> (8u * (unsigned)(p & 3ull))) & 0xffu);
    };
    int cnt[6] = {0, 0, 0, 0, 0, 0};                                     // verdicts 0 ... 4, and the candidates that are pairs
    int cur = -1, best_ps = -1, best_n1 = 0, best_n2 = 0, best_first = 0, n_sets = 0;
    for (;;) {
        int n1 = 0, n2 = 0, first = 0x7fffffff, nxt = 0x7fffffff;
        for (int k = lane; k < n; k += 64) {
            const int v = verdict(k);
            if (cur < 0) {
                in.verdict[off + (unsigned long long)k] = (uint8_t)v;    // bound: k < n_cand, the record's share of the candidates
                if (v != LCD_HTAG_NO_PAIR) { ++cnt[v]; ++cnt[5]; }
            }
            if (v != LCD_HTAG_REF && v != LCD_HTAG_ALT) continue;
            const long long s = rc.lo + k;
            const int ps = t.ps_idx[s];
            if (ps == cur) {
                const int ha = (int)((t.meta[s] >> 2) & 3u), h = v == LCD_HTAG_ALT ? ha : 3 - ha;
                if (h == 1) ++n1; else ++n2;
                if (k < first) first = k;
            } else if (ps > cur && ps < nxt) nxt = ps;
        }
        if (cur >= 0) {
            n1 = wave_sum32(n1); n2 = wave_sum32(n2); first = wave_min32(first);
            ++n_sets;
            if (best_ps < 0 || n1 + n2 > best_n1 + best_n2 || (n1 + n2 == best_n1 + best_n2 && first < best_first)) { best_ps = cur; best_n1 = n1; best_n2 = n2; best_first = first; }
        }
        nxt = wave_min32(nxt);
        if (nxt == 0x7fffffff) break;
        cur = nxt;                                                       // (strictly increasing: at most n_ps passes)
    }
#pragma unroll
    for (int z = 0; z < 6; ++z) cnt[z] = wave_sum32(cnt[z]);
    if (lane != 0) return;
    int hap = 0;
    if (best_ps >= 0) hap = best_n1 - best_n2 >= in.min_diff ? 1 : best_n2 - best_n1 >= in.min_diff ? 2 : 0;
    in.haps[read] = hap; in.ps[read] = hap && best_ps < t.n_ps ? t.ps_value[best_ps] : 0; in.n1[read] = best_n1; in.n2[read] = best_n2;
    stat_add(in, lane, HS_PAIRS, (unsigned long long)cnt[5]);
    for (int z = 0; z < 5; ++z) stat_add(in, lane, HS_VERDICT + z, (unsigned long long)cnt[z]);
    stat_add(in, lane, HS_TAGGED + hap, 1);
    if (n_sets > 1) stat_add(in, lane, HS_MULTI_PS, 1);
}

void lcd_launch_htag_measure(const HtagIn &in, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_htag_measure_kernel, dim3(in.n_jobs), dim3(64), 0, st, in);
}
void lcd_launch_htag_scan(const HtagIn &in, hipStream_t st) {
    hipLaunchKernelGGL(lcd_htag_scan_kernel, dim3(1), dim3(64), 0, st, in);
}
void lcd_launch_htag_mark(const HtagIn &in, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_htag_mark_kernel, dim3(in.n_jobs), dim3(64), 0, st, in);
}
void lcd_launch_htag_reduce(const HtagIn &in, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_htag_reduce_kernel, dim3(in.n_jobs), dim3(64), 0, st, in);
}
