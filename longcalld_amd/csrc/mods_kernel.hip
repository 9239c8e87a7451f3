// mods_kernel.hip -- the per-haplotype CpG methylation table of a chunk from the MM / ML tags of its records, where the inflate left them in HBM (the rules:
// include/lcd_hotpath.h, lcd_chunk_mod_pileup; the same rules in Python: tests/mods_common.py):
//   lcd_mods_sites_kernel    one lane per position of the region: 1 where the reference window has a CpG site ('+': C with G behind it, '-': G with C in front),
//                            0 elsewhere; lcd_launch_cv_scan turns the flags into each site's index of the dense counter table;
//   lcd_mods_pileup_kernel   one wavefront per kept record: hops the auxiliary fields for MM / ML / MN, walks the MM text twice with the SAME walk (walk_deltas:
//                            pass A validates every group and measures the wanted one, so that a bad record falls into its counter before anything is added;
//                            pass B turns the wanted group's calls into one class byte per occurrence of the base), then walks the stored bases 64 at a time
//                            against a window of 64 CIGAR ops, classifies every occurrence and adds it to its site's counter;
//   lcd_mods_compact_kernel  one lane per position: the sites with a counter above zero as dense rows (any order: the host sorts them by position).
// The delta text is parsed 64 bytes per step: the separators are balloted, the lane at a number's first digit converts it, a number that runs into the step's end is
// carried (value and digit count) and finished by lane 0 of the next step; ordinals come from a 64-bit wave scan of delta + 1 carried from step to step.  Counters
// are 32-bit integers added with vector global atomics: the table does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "bam_aux_hop.h"

namespace {
using lcd_wave::ld32u;
using lcd_aux::aux2i;

__device__ __forceinline__ unsigned long long scan_add64(unsigned long long v, const int lane) { // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ unsigned ref_at(const ModsIn &in, const long long p) { return p >= in.ref_beg && p <= in.ref_end ? (unsigned)in.ref[p - in.ref_beg] : 4u; }
// 1: '+' site at p, 2: '-' site at p, 0: none (N matches nothing; a position outside the window reads as N)
__device__ __forceinline__ int site_at(const ModsIn &in, const long long p) {
    const unsigned c = ref_at(in, p);
    if (c == 1u) return ref_at(in, p + 1) == 2u ? 1 : 0;
    if (c == 2u) return ref_at(in, p - 1) == 1u ? 2 : 0;
    return 0;
}

// the MM text is [t, t + tlen): byte p of it, 0 behind its end (0 is no character of the syntax: a text that ends early is a syntax error by itself)
__device__ __forceinline__ unsigned tx(const uint8_t *t, const long long tlen, const long long p) { return p < tlen ? (unsigned)t[p] : 0u; }

struct Head { bool ok; long long n_codes; long long ci; unsigned flag; };
// B S codes [flag] at p (the same on all lanes); p is left at the first byte of the delta list.  ci: the index of `code` in a letter list of a C+ group, else -1
__device__ __forceinline__ Head parse_head(const uint8_t *t, const long long tlen, long long &p, const unsigned code) {
    Head g; g.ok = false; g.n_codes = 0; g.ci = -1; g.flag = 0;
    const unsigned B = tx(t, tlen, p), S = tx(t, tlen, p + 1);
    if (!(B == 'A' || B == 'C' || B == 'G' || B == 'T' || B == 'U' || B == 'N') || !(S == '+' || S == '-')) return g;
    p += 2;
    unsigned c = tx(t, tlen, p);
    if (c - 'a' < 26u) {
        for (; (c = tx(t, tlen, p)) - 'a' < 26u; ++p) { if (g.ci < 0 && c == code) g.ci = g.n_codes; ++g.n_codes; }     // ends at the text's end at the latest
    } else if (c - '0' < 10u) {
        while (tx(t, tlen, p) - '0' < 10u) ++p;
        g.n_codes = 1;                                                                                             // a ChEBI id: one code, never the wanted one
    } else return g;
    if (!(B == 'C' && S == '+')) g.ci = -1;
    c = tx(t, tlen, p);
    if (c == '.' || c == '?') { g.flag = c; ++p; }
    g.ok = true;
    return g;
}

struct Deltas { bool ok; unsigned long long n, run; long long p_end; };   // n deltas, run = the sum of delta + 1 (clamped far above any l_seq), p_end: behind the ';'
// (,delta)* ';' from byte p on.  EMIT: the class (1 mod, 2 canon, 3 filtered) of the k-th call goes to cls[its ordinal], from the ML bytes at ml + k * n_codes
template <bool EMIT>
__device__ __forceinline__ Deltas walk_deltas(const uint8_t *t, const long long tlen, long long p, const int lane, const uint8_t *ml, const long long n_codes,
                                              const long long ci, const unsigned T, uint8_t *cls, const unsigned n_occ) {
    Deltas R; R.ok = false; R.n = 0; R.run = 0; R.p_end = p;
    int prev = 0;                                   // class of the byte in front of the step: 0 the group's head, 1 ',', 2 a digit
    unsigned long long cval = 0; int cdig = 0;      // prev == 2: the value and the digits so far of the number the step before ran into
    for (;;) {                                      // every step fails, ends at a ';' or moves 64 bytes on over bytes inside the text: at most tlen / 64 + 1 steps
        const long long q = p + lane;
        const unsigned c = tx(t, tlen, q);          // bound: q < tlen, and [t, t + tlen) is the Z value that value_size found inside the record
        const bool isd = c - '0' < 10u;
        const int cl = isd ? 2 : c == ',' ? 1 : c == ';' ? 3 : 4;
        const unsigned long long semis = __ballot(cl == 3);
        const int last = semis ? __ffsll((long long)semis) - 1 : 63;     // lanes 0 .. last belong to this list
        const bool in = lane <= last;
        int pc = __shfl_up(cl, 1); if (lane == 0) pc = prev;
        const bool good = (cl == 1 && (pc == 0 || pc == 2)) || (cl == 2 && (pc == 1 || pc == 2)) || (cl == 3 && (pc == 0 || pc == 2));
        if (__ballot(in && !good)) return R;
        const unsigned long long nd = ~__ballot(in && isd);              // (lanes behind `last` read as non-digits: the ';' ends the last number)
        // a number is converted by the lane of its first digit in this step; lane 0 also finishes the number the step before ran into (with or without digits here)
        const bool cont = lane == 0 && prev == 2;
        const bool mine = cont || (in && isd && pc != 2);
        bool emit = false, partial = false; unsigned long long val = 0; int digits = 0;
        if (mine) {
            int e = lane;                           // one behind my last digit of this step
            if (in && isd) { const unsigned long long m = nd & ~((2ull << lane) - 1ull); e = m ? __ffsll((long long)m) - 1 : 64; }
            const int k = e - lane;
            val = cont ? cval : 0; digits = (cont ? cdig : 0) + k;
            // bound: q + j < p + 64 and lane + j held a digit of the text, so q + j < tlen.  More than 10 digits are refused below, their value is never used
            for (int j = 0; j < (k < 11 ? k : 11); ++j) val = val * 10ull + (unsigned long long)(t[q + j] - '0');
            partial = e == 64; emit = !partial;
        }
        if (__ballot(mine && digits > 10)) return R;
        const unsigned long long pm = __ballot(partial);                 // at most one lane: the number that holds lane 63
        if (pm) { const int s = __ffsll((long long)pm) - 1; cval = __shfl(val, s); cdig = __shfl(digits, s); }
        const unsigned long long x = emit ? (val < (1ull << 33) ? val + 1ull : (1ull << 33)) : 0ull;       // (l_seq < 2^31: a clamped delta is an overrun all the same)
        const unsigned long long inc = scan_add64(x, lane);
        const unsigned long long em = __ballot(emit);
        if (EMIT && emit) {
            const unsigned long long ord = R.run + inc - 1ull, k = R.n + (unsigned long long)__popcll(em & ((1ull << lane) - 1ull));
            // bound: pass A found the last ordinal below n_occ and ordinals rise, so ord < n_occ <= l_seq, the size of cls; the test stays as the store's own bound.
            // ML: pass A found ml_off + n_codes * n_deltas <= the array's count, and k < n_deltas
            if (ord < (unsigned long long)n_occ) {
                const uint8_t *row = ml + k * (unsigned long long)n_codes;
                unsigned s = 0;
                for (long long z = 0; z < n_codes; ++z) { s += row[z]; if (s > 255u) s = 255u; }
                cls[ord] = (unsigned)row[ci] >= T ? 1 : 255u - s >= T ? 2 : 3;
            }
        }
        R.run += __shfl(inc, 63); if (R.run > (1ull << 40)) R.run = 1ull << 40;       // (a step adds at most 32 * 2^33)
        R.n += (unsigned long long)__popcll(em);
        if (semis) { R.p_end = p + last + 1; R.ok = true; return R; }
        prev = __shfl(cl, 63);
        p += 64;
    }
}

enum { ST_RECORDS, ST_NO_MM, ST_NO_GROUP, ST_HARD_CLIP, ST_MN, ST_SYNTAX, ST_OVERRUN, ST_ML_SHORT, ST_UNALIGNED, ST_OUTSIDE, ST_OFF_CONTEXT, ST_COUNTED };
__device__ __forceinline__ void stat_add(const ModsIn &in, const int lane, const int which, const unsigned long long n) {
    if (lane == 0 && n) atomicAdd(in.stats + which, n);
}
} // namespace

__global__ void __launch_bounds__(256) lcd_mods_sites_kernel(const ModsIn in, int *flag, const long long n_pos) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < n_pos) flag[k] = site_at(in, in.reg_beg + k) != 0;
}

__global__ void __launch_bounds__(64) lcd_mods_pileup_kernel(const ModsIn in) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const ModsJob j = in.jobs[i];
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src, *end = src + j.len, *r = src + 4;      // (at least 36 bytes: the host refuses anything shorter)
    const long long pos = (long long)(int)ld32u(r + 4);
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xffu, nc = w3 & 0xffffu, flag = w3 >> 16;
    const long long lseq = (long long)(int)ld32u(r + 16);
    const uint8_t *cig = src + 36 + lname, *seq = cig + 4ull * nc;
    stat_add(in, lane, ST_RECORDS, 1);
    // everything below reads inside [src, end): name, CIGAR, bases and qualities end at aux0 <= end; a record whose l_seq is not the one its class bytes were sized
    // for (it cannot be: the host took l_seq from the same bytes) is treated as one without tags
    if (lseq < 0 || lseq > (long long)j.cap || (unsigned long long)(end - src) < 36ull + lname + 4ull * nc + (unsigned long long)((lseq + 1) / 2) + (unsigned long long)lseq) {
        stat_add(in, lane, ST_NO_MM, 1); return;
    }
    const uint8_t *aux = seq + (lseq + 1) / 2 + lseq;
    // ---- MM / ML / MN: the first of each spelling; a field that runs past the record ends the walk (lcd_aux::value_size)
    const uint8_t *mm[2] = {nullptr, nullptr}, *ml[2] = {nullptr, nullptr}; long long mm_len[2] = {0, 0}; unsigned ml_cnt[2] = {0, 0};
    bool have_mn = false; long long mn = 0;
    while (aux + 3 <= end) {
        const unsigned h = (unsigned)aux[0] | ((unsigned)aux[1] << 8) | ((unsigned)aux[2] << 16);
        const unsigned tag = h & 0xffffu; const uint8_t ty = (uint8_t)(h >> 16);
        const uint8_t *val = aux + 3;
        size_t sz = 0;
        if (!lcd_aux::value_size(ty, val, end, &sz)) break;
        const int sp = tag == (unsigned)('M' | ('M' << 8)) || tag == (unsigned)('M' | ('L' << 8)) ? 0 : tag == (unsigned)('M' | ('m' << 8)) || tag == (unsigned)('M' | ('l' << 8)) ? 1 : -1;
        const bool is_mm = (tag >> 8) == 'M' || (tag >> 8) == 'm';
        if (sp >= 0 && is_mm && ty == 'Z') { if (!mm[sp]) { mm[sp] = val; mm_len[sp] = (long long)sz - 1; } }
        else if (sp >= 0 && !is_mm && ty == 'B' && val[0] == 'C') { if (!ml[sp]) { ml[sp] = val + 5; ml_cnt[sp] = ld32u(val + 1); } }
        else if (tag == (unsigned)('M' | ('N' << 8)) && !have_mn && (ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I')) {
            // the value's own bytes only (sz of them, inside the record)
            unsigned w = 0; for (size_t b = 0; b < sz; ++b) w |= (unsigned)val[b] << (8 * b);
            have_mn = true; mn = aux2i(ty, w);
        }
        aux = val + sz;
    }
    const int ms = mm[0] ? 0 : 1, ls = ml[0] ? 0 : 1;
    const uint8_t *t = mm[ms]; const long long tlen = mm_len[ms];
    const uint8_t *mlp = ml[ls]; const unsigned long long mlc = mlp ? ml_cnt[ls] : 0ull;
    if (!t) { stat_add(in, lane, ST_NO_MM, 1); return; }
    // ---- hard clip: the ops 64 at a time (bound: k < n_cigar, and the words end at seq <= end)
    for (unsigned base = 0; base < nc; base += 64) {
        const unsigned k = base + (unsigned)lane;
        const unsigned w = k < nc ? ld32u(cig + 4ull * k) : 0u;
        if (__ballot(k < nc && (w & 15u) == 5u)) { stat_add(in, lane, ST_HARD_CLIP, 1); return; }
    }
    if (have_mn && mn != lseq) { stat_add(in, lane, ST_MN, 1); return; }
    // ---- pass A: every group's syntax; of the first wanted group: where its list starts, its codes, its flag, its calls, its place in ML
    bool wanted = false; long long w_p = 0, w_codes = 0, w_ci = 0; unsigned w_flag = 0; unsigned long long w_n = 0, w_run = 0, ml_off = 0;
    for (long long p = 0; p < tlen;) {
        const Head g = parse_head(t, tlen, p, (unsigned)in.code);
        if (!g.ok) { stat_add(in, lane, ST_SYNTAX, 1); return; }
        const Deltas d = walk_deltas<false>(t, tlen, p, lane, nullptr, 0, 0, 0, nullptr, 0);
        if (!d.ok) { stat_add(in, lane, ST_SYNTAX, 1); return; }
        if (!wanted) {
            if (g.ci >= 0) { wanted = true; w_p = p; w_codes = g.n_codes; w_ci = g.ci; w_flag = g.flag; w_n = d.n; w_run = d.run; }
            else ml_off += (unsigned long long)g.n_codes * d.n;          // (codes and calls are bytes of one text below 2^31: the sum stays below 2^62)
        }
        p = d.p_end;
    }
    if (!wanted) { stat_add(in, lane, ST_NO_GROUP, 1); return; }
    // ---- the occurrences of the base as stored: C, or G for a reverse record (two bases per lane and step; bound: byte k < (l_seq + 1) / 2, base 2k + 1 < l_seq)
    const bool rev = (flag & 16u) != 0; const unsigned Bs = rev ? 4u : 2u;
    unsigned n_occ = 0;
    for (long long b0 = 0, nb = (lseq + 1) / 2; b0 < nb; b0 += 64) {
        const long long k = b0 + lane;
        const unsigned by = k < nb ? (unsigned)seq[k] : 0u;
        n_occ += (unsigned)__popcll(__ballot(k < nb && (by >> 4) == Bs)) + (unsigned)__popcll(__ballot(2 * k + 1 < lseq && (by & 15u) == Bs));
    }
    if (w_n > 0 && w_run - 1ull >= (unsigned long long)n_occ) { stat_add(in, lane, ST_OVERRUN, 1); return; }
    if (mlc < ml_off + (unsigned long long)w_codes * w_n) { stat_add(in, lane, ST_ML_SHORT, 1); return; }
    // ---- pass B: one class byte per occurrence (0: not listed), in the record's own l_seq bytes of the scratch (n_occ <= l_seq <= cap)
    uint8_t *cls = (uint8_t *)(uintptr_t)j.cls;
    for (unsigned k = (unsigned)lane; k < n_occ; k += 64) cls[k] = 0;
    __syncthreads();                                                     // (one wavefront: orders the stores above, the walk's stores and the loads below)
    (void)walk_deltas<true>(t, tlen, w_p, lane, mlp + ml_off, w_codes, w_ci, (unsigned)in.threshold, cls, n_occ);
    __syncthreads();
    // ---- the bases 64 at a time against a window of 64 CIGAR ops (both rise): per op its first base qb, one behind its last base qe and its first position rb
    unsigned w0 = 0; long long wq0 = 0, wr0 = pos + 1;
    long long qe = 0, qb = 0, rb = 0, win_qend = 0, win_rend = wr0; int al = 0;
    auto load_window = [&]() {                                           // bound: k < n_cigar
        const unsigned k = w0 + (unsigned)lane;
        const unsigned w = k < nc ? ld32u(cig + 4ull * k) : 0u;
        const unsigned op = w & 15u; const unsigned long long len = k < nc ? (unsigned long long)(w >> 4) : 0ull;
        const unsigned long long ql = (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) ? len : 0ull, rl = (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ? len : 0ull;
        qe = wq0 + (long long)scan_add64(ql, lane); qb = qe - (long long)ql;
        const long long re = wr0 + (long long)scan_add64(rl, lane); rb = re - (long long)rl;
        al = op == 0u || op == 7u || op == 8u;
        win_qend = __shfl(qe, 63); win_rend = __shfl(re, 63);
    };
    load_window();
    unsigned occ_before = 0; long long qdone = 0;
    unsigned long long n_un = 0, n_out = 0, n_off = 0, n_cnt = 0;
    for (long long i0 = 0; i0 < lseq; i0 += 64) {
        const long long i = i0 + lane; const bool valid = i < lseq;
        const unsigned nib = valid ? ((unsigned)seq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15u : 0u;       // bound: i < l_seq
        const bool isB = valid && nib == Bs;
        const unsigned long long bm = __ballot(isB);
        const unsigned o_fwd = occ_before + (unsigned)__popcll(bm & ((1ull << lane) - 1ull));
        const long long step_end = i0 + 64 < lseq ? i0 + 64 : lseq;
        for (;;) {                                                       // every round finishes the step or moves the window on; behind the last op every base is unaligned
            const bool beyond = w0 >= nc;
            const bool now = valid && i >= qdone && (beyond || i < win_qend);
            // the op of base i: the first lane whose qe is above i (all lanes search: the shuffles need every lane)
            int lo = 0, hi = 63;
#pragma unroll
            for (int s = 0; s < 6; ++s) { const int mid = (lo + hi) >> 1; const long long qm = __shfl(qe, mid); if (qm > i) hi = mid; else lo = mid + 1; }
            const long long rb_j = __shfl(rb, lo), qb_j = __shfl(qb, lo); const int al_j = __shfl(al, lo);
            int kind = 0;                                                // 1 unaligned, 2 outside, 3 off context, 4 counted
            if (now && isB) {
                const unsigned o = rev ? n_occ - 1u - o_fwd : o_fwd;     // bound: the same bases were counted into n_occ, so o_fwd < n_occ
                unsigned c = cls[o];
                if (c == 0u && w_flag != '?') c = 2u;
                if (c) {
                    const long long p = rb_j + (i - qb_j);
                    if (beyond || !al_j) kind = 1;
                    else if (p < in.reg_beg || p > in.reg_end) kind = 2;
                    else if (site_at(in, p) != (rev ? 2 : 1)) kind = 3;
                    else {
                        // bound: p is inside the region, whose positions site_idx covers; a site's index is below n_sites, and hap is 0, 1 or 2 (the host refuses others)
                        kind = 4;
                        atomicAdd(in.tab + (unsigned long long)in.site_idx[p - in.reg_beg] * 9ull + (unsigned)j.hap * 3u + (c - 1u), 1u);
                    }
                }
            }
            n_un += (unsigned long long)__popcll(__ballot(kind == 1)); n_out += (unsigned long long)__popcll(__ballot(kind == 2));
            n_off += (unsigned long long)__popcll(__ballot(kind == 3)); n_cnt += (unsigned long long)__popcll(__ballot(kind == 4));
            const long long upto = beyond || win_qend > step_end ? step_end : win_qend;
            if (upto > qdone) qdone = upto;
            if (qdone >= step_end) break;
            w0 += 64; wq0 = win_qend; wr0 = win_rend;
            load_window();
        }
        occ_before += (unsigned)__popcll(bm);
    }
    stat_add(in, lane, ST_UNALIGNED, n_un); stat_add(in, lane, ST_OUTSIDE, n_out); stat_add(in, lane, ST_OFF_CONTEXT, n_off); stat_add(in, lane, ST_COUNTED, n_cnt);
}

__global__ void __launch_bounds__(256) lcd_mods_compact_kernel(const ModsIn in, const long long n_pos, ModsRow *rows, int *n_rows) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_pos) return;
    const int s = site_at(in, in.reg_beg + k);
    if (!s) return;
    const unsigned *c = in.tab + (unsigned long long)in.site_idx[k] * 9ull;
    unsigned any = 0;
    for (int z = 0; z < 9; ++z) any |= c[z];
    if (!any) return;
    ModsRow &o = rows[atomicAdd(n_rows, 1)];                             // (at most one row per site: rows has n_sites entries)
    o.pos = in.reg_beg + k; o.strand = s; o.pad = 0;
    for (int z = 0; z < 9; ++z) o.count[z] = c[z];
}

void lcd_launch_mods_sites(const ModsIn &in, int *flag, long long n_pos, hipStream_t st) {
    if (n_pos > 0) hipLaunchKernelGGL(lcd_mods_sites_kernel, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, st, in, flag, n_pos);
}
void lcd_launch_mods_pileup(const ModsIn &in, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_mods_pileup_kernel, dim3(in.n_jobs), dim3(64), 0, st, in);
}
void lcd_launch_mods_compact(const ModsIn &in, long long n_pos, ModsRow *rows, int *n_rows, hipStream_t st) {
    if (n_pos > 0) hipLaunchKernelGGL(lcd_mods_compact_kernel, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, st, in, n_pos, rows, n_rows);
}
