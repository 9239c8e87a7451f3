// split_kernel.hip -- the records of a chunk's plan as per-haplotype FASTQ entries and haplotag list lines (lcd_chunk_split_reads; the rules are in
// include/lcd_hotpath.h), one wavefront per record in both kernels:
//   lcd_split_measure_kernel  one SplitRow per record: its stream, the exact byte lengths of its entry and its line, its flag bits;
//   lcd_split_emit_kernel     after the host's four 64-bit prefix sums: the entry at its offset of its haplotype's buffer, the line at its offset of the list.
// Both run the SAME walks (fastq<EMIT>, list_line<EMIT>), as bam_sam_kernel.hip does: the measure pass advances the offset where the emit pass writes.  Lanes
// stride the name, the packed bases and the qualities 64 stores per step: a byte head up to the destination's 4-byte boundary, aligned dword stores of four
// characters each, a byte tail.  A reverse record runs the same loop with the source index mirrored (q = l_seq - 1 - p): lane k's four characters come from the
// dword that ends where lane k - 1's begins, so a step's loads are as contiguous across the wavefront as its stores; an odd l_seq only flips which nibble of a
// byte q names, and the nibble is picked by q's own parity.  No LDS, no atomics, no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "sam_fmt.h"

namespace {
using lcd_wave::ld32u;

// the text being measured (EMIT false: only `at` moves) or written; every value but `lane` is the same on all lanes
template <bool EMIT> struct Txt {
    uint8_t *dst; unsigned long long at; int lane;
    __device__ __forceinline__ void ch(const unsigned c) { if (EMIT && lane == 0) dst[at] = (uint8_t)c; ++at; }
    // n <= 8 bytes, the first in the low byte
    __device__ __forceinline__ void small(const unsigned long long packed, const int n) { if (EMIT && lane < n) dst[at + lane] = (uint8_t)(packed >> (8 * lane)); at += (unsigned)n; }
    __device__ __forceinline__ void dec(const long long v) {
        const int n = sam_fmt::len_i(v);
        if (EMIT && lane < n) dst[at + lane] = (uint8_t)sam_fmt::char_i(v, n, lane);
        at += (unsigned)n;
    }
    __device__ __forceinline__ void bytes(const uint8_t *src, const long long n) {
        if (n <= 0) return;
        if (EMIT) lcd_wave::wave_copy(dst + at, src, n, lane);
        at += (unsigned long long)n;
    }
};

// "=ACMGRSVTWYHKDBN"[nib], or its complement "=TGKCYSBAWRDMHVN"[nib], without a table in memory
__device__ __forceinline__ unsigned base_of(const unsigned nib, const bool rev) {
    const unsigned long long lo = rev ? 0x425359434b47543dull /* "=TGKCYSB" */ : 0x565352474d43413dull /* "=ACMGRSV" */;
    const unsigned long long hi = rev ? 0x4e56484d44525741ull /* "AWRDMHVN" */ : 0x4e42444b48595754ull /* "TWYHKDBN" */;
    return (unsigned)((nib < 8u ? lo >> (8u * nib) : hi >> (8u * (nib - 8u))) & 0xffu);
}
__device__ __forceinline__ unsigned qual_of(const unsigned b) { return (b < 93u ? b : 93u) + 33u; }

// what both passes need of a record; the same on all lanes
struct Rec { const uint8_t *name, *seq, *qual; long long lseq; int qn, refid; unsigned flag; bool ok; };

__device__ __forceinline__ Rec parse(const SplitJob &j, const int lane) {
    Rec R;
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src;
    unsigned long long lim = 4ull + ld32u(src);                                  // (the host refuses a table entry shorter than 36)
    if (lim > j.len) lim = j.len;
    const uint8_t *r = src + 4;
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xffu, nc = w3 & 0xffffu;
    R.refid = (int)ld32u(r); R.flag = w3 >> 16; R.lseq = (long long)(int)ld32u(r + 16);
    R.name = src + 36; R.seq = R.name + lname + 4ull * nc;
    R.ok = R.lseq >= 0 && 36ull + lname + 4ull * nc + (unsigned long long)((R.lseq + 1) / 2) + (unsigned long long)R.lseq <= lim;
    R.qual = R.seq + (R.ok ? (R.lseq + 1) / 2 : 0);
    R.qn = 0;
    if (R.ok) {                                                                  // the bytes in front of the first NUL
        R.qn = (int)lname;
        for (int b = 0; b < (int)lname; b += 64) {
            const int k = b + lane;
            const unsigned long long bal = __ballot(k < (int)lname && R.name[k] == 0);
            if (bal) { R.qn = b + (int)__ffsll((long long)bal) - 1; break; }
        }
    }
    return R;
}

template <bool EMIT> __device__ __forceinline__ void put_name(Txt<EMIT> &T, const Rec &R) { if (R.qn == 0) T.ch('*'); else T.bytes(R.name, R.qn); }

// n bases from the packed nibbles, forward or mirrored and complemented: output position p shows source base q = rev ? n - 1 - p : p
template <bool EMIT> __device__ __forceinline__ void put_bases(Txt<EMIT> &T, const uint8_t *seq, const long long n, const bool rev) {
    if (EMIT) {
        uint8_t *d = T.dst + T.at; const int lane = T.lane;
        auto one = [&](const long long p) { const long long q = rev ? n - 1 - p : p; return base_of((seq[q >> 1] >> ((q & 1) ? 0 : 4)) & 15u, rev); };
        long long h = (long long)((4 - ((uintptr_t)d & 3)) & 3);
        if (h > n) h = n;
        if (lane < h) d[lane] = (uint8_t)one(lane);
        const long long nw = (n - h) >> 2;
        unsigned *d32 = (unsigned *)(d + h);
        for (long long k = lane; k < nw; k += 64) {
            const long long p = h + 4 * k, qa = rev ? n - 4 - p : p, b0 = qa >> 1;         // source bases [qa, qa + 3]: at most three bytes from b0 on
            const unsigned w = ld32u(seq + b0);
            unsigned out = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long q = rev ? qa + 3 - c : qa + c;
                const unsigned sh = 8u * (unsigned)((q >> 1) - b0) + ((q & 1) ? 0u : 4u);
                out |= base_of((w >> sh) & 15u, rev) << (8 * c);
            }
            d32[k] = out;
        }
        const long long t = (n - h) & 3, o = h + 4 * nw;
        if (lane < t) d[o + lane] = (uint8_t)one(o + lane);
    }
    T.at += (unsigned long long)n;
}
// n qualities as min(byte, 93) + 33, forward or mirrored; bang: every position prints '!'
template <bool EMIT> __device__ __forceinline__ void put_quals(Txt<EMIT> &T, const uint8_t *qual, const long long n, const bool rev, const bool bang) {
    if (EMIT) {
        uint8_t *d = T.dst + T.at; const int lane = T.lane;
        auto one = [&](const long long p) { return bang ? (unsigned)'!' : qual_of(qual[rev ? n - 1 - p : p]); };
        long long h = (long long)((4 - ((uintptr_t)d & 3)) & 3);
        if (h > n) h = n;
        if (lane < h) d[lane] = (uint8_t)one(lane);
        const long long nw = (n - h) >> 2;
        unsigned *d32 = (unsigned *)(d + h);
        for (long long k = lane; k < nw; k += 64) {
            const long long p = h + 4 * k;
            unsigned w = bang ? 0u : ld32u(qual + (rev ? n - 4 - p : p));
            if (rev) w = __builtin_bswap32(w);
            d32[k] = qual_of(w & 0xffu) | (qual_of((w >> 8) & 0xffu) << 8) | (qual_of((w >> 16) & 0xffu) << 16) | (qual_of(w >> 24) << 24);
        }
        const long long t = (n - h) & 3, o = h + 4 * nw;
        if (lane < t) d[o + lane] = (uint8_t)one(o + lane);
    }
    T.at += (unsigned long long)n;
}

// the FASTQ entry of a record with bases; returns its length
template <bool EMIT> __device__ __forceinline__ unsigned long long fastq(const Rec &R, const SplitJob &j, const int comment, uint8_t *dst, const int lane) {
    Txt<EMIT> T; T.dst = dst; T.at = 0; T.lane = lane;
    const bool rev = (R.flag & 0x10u) != 0;
    T.ch('@'); put_name(T, R);
    if (comment) {
        if (j.hap != 0) T.small(0x3a693a504809ull /* "\tHP:i:" */ | ((unsigned long long)('0' + j.hap) << 48), 7);
        if (j.ps > 0) { T.small(0x3a693a535009ull /* "\tPS:i:" */, 6); T.dec(j.ps); }
    }
    T.ch('\n');
    put_bases(T, R.seq, R.lseq, rev);
    T.small(0x0a2b0aull /* "\n+\n" */, 3);
    put_quals(T, R.qual, R.lseq, rev, R.qual[0] == 0xff);
    T.ch('\n');
    return T.at;
}
// the haplotag list's line of a record; returns its length
template <bool EMIT> __device__ __forceinline__ unsigned long long list_line(const Rec &R, const SplitJob &j, const SplitIn &in, uint8_t *dst, const int lane) {
    Txt<EMIT> T; T.dst = dst; T.at = 0; T.lane = lane;
    const unsigned long long none = 0x656e6f6eull;                               // "none"
    put_name(T, R);
    T.ch('\t');
    if (j.hap != 0) T.small(0x48ull | ((unsigned long long)('0' + j.hap) << 8), 2); else T.small(none, 4);
    T.ch('\t');
    if (j.ps > 0) T.dec(j.ps); else T.small(none, 4);
    T.ch('\t');
    unsigned b = 0, e = 0;
    if (R.refid >= 0 && R.refid < in.n_ref) { b = in.name_off[R.refid]; e = in.name_off[R.refid + 1]; }
    if (e <= b) T.ch('*'); else T.bytes(in.names + b, (long long)(e - b));
    T.ch('\n');
    return T.at;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_split_measure_kernel(const SplitIn in, SplitRow *rows) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const SplitJob j = in.jobs[i];
    const Rec R = parse(j, lane);
    SplitRow o; o.fq_len = o.list_len = o.fq_off = o.list_off = 0; o.stream = -1; o.flags = 0;
    if (R.flag & 0x900u) o.flags = LCD_SPLIT_NOT_PRIMARY;
    else if (!R.ok) o.flags = LCD_SPLIT_BAD_LAYOUT;
    else {
        o.stream = j.hap;
        if (R.flag & 0x10u) o.flags |= LCD_SPLIT_REVERSE;
        if (R.lseq == 0) o.flags |= LCD_SPLIT_NO_SEQ; else o.fq_len = fastq<false>(R, j, in.comment, nullptr, lane);
        if (in.list) o.list_len = list_line<false>(R, j, in, nullptr, lane);
    }
    if (lane == 0) rows[i] = o;
}
__global__ void __launch_bounds__(64) lcd_split_emit_kernel(const SplitIn in, const SplitRow *rows, uint8_t *fq0, uint8_t *fq1, uint8_t *fq2, uint8_t *list) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const SplitRow o = rows[i];
    if (o.stream < 0 || o.stream > 2) return;
    const SplitJob j = in.jobs[i];
    const Rec R = parse(j, lane);
    uint8_t *fq = o.stream == 0 ? fq0 : o.stream == 1 ? fq1 : fq2;
    if (o.fq_len) (void)fastq<true>(R, j, in.comment, fq + o.fq_off, lane);
    if (o.list_len) (void)list_line<true>(R, j, in, list + o.list_off, lane);
}

void lcd_launch_split_measure(const SplitIn &in, SplitRow *rows, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_split_measure_kernel, dim3(in.n_jobs), dim3(64), 0, st, in, rows);
}
void lcd_launch_split_emit(const SplitIn &in, const SplitRow *rows, uint8_t *fq0, uint8_t *fq1, uint8_t *fq2, uint8_t *list, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_split_emit_kernel, dim3(in.n_jobs), dim3(64), 0, st, in, rows, fq0, fq1, fq2, list);
}
