// bam_sam_kernel.hip -- BAM records in HBM (a tagged / refined stream, or any back-to-back block_size-prefixed records) as SAM text lines (SAM specification 1.4),
// one wavefront per record in both kernels:
//   lcd_bam_sam_measure_kernel  the byte length of every record's line, with its flags and the number of float values;
//   lcd_bam_sam_emit_kernel     after the host's 64-bit prefix sum: the lines, each at its offset of the text stream.
// Both run the SAME walk (sam_line<EMIT>): the measure pass advances the offset where the emit pass writes, so the two cannot disagree.  Lanes stride the long
// parts 64 at a time -- CIGAR words, bases, qualities, the elements of a B array (PacBio kinetics arrays are as long as the read); items of variable width (a CIGAR
// word, an array element) get their place from a wave prefix scan carried from one round of 64 to the next; bases and qualities have a fixed width and go as aligned
// dword stores with a byte head and tail; the auxiliary fields are hopped one after the other, the same on all lanes, exactly as lcd_aux::value_size walks them (a
// field that runs past the record or has an unknown type ends the walk, nothing behind it is printed).  Numbers come from sam_fmt.h (floats: glibc's %g, exact).
// The rules where htslib's sam_format1 would decide are in include/lcd_hotpath.h (lcd_tagged_to_sam).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "wave_copy.h"
#include "bam_aux_hop.h"
#include "sam_fmt.h"

namespace {
using lcd_wave::ld32u;
using lcd_aux::aux2i;

__device__ __forceinline__ int scan_add(int v, const int lane) { // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __noinline__ sam_fmt::Txt16 fmt_g_dev(const uint32_t bits) { return sam_fmt::fmt_g(bits); }
// "=ACMGRSVTWYHKDBN"[nib] without a table in memory
__device__ __forceinline__ unsigned base_char(const uint8_t *seq, const long long q) {
    const unsigned nib = (seq[q >> 1] >> ((q & 1) ? 0 : 4)) & 15u;
    const unsigned long long lo = 0x565352474d43413dull /* "=ACMGRSV" */, hi = 0x4e42444b48595754ull /* "TWYHKDBN" */;
    return (unsigned)(((nib < 8u ? lo >> (8u * nib) : hi >> (8u * (nib - 8u)))) & 0xffu);
}

// the line being measured (EMIT false: only `at` moves) or written; every value but `lane` is the same on all lanes
template <bool EMIT> struct Line {
    uint8_t *dst; unsigned long long at; int lane;
    __device__ __forceinline__ void ch(const unsigned c) { if (EMIT && lane == 0) dst[at] = (uint8_t)c; ++at; }
    // n <= 8 bytes, the first in the low byte
    __device__ __forceinline__ void small(const unsigned long long packed, const int n) { if (EMIT && lane < n) dst[at + lane] = (uint8_t)(packed >> (8 * lane)); at += (unsigned)n; }
    __device__ __forceinline__ void dec(const long long v) {
        const int n = sam_fmt::len_i(v);
        if (EMIT && lane < n) dst[at + lane] = (uint8_t)sam_fmt::char_i(v, n, lane);
        at += (unsigned)n;
    }
    __device__ __forceinline__ void flt(const uint32_t bits) {
        const sam_fmt::Txt16 t = fmt_g_dev(bits);
        if (EMIT && lane < t.n) dst[at + lane] = (uint8_t)t.at(lane);
        at += (unsigned)t.n;
    }
    __device__ __forceinline__ void bytes(const uint8_t *src, const long long n) {
        if (n <= 0) return;
        if (EMIT) lcd_wave::wave_copy(dst + at, src, n, lane);
        at += (unsigned long long)n;
    }
    // n CIGAR words at p (any alignment) as <len><op>
    __device__ __forceinline__ void cigar(const uint8_t *p, const unsigned n) {
        for (unsigned base = 0; base < n; base += 64) {
            const unsigned k = base + (unsigned)lane; const bool valid = k < n;
            const unsigned w = valid ? ld32u(p + 4ull * k) : 0u;
            const int nd = sam_fmt::len_u(w >> 4), len = valid ? nd + 1 : 0;
            const int inc = scan_add(len, lane);
            if (EMIT && valid) {
                uint8_t *o = dst + at + (unsigned)(inc - len);
                unsigned x = w >> 4;
                for (int d = nd - 1; d >= 0; --d) { o[d] = (uint8_t)('0' + x % 10u); x /= 10u; }
                const unsigned op = w & 15u;
                const unsigned long long ops = 0x3d5048534e44494dull;            // "MIDNSHP="
                o[nd] = (uint8_t)(op < 8u ? (ops >> (8u * op)) & 0xffu : op == 8u ? 'X' : op == 9u ? 'B' : '?');
            }
            at += (unsigned)__shfl(inc, 63);
        }
    }
    // n bases from the packed nibbles: byte head, aligned dwords, byte tail
    __device__ __forceinline__ void bases(const uint8_t *seq, const long long n) {
        if (EMIT) {
            uint8_t *d = dst + at;
            long long h = (long long)((4 - ((uintptr_t)d & 3)) & 3);
            if (h > n) h = n;
            if (lane < h) d[lane] = (uint8_t)base_char(seq, lane);
            const long long nw = (n - h) >> 2;
            unsigned *d32 = (unsigned *)(d + h);
            for (long long k = lane; k < nw; k += 64) {
                const long long q = h + 4 * k;
                d32[k] = base_char(seq, q) | (base_char(seq, q + 1) << 8) | (base_char(seq, q + 2) << 16) | (base_char(seq, q + 3) << 24);
            }
            const long long t = (n - h) & 3, o = h + 4 * nw;
            if (lane < t) d[o + lane] = (uint8_t)base_char(seq, o + lane);
        }
        at += (unsigned long long)n;
    }
    // n qualities + 33 (each byte on its own, modulo 256)
    __device__ __forceinline__ void quals(const uint8_t *qual, const long long n) {
        if (EMIT) {
            uint8_t *d = dst + at;
            long long h = (long long)((4 - ((uintptr_t)d & 3)) & 3);
            if (h > n) h = n;
            if (lane < h) d[lane] = (uint8_t)(qual[lane] + 33u);
            const long long nw = (n - h) >> 2;
            unsigned *d32 = (unsigned *)(d + h);
            for (long long k = lane; k < nw; k += 64) {
                const unsigned w = ld32u(qual + h + 4 * k);
                d32[k] = ((w & 0x7f7f7f7fu) + 0x21212121u) ^ (w & 0x80808080u);
            }
            const long long t = (n - h) & 3, o = h + 4 * nw;
            if (lane < t) d[o + lane] = (uint8_t)(qual[o + lane] + 33u);
        }
        at += (unsigned long long)n;
    }
    // the elements of a B array as ,<value> each
    __device__ __forceinline__ void array(const uint8_t sub, const uint8_t *p, const unsigned cnt) {
        const unsigned es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : 4u;
        for (unsigned long long base = 0; base < cnt; base += 64) {
            const unsigned long long k = base + (unsigned)lane; const bool valid = k < cnt;
            long long v = 0; sam_fmt::Txt16 t; t.lo = t.hi = 0; t.n = 0;
            int len = 0;
            if (valid) {
                const uint8_t *e = p + k * es;
                const unsigned w = es == 1u ? (unsigned)e[0] : ld32u(e);
                if (sub == 'f') { t = fmt_g_dev(w); len = 1 + t.n; }
                else { v = aux2i(sub, w); len = 1 + sam_fmt::len_i(v); }
            }
            const int inc = scan_add(len, lane);
            if (EMIT && valid) {
                uint8_t *o = dst + at + (unsigned)(inc - len);
                o[0] = ',';
                if (sub == 'f') for (int c = 0; c < t.n; ++c) o[1 + c] = (uint8_t)t.at(c);
                else for (int c = 0; c < len - 1; ++c) o[1 + c] = (uint8_t)sam_fmt::char_i(v, len - 1, c);
            }
            at += (unsigned)__shfl(inc, 63);
        }
    }
};

template <bool EMIT> __device__ __forceinline__ void name_or_star(Line<EMIT> &L, const BamSamIn &in, const int refid) {
    if (refid < 0 || refid >= in.n_ref) { L.ch('*'); return; }
    const unsigned b = in.name_off[refid], e = in.name_off[refid + 1];
    if (e <= b) { L.ch('*'); return; }
    L.bytes(in.names + b, (long long)(e - b));
}

// the line of record i; returns its length.  flags / n_float as BamSamOut describes them
template <bool EMIT>
__device__ __forceinline__ unsigned long long sam_line(const BamSamIn &in, const int i, uint8_t *dst, const int lane, uint32_t &flags, uint32_t &n_float) {
    const unsigned long long r0 = in.rec_off[i], r1 = in.rec_off[i + 1];
    const uint8_t *src = in.base + r0, *end = in.base + r1;
    const unsigned long long len = r1 - r0;                                 // (at least 36: the host refuses anything shorter)
    const uint8_t *r = src + 4;
    const int refid = (int)ld32u(r), pos = (int)ld32u(r + 4);
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xffu, mapq = (w2 >> 8) & 0xffu, nc = w3 & 0xffffu, flag = w3 >> 16;
    const int lseq = (int)ld32u(r + 16), next_refid = (int)ld32u(r + 20), next_pos = (int)ld32u(r + 24), tlen = (int)ld32u(r + 28);
    const uint8_t *cig = src + 36 + lname, *seq = cig + 4ull * nc;
    const uint8_t *qual = seq + (unsigned long long)(((long long)lseq + 1) / 2), *aux0 = qual + (unsigned long long)(long long)lseq;
    const bool layout_ok = lseq >= 0 && aux0 <= end, name_ok = 36ull + lname <= len;
    flags = layout_ok ? 0u : 4u; n_float = 0;

    // a CIGAR that lives in a CG field: <l_seq>S <n>N and a first CG field of type B, subtype I
    const uint8_t *cg_fld = nullptr, *cg_words = nullptr; unsigned cg_n = 0;
    if (layout_ok && nc == 2u && ld32u(cig) == (((uint32_t)lseq << 4) | 4u) && (ld32u(cig + 4) & 15u) == 3u) {
        const uint8_t *aux = aux0;
        while (aux + 3 <= end) {
            const unsigned h = ld32u(aux);
            const uint8_t ty = (uint8_t)((h >> 16) & 0xff);
            const uint8_t *val = aux + 3;
            size_t sz = 0;
            if (!lcd_aux::value_size(ty, val, end, &sz)) break;
            if ((h & 0xffffu) == (unsigned)('C' | ('G' << 8))) {
                if (ty == 'B' && val[0] == 'I') { cg_fld = aux; cg_words = val + 5; cg_n = ld32u(val + 1); flags |= 1u; }
                break;
            }
            aux = val + sz;
        }
    }

    Line<EMIT> L; L.dst = dst; L.at = 0; L.lane = lane;
    // QNAME
    int qn = (int)lname;
    if (name_ok)
        for (int b = 0; b < (int)lname; b += 64) {
            const int k = b + lane;
            const unsigned long long bal = __ballot(k < (int)lname && src[36 + k] == 0);
            if (bal) { qn = b + (int)__ffsll((long long)bal) - 1; break; }
        }
    if (!name_ok || qn == 0) L.ch('*'); else L.bytes(src + 36, qn);
    L.ch('\t'); L.dec((long long)flag);
    L.ch('\t'); name_or_star(L, in, refid);
    L.ch('\t'); L.dec((long long)pos + 1);
    L.ch('\t'); L.dec((long long)mapq);
    L.ch('\t');
    if (!layout_ok || nc == 0u) L.ch('*'); else if (cg_fld) { if (cg_n) L.cigar(cg_words, cg_n); else L.ch('*'); } else L.cigar(cig, nc);
    L.ch('\t');
    if (next_refid < 0 || next_refid >= in.n_ref) L.ch('*'); else if (next_refid == refid) L.ch('='); else name_or_star(L, in, next_refid);
    L.ch('\t'); L.dec((long long)next_pos + 1);
    L.ch('\t'); L.dec((long long)tlen);
    L.ch('\t');
    if (!layout_ok || lseq == 0) L.ch('*'); else L.bases(seq, lseq);
    L.ch('\t');
    if (!layout_ok || lseq == 0 || qual[0] == 0xff) L.ch('*'); else L.quals(qual, lseq);
    // the auxiliary fields
    if (layout_ok) {
        const uint8_t *aux = aux0;
        while (aux + 3 <= end) {
            const unsigned h = ld32u(aux);
            const uint8_t ty = (uint8_t)((h >> 16) & 0xff);
            const uint8_t *val = aux + 3;
            size_t sz = 0;
            if (!lcd_aux::value_size(ty, val, end, &sz)) break;
            if (aux != cg_fld) {
                const bool is_int = ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I';
                // \tXX:T:
                L.small(0x09ull | ((unsigned long long)(h & 0xffffu) << 8) | ((unsigned long long)':' << 24) | ((unsigned long long)(is_int ? 'i' : ty) << 32) |
                        ((unsigned long long)':' << 40), 6);
                if (ty == 'A') L.ch(val[0]);
                else if (is_int) L.dec(aux2i(ty, ty == 'c' || ty == 'C' ? (unsigned)val[0] : ld32u(val)));
                else if (ty == 'f') { L.flt(ld32u(val)); ++n_float; }
                else if (ty == 'Z' || ty == 'H') L.bytes(val, (long long)sz - 1);
                else {                                                        // B
                    const unsigned cnt = ld32u(val + 1);
                    L.ch(val[0]);
                    L.array(val[0], val + 5, cnt);
                    if (val[0] == 'f') n_float += cnt;
                }
            }
            aux = val + sz;
        }
        if (aux != end) flags |= 2u;
    }
    L.ch('\n');
    return L.at;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_bam_sam_measure_kernel(const BamSamIn in, BamSamOut *outs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_rec) return;
    BamSamOut o;
    o.len = sam_line<false>(in, i, nullptr, lane, o.flags, o.n_float);
    if (lane == 0) outs[i] = o;
}
__global__ void __launch_bounds__(64) lcd_bam_sam_emit_kernel(const BamSamIn in, const unsigned long long *text_off, uint8_t *text) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_rec) return;
    uint32_t flags, n_float;
    (void)sam_line<true>(in, i, text + text_off[i], lane, flags, n_float);
}

void lcd_launch_bam_sam_measure(const BamSamIn &in, BamSamOut *outs, hipStream_t st) {
    if (in.n_rec > 0) hipLaunchKernelGGL(lcd_bam_sam_measure_kernel, dim3(in.n_rec), dim3(64), 0, st, in, outs);
}
void lcd_launch_bam_sam_emit(const BamSamIn &in, const unsigned long long *text_off, uint8_t *text, hipStream_t st) {
    if (in.n_rec > 0) hipLaunchKernelGGL(lcd_bam_sam_emit_kernel, dim3(in.n_rec), dim3(64), 0, st, in, text_off, text);
}
