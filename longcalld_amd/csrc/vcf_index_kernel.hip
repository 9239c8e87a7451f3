// The .tbi / .csi of VCF text that lies in HBM (the rules are written out in include/lcd_hotpath.h, "VCF indexes").  Per stream:
//   lcd_vidx_nl_count_kernel / _nl_compact_kernel   the line table: lanes over bytes, a ballot per 64 bytes, per-workgroup counts of '\n', the scan, the line starts;
//   lcd_vidx_flag_kernel / _rank_kernel             one lane per line: is it a data line (first byte not '#'); the data lines' dense numbering;
//   lcd_vidx_parse_kernel                           ONE WAVEFRONT PER LINE, lanes striding 64 bytes with ballots: the tabs that end columns 1-8, CHROM against the
//                                                   CHROM of the data line before it (the contig-run head flag), POS, the length of REF, END by htslib's rule; of a
//                                                   meta line the length= of a ##contig line;
//   lcd_vidx_head_count_kernel / _head_kernel       one lane per data line: the contig run it belongs to, the run heads' CHROM places (only those names go to
//                                                   the host), per run the largest end (the host sizes the contig's window array from it);
//   lcd_vidx_names_kernel                           the heads' names gathered into one block;
//   lcd_vidx_entry_kernel / _compact_kernel         what lcd_bai_entry_kernel / lcd_bai_compact_kernel do for a record: bin key, the two virtual offsets, the order
//                                                   test, the run-head flag for equal (contig run, bin), the 64-bit atomicMin of vbeg into every 16 kb window, the
//                                                   per-run counters, the dense chunk list.
// The device helpers (stream offset -> virtual offset, the compaction scheme) are copies of bai_kernel.hip's: that file stays as it is.
// Integer min / max / add atomics only: the result does not depend on the order in which lanes arrive.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"

#define VIDX_BLOCK 256
#define VIDX_WAVE_BYTES 1024                    // bytes of the stream per wavefront of the line-table kernels (16 ballots)
#define VIDX_BLOCK_BYTES (VIDX_WAVE_BYTES * (VIDX_BLOCK / 64))
#define VIDX_MAX_LEVEL 8

namespace {
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
    const int lo = __shfl_xor((int)(unsigned)v, d, 64), hi = __shfl_xor((int)(v >> 32), d, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
// rule 5 (bai_kernel.hip's voff)
__device__ __forceinline__ uint64_t voff(const BaiMember *m, const int n, const uint64_t end_coff, const uint64_t p) {
    if (n <= 0) return end_coff << 16;
    if (p <= m[0].uoff) return m[0].coff << 16;
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (m[mid].uoff + m[mid].ulen >= p) hi = mid; else lo = mid + 1; }
    if (lo >= n) return end_coff << 16;
    const uint64_t e = m[lo].uoff + m[lo].ulen;
    if (p < e) return (m[lo].coff << 16) | (p - m[lo].uoff);
    return (lo + 1 < n ? m[lo + 1].coff : end_coff) << 16;
}
// the bin as (level << 28) | index, level 0 = the 16 kb leaves (lcd_bai::vidx_key)
__device__ __forceinline__ uint32_t bin_key(const long long beg, long long end) {
    --end;
    int l = 0;
    while (l < VIDX_MAX_LEVEL && (beg >> (14 + 3 * l)) != (end >> (14 + 3 * l))) ++l;
    return ((uint32_t)l << 28) | (uint32_t)(beg >> (14 + 3 * l));
}
__device__ __forceinline__ bool lit(const uint8_t *p, const char *s, const int n) { for (int k = 0; k < n; ++k) if (p[k] != (uint8_t)s[k]) return false; return true; }
// decimal digits of [p, e): the value (saturated at 2^62 behind 18 digits), returns the number of digits
__device__ __forceinline__ int dec(const uint8_t *s, const uint64_t p, const uint64_t e, long long *v) {
    long long x = 0; int n = 0;
    while (p + n < e && s[p + n] >= '0' && s[p + n] <= '9') { if (n < 18) x = x * 10 + (s[p + n] - '0'); else x = 1ll << 62; ++n; }
    *v = x;
    return n;
}
// the '\n' of this wavefront's share of the stream: calls f(ballot, first byte of the 64) for each of its 16 steps
template <class F> __device__ __forceinline__ void nl_steps(const VIdxJob &j, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *s = (const uint8_t *)(uintptr_t)j.stream;
    const uint64_t w0 = j.first + (uint64_t)blockIdx.x * VIDX_BLOCK_BYTES + (uint64_t)wave * VIDX_WAVE_BYTES;
    for (int k = 0; k < VIDX_WAVE_BYTES / 64; ++k) {
        const uint64_t p0 = w0 + (uint64_t)k * 64, p = p0 + lane;
        if (p0 >= j.n_bytes) break;                                       // (uniform over the wavefront)
        f(__ballot(p < j.n_bytes && s[p] == '\n'), p0);
    }
}
} // namespace

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_nl_count_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    int c = 0;
    nl_steps(j, [&](const unsigned long long m, const uint64_t) { c += __popcll(m); });
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < VIDX_BLOCK / 64; ++k) s += wcnt[k]; ((int *)(uintptr_t)j.block_cnt)[blockIdx.x] = s; }
}

// exclusive prefix of nb counts, the total at off[nb] (bai_kernel.hip's scan: 64 lanes, each a contiguous share)
__global__ void __launch_bounds__(64) lcd_vidx_scan_kernel(const int *cnt, int *off, const int nb) {
    const int lane = threadIdx.x, per = (nb + 63) / 64, lo = min(nb, lane * per), hi = min(nb, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += cnt[k];
    int incl = s;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    int run = incl - s;
    for (int k = lo; k < hi; ++k) { off[k] = run; run += cnt[k]; }
    if (lane == 63) off[nb] = incl;
}

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_nl_compact_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c = 0;
    nl_steps(j, [&](const unsigned long long m, const uint64_t) { c += __popcll(m); });
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int base = ((const int *)(uintptr_t)j.block_off)[blockIdx.x];
    for (int k = 0; k < wave; ++k) base += wcnt[k];
    uint64_t *ls = (uint64_t *)(uintptr_t)j.lstart;
    if (blockIdx.x == 0 && threadIdx.x == 0) ls[0] = j.first;
    nl_steps(j, [&](const unsigned long long m, const uint64_t p0) {
        if ((m >> lane) & 1) ls[base + __popcll(m & ((1ull << lane) - 1)) + 1] = p0 + lane + 1;     // the line behind this '\n' starts here
        base += __popcll(m);
    });
}

// one lane per line: a data line does not begin with '#'
__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_flag_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int k = blockIdx.x * VIDX_BLOCK + threadIdx.x;
    bool data = false;
    if (k < j.n_lines) { const uint64_t a = ((const uint64_t *)(uintptr_t)j.lstart)[k]; data = a >= j.n_bytes || ((const uint8_t *)(uintptr_t)j.stream)[a] != '#'; }
    const unsigned long long m = __ballot(data);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int q = 0; q < VIDX_BLOCK / 64; ++q) s += wcnt[q]; ((int *)(uintptr_t)j.block_cnt)[blockIdx.x] = s; }
}
__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_rank_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int k = blockIdx.x * VIDX_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool data = false;
    if (k < j.n_lines) { const uint64_t a = ((const uint64_t *)(uintptr_t)j.lstart)[k]; data = a >= j.n_bytes || ((const uint8_t *)(uintptr_t)j.stream)[a] != '#'; }
    const unsigned long long m = __ballot(data);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (k >= j.n_lines) return;
    int base = ((const int *)(uintptr_t)j.block_off)[blockIdx.x];
    for (int q = 0; q < wave; ++q) base += wcnt[q];
    const int r = base + __popcll(m & ((1ull << lane) - 1));
    ((int *)(uintptr_t)j.rank)[k] = data ? r : -1;
    if (data) ((int *)(uintptr_t)j.dline)[r] = k;
}

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_parse_kernel(const VIdxJob j) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * (VIDX_BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= j.n_lines) return;                                            // (the whole wavefront)
    const uint8_t *s = (const uint8_t *)(uintptr_t)j.stream;
    const uint64_t *ls = (const uint64_t *)(uintptr_t)j.lstart;
    const uint64_t a = ls[k], e = ls[k + 1] - 1;                           // the line without its '\n'
    const int r = ((const int *)(uintptr_t)j.rank)[k];
    if (r < 0) {                                                           // a meta line: the length= of a ##contig line
        if (e - a < 10 || !lit(s + a, "##contig=<", 10)) return;
        for (uint64_t p0 = a + 9; p0 + 8 <= e; p0 += 64) {
            const uint64_t p = p0 + lane;
            const unsigned long long m = __ballot(p + 8 <= e && (s[p] == '<' || s[p] == ',') && lit(s + p + 1, "length=", 7));
            if (!m) continue;
            long long v = 0;
            if (dec(s, p0 + (uint64_t)(__ffsll((long long)m) - 1) + 8, e, &v) > 0 && lane == 0) atomicMax((unsigned long long *)(uintptr_t)j.max_clen, (unsigned long long)v);
            break;
        }
        return;
    }
    // the tabs that end columns 1 ... 8
    uint64_t tab[8]; int nt = 0;
    for (uint64_t p0 = a; p0 < e && nt < 8; p0 += 64) {
        const uint64_t p = p0 + lane;
        unsigned long long m = __ballot(p < e && s[p] == '\t');
        while (m && nt < 8) { tab[nt++] = p0 + (uint64_t)(__ffsll((long long)m) - 1); m &= m - 1; }
    }
    VIdxLine L; L.beg = 0; L.end = 0; L.a = a; L.next = ls[k + 1] < j.n_bytes ? ls[k + 1] : j.n_bytes; L.name_len = 0; L.flags = 0; L.run = 0; L.pad = 0;
    int code = 0;
    long long pos = 0;
    if (nt < 7 || tab[0] == a) code = 2;
    else { const int nd = dec(s, tab[0] + 1, tab[1], &pos); if (nd == 0 || tab[0] + 1 + (uint64_t)nd != tab[1]) code = 2; }
    if (!code) {
        L.name_len = (uint32_t)(tab[0] - a);
        L.beg = pos > 0 ? pos - 1 : 0;
        const long long reflen = (long long)(tab[3] - tab[2] - 1);
        L.end = L.beg + (reflen > 0 ? reflen : 1);
        // END: "END=" at the very start of INFO, or else the first ";END=" inside it
        const uint64_t i0 = tab[6] + 1, i1 = nt >= 8 ? tab[7] : e;
        uint64_t vp = 0; bool have = false;
        if (i1 - i0 >= 4 && lit(s + i0, "END=", 4)) { vp = i0 + 4; have = true; }
        else for (uint64_t p0 = i0; p0 + 5 <= i1; p0 += 64) {
            const uint64_t p = p0 + lane;
            const unsigned long long m = __ballot(p + 5 <= i1 && lit(s + p, ";END=", 5));
            if (m) { vp = p0 + (uint64_t)(__ffsll((long long)m) - 1) + 5; have = true; break; }
        }
        if (have) { long long v = 0; if (dec(s, vp, i1, &v) > 0 && v > L.beg) L.end = v; }
        if (L.end > j.cap) code = 3;
        // the contig-run head flag: CHROM against the CHROM of the data line before this one (of the stream, or the carried one)
        const uint8_t *q = nullptr;
        if (r > 0) { q = s + ls[((const int *)(uintptr_t)j.dline)[r - 1]]; }
        else if (j.c_have && (uint32_t)j.c_name_len == L.name_len) q = (const uint8_t *)(uintptr_t)j.carry_name;
        bool diff = q == nullptr;
        if (q) {
            for (uint32_t x = lane; x < L.name_len; x += 64) diff |= q[x] != s[a + x];
            if (r > 0 && lane == 0) diff |= q[L.name_len] != '\t';
            diff = __ballot(diff) != 0;
        }
        L.flags = diff ? 1u : 0u;
    }
    L.flags |= (uint32_t)code << 4;
    if (lane == 0) {
        ((VIdxLine *)(uintptr_t)j.lines)[r] = L;
        if (code) atomicMin((unsigned long long *)(uintptr_t)j.err, ((unsigned long long)(j.line0 + r) << 4) | (unsigned)code);
    }
}

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_head_count_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int r = blockIdx.x * VIDX_BLOCK + threadIdx.x;
    const bool head = r < j.n_data && (((const VIdxLine *)(uintptr_t)j.lines)[r].flags & 1);
    const unsigned long long m = __ballot(head);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int q = 0; q < VIDX_BLOCK / 64; ++q) s += wcnt[q]; ((int *)(uintptr_t)j.block_cnt)[blockIdx.x] = s; }
}
__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_head_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int r = blockIdx.x * VIDX_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    VIdxLine *lines = (VIdxLine *)(uintptr_t)j.lines;
    VIdxLine L; L.flags = 0; L.end = 0; L.a = 0; L.name_len = 0;
    if (r < j.n_data) L = lines[r];
    const bool head = r < j.n_data && (L.flags & 1);
    const unsigned long long m = __ballot(head);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int base = ((const int *)(uintptr_t)j.block_off)[blockIdx.x];
    for (int q = 0; q < wave; ++q) base += wcnt[q];
    const int run = base + __popcll(m & (~0ull >> (63 - lane)));          // heads up to and including this line: run 0 is the carried contig's
    const bool ok = r < j.n_data && (L.flags >> 4) == 0;
    if (r < j.n_data) {
        lines[r].run = run;
        if (head) { VIdxHead h; h.a = L.a; h.name_len = L.name_len; h.line = r; ((VIdxHead *)(uintptr_t)j.heads)[run - 1] = h; }
    }
    // per run the largest end: one atomic per wavefront when its lines are of one run
    const unsigned long long act = __ballot(ok);
    if (!act) return;
    const int first = __ffsll((long long)act) - 1, r0 = __shfl(run, first, 64);
    VIdxRun *runs = (VIdxRun *)(uintptr_t)j.runs;
    if (__ballot(ok && run != r0) == 0) {
        unsigned long long mx = ok ? (unsigned long long)L.end : 0ull;
        for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = shfl_xor64(mx, d); mx = o > mx ? o : mx; }
        if (lane == first) atomicMax(&runs[r0].max_end, mx);
    } else if (ok) atomicMax(&runs[run].max_end, (unsigned long long)L.end);
}

// one workgroup per head: its CHROM to names + name_offs[head]
__global__ void __launch_bounds__(64) lcd_vidx_names_kernel(const VIdxJob j) {
    const VIdxHead h = ((const VIdxHead *)(uintptr_t)j.heads)[blockIdx.x];
    const uint8_t *s = (const uint8_t *)(uintptr_t)j.stream + h.a;
    uint8_t *d = (uint8_t *)(uintptr_t)j.names + ((const uint64_t *)(uintptr_t)j.name_offs)[blockIdx.x];
    for (uint32_t x = threadIdx.x; x < h.name_len; x += 64) d[x] = s[x];
}

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_entry_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int r = blockIdx.x * VIDX_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const VIdxLine *lines = (const VIdxLine *)(uintptr_t)j.lines;
    const BaiMember *mem = (const BaiMember *)(uintptr_t)j.members;
    BaiEntry e; e.vbeg = 0; e.vend = 0; e.refid = -1; e.bin = 0; e.cls = 0; e.head = 0;
    bool ok = false;
    long long beg = 0, end = 0;
    if (r < j.n_data) {
        const VIdxLine L = lines[r];
        if ((L.flags >> 4) == 0) {
            beg = L.beg; end = L.end;
            // the data line in front: of this stream, or the carried one
            bool p_ok = false, p_in = false; long long p_beg = 0; uint32_t p_key = 0;
            if (r > 0) { const VIdxLine P = lines[r - 1]; p_in = true; p_ok = (P.flags >> 4) == 0; p_beg = P.beg; if (p_ok) p_key = bin_key(P.beg, P.end); }
            else if (j.c_have) { p_ok = true; p_beg = j.c_beg; }
            const bool same = !(L.flags & 1);
            int code = 0;
            if (same && p_ok && beg < p_beg) code = 1;
            else {
                const uint64_t wbase = ((const uint64_t *)(uintptr_t)j.run_win)[L.run];
                const uint32_t nwin = ((const uint32_t *)(uintptr_t)j.run_nwin)[L.run];
                if (!wbase || (uint64_t)((end - 1) >> 14) >= nwin) code = 5;
            }
            if (code) atomicMin((unsigned long long *)(uintptr_t)j.err, ((unsigned long long)(j.line0 + r) << 4) | (unsigned)code);
            else {
                ok = true;
                e.refid = L.run; e.bin = bin_key(beg, end); e.cls = 1;
                e.vbeg = voff(mem, j.n_members, j.end_coff, L.a);
                e.vend = voff(mem, j.n_members, j.end_coff, L.next);
                // (the first data line of a stream is always a head: the host joins it to the run in front when (contig, bin) are the carried pair)
                e.head = (!p_in || !p_ok || !same || p_key != e.bin) ? 1u : 0u;
            }
        }
        ((BaiEntry *)(uintptr_t)j.entries)[r] = e;
    }
    if (ok) {
        unsigned long long *w = (unsigned long long *)(uintptr_t)((const uint64_t *)(uintptr_t)j.run_win)[e.refid];
        for (long long k = beg >> 14; k <= (end - 1) >> 14; ++k) atomicMin(w + k, (unsigned long long)e.vbeg);
    }
    {
        const unsigned long long act = __ballot(ok);
        if (act) {
            const int first = __ffsll((long long)act) - 1, r0 = __shfl(e.refid, first, 64);
            VIdxRun *runs = (VIdxRun *)(uintptr_t)j.runs;
            if (__ballot(ok && e.refid != r0) == 0) {
                unsigned long long n = ok ? 1 : 0, vb = ok ? e.vbeg : ~0ull, ve = ok ? e.vend : 0ull;
                for (int d = 32; d >= 1; d >>= 1) {
                    n += shfl_xor64(n, d);
                    const unsigned long long b2 = shfl_xor64(vb, d), e2 = shfl_xor64(ve, d);
                    vb = b2 < vb ? b2 : vb; ve = e2 > ve ? e2 : ve;
                }
                if (lane == first) { atomicAdd(&runs[r0].n_lines, n); atomicMin(&runs[r0].first_vbeg, vb); atomicMax(&runs[r0].last_vend, ve); }
            } else if (ok) {
                atomicAdd(&runs[e.refid].n_lines, 1ull); atomicMin(&runs[e.refid].first_vbeg, (unsigned long long)e.vbeg); atomicMax(&runs[e.refid].last_vend, (unsigned long long)e.vend);
            }
        }
    }
    const unsigned long long heads = __ballot(e.head != 0);
    if (lane == 0) wcnt[wave] = __popcll(heads);
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < VIDX_BLOCK / 64; ++k) s += wcnt[k]; ((int *)(uintptr_t)j.block_cnt)[blockIdx.x] = s; }
}

__global__ void __launch_bounds__(VIDX_BLOCK) lcd_vidx_compact_kernel(const VIdxJob j) {
    __shared__ int wcnt[VIDX_BLOCK / 64];
    const int i = blockIdx.x * VIDX_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BaiEntry *entries = (const BaiEntry *)(uintptr_t)j.entries;
    BaiEntry e; e.vbeg = 0; e.vend = 0; e.refid = -1; e.bin = 0; e.cls = 0; e.head = 0;
    if (i < j.n_data) e = entries[i];
    const unsigned long long heads = __ballot(e.head != 0);
    if (lane == 0) wcnt[wave] = __popcll(heads);
    __syncthreads();
    if (i >= j.n_data || e.cls == 0) return;
    int base = ((const int *)(uintptr_t)j.block_off)[blockIdx.x];
    for (int k = 0; k < wave; ++k) base += wcnt[k];
    const int run = base + __popcll(heads & (~0ull >> (63 - lane))) - 1;
    if (run < 0) return;
    BaiChunk *c = (BaiChunk *)(uintptr_t)j.chunks + run;
    if (e.head) { c->refid = e.refid; c->bin = e.bin; c->vbeg = e.vbeg; }
    bool tail = i == j.n_data - 1;
    if (!tail) { const BaiEntry nx = entries[i + 1]; tail = nx.head != 0 || nx.cls == 0; }
    if (tail) c->vend = e.vend;
}

static inline int nblk(const long long n, const int per) { return (int)((n + per - 1) / per); }
void lcd_launch_vidx_scan(const VIdxJob &j, int nb, hipStream_t st) { hipLaunchKernelGGL(lcd_vidx_scan_kernel, dim3(1), dim3(64), 0, st, (const int *)(uintptr_t)j.block_cnt, (int *)(uintptr_t)j.block_off, nb); }
void lcd_launch_vidx_nl_count(const VIdxJob &j, hipStream_t st) { if (j.n_blocks > 0) hipLaunchKernelGGL(lcd_vidx_nl_count_kernel, dim3(j.n_blocks), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_nl_compact(const VIdxJob &j, hipStream_t st) { if (j.n_blocks > 0) hipLaunchKernelGGL(lcd_vidx_nl_compact_kernel, dim3(j.n_blocks), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_flag(const VIdxJob &j, hipStream_t st) { if (j.n_lines > 0) hipLaunchKernelGGL(lcd_vidx_flag_kernel, dim3(nblk(j.n_lines, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_rank(const VIdxJob &j, hipStream_t st) { if (j.n_lines > 0) hipLaunchKernelGGL(lcd_vidx_rank_kernel, dim3(nblk(j.n_lines, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_parse(const VIdxJob &j, hipStream_t st) { if (j.n_lines > 0) hipLaunchKernelGGL(lcd_vidx_parse_kernel, dim3(nblk(j.n_lines, VIDX_BLOCK / 64)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_head_count(const VIdxJob &j, hipStream_t st) { if (j.n_data > 0) hipLaunchKernelGGL(lcd_vidx_head_count_kernel, dim3(nblk(j.n_data, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_head(const VIdxJob &j, hipStream_t st) { if (j.n_data > 0) hipLaunchKernelGGL(lcd_vidx_head_kernel, dim3(nblk(j.n_data, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_names(const VIdxJob &j, hipStream_t st) { if (j.n_heads > 0) hipLaunchKernelGGL(lcd_vidx_names_kernel, dim3(j.n_heads), dim3(64), 0, st, j); }
void lcd_launch_vidx_entry(const VIdxJob &j, hipStream_t st) { if (j.n_data > 0) hipLaunchKernelGGL(lcd_vidx_entry_kernel, dim3(nblk(j.n_data, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
void lcd_launch_vidx_compact(const VIdxJob &j, hipStream_t st) { if (j.n_data > 0) hipLaunchKernelGGL(lcd_vidx_compact_kernel, dim3(nblk(j.n_data, VIDX_BLOCK)), dim3(VIDX_BLOCK), 0, st, j); }
