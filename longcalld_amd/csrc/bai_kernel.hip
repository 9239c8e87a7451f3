// The .bai of a BAM whose inflated records lie in HBM (SAM specification 5.2; the rules are written out in include/lcd_hotpath.h).  lcd_bam_walk_kernel has left
// one descriptor per record, lcd_bam_stat_kernel its reference length (the CG tag of a long CIGAR included); here, per batch of records:
//   lcd_bai_prep_kernel     one lane per record: the stat kernel's job from the descriptor, the smallest / largest contig of the batch and one presence byte per
//                           contig (the host allocates the window arrays of the contigs that have a record before the entry kernel runs);
//   lcd_bai_entry_kernel    one lane per record: interval, bin, the two virtual offsets (binary search of the stream's member table), the record's class, the
//                           order test against the record in front of it, the run-head flag, the 64-bit atomicMin of vbeg into every 16 kb window the record
//                           overlaps, the per-contig counters, and per workgroup the number of run heads;
//   lcd_bai_scan_kernel     exclusive prefix of the workgroups' head counts;
//   lcd_bai_compact_kernel  run heads -> the dense chunk list (refid, bin, vbeg, vend) in file order: ballot + prefix inside a wavefront, the wavefronts of a
//                           workgroup through LDS, the workgroups through the scan; a run's vend is written by the lane of its last record.
// Integer min / max / add atomics only: the result does not depend on the order in which lanes arrive.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"

#define BAI_BLOCK 256

namespace {
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
    const int lo = __shfl_xor((int)(unsigned)v, d, 64), hi = __shfl_xor((int)(v >> 32), d, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ uint32_t reg2bin(long long beg, long long end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
__device__ __forceinline__ bool has_coor(const BamRecDesc &d) { return d.refid >= 0 && d.pos >= 0; }
// bam_endpos under the project's rule: the unmapped flag, or a CIGAR without reference bases, spans one base
__device__ __forceinline__ long long rec_end(const BamRecDesc &d, const long long rl) { return (long long)d.pos + (((d.flag & 4) || rl <= 0) ? 1 : rl); }
// rule 5: stream offset p -> virtual offset.  The member whose payload holds byte p - 1 (the first one with uoff + ulen >= p: an empty member never is); a
// position at that payload's end is the following member's start (end_coff behind the last); the stream's first byte is its first member's start
__device__ __forceinline__ uint64_t voff(const BaiMember *m, const int n, const uint64_t end_coff, const uint64_t p) {
    if (n <= 0) return end_coff << 16;
    if (p <= m[0].uoff) return m[0].coff << 16;
    int lo = 0, hi = n;                          // first k with uoff + ulen >= p
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (m[mid].uoff + m[mid].ulen >= p) hi = mid; else lo = mid + 1; }
    if (lo >= n) return end_coff << 16;          // (behind the table: the caller's stream is longer than its members say)
    const uint64_t e = m[lo].uoff + m[lo].ulen;
    if (p < e) return (m[lo].coff << 16) | (p - m[lo].uoff);
    return (lo + 1 < n ? m[lo + 1].coff : end_coff) << 16;
}
} // namespace

__global__ void __launch_bounds__(BAI_BLOCK) lcd_bai_prep_kernel(const BaiJob j) {
    const int i = blockIdx.x * BAI_BLOCK + threadIdx.x;
    int mn = 0x7fffffff, mx = -1;
    if (i < j.n) {
        const BamRecDesc d = ((const BamRecDesc *)(uintptr_t)j.descs)[i];
        BamStatJob s; s.rec = j.stream + d.off; s.bs = d.bs; s.lname = d.lname; s.nc = d.nc; s.lseq = d.lseq;
        ((BamStatJob *)(uintptr_t)j.statjobs)[i] = s;
        if (has_coor(d)) {
            mn = d.refid; mx = d.refid;
            if (d.refid < j.n_ref) ((unsigned char *)(uintptr_t)j.minmax)[8 + d.refid] = 1;   // presence: which contigs of [mn, mx] have a record in this batch
        }
    }
    for (int k = 32; k >= 1; k >>= 1) { mn = min(mn, __shfl_xor(mn, k, 64)); mx = max(mx, __shfl_xor(mx, k, 64)); }
    if ((threadIdx.x & 63) == 0 && mx >= 0) { int *mm = (int *)(uintptr_t)j.minmax; atomicMin(mm, mn); atomicMax(mm + 1, mx); }
}

__global__ void __launch_bounds__(BAI_BLOCK) lcd_bai_entry_kernel(const BaiJob j) {
    __shared__ int wcnt[BAI_BLOCK / 64];
    const int i = blockIdx.x * BAI_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BamRecDesc *descs = (const BamRecDesc *)(uintptr_t)j.descs;
    const BamStatOut *stats = (const BamStatOut *)(uintptr_t)j.stats;
    const BaiMember *mem = (const BaiMember *)(uintptr_t)j.members;
    BaiEntry e; e.vbeg = 0; e.vend = 0; e.refid = -1; e.bin = 0; e.cls = 0; e.head = 0;
    bool ok = false;                             // an indexed record that passed every test
    long long beg = 0, end = 0;
    if (i < j.n) {
        const BamRecDesc d = descs[i];
        if (has_coor(d)) {
            beg = d.pos; end = rec_end(d, stats[i].rl);
            // the record in front: of this batch, or the carried one
            bool p_have = j.c_have != 0, p_coor = !j.c_nocoor; int p_refid = j.c_refid, p_pos = j.c_pos; uint32_t p_bin = 0; bool p_in_batch = false;
            if (i > 0) {
                const BamRecDesc q = descs[i - 1];
                p_have = true; p_coor = has_coor(q); p_refid = q.refid; p_pos = q.pos; p_in_batch = true;
                if (p_coor) p_bin = reg2bin(q.pos, rec_end(q, stats[i - 1].rl));
            }
            int code = 0;
            if ((p_have && !p_coor) || j.c_nocoor) code = 2;
            else if (p_have && (d.refid < p_refid || (d.refid == p_refid && d.pos < p_pos))) code = 1;
            else if (d.refid >= j.n_ref) code = 4;
            else if (end > (1ll << 29)) code = 3;
            else {
                const uint64_t wbase = ((const uint64_t *)(uintptr_t)j.win)[d.refid];
                const uint32_t nwin = ((const uint32_t *)(uintptr_t)j.n_win)[d.refid];
                if (!wbase || (uint64_t)((end - 1) >> 14) >= nwin) code = 5;   // (the window arrays are sized from the header: the test is made in 16 kb windows)
            }
            if (code) atomicMin((unsigned long long *)(uintptr_t)j.err, ((unsigned long long)(j.rec0 + i) << 4) | (unsigned)code);
            else {
                ok = true;
                e.refid = d.refid; e.bin = reg2bin(beg, end); e.cls = (d.flag & 4) ? 2u : 1u;
                e.vbeg = voff(mem, j.n_members, j.end_coff, d.off - 4);
                e.vend = voff(mem, j.n_members, j.end_coff, d.off + (uint64_t)d.bs);
                // (the first record of a batch is always a head: the host joins it to the run in front when (refid, bin) are the carried pair)
                e.head = (!p_in_batch || !p_coor || p_refid != d.refid || p_bin != e.bin) ? 1u : 0u;
            }
        }
        ((BaiEntry *)(uintptr_t)j.entries)[i] = e;
    }
    if (ok) { // rule 8: the smallest vbeg per 16 kb window (a 25 kb read spans two or three windows, a 1 Mb read 64)
        unsigned long long *w = (unsigned long long *)(uintptr_t)((const uint64_t *)(uintptr_t)j.win)[e.refid];
        for (long long k = beg >> 14; k <= (end - 1) >> 14; ++k) atomicMin(w + k, (unsigned long long)e.vbeg);
    }
    // per-contig counters: one set of atomics per wavefront when all its records are of one contig (the usual case), else per lane
    {
        const unsigned long long act = __ballot(ok);
        if (act) {
            const int first = __ffsll((long long)act) - 1;
            const int r0 = __shfl(e.refid, first, 64);
            const bool uniform = __ballot(ok && e.refid != r0) == 0;
            BaiCtg *ctg = (BaiCtg *)(uintptr_t)j.ctg;
            if (uniform) {
                unsigned long long nm = ok && e.cls == 1, nu = ok && e.cls == 2, vb = ok ? e.vbeg : ~0ull, ve = ok ? e.vend : 0ull;
                for (int k = 32; k >= 1; k >>= 1) {
                    nm += shfl_xor64(nm, k); nu += shfl_xor64(nu, k);
                    const unsigned long long b2 = shfl_xor64(vb, k), e2 = shfl_xor64(ve, k);
                    vb = b2 < vb ? b2 : vb; ve = e2 > ve ? e2 : ve;
                }
                if (lane == first) {
                    if (nm) atomicAdd(&ctg[r0].n_mapped, nm);
                    if (nu) atomicAdd(&ctg[r0].n_unmapped, nu);
                    atomicMin(&ctg[r0].first_vbeg, vb); atomicMax(&ctg[r0].last_vend, ve);
                }
            } else if (ok) {
                atomicAdd(e.cls == 1 ? &ctg[e.refid].n_mapped : &ctg[e.refid].n_unmapped, 1ull);
                atomicMin(&ctg[e.refid].first_vbeg, (unsigned long long)e.vbeg); atomicMax(&ctg[e.refid].last_vend, (unsigned long long)e.vend);
            }
        }
    }
    const unsigned long long heads = __ballot(e.head != 0);
    if (lane == 0) wcnt[wave] = __popcll(heads);
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < BAI_BLOCK / 64; ++k) s += wcnt[k]; ((int *)(uintptr_t)j.block_cnt)[blockIdx.x] = s; }
}

__global__ void __launch_bounds__(64) lcd_bai_scan_kernel(const int *cnt, int *off, const int nb) {
    // nb workgroups of 256 records (a batch is at most 2^18 records: 1 024 counts): 64 lanes, each a contiguous share, then the lanes' sums across the wavefront
    const int lane = threadIdx.x, per = (nb + 63) / 64, lo = min(nb, lane * per), hi = min(nb, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += cnt[k];
    int incl = s;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    int run = incl - s;
    for (int k = lo; k < hi; ++k) { off[k] = run; run += cnt[k]; }
    if (lane == 63) off[nb] = incl;
}

__global__ void __launch_bounds__(BAI_BLOCK) lcd_bai_compact_kernel(const BaiJob j) {
    __shared__ int wcnt[BAI_BLOCK / 64];
    const int i = blockIdx.x * BAI_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BaiEntry *entries = (const BaiEntry *)(uintptr_t)j.entries;
    BaiEntry e; e.vbeg = 0; e.vend = 0; e.refid = -1; e.bin = 0; e.cls = 0; e.head = 0;
    if (i < j.n) e = entries[i];
    const unsigned long long heads = __ballot(e.head != 0);
    if (lane == 0) wcnt[wave] = __popcll(heads);
    __syncthreads();
    if (i >= j.n || e.cls == 0) return;
    int base = ((const int *)(uintptr_t)j.block_off)[blockIdx.x];
    for (int k = 0; k < wave; ++k) base += wcnt[k];
    const int run = base + __popcll(heads & (~0ull >> (63 - lane))) - 1;   // heads up to and including this lane, over the whole batch, - 1
    if (run < 0) return;                         // (cannot happen: the first indexed record of a batch is a head)
    BaiChunk *c = (BaiChunk *)(uintptr_t)j.chunks + run;
    if (e.head) { c->refid = e.refid; c->bin = e.bin; c->vbeg = e.vbeg; }
    bool tail = i == j.n - 1;
    if (!tail) { const BaiEntry nx = entries[i + 1]; tail = nx.head != 0 || nx.cls == 0; }
    if (tail) c->vend = e.vend;
}

void lcd_launch_bai_prep(const BaiJob &j, hipStream_t st) { if (j.n > 0) hipLaunchKernelGGL(lcd_bai_prep_kernel, dim3((j.n + BAI_BLOCK - 1) / BAI_BLOCK), dim3(BAI_BLOCK), 0, st, j); }
void lcd_launch_bai_entry(const BaiJob &j, hipStream_t st) { if (j.n > 0) hipLaunchKernelGGL(lcd_bai_entry_kernel, dim3((j.n + BAI_BLOCK - 1) / BAI_BLOCK), dim3(BAI_BLOCK), 0, st, j); }
void lcd_launch_bai_compact(const BaiJob &j, hipStream_t st) {
    if (j.n <= 0) return;
    const int nb = (j.n + BAI_BLOCK - 1) / BAI_BLOCK;
    hipLaunchKernelGGL(lcd_bai_scan_kernel, dim3(1), dim3(64), 0, st, (const int *)(uintptr_t)j.block_cnt, (int *)(uintptr_t)j.block_off, nb);
    hipLaunchKernelGGL(lcd_bai_compact_kernel, dim3(nb), dim3(BAI_BLOCK), 0, st, j);
}
