// merge_vars_kernel.hip -- the read x variant profile after merge_var_profile (src/collect_var.c:1298-1387) for every region of a pass at once.
// The variant-table walk is sequential and tiny and stays on the host (lcd_chunk_vars.cpp, lcd_merge_region_vars); it yields, per chunk, the composed index maps
// old variant -> merged variant and region variant -> merged variant (-1: dropped as equal to a kept one).  What scales with reads x variants runs here, for
// all chunks of a call in one set of launches (sources carry absolute addresses and an index into the call's read table):
//   span     one lane per source (a read's current profile, or one region row): min / max of the merged indices its cells move to, integer atomics on the
//            read's new start / end
//   scan     end - start + 1 per read -> 64-bit CSR offsets over the whole read table: per-workgroup scan + workgroup totals, one workgroup scans the totals,
//            the third launch adds them (no workgroup waits for another one)
//   fill     every cell -1
//   scatter  one lane per source cell; no atomics: a read is in at most one row per region and merged indices are distinct, so a destination cell has at
//            most one source
// Every lane checks its destination against the cell capacity the host allocated; a miss sets *flag instead of writing.
#include <hip/hip_runtime.h>
#include "lcd_types.h"
#include "lcd_kernels.h"

namespace {
constexpr int MV_T = 256;
inline int mv_blocks(unsigned long long n) { return (int)((n + MV_T - 1) / MV_T); }

__global__ void __launch_bounds__(MV_T) mv_span_kernel(const MvSrc *srcs, int n_src, int *start, int *end) {
    const int s = blockIdx.x * MV_T + threadIdx.x;
    if (s >= n_src) return;
    const MvSrc src = srcs[s];
    const int *map = (const int *)src.map + src.first;
    int lo = 0x7fffffff, hi = -1;
    for (int k = 0; k < src.n; ++k) { const int m = map[k]; if (m >= 0) { lo = min(lo, m); hi = max(hi, m); } }
    if (hi >= 0) { atomicMin(start + src.read, lo); atomicMax(end + src.read, hi); }
}
// per workgroup: the reads' cell counts, scanned; off[r] = exclusive prefix inside the workgroup, bsum[block] = the workgroup's total.
// A read nobody moved a cell to gets (-1, -2).
__global__ void __launch_bounds__(MV_T) mv_scan_local_kernel(int *start, int *end, int n_reads, unsigned long long *off, unsigned long long *bsum) {
    __shared__ unsigned long long part[MV_T];
    const int t = threadIdx.x, r = blockIdx.x * MV_T + t;
    unsigned long long len = 0;
    if (r < n_reads) {
        const int s = start[r], e = end[r];
        if (e >= 0 && s <= e) len = (unsigned long long)(e - s + 1);
        else { start[r] = -1; end[r] = -2; }
    }
    part[t] = len;
    __syncthreads();
    for (int o = 1; o < MV_T; o <<= 1) { const unsigned long long v = t >= o ? part[t - o] : 0; __syncthreads(); part[t] += v; __syncthreads(); }
    if (r < n_reads) off[r] = part[t] - len;
    if (t == MV_T - 1) bsum[blockIdx.x] = part[t];
}
// one workgroup: exclusive scan of the workgroup totals in place, MV_T at a time with a running carry; off[n_reads] = the number of cells
__global__ void __launch_bounds__(MV_T) mv_scan_sums_kernel(unsigned long long *bsum, int n_blocks, unsigned long long *total) {
    __shared__ unsigned long long part[MV_T];
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n_blocks; base += MV_T) {
        const int i = base + t;
        const unsigned long long x = i < n_blocks ? bsum[i] : 0;
        part[t] = x;
        __syncthreads();
        for (int o = 1; o < MV_T; o <<= 1) { const unsigned long long v = t >= o ? part[t - o] : 0; __syncthreads(); part[t] += v; __syncthreads(); }
        if (i < n_blocks) bsum[i] = carry + part[t] - x;
        carry += part[MV_T - 1];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}
__global__ void __launch_bounds__(MV_T) mv_scan_add_kernel(unsigned long long *off, int n_reads, const unsigned long long *bsum) {
    const int r = blockIdx.x * MV_T + threadIdx.x;
    if (r < n_reads) off[r] += bsum[blockIdx.x];
}
__global__ void __launch_bounds__(MV_T) mv_fill_kernel(int *cells, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * MV_T + threadIdx.x;
    if (i < n) cells[i] = -1;
}
__global__ void __launch_bounds__(MV_T) mv_scatter_kernel(const MvSrc *srcs, int n_src, unsigned long long n_cells, const int *start, const unsigned long long *off,
                                                          int *alleles, int *alt_qi, unsigned long long cap, int *flag) {
    const unsigned long long c = (unsigned long long)blockIdx.x * MV_T + threadIdx.x;
    if (c >= n_cells) return;
    int lo = 0, hi = n_src - 1; // the last source whose first lane is <= c
    while (lo < hi) { const int mid = lo + ((hi - lo + 1) >> 1); if (srcs[mid].cell0 <= c) lo = mid; else hi = mid - 1; }
    const MvSrc src = srcs[lo];
    const int k = (int)(c - src.cell0);
    if (k >= src.n) return;
    const int m = ((const int *)src.map)[src.first + k];
    if (m < 0) return;
    const int s = start[src.read];
    const unsigned long long dst = off[src.read] + (unsigned long long)(m - s);
    if (s < 0 || m < s || dst >= cap) { *flag = 1; return; }
    alleles[dst] = ((const int *)src.alleles)[k];
    alt_qi[dst] = src.alt_qi ? ((const int *)src.alt_qi)[k] : -1;
}
} // namespace

void lcd_launch_mv_span(const MvSrc *srcs, int n_src, int *start, int *end, hipStream_t st) {
    if (n_src > 0) mv_span_kernel<<<mv_blocks(n_src), MV_T, 0, st>>>(srcs, n_src, start, end);
}
void lcd_launch_mv_scan(int *start, int *end, int n_reads, unsigned long long *off, unsigned long long *bsum, hipStream_t st) {
    if (n_reads <= 0) return;
    const int nb = mv_blocks(n_reads);
    mv_scan_local_kernel<<<nb, MV_T, 0, st>>>(start, end, n_reads, off, bsum);
    mv_scan_sums_kernel<<<1, MV_T, 0, st>>>(bsum, nb, off + n_reads);
    mv_scan_add_kernel<<<nb, MV_T, 0, st>>>(off, n_reads, bsum);
}
void lcd_launch_mv_fill(int *cells, unsigned long long n, hipStream_t st) {
    if (n > 0) mv_fill_kernel<<<mv_blocks(n), MV_T, 0, st>>>(cells, n);
}
void lcd_launch_mv_scatter(const MvSrc *srcs, int n_src, unsigned long long n_cells, const int *start, const unsigned long long *off, int *alleles, int *alt_qi,
                           unsigned long long cap, int *flag, hipStream_t st) {
    if (n_src > 0 && n_cells > 0) mv_scatter_kernel<<<mv_blocks(n_cells), MV_T, 0, st>>>(srcs, n_src, n_cells, start, off, alleles, alt_qi, cap, flag);
}
