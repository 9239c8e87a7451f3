// plan_kernel.hip -- the plan of one noisy-region pass of collect_var_main (src/collect_var.c:2946-2977) for device-resident chunks: per pending region what
// collect_noisy_vars1 (:2650-2663) and collect_noisy_read_info (src/align.c:1377-1461) work out before the alignment -- the reads of collect_noisy_reg_reads1
// (:1047-1061) in ordered_read_ids order, and per (region, read) pair the read's slice and cover flag.  All regions of all chunks of a call share one grid:
//   count    one wavefront per region; 64 entries of ordered_read_ids per step, overlap tested on the chunk's PlanRead table in HBM, counted by ballot + popcount;
//            writes the region's status (deep / no reads / submit) and, for a submitted region, its number of reads
//   scan     exclusive scan of the counts into 64-bit pair offsets (one workgroup: a call has tens to thousands of regions)
//   fill     the count's walk again; a lane that hits writes its read id at off + popcount(ballot below the lane): ordered_read_ids order, no atomics
//   slices   one wavefront per pair: lcd_slice_walk (slice_walk.h), the device function of lcd_slice_kernel, on the chunk's digars in HBM
// Regions that were done before, are too long or too deep get no pair.  The host checked every ordered_read_ids entry against the chunk's read count.
#include <hip/hip_runtime.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "slice_walk.h"

namespace {
// the walk count and fill share: -> the number of reads of `order` that are not skipped and satisfy !(beg > reg_end || end <= reg_beg) (the reference's asymmetric
// test); FILL: read ids to ids[0 .. cap) and the region index to pair_reg, in order
template <bool FILL>
__device__ __forceinline__ int plan_walk(const PlanChunk &c, const long long reg_beg, const long long reg_end, const int lane, int *ids, int *pair_reg, const int reg,
                                         const unsigned long long cap) {
    const PlanRead *reads = (const PlanRead *)c.reads; const int *order = (const int *)c.order; const unsigned char *skipped = (const unsigned char *)c.skipped;
    int n = 0;
    for (int base = 0; base < c.n_reads; base += 64) {
        const int i = base + lane;
        bool hit = false; int r = -1;
        if (i < c.n_reads) {
            r = order[i];
            if (!skipped[r]) { const PlanRead x = reads[r]; hit = x.status == 0 && !(x.beg > reg_end || x.end <= reg_beg); }
        }
        const unsigned long long m = __ballot(hit);
        if (FILL && hit) {
            const unsigned long long at = (unsigned long long)n + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (at < cap) { ids[at] = r; pair_reg[at] = reg; }
        }
        n += __popcll(m);
    }
    return n;
}

__global__ void __launch_bounds__(64) plan_count_kernel(const PlanChunk *chunks, const PlanReg *regs, const int n_regs, const int max_cov, int *cnt, int *status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_regs) return;
    const PlanReg reg = regs[g];
    int st = reg.status, n = 0;
    if (st == LCD_PLAN_SUBMIT) {
        n = plan_walk<false>(chunks[reg.chunk], reg.beg, reg.end, lane, nullptr, nullptr, g, 0);
        st = n > max_cov ? LCD_PLAN_SKIP_DEEP : n <= 0 ? LCD_PLAN_NO_READS : LCD_PLAN_SUBMIT;
        if (st != LCD_PLAN_SUBMIT) n = 0;
    }
    if (lane == 0) { cnt[g] = n; status[g] = st; }
}

constexpr int PS_T = 256;
__global__ void __launch_bounds__(PS_T) plan_scan_kernel(const int *cnt, const int n, unsigned long long *off) {
    __shared__ unsigned long long wsum[PS_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += PS_T) {
        const int i = base + tid;
        const unsigned long long v = i < n ? (unsigned long long)cnt[i] : 0ull;
        unsigned long long x = v;
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned long long before = 0, tot = 0;
        for (int w = 0; w < PS_T / 64; ++w) { if (w < wave) before += wsum[w]; tot += wsum[w]; }
        if (i < n) off[i] = carry + before + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) off[n] = carry;
}

__global__ void __launch_bounds__(64) plan_fill_kernel(const PlanChunk *chunks, const PlanReg *regs, const int n_regs, const int *status, const unsigned long long *off,
                                                       int *read_ids, int *pair_reg) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_regs || status[g] != LCD_PLAN_SUBMIT) return;
    const PlanReg reg = regs[g];
    const unsigned long long o = off[g];
    plan_walk<true>(chunks[reg.chunk], reg.beg, reg.end, lane, read_ids + o, pair_reg + o, g, off[g + 1] - o);
}

__global__ void __launch_bounds__(64) plan_slice_kernel(const PlanChunk *chunks, const PlanReg *regs, const int *read_ids, const int *pair_reg,
                                                        const unsigned long long n_pairs, const int flank, SliceOut *outs) {
    const unsigned long long p = blockIdx.x; const int lane = threadIdx.x;
    if (p >= n_pairs) return;
    const PlanReg reg = regs[pair_reg[p]];
    const PlanChunk c = chunks[reg.chunk];
    const PlanRead x = ((const PlanRead *)c.reads)[read_ids[p]];
    const SliceOut o = lcd_slice_walk((const DigarRec *)c.digars + x.digar_off, x.n_digar, x.qlen, reg.beg, reg.end, flank, lane);
    if (lane == 0) outs[p] = o;
}
} // namespace

void lcd_launch_plan_count(const PlanChunk *chunks, const PlanReg *regs, int n_regs, int max_cov, int *cnt, int *status, hipStream_t st) {
    if (n_regs > 0) hipLaunchKernelGGL(plan_count_kernel, dim3(n_regs), dim3(64), 0, st, chunks, regs, n_regs, max_cov, cnt, status);
}
void lcd_launch_plan_scan(const int *cnt, int n_regs, unsigned long long *off, hipStream_t st) {
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(PS_T), 0, st, cnt, n_regs, off);
}
void lcd_launch_plan_fill(const PlanChunk *chunks, const PlanReg *regs, int n_regs, const int *status, const unsigned long long *off, int *read_ids, int *pair_reg,
                          hipStream_t st) {
    if (n_regs > 0) hipLaunchKernelGGL(plan_fill_kernel, dim3(n_regs), dim3(64), 0, st, chunks, regs, n_regs, status, off, read_ids, pair_reg);
}
void lcd_launch_plan_slices(const PlanChunk *chunks, const PlanReg *regs, const int *read_ids, const int *pair_reg, unsigned long long n_pairs, int flank,
                            SliceOut *outs, hipStream_t st) {
    if (n_pairs > 0) hipLaunchKernelGGL(plan_slice_kernel, dim3((unsigned)n_pairs), dim3(64), 0, st, chunks, regs, read_ids, pair_reg, n_pairs, flank, outs);
}
