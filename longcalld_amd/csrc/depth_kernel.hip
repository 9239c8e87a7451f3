// depth_kernel.hip -- the per-haplotype depth track of a chunk from its kept records, where the inflate left them in HBM (the rules: include/lcd_hotpath.h,
// lcd_chunk_depth; the same rules in Python: tests/depth_common.py):
//   lcd_depth_mark_kernel    one wavefront per kept record: the operation words 64 at a time (the record's own, or its CG field's: lcd_aux::cg_ops).  Per step a
//                            64-bit wave scan of the reference lengths carried from step to step, a ballot of "consumes reference" and one of "covers"; a lane's
//                            state in front of its op is the cover bit of the nearest consuming op below it, or the state the step before ended in.  Cover that
//                            goes on over insertions, clips, zero-length ops (and deletions, unless skip_dels) is ONE interval: the lane of the op that ends it --
//                            lane 0 behind the last op -- looks up where it began (the nearest begin below it, or the carried one), clips it to the region and adds
//                            +1 at its first position and -1 behind its last one to the haplotype's plane of the difference array.  32-bit integer vector
//                            atomics: the result does not depend on the order of arrival.  A HiFi read costs two atomics, whatever its CIGAR's length;
//   lcd_depth_tiles_kernel   per tile of LCD_DEPTH_TILE positions: the three plane sums and the number of run heads (a position where some plane is non-zero, and
//                            the region's first);
//   lcd_depth_scan_kernel    ONE workgroup: the exclusive prefix of the tiles' partials, 256 tiles per round, and the number of rows;
//   lcd_depth_rows_kernel    per tile again: the scan of the planes and the head flags inside the tile (per thread, per wavefront, across the four wavefronts
//                            through LDS), offset by the tile's prefix; the thread of a head writes its row (first position, three depths) at its index.
// No depth array exists in HBM, no workgroup waits for another (three launches instead), and the rows come out in position order.
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
__device__ __forceinline__ int scan_add32(int v, const int lane) {                               // inclusive, 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ int top_bit(const unsigned long long m) { return 63 - __clzll((long long)m); }        // m != 0

enum { DS_RECORDS, DS_NO_CIGAR, DS_CG, DS_NO_OVERLAP, DS_INTERVALS, DS_BASES };
__device__ __forceinline__ void stat_add(const DepthIn &in, const int lane, const int which, const unsigned long long n) {
    if (lane == 0 && n) atomicAdd(in.stats + which, n);
}

// the exclusive prefix of v[4] over the 256 threads of the workgroup and the workgroup's totals; lds: one row per wavefront, free again on return
__device__ __forceinline__ void block_scan4(const int v[4], int excl[4], int total[4], int (*lds)[4], const int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    int inc[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) inc[z] = scan_add32(v[z], lane);
    if (lane == 63) for (int z = 0; z < 4; ++z) lds[wv][z] = inc[z];
    __syncthreads();
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        int off = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { const int t = lds[w][z]; if (w < wv) off += t; tot += t; }
        excl[z] = off + inc[z] - v[z]; total[z] = tot;
    }
    __syncthreads();
}

// the thread's four positions of the three planes (bound: pitch is whole tiles and the planes are 16-byte aligned, so every tile is read in full), its plane sums
// and its run heads: v[0..2], v[3]
struct Quad { int d[3][4]; bool head[4]; };
__device__ __forceinline__ Quad load_quad(const DepthIn &in, const long long k0, int v[4]) {
    Quad q;
    v[3] = 0;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int4 x = *(const int4 *)(in.diff + (long long)h * in.pitch + k0);
        q.d[h][0] = x.x; q.d[h][1] = x.y; q.d[h][2] = x.z; q.d[h][3] = x.w;
        v[h] = x.x + x.y + x.z + x.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long k = k0 + e;
        q.head[e] = k < in.n_pos && (k == 0 || (q.d[0][e] | q.d[1][e] | q.d[2][e]) != 0);
        v[3] += q.head[e];
    }
    return q;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_depth_mark_kernel(const DepthIn in) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= in.n_jobs) return;
    const DepthJob j = in.jobs[i];
    const uint8_t *src = (const uint8_t *)(uintptr_t)j.src, *end = src + j.len, *r = src + 4;      // (at least 36 bytes: the host refuses anything shorter)
    const long long pos1 = (long long)(int)ld32u(r + 4) + 1;
    const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
    const unsigned lname = w2 & 0xffu, nc16 = w3 & 0xffffu;
    const long long lseq = (long long)(int)ld32u(r + 16);
    stat_add(in, lane, DS_RECORDS, 1);
    // everything below reads inside [src, end): name, CIGAR, bases and qualities end in front of the auxiliary fields, and lcd_aux::cg_ops keeps inside the
    // record by itself.  A record whose fields run past its end is one without operations
    if (lseq < 0 || lseq > (long long)j.cap || (unsigned long long)(end - src) < 36ull + lname + 4ull * nc16 + (unsigned long long)((lseq + 1) / 2) + (unsigned long long)lseq) {
        stat_add(in, lane, DS_NO_CIGAR, 1); return;
    }
    const uint8_t *cig = src + 36 + lname; int nc = (int)nc16;
    if (lcd_aux::cg_ops(r, lname, nc, (int)lseq, (int)j.len - 4, lane, &cig, &nc)) stat_add(in, lane, DS_CG, 1);
    if (nc <= 0) { stat_add(in, lane, DS_NO_CIGAR, 1); return; }
    int *plane = in.diff + (long long)j.hap * in.pitch;                  // (hap is 0, 1 or 2: the host refuses others)
    unsigned long long n_iv = 0, n_bases = 0;
    // cover [s, e] of this record, clipped; bound: both indices are inside [0, n_pos), the -1 that would fall behind reg_end is not stored
    auto interval = [&](const long long s, const long long e) {
        if (e < in.reg_beg || s > in.reg_end) return;
        const long long a = s > in.reg_beg ? s : in.reg_beg, b = e < in.reg_end ? e : in.reg_end;
        atomicAdd(plane + (a - in.reg_beg), 1);
        if (e < in.reg_end) atomicAdd(plane + (e + 1 - in.reg_beg), -1);
        ++n_iv; n_bases += (unsigned long long)(b - a + 1);
    };
    unsigned long long ref_done = 0;                                     // reference bases of the steps before (64-bit: below 2^29 ops of below 2^28 bases)
    bool open = false; long long s_open = 0;                             // the state behind the last consuming op so far; where that cover began
    for (unsigned base = 0; base < (unsigned)nc; base += 64) {
        const unsigned k = base + (unsigned)lane;
        const unsigned w = k < (unsigned)nc ? ld32u(cig + 4ull * k) : 0u;               // bound: k < the operations' count, whose words lie inside the record
        const unsigned op = w & 15u; const unsigned long long len = w >> 4;
        const bool cons = len != 0ull && (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u);      // (a zero-length op does nothing)
        const bool cov = cons && (op == 0u || op == 7u || op == 8u || (op == 2u && !in.skip_dels));
        const unsigned long long rl = cons ? len : 0ull;
        const unsigned long long inc = scan_add64(rl, lane);
        const long long rb = pos1 + (long long)(ref_done + inc - rl);    // the op's first position
        const unsigned long long consm = __ballot(cons), covm = __ballot(cov), lower = (1ull << lane) - 1ull;
        const unsigned long long cb = consm & lower;
        const bool before = cb ? ((covm >> top_bit(cb)) & 1ull) != 0ull : open;
        const bool begins = cov && !before, ends = cons && !cov && before;
        const unsigned long long begm = __ballot(begins), bb = begm & lower;
        const long long s_near = __shfl(rb, bb ? top_bit(bb) : 0);       // (every lane shuffles)
        if (ends) interval(bb ? s_near : s_open, rb - 1);
        const long long s_last = __shfl(rb, begm ? top_bit(begm) : 0);
        if (consm) open = ((covm >> top_bit(consm)) & 1ull) != 0ull;
        if (open && begm) s_open = s_last;                               // (open at the step's end: its last event, if it has one, is a begin)
        ref_done += __shfl(inc, 63);
    }
    if (open && lane == 0) interval(s_open, pos1 + (long long)ref_done - 1);
    n_iv = __shfl(scan_add64(n_iv, lane), 63); n_bases = __shfl(scan_add64(n_bases, lane), 63);
    if (!n_iv) stat_add(in, lane, DS_NO_OVERLAP, 1);
    stat_add(in, lane, DS_INTERVALS, n_iv); stat_add(in, lane, DS_BASES + j.hap, n_bases);
}

__global__ void __launch_bounds__(256) lcd_depth_tiles_kernel(const DepthIn in, DepthPart *parts) {
    __shared__ int lds[4][4];
    int v[4], excl[4], total[4];
    (void)load_quad(in, (long long)blockIdx.x * LCD_DEPTH_TILE + 4 * (long long)threadIdx.x, v);
    block_scan4(v, excl, total, lds, threadIdx.x);
    if (threadIdx.x == 0) { DepthPart p; p.s[0] = total[0]; p.s[1] = total[1]; p.s[2] = total[2]; p.heads = total[3]; parts[blockIdx.x] = p; }
}

__global__ void __launch_bounds__(256) lcd_depth_scan_kernel(DepthPart *parts, const long long n_tiles, int *n_rows) {
    __shared__ int lds[4][4];
    int carry[4] = {0, 0, 0, 0};
    for (long long b = 0; b < n_tiles; b += 256) {                       // (every thread makes every round: the scan has barriers)
        const long long t = b + threadIdx.x;
        int v[4] = {0, 0, 0, 0}, excl[4], total[4];
        if (t < n_tiles) { const DepthPart p = parts[t]; v[0] = p.s[0]; v[1] = p.s[1]; v[2] = p.s[2]; v[3] = p.heads; }
        block_scan4(v, excl, total, lds, threadIdx.x);
        if (t < n_tiles) { DepthPart p; p.s[0] = carry[0] + excl[0]; p.s[1] = carry[1] + excl[1]; p.s[2] = carry[2] + excl[2]; p.heads = carry[3] + excl[3]; parts[t] = p; }
#pragma unroll
        for (int z = 0; z < 4; ++z) carry[z] += total[z];
    }
    if (threadIdx.x == 0) *n_rows = carry[3];
}

__global__ void __launch_bounds__(256) lcd_depth_rows_kernel(const DepthIn in, const DepthPart *parts, DepthRow *rows, const int cap) {
    __shared__ int lds[4][4];
    int v[4], excl[4], total[4];
    const long long k0 = (long long)blockIdx.x * LCD_DEPTH_TILE + 4 * (long long)threadIdx.x;
    const Quad q = load_quad(in, k0, v);
    block_scan4(v, excl, total, lds, threadIdx.x);
    const DepthPart p = parts[blockIdx.x];
    int run[3] = {p.s[0] + excl[0], p.s[1] + excl[1], p.s[2] + excl[2]}, idx = p.heads + excl[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        run[0] += q.d[0][e]; run[1] += q.d[1][e]; run[2] += q.d[2][e];
        if (q.head[e]) {
            // bound: the scan counted the same heads, so idx < *n_rows <= cap, the rows' count; the test stays as the store's own bound
            if (idx >= 0 && idx < cap) { DepthRow o; o.beg = in.reg_beg + k0 + e; o.d[0] = (unsigned)run[0]; o.d[1] = (unsigned)run[1]; o.d[2] = (unsigned)run[2]; o.pad = 0; rows[idx] = o; }
            ++idx;
        }
    }
}

void lcd_launch_depth_mark(const DepthIn &in, hipStream_t st) {
    if (in.n_jobs > 0) hipLaunchKernelGGL(lcd_depth_mark_kernel, dim3(in.n_jobs), dim3(64), 0, st, in);
}
void lcd_launch_depth_tiles(const DepthIn &in, DepthPart *parts, hipStream_t st) {
    hipLaunchKernelGGL(lcd_depth_tiles_kernel, dim3((unsigned)(in.pitch / LCD_DEPTH_TILE)), dim3(256), 0, st, in, parts);
}
void lcd_launch_depth_scan(DepthPart *parts, long long n_tiles, int *n_rows, hipStream_t st) {
    hipLaunchKernelGGL(lcd_depth_scan_kernel, dim3(1), dim3(256), 0, st, parts, n_tiles, n_rows);
}
void lcd_launch_depth_rows(const DepthIn &in, const DepthPart *parts, DepthRow *rows, int cap, hipStream_t st) {
    hipLaunchKernelGGL(lcd_depth_rows_kernel, dim3((unsigned)(in.pitch / LCD_DEPTH_TILE)), dim3(256), 0, st, in, parts, rows, cap);
}
