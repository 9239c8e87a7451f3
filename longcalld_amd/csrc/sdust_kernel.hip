// sdust_kernel.hip -- symmetric DUST low-complexity intervals of a chunk's reference on gfx950 (chunk->low_comp_cr, src/bam_utils.c:1573-1581;
// the algorithm is sdust, src/sdust.c:78-163 -- Morgulis et al. 2006 as implemented by H. Li -- a sequential automaton over the sequence).
// What makes it parallel: everything the automaton keeps (the window of the last W - 2 triplets with their counts, the longest suffix in which no
// triplet is over-represented, the "perfect intervals" P that start inside the window) is a function of a bounded stretch behind the current base.
// So the sequence is cut into segments, one LANE per segment, and a lane owns the STEPS i of its segment [a, b) (the last lane also the flush at
// i == len): it reports every interval the automaton saves at one of its steps, WHATEVER the interval's coordinates, folded with sdust's own merge
// rule (adjacent or overlapping intervals are joined), and the host folds the lanes' lists in lane order -- the order in which the reference saves.
// Ownership is by step and not by the interval's start because an N resets l and t but not the window (src/sdust.c:155-158): the first words
// behind an N see words from before it, the window start is computed from l, and the intervals found then carry coordinates up to W - 5 behind
// the current base, at or past len included.  The order of their starts is not the order of the saves, and the merge depends on that order.
// The lead-in: an entry of P at step i was inserted at i - 2W + 5 or later (its start is at most W - 5 behind the step of its insertion; it
// leaves P once the window start, >= i + 1 - W between two N, has passed it; an N empties P), and so was every entry that insertion looked at
// (they start at or behind it, so they are still in P).  The lane therefore needs window, counters, L and l exact at a - 2W: it starts W + 4
// triplet words before that base (counted by the host: W - 2 words fill the window; l is exact behind the first N and past W it cancels from the
// window start), and what it inserts into P before that is gone before step a by the same bound.  A lane's folded list is strictly increasing
// with starts in [a - 3W, b + W], one per four bases at most: seg / 4 + W + 1 <= cap = seg + 8 (unfolded, a lane can save W intervals per base).
// Checked against the reference's sdust.c itself (oracle/_ref) and against the sequential and the segmented model of tests/sdust_model.py,
// tests/test_gpu_digar.py and tests/test_gpu_sdust_seams.py (N-dense sequences: seams, displaced intervals, sequence ends, long P).
#include <hip/hip_runtime.h>
#include <mutex>
#include "lcd_types.h"
#include "lcd_kernels.h"

namespace {
constexpr int SD_LANES = 16; // lanes (segments) per workgroup.  The kernel is latency-bound per lane, so what counts is lanes resident per CU: the window ring and the
                             // triplet counters are BYTES (a count never exceeds W <= 64), 256 B per lane, and the first 32 perfect intervals sit in LDS (512 B per
                             // lane; segments inside a tandem repeat spill the rest of their list to the HBM slab): 12 KB per workgroup = 13 workgroups per CU
struct SdPerf { int start, finish, r, l; };
__device__ __forceinline__ int sd_code(unsigned char c) { // seq_nt4_table, src/sdust.c:22-39: raw codes 0..3 and the letters ACGT / acgt
    if (c < 4) return c;
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
}

__global__ void __launch_bounds__(SD_LANES) lcd_sdust_kernel(const unsigned char *pool, const SdSeg *segs, int T, int W, int seg, int n_seg, int cap, int *n_out, int2 *out, int4 *pbuf, int pcap, int SD_PL) {
    const int sid = blockIdx.x * SD_LANES + threadIdx.x;
    if (sid >= n_seg) return;
    // one launch serves the segments of MANY sequences (a lane is latency-bound on its own automaton: throughput comes from lanes, i.e. from chunks in flight)
    const SdSeg sg = segs[sid];
    const unsigned char *seq = pool + sg.seq_off;
    const int len = sg.len, a = sg.a;
    // sg.from: where the automaton has to start so that its state is exact 2W bases before the segment (the host counts W + 4 triplet words
    // back from there: the window is made of words, and words on both sides of a run of N share it); i == len is the end-of-sequence flush,
    // the last lane's
    const int from = sg.from, end = a + seg >= len ? len : a + seg - 1;
    // per-lane tables in LDS, lane-interleaved (entry k of lane t at [k * SD_LANES + t]): window ring, the two triplet counters, find_perfect's copy
    extern __shared__ int sd_lds[];
    unsigned char *const wq = (unsigned char *)sd_lds + threadIdx.x, *const cv = wq + 64 * SD_LANES, *const cw = cv + 64 * SD_LANES, *const c = cw + 64 * SD_LANES;
#define SDX(k) ((k) * SD_LANES)
    // the perfect intervals of the current window (descending start): at most one per (start inside the window, step it was found at) = W x W
    // entries; the first SD_PL = min(pcap, 32) of them in LDS, lane-interleaved, the rest in an HBM slab (a lane inside a tandem repeat holds hundreds at W = 20)
    int4 *const Pl = (int4 *)((unsigned char *)sd_lds + 4 * 64 * SD_LANES) + threadIdx.x; int4 *const Pg = pbuf + (size_t)sid * pcap;
    // (macros, not lambdas: by-reference captures would put the whole automaton state into scratch memory -- measured 30x slower)
#define Pget(j) ((j) < SD_PL ? Pl[(j) * SD_LANES] : Pg[(j)])   /* (x, y, z, w) = (start, finish, r, l) */
#define Pset(j, v) do { const int4 v_ = (v); if ((j) < SD_PL) Pl[(j) * SD_LANES] = v_; else Pg[(j)] = v_; } while (0)
    int qfront = 0, qcount = 0, pn = 0, rv = 0, rw = 0, L = 0, l = 0, nout = 0, bad = 0, have = 0, cs = 0, cf = 0; // (cs, cf): the lane's last interval, still open
    unsigned t = 0;
    for (int k = 0; k < 64; ++k) { cv[SDX(k)] = 0; cw[SDX(k)] = 0; }
    int2 *mine = out + (size_t)sid * cap;
#define AT(i) (wq[SDX((qfront + (i)) & 63)])
    /* save_masked_regions :91-106 at step i: from step a on the interval is the lane's, merged into its previous one or opened (the host does the same over the lanes' lists) */
#define SD_SAVE(start_)                                                                                                    \
    do {                                                                                                                   \
        if (pn == 0) break;                                                                                                \
        const int4 p_ = Pget(pn - 1);                                                                                      \
        if (p_.x >= (start_)) break;                                                                                       \
        if (i >= a) {                                                                                                      \
            if (have && p_.x <= cf) { if (p_.y > cf) cf = p_.y; }                                                          \
            else { if (have) { if (nout < cap) mine[nout] = make_int2(cs, cf); ++nout; } cs = p_.x; cf = p_.y; have = 1; } \
        }                                                                                                                  \
        int i_ = pn - 2;                                                                                                   \
        while (i_ >= 0 && Pget(i_).x < (start_)) --i_;                                                                     \
        pn = i_ + 1;                                                                                                       \
    } while (0)
    for (int i = from; i <= end; ++i) {
        const int bcode = i < len ? sd_code(seq[i]) : 4;
        if (bcode < 4) {
            ++l; t = (t << 2 | (unsigned)bcode) & 63u;
            if (l >= 3) {
                const int start = (l - W > 0 ? l - W : 0) + (i + 1 - l);
                SD_SAVE(start);
                { // shift_window :68-89
                    if (qcount >= W - 3 + 1) { const int s = wq[SDX(qfront)]; qfront = (qfront + 1) & 63; --qcount; rw -= --cw[SDX(s)]; if (L > qcount) { --L; rv -= --cv[SDX(s)]; } }
                    wq[SDX((qfront + qcount) & 63)] = (unsigned char)t; ++qcount;
                    ++L; rw += cw[SDX(t)]++; rv += cv[SDX(t)]++;
                    if (cv[SDX(t)] * 10 > T << 1) { int s; do { s = AT(qcount - L); rv -= --cv[SDX(s)]; --L; } while (s != (int)t); }
                }
                if (rw * 10 > L * T) { // find_perfect :108-135
                    for (int k = 0; k < 64; ++k) c[SDX(k)] = cv[SDX(k)];
                    int r = rv, max_r = 0, max_l = 0;
                    for (int x = qcount - L - 1; x >= 0; --x) {
                        const int tt = AT(x);
                        r += c[SDX(tt)]++;
                        const int new_r = r, new_l = qcount - x - 1;
                        if (new_r * 10 > T * new_l) {
                            int j = 0;
                            for (; j < pn; ++j) { const int4 q = Pget(j); if (q.x < x + start) break; if (max_r == 0 || q.z * max_l > max_r * q.w) { max_r = q.z; max_l = q.w; } }
                            if (max_r == 0 || new_r * max_l >= max_r * new_l) {
                                max_r = new_r; max_l = new_l;
                                if (pn >= pcap) { bad = 1; break; }
                                for (int m = pn; m > j; --m) Pset(m, Pget(m - 1));
                                ++pn;
                                Pset(j, make_int4(x + start, qcount + 2 + start, new_r, new_l));
                            }
                        }
                    }
                }
            }
        } else { // N or the end of the sequence: independent pieces (:152-156)
            int start = (l - W + 1 > 0 ? l - W + 1 : 0) + (i + 1 - l);
            while (pn) { SD_SAVE(start); ++start; }
            l = 0; t = 0;
            // (the reference keeps the window and its counters across an N: the next piece's first words see them; kept here as well)
        }
    }
#undef SDX
#undef AT
#undef Pget
#undef Pset
#undef SD_SAVE
    if (have) { if (nout < cap) mine[nout] = make_int2(cs, cf); ++nout; }
    n_out[sid] = bad ? -1 : nout;
}

void lcd_launch_sdust(const unsigned char *pool, const SdSeg *segs, int T, int W, int seg, int n_seg, int cap, int *n_out, int2 *out, int4 *pbuf, int pcap, hipStream_t stream) {
    static std::once_flag attr_once[16]; // (function attributes are per device)
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    std::call_once(attr_once[dev], [] { (void)hipFuncSetAttribute((const void *)lcd_sdust_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); });
    const int pl = pcap < 32 ? pcap : 32;
    const size_t lds = (size_t)SD_LANES * (4 * 64 + (size_t)pl * sizeof(int4));
    if (n_seg > 0) hipLaunchKernelGGL(lcd_sdust_kernel, dim3((n_seg + SD_LANES - 1) / SD_LANES), dim3(SD_LANES), lds, stream, pool, segs, T, W, seg, n_seg, cap, n_out, out, pbuf, pcap, pl);
}
