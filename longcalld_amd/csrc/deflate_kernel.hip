// deflate_kernel.hip -- the inverse of inflate_kernel.hip: BGZF blocks COMPRESSED on the device (gfx950), one wavefront per block.
//
// The reference writes its phased BAM through htslib's bgzf writer (write_read_to_bam, src/bam_utils.c:1944-2006 -> sam_write1 -> bgzf_write -> zlib deflate on
// hts_set_threads host threads).  A BGZF block is an independent gzip member of <= 64 KB (SAM specification 4.1), so a file image is thousands of independent
// jobs.  Every lane of the wavefront works on the same block; control flow is uniform and the lanes split what is parallel inside a block:
//   * matches: LZ77 over the block's own bytes in HBM.  The 64 lanes hash the 3 bytes at 64 consecutive positions, look their candidate up in a hash table in LDS
//     (4 096 positions as u16, the most recent one per bucket: the candidate depth is capped at ONE), verify and extend it (<= 258 bytes, distance <= 32 768) and a
//     ballot-driven pass walks the 64 results in stream order: runs of literals are taken at once, a match skips the lanes it covers.  Only the positions a pass
//     consumed (its first 64) enter the table, after the pass -- a position never finds itself;
//   * codes: symbol histograms in LDS (LDS atomics), dynamic Huffman lengths by the in-place minimum-redundancy construction (Moffat & Katajainen 1995) on the
//     rank-sorted frequencies, limited to 15 bits by moving codes down the Kraft sum (measured at most 0.016 % over the optimal limited code) and, for the
//     code-length alphabet, to 7 bits by package-merge (the optimum: 19 symbols fit one wavefront); canonical codes by ballot ranks; the code lengths are written
//     with the run-length symbols 16 / 17 / 18;
//   * bits: 64 tokens at a time -- each lane makes its token's bits (<= 48), an inclusive prefix sum of the bit lengths gives every lane its bit offset, the
//     lanes OR their bits into a 512-byte staging area in LDS and finished dwords go to HBM as one coalesced store;
//   * the cheapest of stored / fixed / dynamic is written; a block whose coded form is not smaller than the stored form (payload + 5 bytes) is stored, so a
//     member is at most payload + 5 + 26 bytes and a 0xff00 payload always fits 64 KB;
//   * CRC-32 by crc32_gf2.h (the inflate kernel's slice-and-combine arithmetic).
// Tokens (4 bytes each) wait in HBM between the match pass and the bit pass: a workspace of `payload` words per WORKGROUP; the grid strides over the blocks.
// Every loop is bounded by the block's byte count or by a constant written in its header; none ends on data alone.
// LDS: 14 540 bytes per block (8 KB of it the hash table) -> 11 blocks per CU (160 KB; 151 VGPRs allow 12); inflate_kernel.hip measured that small footprints win for this kind of
// serial-per-wavefront work, so the 32 KB window is NOT kept in LDS: candidates are verified against the block's bytes in HBM (L2).
// Written from RFC 1951 / RFC 1952 and the SAM specification's BGZF section only; no zlib source was consulted.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "crc32_gf2.h"
#include "wave_copy.h"

namespace {
constexpr int HBITS = 12, HSIZE = 1 << HBITS;
constexpr int SB_WORDS = 128;       // bit staging: 64 tokens x 48 bits + 31 carried bits < 4 096 bits
constexpr int TOO_FAR = 4096;       // a 3-byte match further back than this costs more bits than its literals

struct DeflLds {
    unsigned hist_l[288], hist_d[32], hist_c[20];
    unsigned key[288];               // Huffman workspace: sorted frequencies -> parents -> depths
    unsigned cnt[16];                // codes per length
    unsigned sb[SB_WORDS];
    unsigned crct[256];
    unsigned short head[HSIZE];      // most recent position per hash bucket, 0xffff: none (a block has at most 65 280 positions)
    unsigned short ssym[288];        // symbols in frequency order
    unsigned short code_l[288], code_d[32], code_c[20];   // bit-reversed canonical codes
    unsigned short cltok[320];       // the run-length coded code lengths: symbol | extra value << 5
    unsigned char len_l[288], len_d[32], len_c[20];
};

__constant__ unsigned char d_clord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int ufl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// 4 bytes at in[p] (little endian); `room` bytes are readable from in[0] on, bytes behind them read as 0
__device__ __forceinline__ unsigned ld4(const uint8_t *in, const long long p, const long long room) {
    if (p + 8 <= room) return lcd_wave::ld32u(in + p);
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (p + k < room) w |= (unsigned)in[p + k] << (8 * k);
    return w;
}
__device__ __forceinline__ unsigned hash3(unsigned w) { return ((w & 0xffffffu) * 0x9e3779b1u) >> (32 - HBITS); }

// length 3..258 -> literal/length symbol, its extra bits and their value (RFC 1951 3.2.5, in closed form)
__device__ __forceinline__ int len_sym(int len, int &nb, int &ev) {
    if (len == 258) { nb = 0; ev = 0; return 285; }
    const int l = len - 3;
    if (l < 8) { nb = 0; ev = 0; return 257 + l; }
    nb = (31 - __clz(l)) - 2; ev = l & ((1 << nb) - 1);
    return 257 + 4 * (nb + 1) + ((l >> nb) & 3);
}
__device__ __forceinline__ int dist_sym(int dist, int &nb, int &ev) {
    const int d = dist - 1;
    if (d < 4) { nb = 0; ev = 0; return d; }
    nb = (31 - __clz(d)) - 1; ev = d & ((1 << nb) - 1);
    return 2 * (nb + 1) + ((d >> nb) & 1);
}
__device__ __forceinline__ int lext_of(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }
__device__ __forceinline__ int dext_of(int d) { return d < 4 ? 0 : (d >> 1) - 1; }
__device__ __forceinline__ int fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

__device__ __forceinline__ long long wave_sum_ll(long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)v, d, 64), hi = __shfl_xor((int)(v >> 32), d, 64);
        v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}

// Optimal lengths of at most `limit` bits for a SMALL alphabet whose unrestricted code is deeper than that: package-merge (Larmore & Hirschberg 1990), one list item
// per lane.  n <= 21 symbols in use and limit <= 7, so that a list (n leaves and the pairs of the list before it: fewer than 2 n items) fits the wavefront and an
// item's record of how often it holds each leaf (at most once per level: 3 bits each) fits 64 bits.  The leaves are the symbols in rank order (S.ssym); level by
// level the pairs of the current list are merged with the leaves (a leaf goes in front of a pair of its weight), every item finding its place by counting; the
// first 2 n - 2 items of the last list hold leaf i as often as its code is long.  -> S.cnt: the codes per length.  S.key is the staging area (free by now).
__device__ void package_merge_counts(DeflLds &S, const unsigned *hist, const int n, const int limit, const int lane) {
    const unsigned lw = lane < n ? hist[S.ssym[lane]] : 0u;
    const unsigned long long lc = lane < n ? 1ull << (3 * imin(lane, 20)) : 0ull;
    unsigned w = lw;
    unsigned long long c = lc;
    int m = n;
    auto sh64 = [](const unsigned long long v, const int src) -> unsigned long long {
        return ((unsigned long long)(unsigned)__shfl((int)(v >> 32), src, 64) << 32) | (unsigned long long)(unsigned)__shfl((int)(unsigned)v, src, 64);
    };
    for (int level = 2; level <= limit; ++level) {
        const int np = m >> 1, a = imin(2 * lane, 63), b = imin(2 * lane + 1, 63);
        const unsigned pw = (unsigned)__shfl((int)w, a, 64) + (unsigned)__shfl((int)w, b, 64);
        const unsigned long long pc = sh64(c, a) + sh64(c, b);
        int posl = lane, posp = lane;
        for (int k = 0; k < np; ++k) posl += (unsigned)__shfl((int)pw, k, 64) < lw ? 1 : 0;
        for (int i = 0; i < n; ++i) posp += (unsigned)__shfl((int)lw, i, 64) <= pw ? 1 : 0;
        __syncthreads();
        if (lane < n) { S.key[posl] = lw; S.key[64 + posl] = (unsigned)lc; S.key[128 + posl] = (unsigned)(lc >> 32); }     // posl, posp < n + np <= 41
        if (lane < np) { S.key[posp] = pw; S.key[64 + posp] = (unsigned)pc; S.key[128 + posp] = (unsigned)(pc >> 32); }
        __syncthreads();
        m = n + np;
        w = lane < m ? S.key[lane] : 0u;
        c = lane < m ? ((unsigned long long)S.key[128 + lane] << 32) | S.key[64 + lane] : 0ull;
    }
    const unsigned long long tot = (unsigned long long)wave_sum_ll((long long)(lane < 2 * n - 2 ? c : 0ull));
    __syncthreads();
    if (lane < 16) S.cnt[lane] = 0;
    __syncthreads();
    if (lane < n) atomicAdd(&S.cnt[(int)((tot >> (3 * imin(lane, 20))) & 7ull)], 1u);
}

// Code lengths of one alphabet (nsym <= 288 symbols, frequencies in hist) limited to `limit` bits -> lens.  At least two symbols get a code (a lone symbol
// would need a zero-bit code; the frequencies of the first free symbols are raised to 1 while the lengths are made), so the code is always complete.
__device__ void huff_lengths(DeflLds &S, unsigned *hist, const int nsym, const int limit, unsigned char *lens, const int lane) {
    __syncthreads();
    int n = 0;
    for (int r = 0; r < 5; ++r) { const int s = r * 64 + lane; n += __popcll(__ballot(s < nsym && hist[s] > 0)); }
    n = ufl(n);
    int raised = 0;                                                       // the symbols that were given a frequency here: they get a code and go back to 0
    if (n < 2) {
        if (lane == 0) { int need = 2 - n; for (int s = 0; s < 3 && need > 0; ++s) if (!hist[s]) { hist[s] = 1; --need; raised |= 1 << s; } }
        raised = ufl(raised);
        n = 2;
        __syncthreads();
    }
    // symbols in (frequency, symbol) order: the rank of each by counting
    for (int r = 0; r < 5; ++r) {
        const int s = r * 64 + lane;
        if (s < nsym) lens[s] = 0;
        const unsigned f = s < nsym ? hist[s] : 0;
        if (f) {
            int rank = 0;
            for (int t = 0; t < nsym; ++t) { const unsigned g = hist[t]; rank += (g != 0 && (g < f || (g == f && t < s))) ? 1 : 0; }
            S.key[rank] = f; S.ssym[rank] = (unsigned short)s;
        }
    }
    if (lane < 16) S.cnt[lane] = 0;
    __syncthreads();
    // in-place minimum-redundancy code lengths (Moffat & Katajainen): uniform serial code, lane 0 writes, every lane follows lane 0's view
    auto K = [&](const int i) -> int { return ufl((int)S.key[i]); };
    auto SK = [&](const int i, const int v) { if (lane == 0) S.key[i] = (unsigned)v; };
    SK(0, K(0) + K(1));
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        int v;
        if (leaf >= n || K(root) < K(leaf)) { v = K(root); SK(root, next); ++root; } else { v = K(leaf); ++leaf; }
        if (leaf >= n || (root < next && K(root) < K(leaf))) { v += K(root); SK(root, next); ++root; } else { v += K(leaf); ++leaf; }
        SK(next, v);
    }
    SK(n - 2, 0);
    for (int next = n - 3; next >= 0; --next) SK(next, K(K(next)) + 1);
    {
        int avbl = 1, used = 0, dpth = 0, next = n - 1;
        root = n - 2;
        for (int g = 0; g < 300 && avbl > 0; ++g) {                       // one step per depth: at most nsym - 1 of them
            for (int q = 0; q < 288 && root >= 0 && K(root) == dpth; ++q) { ++used; --root; }
            for (int q = 0; q < 288 && avbl > used && next >= 0; ++q) { SK(next, dpth); --next; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
    }
    __syncthreads();
    // codes per length, depths beyond the limit counted at the limit
    for (int i = lane; i < n; i += 64) atomicAdd(&S.cnt[imin((int)S.key[i], limit)], 1u);
    __syncthreads();
    auto Cn = [&](const int i) -> int { return ufl((int)S.cnt[i]); };
    auto SC = [&](const int i, const int v) { if (lane == 0) S.cnt[i] = (unsigned)v; };
    int total = 0;
    for (int i = limit; i > 0; --i) total += Cn(i) << (limit - i);
    if (total != (1 << limit) && limit <= 7 && n <= 21) package_merge_counts(S, hist, n, limit, lane);   // the code-length alphabet: the optimum (its cost is a few hundred
                                                                                                         // bits, where one bit given away is 0.15 %)
    else for (int g = 0; g < 512 && total != (1 << limit); ++g) {         // the Kraft sum is over by less than one per clamped symbol
        SC(limit, Cn(limit) - 1);
        for (int i = limit - 1; i > 0; --i) if (Cn(i)) { SC(i, Cn(i) - 1); SC(i + 1, Cn(i + 1) + 2); break; }
        --total;
    }
    __syncthreads();
    // the most frequent symbols take the shortest lengths
    for (int j = lane; j < n; j += 64) {
        const int q = n - 1 - j;
        int L = limit, acc = 0;
        for (int i = 1; i <= 15; ++i) { if (i <= limit) { acc += (int)S.cnt[i]; if (q < acc) { L = i; break; } } }
        lens[S.ssym[j]] = (unsigned char)L;
    }
    if (lane < 3 && ((raised >> lane) & 1)) hist[lane] = 0;               // a symbol that never occurs costs the block no bits (the dynamic form's size is counted from hist)
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2) of the lengths, bit-reversed for the LSB-first stream
__device__ void assign_codes(const unsigned char *lens, const int nsym, unsigned short *codes, const int lane) {
    int run[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) run[l] = 0;
    int myrank[5], mylen[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int sym = r * 64 + lane;
        const int L = sym < nsym ? lens[sym] : 0;
        mylen[r] = L; myrank[r] = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) {
            const unsigned long long m = __ballot(L == l);
            if (L == l) myrank[r] = run[l] + __popcll(m & ((1ull << lane) - 1ull));
            run[l] += __popcll(m);
        }
    }
    int first[16], code = 0;
    first[0] = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) { code = (code + run[l - 1]) << 1; first[l] = code; }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int L = mylen[r], sym = r * 64 + lane;
        int fc = 0;
#pragma unroll
        for (int l = 1; l < 16; ++l) fc = L == l ? first[l] : fc;
        if (L > 0 && sym < nsym) codes[sym] = (unsigned short)(__brev((unsigned)(fc + myrank[r])) >> (32 - L));
    }
    __syncthreads();
}

// the bit stream: bits wait in S.sb, whole dwords go to out
struct Emit { unsigned *out; int outw, carry, cap_words, over; };
// every lane adds nb (<= 48) bits v, lane order = stream order
__device__ void emit(DeflLds &S, Emit &e, const unsigned long long v, const int nb, const int lane) {
    int inc = nb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    const int total = ufl(__shfl(inc, 63, 64));
    if (nb > 0) {
        const int off = e.carry + inc - nb, w = off >> 5, s = off & 31;
        const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        const unsigned d0 = lo << s, d1 = s ? (lo >> (32 - s)) | (hi << s) : hi, d2 = s ? hi >> (32 - s) : 0u;
        if (d0) atomicOr(&S.sb[w], d0);
        if (d1) atomicOr(&S.sb[w + 1], d1);
        if (d2) atomicOr(&S.sb[w + 2], d2);
    }
    __syncthreads();
    const int tot = e.carry + total, nfull = tot >> 5;
    if (e.outw + nfull + 1 > e.cap_words) e.over = 1;                     // (cannot happen for a form chosen as smaller than stored: the slot holds payload + 5 bytes)
    else for (int k = lane; k < nfull; k += 64) e.out[e.outw + k] = S.sb[k];
    const unsigned rem = (unsigned)ufl((int)S.sb[nfull]);
    __syncthreads();
    for (int k = lane; k <= nfull + 2 && k < SB_WORDS; k += 64) S.sb[k] = 0;
    __syncthreads();
    if (lane == 0) S.sb[0] = rem;
    __syncthreads();
    if (!e.over) e.outw += nfull;
    e.carry = tot & 31;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_deflate_kernel(const uint8_t *data, const unsigned long long n_total, const int payload, const int n_blocks, uint8_t *slots,
                                                         const unsigned slot_stride, unsigned *toks, DeflateOut *outs) {
    __shared__ DeflLds S;
    const int lane = threadIdx.x;
    unsigned *tok = toks + (size_t)blockIdx.x * (size_t)payload;
    for (int j = blockIdx.x; j < n_blocks; j += gridDim.x) {
        const unsigned long long boff = (unsigned long long)j * (unsigned long long)payload;
        const uint8_t *in = data + boff;
        const long long room = (long long)(n_total - boff);
        const int n = (int)(room < payload ? room : payload);
        uint8_t *slot = slots + (size_t)j * slot_stride;
        __syncthreads();
        for (int k = lane; k < 288; k += 64) S.hist_l[k] = 0;
        if (lane < 32) S.hist_d[lane] = 0;
        if (lane < 20) S.hist_c[lane] = 0;
        for (int k = lane; k < HSIZE; k += 64) S.head[k] = 0xffff;
        for (int k = lane; k < SB_WORDS; k += 64) S.sb[k] = 0;
        lcd_crc::crc32_fill_table((lcd_crc::crc_lds_u32 *)S.crct, lane);
        __syncthreads();
        const unsigned crc = lcd_crc::crc32_wave(in, n, (const lcd_crc::crc_lds_u32 *)S.crct, lane);

        // ---- matches: 64 positions per pass ----
        int pos = 0, ntok = 0;
        for (int it = 0; it < n && pos < n; ++it) {                       // a pass consumes at least one byte
            const int p = pos + lane;
            const unsigned w = p < n ? ld4(in, p, room) : 0u;
            const unsigned h = hash3(w);
            int mlen = 0, mdist = 0;
            if (p + 3 <= n) {
                const int c = (int)S.head[h];
                if (c != 0xffff && c < p && p - c <= 32768) {
                    const int maxl = imin(258, n - p);
                    int l = 0;
                    for (int k = 0; k < 65 && l < maxl; ++k) {             // 4 bytes per step, 258 at most
                        const unsigned x = ld4(in, c + l, room) ^ ld4(in, p + l, room);
                        if (x) { l += (__ffs((int)x) - 1) >> 3; break; }
                        l += 4;
                    }
                    l = imin(l, maxl);
                    if (l >= 4 || (l == 3 && p - c <= TOO_FAR)) { mlen = l; mdist = p - c; }
                }
            }
            // the pass's tokens in stream order
            const unsigned long long M = __ballot(mlen >= 3);
            const int avail = imin(64, n - pos);
            unsigned long long starts = 0;
            int cur = 0;
            for (int g = 0; g < 64 && cur < avail; ++g) {                  // each step takes a run of literals and one match
                const unsigned long long rest = M >> cur;
                const int last = rest ? cur + (__ffsll((long long)rest) - 1) : avail - 1;   // the match's lane, or the pass's last literal
                const unsigned long long upto = last >= 63 ? ~0ull : ((1ull << (last + 1)) - 1ull);
                starts |= upto & ~((1ull << cur) - 1ull);
                cur = rest ? last + ufl(__shfl(mlen, last, 64)) : avail;
            }
            const bool mine = (starts >> lane) & 1ull;
            if (mine) {
                const int at = ntok + __popcll(starts & ((1ull << lane) - 1ull));
                if (mlen >= 3) {
                    int nb, ev;
                    tok[at] = ((unsigned)mdist << 9) | (unsigned)mlen;
                    atomicAdd(&S.hist_l[len_sym(mlen, nb, ev)], 1u);
                    atomicAdd(&S.hist_d[dist_sym(mdist, nb, ev)], 1u);
                } else {
                    tok[at] = w & 0xffu;
                    atomicAdd(&S.hist_l[w & 0xffu], 1u);
                }
            }
            ntok = ufl(ntok + __popcll(starts));
            if (lane < cur && p + 3 <= n) S.head[h] = (unsigned short)p;  // the consumed positions of this pass (a collision keeps either one)
            pos = ufl(pos + cur);
            __syncthreads();
        }
        if (lane == 0) S.hist_l[256] = 1;                                 // end of block
        __builtin_amdgcn_s_waitcnt(0x0f70);                               // vmcnt(0): the tokens have landed before the bit pass reads them
        __syncthreads();

        // ---- the three forms' sizes ----
        long long fixed_bits = 0;
        for (int s = lane; s < 286; s += 64) fixed_bits += (long long)S.hist_l[s] * (fixed_len(s) + lext_of(s));
        if (lane < 30) fixed_bits += (long long)S.hist_d[lane] * (5 + dext_of(lane));
        fixed_bits = 3 + wave_sum_ll(fixed_bits);
        huff_lengths(S, S.hist_l, 286, 15, S.len_l, lane);
        huff_lengths(S, S.hist_d, 30, 15, S.len_d, lane);
        int hlit = 257, hdist = 1;
        for (int r = 4; r < 5; ++r) { const int s = r * 64 + lane; const unsigned long long m = __ballot(s < 286 && S.len_l[s] != 0); if (m) hlit = r * 64 + (64 - __clzll((long long)m)); }
        { const unsigned long long m = __ballot(lane < 30 && S.len_d[lane] != 0); if (m) hdist = 64 - __clzll((long long)m); }
        hlit = ufl(hlit < 257 ? 257 : hlit); hdist = ufl(hdist);
        // the code lengths, run-length coded (uniform serial code; lane 0 writes)
        const int total_cl = hlit + hdist;
        auto V = [&](const int i) -> int { return ufl((int)(i < hlit ? S.len_l[i] : S.len_d[i - hlit])); };
        int nct = 0;
        {
            int i = 0, prev = -1;
            for (int g = 0; g < 320 && i < total_cl; ++g) {               // a token covers at least one length
                const int v = V(i), cap = v == 0 ? 138 : 6;
                int run = 1;
                for (int q = 0; q < 138 && run < cap && i + run < total_cl && V(i + run) == v; ++q) ++run;
                int sym, ev = 0, r = 1;
                if (v == 0 && run >= 11) { sym = 18; r = run; ev = run - 11; }
                else if (v == 0 && run >= 3) { sym = 17; r = run; ev = run - 3; }
                else if (v == prev && run >= 3) { sym = 16; r = run; ev = run - 3; }
                else sym = v;
                if (lane == 0) { S.cltok[nct] = (unsigned short)(sym | (ev << 5)); S.hist_c[sym] += 1; }
                ++nct; i += r; prev = v;
            }
        }
        __syncthreads();
        huff_lengths(S, S.hist_c, 19, 7, S.len_c, lane);
        int hclen = 4;
        { const unsigned long long m = __ballot(lane < 19 && S.len_c[d_clord[lane < 19 ? lane : 0]] != 0); if (m) hclen = 64 - __clzll((long long)m); }
        hclen = ufl(hclen < 4 ? 4 : hclen);
        long long dyn_bits = 0;
        for (int s = lane; s < 286; s += 64) dyn_bits += (long long)S.hist_l[s] * (S.len_l[s] + lext_of(s));
        if (lane < 30) dyn_bits += (long long)S.hist_d[lane] * (S.len_d[lane] + dext_of(lane));
        for (int k = lane; k < nct; k += 64) { const int sym = S.cltok[k] & 31; dyn_bits += S.len_c[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0); }
        dyn_bits = 3 + 14 + 3 * hclen + wave_sum_ll(dyn_bits);
        int kind = dyn_bits < fixed_bits ? 2 : 1;
        const long long coded = ((kind == 2 ? dyn_bits : fixed_bits) + 7) >> 3;
        if (coded >= (long long)n + 5) kind = 0;
        kind = ufl(kind);

        unsigned clen = 0;
        if (kind != 0) {
            if (kind == 1) {
                for (int s = lane; s < 288; s += 64) S.len_l[s] = (unsigned char)fixed_len(s);
                if (lane < 32) S.len_d[lane] = 5;
                __syncthreads();
                assign_codes(S.len_l, 288, S.code_l, lane);
                assign_codes(S.len_d, 32, S.code_d, lane);
            } else {
                assign_codes(S.len_l, 286, S.code_l, lane);
                assign_codes(S.len_d, 30, S.code_d, lane);
                assign_codes(S.len_c, 19, S.code_c, lane);
            }
            Emit e; e.out = (unsigned *)slot; e.outw = 0; e.carry = 0; e.cap_words = (int)(slot_stride >> 2); e.over = 0;
            // BFINAL = 1, BTYPE; HLIT, HDIST, HCLEN
            emit(S, e, lane == 0 ? (kind == 1 ? 0x3ull : (0x5ull | ((unsigned long long)(hlit - 257) << 3) | ((unsigned long long)(hdist - 1) << 8) | ((unsigned long long)(hclen - 4) << 13))) : 0ull,
                 lane == 0 ? (kind == 1 ? 3 : 17) : 0, lane);
            if (kind == 2) {
                emit(S, e, lane < hclen ? (unsigned long long)S.len_c[d_clord[lane < 19 ? lane : 0]] : 0ull, lane < hclen ? 3 : 0, lane);
                for (int b = 0; b < 320 && b < nct; b += 64) {
                    unsigned long long v = 0; int nb = 0;
                    if (b + lane < nct) {
                        const int t = S.cltok[b + lane], sym = t & 31, ev = t >> 5;
                        nb = S.len_c[sym]; v = S.code_c[sym];
                        v |= (unsigned long long)ev << nb; nb += sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                    }
                    emit(S, e, v, nb, lane);
                }
            }
            for (int b = 0; b < ntok; b += 64) {                          // ntok <= n
                unsigned long long v = 0; int nb = 0;
                if (b + lane < ntok) {
                    const unsigned t = tok[b + lane];
                    if (t >> 9) {
                        int xb, xv;
                        const int ls = len_sym((int)(t & 511u), xb, xv);
                        v = S.code_l[ls]; nb = S.len_l[ls];
                        v |= (unsigned long long)xv << nb; nb += xb;
                        const int ds = dist_sym((int)(t >> 9), xb, xv);
                        v |= (unsigned long long)S.code_d[ds] << nb; nb += S.len_d[ds];
                        v |= (unsigned long long)xv << nb; nb += xb;
                    } else { v = S.code_l[t & 255u]; nb = S.len_l[t & 255u]; }
                }
                emit(S, e, v, nb, lane);
            }
            emit(S, e, lane == 0 ? (unsigned long long)S.code_l[256] : 0ull, lane == 0 ? S.len_l[256] : 0, lane);
            if (e.over) kind = 0;
            else {
                if (e.carry > 0 && lane == 0) e.out[e.outw] = S.sb[0];
                clen = (unsigned)(e.outw * 4 + ((e.carry + 7) >> 3));
            }
        }
        if (kind == 0) {                                                   // one stored block: payload < 65 536
            if (lane == 0) { slot[0] = 1; slot[1] = (uint8_t)(n & 255); slot[2] = (uint8_t)(n >> 8); slot[3] = (uint8_t)(~n & 255); slot[4] = (uint8_t)((~n >> 8) & 255); }
            for (int k = lane; k < n; k += 64) slot[5 + k] = in[k];
            clen = (unsigned)n + 5u;
        }
        if (lane == 0) { DeflateOut o; o.clen = clen; o.crc = crc; o.kind = (unsigned)kind; o.n_tok = (unsigned)ntok; outs[j] = o; }
    }
}

// the members at their places of the file image: 18-byte header with the BC field, the slot's stream, CRC-32, ISIZE
__global__ void __launch_bounds__(64) lcd_deflate_pack_kernel(const uint8_t *slots, const unsigned slot_stride, const DeflateOut *outs, const unsigned long long *offs,
                                                              uint8_t *image, const unsigned long long n_total, const int payload, const int n_blocks) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_blocks) return;
    const DeflateOut o = outs[j];
    uint8_t *dst = image + offs[j];
    const unsigned long long boff = (unsigned long long)j * (unsigned long long)payload;
    const unsigned isize = (unsigned)(n_total - boff < (unsigned long long)payload ? n_total - boff : (unsigned long long)payload);
    const unsigned bsize = 18u + o.clen + 8u - 1u;
    if (lane < 18) {
        const unsigned char hd[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, (unsigned char)(bsize & 255u), (unsigned char)(bsize >> 8)};
        dst[lane] = hd[lane];
    }
    lcd_wave::wave_copy(dst + 18, slots + (size_t)j * slot_stride, (long long)o.clen, lane);
    if (lane < 8) dst[18 + o.clen + lane] = (uint8_t)((lane < 4 ? o.crc >> (8 * lane) : isize >> (8 * (lane - 4))) & 255u);
}

int lcd_deflate_lds_bytes() { return (int)sizeof(DeflLds); }
void lcd_deflate_set_x2n(const unsigned *t32, hipStream_t st) { (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(lcd_crc::c_x2n), t32, 32 * sizeof(unsigned), 0, hipMemcpyHostToDevice, st); }
void lcd_launch_deflate(const uint8_t *data, unsigned long long n, int payload, int n_blocks, uint8_t *slots, unsigned slot_stride, unsigned *toks, DeflateOut *outs, int grid,
                        hipStream_t st) {
    if (n_blocks > 0 && grid > 0) hipLaunchKernelGGL(lcd_deflate_kernel, dim3(grid), dim3(64), 0, st, data, n, payload, n_blocks, slots, slot_stride, toks, outs);
}
void lcd_launch_deflate_pack(const uint8_t *slots, unsigned slot_stride, const DeflateOut *outs, const unsigned long long *offs, uint8_t *image, unsigned long long n, int payload,
                             int n_blocks, hipStream_t st) {
    if (n_blocks > 0) hipLaunchKernelGGL(lcd_deflate_pack_kernel, dim3(n_blocks), dim3(64), 0, st, slots, slot_stride, outs, offs, image, n, payload, n_blocks);
}
