// SURVEY 8(f) f3 on the device, behind the inflate: BAM records are found, measured and their CIGARs collected in the inflated stream in HBM -- what bam_read1 and
// the record loop of collect_ref_seq_bam_main (src/bam_utils.c:1672-1706) do on the calling thread for the reference, one record at a time.
//   lcd_bam_walk_kernel   one lane per range of the stream (a .bai chunk): hops from block_size to block_size (the only serial dependency of the format: ~1 000
//                         records of ~25 KB per 500 kb HiFi chunk, one dependent load each) and leaves a 40-byte descriptor per record;
//   lcd_bam_stat_kernel   one wavefront per record of the wanted reference: reference span (bam_endpos), digar / window-event capacities of its CIGAR (the counts
//                         lcd_digar_batch's host pass makes), the CG:B,I tag behind the placeholder CIGAR of a read with more than 65 535 operations;
//   lcd_bam_aux_kernel    one wavefront per kept record: the digar source the reference would choose for it (EQX CIGAR / cs / MD / reference comparison), where
//                         its cs / MD value lies, and the SA tag's palindrome test of ONT reads;
//   lcd_bam_nm_kernel     one lane per kept record: the value of its first NM field (bam_get_NM, src/bam_utils.c:1632-1639), a key of the chunk's read order;
//   lcd_bam_cigar_kernel  the kept records' CIGAR words -> a 4-byte aligned pool (records sit at any byte offset of the stream);
//   lcd_errrate_kernel    calc_read_error_rate (src/seq.c:429-436) of a read slice on the qualities in HBM: the same table values added in the same order as the
//                         host loop, so the doubles are the host's.
// Bases and qualities are not moved at all: the digar kernel and the unpack kernel read them where the inflate left them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lcd_types.h"
#include "lcd_kernels.h"
#include "bam_aux_hop.h"

namespace {
// four bytes at any alignment from two aligned words (the stream buffer is padded: the second word may lie behind its end)
__device__ __forceinline__ unsigned ld32u(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const unsigned *q = (const unsigned *)(a & ~(uintptr_t)3);
    const unsigned lo = q[0], hi = q[1];
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(a & 3));
}
__device__ __forceinline__ long long wave_sum(long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)v, d, 64), hi = __shfl_xor((int)(v >> 32), d, 64);
        v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}
} // namespace

__global__ void __launch_bounds__(64) lcd_bam_walk_kernel(const BamWalkJob *jobs, BamWalkOut *outs) {
    if (threadIdx.x) return;
    const BamWalkJob j = jobs[blockIdx.x];
    const uint8_t *s = (const uint8_t *)(uintptr_t)j.stream;
    BamRecDesc *d = (BamRecDesc *)(uintptr_t)j.descs;
    uint64_t o = j.ubeg;
    int n = 0, status = 0;
    while (o < j.uend) {
        if (o + 4 > j.usize) break;                                  // end of the file
        const int bs = (int)ld32u(s + o);
        if (bs < 32 || o + 4 + (uint64_t)bs > j.usize) { status = 1; break; } // truncated record
        const uint8_t *r = s + o + 4;
        const unsigned w2 = ld32u(r + 8), w3 = ld32u(r + 12);
        BamRecDesc x;
        x.off = o + 4; x.bs = bs; x.refid = (int)ld32u(r); x.pos = (int)ld32u(r + 4); x.lseq = (int)ld32u(r + 16);
        x.lname = (uint8_t)(w2 & 0xff); x.mapq = (uint8_t)((w2 >> 8) & 0xff); x.nc = (uint16_t)(w3 & 0xffff); x.flag = (uint16_t)(w3 >> 16); x.pad = 0; x.pad2 = 0;
        if (x.lseq < 0 || 32ull + x.lname + 4ull * x.nc + ((uint64_t)x.lseq + 1) / 2 + (uint64_t)x.lseq > (uint64_t)bs) { status = 2; break; } // a field runs past the record
        if (n >= j.cap) { status = 3; break; }
        d[n++] = x;
        if (x.refid == j.tid && (long long)x.pos >= j.reg_end) { status = 4; break; } // sorted input: nothing further overlaps (this record is kept in the list: the loader's checks see it)
        o += 4 + (uint64_t)bs;
    }
    BamWalkOut w; w.n = n; w.status = status; w.next = o; outs[blockIdx.x] = w;
}

// the operations of the record's CIGAR, or of its CG tag when the 16-bit field holds the placeholder `<l_seq>S<ref_len>N`
__global__ void __launch_bounds__(64) lcd_bam_stat_kernel(const BamStatJob *jobs, BamStatOut *outs, const int n_jobs) {
    const int jb = blockIdx.x;
    if (jb >= n_jobs) return;
    const BamStatJob j = jobs[jb];
    const int lane = threadIdx.x;
    const uint8_t *r = (const uint8_t *)(uintptr_t)j.rec;
    const uint8_t *cg = r + 32 + j.lname;
    int nc = j.nc, kind = 0;
    if (lcd_aux::cg_ops(r, (unsigned)j.lname, nc, j.lseq, j.bs, lane, &cg, &nc)) kind = 1;
    long long rl = 0, nd = 0, nev = 0, nid = 0;
    if (kind >= 0)
        for (int k = lane; k < nc; k += 64) {
            const unsigned c = ld32u(cg + 4 * (size_t)k); const int op = (int)(c & 0xf); const long long len = (long long)(c >> 4);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += len;            // bam_cigar2rlen
            if (op == 8) { nd += len; nev += len; } else if (op != 3 && op != 9) { ++nd; if (op == 1 || op == 2) { ++nev; ++nid; } } // (lcd_digar_batch's capacity pass)
        }
    rl = wave_sum(rl); nd = wave_sum(nd); nev = wave_sum(nev); nid = wave_sum(nid);
    if (lane == 0) { BamStatOut o; o.rl = rl; o.nd = nd; o.nev = nev; o.nid = nid; o.cig_src = (uint64_t)(uintptr_t)cg; o.nc = nc; o.kind = kind; outs[jb] = o; }
}

__global__ void __launch_bounds__(64) lcd_bam_cigar_kernel(const GatherJob *jobs, const int n_jobs) { // bytes = 4 x operations; dst 4-byte aligned, src anywhere
    const int jb = blockIdx.x;
    if (jb >= n_jobs) return;
    const GatherJob g = jobs[jb];
    const uint8_t *src = (const uint8_t *)(uintptr_t)g.src; unsigned *dst = (unsigned *)(uintptr_t)g.dst;
    const unsigned nw = g.bytes >> 2;
    for (unsigned k = threadIdx.x; k < nw; k += 64) dst[k] = ld32u(src + 4 * (size_t)k);
}

// ---- lcd_bam_aux_kernel: which of the reference's four digar sources a kept record gets (collect_digar_from_bam, src/collect_var.c:1072-1079), where its cs / MD
// value lies, and is_ont_palindrome_clip (src/bam_utils.c:642-698) on its SA tag.  One wavefront per record.  The auxiliary fields are hopped as bam_aux_get does:
// a field that runs past the record ends the walk, and what lies behind it does not exist.  Every lane walks the same fields (the loads are wave-uniform); the NUL
// search of a Z / H value is cooperative -- cs strings of long reads run to hundreds of kilobytes -- and bounded by the record's end. ----
namespace {
// offset of the first NUL in [p, end), or -1: four independent byte loads per lane and step, one ballot of 64 bytes each
__device__ __forceinline__ long long wave_find_nul(const uint8_t *p, const uint8_t *end, const int lane) {
    const long long n = end - p;
    for (long long k = 0; k < n; k += 256) {
        unsigned b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const long long i = k + 64 * u + lane; b[u] = i < n ? p[i] : 1u; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const unsigned long long m = __ballot(b[u] == 0); if (m) return k + 64 * u + (__ffsll((long long)m) - 1); }
    }
    return -1;
}
__device__ __forceinline__ bool is_dig(const uint8_t c) { return c >= '0' && c <= '9'; }
// the SA value s[0, n): entries between ';' (empty ones skipped), each `rname,pos,strand,cigar[,...]` with a non-empty rname and cigar, a decimal pos (one optional
// sign) and a one-character strand -- an entry that does not give these four is skipped (the reference's sscanf leaves its variables unset there).  sa_end = pos +
// the lengths of the M / D / = / X operations (an operation letter without digits counts 0); check_ont_palindrome's four overlap cases; any entry decides.
__device__ int sa_is_palindrome(const uint8_t *s, const int n, const long long prim_pos, const long long prim_end) {
    const long long prim_len = prim_end - prim_pos + 1;
    int i = 0;
    while (i < n) {
        int e = i; while (e < n && s[e] != ';') ++e;
        int p = i;                                                     // the entry is s[i, e)
        i = e + 1;
        const int r0 = p; while (p < e && s[p] != ',') ++p;
        if (p == r0 || p >= e) continue;                               // rname
        ++p;
        bool neg = false;
        if (p < e && (s[p] == '-' || s[p] == '+')) { neg = s[p] == '-'; ++p; }
        const int d0 = p; long long pos = 0;
        while (p < e && is_dig(s[p])) { pos = pos * 10 + (s[p] - '0'); if (pos > 2147483647ll) pos = 2147483647ll; ++p; }
        if (p == d0 || p >= e || s[p] != ',') continue;                // pos
        if (neg) pos = -pos;
        ++p;
        if (p + 1 >= e || s[p + 1] != ',') continue;                   // strand
        p += 2;
        int ce = p; while (ce < e && s[ce] != ',') ++ce;
        if (ce == p) continue;                                         // cigar
        long long sa_end = pos;
        while (p < ce) {
            long long len = 0;
            while (p < ce && is_dig(s[p])) { len = len * 10 + (s[p] - '0'); if (len > 2147483647ll) len = 2147483647ll; ++p; }
            if (p >= ce) break;
            const uint8_t c = s[p++];
            if (c == 'M' || c == 'D' || c == '=' || c == 'X') sa_end += len;
        }
        const long long sa_len = sa_end - pos + 1;
        long long ov = 0;                                              // check_ont_palindrome (src/bam_utils.c:642-654)
        if (pos <= prim_pos) { if (sa_end >= prim_end) ov = prim_len; else if (sa_end >= prim_pos) ov = sa_end - prim_pos + 1; }
        else if (pos <= prim_end) { if (sa_end >= prim_end) ov = prim_end - pos + 1; else ov = sa_len; }
        if ((double)ov >= (double)prim_len * 0.9) return 1;
    }
    return 0;
}
} // namespace
__global__ void __launch_bounds__(64) lcd_bam_aux_kernel(const BamAuxJob *jobs, BamAuxOut *outs, const int is_ont, const int n_jobs) {
    const int jb = blockIdx.x;
    if (jb >= n_jobs) return;
    const BamAuxJob j = jobs[jb];
    const int lane = threadIdx.x;
    const uint8_t *r = (const uint8_t *)(uintptr_t)j.rec, *cig = (const uint8_t *)(uintptr_t)j.cig;
    // has_equal_X_in_bam_cigar (src/bam_utils.c:51-66): the first of '=' / 'X' / 'M' decides
    bool eqx = false;
    for (int c0 = 0; c0 < j.nc; c0 += 64) {
        const int k = c0 + lane;
        const int op = k < j.nc ? (int)(ld32u(cig + 4 * (size_t)k) & 0xf) : -1;
        const unsigned long long m = __ballot(op == 0 || op == 7 || op == 8);
        if (m) { eqx = __shfl(op, __ffsll((long long)m) - 1) != 0; break; }
    }
    long long cig_qlen = 0;
    if (!eqx) {
        for (int k = lane; k < j.nc; k += 64) { const unsigned c = ld32u(cig + 4 * (size_t)k); const int op = (int)(c & 0xf); if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) cig_qlen += (long long)(c >> 4); }
        cig_qlen = wave_sum(cig_qlen);
    }
    const uint8_t *v_cs = nullptr, *v_md = nullptr, *v_sa = nullptr; long long l_cs = 0, l_md = 0, l_sa = 0; uint8_t t_cs = 0, t_md = 0, t_sa = 0; // the first cs / MD / SA field: value, strlen, type
    if (!eqx || is_ont) {
        const uint8_t *aux = r + 32 + j.lname + 4 * (size_t)j.nc16 + ((size_t)j.lseq + 1) / 2 + (size_t)j.lseq, *end = r + j.bs;
        while (aux + 3 <= end) {
            const uint8_t t0 = aux[0], t1 = aux[1], ty = aux[2]; aux += 3;
            size_t sz = 0; bool bad = false; long long zl = 0;
            if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
            else if (ty == 's' || ty == 'S') sz = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
            else if (ty == 'Z' || ty == 'H') { zl = wave_find_nul(aux, end, lane); if (zl < 0) bad = true; else sz = (size_t)zl + 1; }
            else if (ty == 'B') {
                if (aux + 5 > end) bad = true;
                else {
                    const uint8_t sub = aux[0]; const unsigned cnt = ld32u(aux + 1);
                    const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                    if (!es || (size_t)(end - (aux + 5)) < (size_t)cnt * es) bad = true;
                    else sz = 5 + (size_t)cnt * es;
                }
            } else bad = true;
            if (bad || (size_t)(end - aux) < sz) break;
            if (t0 == 'c' && t1 == 's') { if (!t_cs) { t_cs = ty; v_cs = aux; l_cs = zl; } }
            else if (t0 == 'M' && t1 == 'D') { if (!t_md) { t_md = ty; v_md = aux; l_md = zl; } }
            else if (t0 == 'S' && t1 == 'A') { if (!t_sa) { t_sa = ty; v_sa = aux; l_sa = zl; } }
            if ((eqx || t_cs) && (!is_ont || t_sa)) break;      // nothing a later field could change
            aux += sz;
        }
    }
    const int source = eqx ? 0 : t_cs ? 1 : t_md ? 2 : 3;
    int pal = 0;
    if (is_ont && t_sa == 'Z') {
        if (lane == 0) pal = sa_is_palindrome(v_sa, (int)l_sa, j.prim_pos, j.prim_end);
        pal = __builtin_amdgcn_readfirstlane(pal);
    }
    if (lane == 0) {
        BamAuxOut o; o.tag = 0; o.tag_len = 0; o.source = (uint8_t)source; o.pal = (uint8_t)(pal ? ((j.flag & 16) ? 1 : 2) : 0); o.bad_type = 0; o.pad = 0; o.cig_qlen = cig_qlen;
        if (source == 1 || source == 2) {
            if ((source == 1 ? t_cs : t_md) != 'Z') o.bad_type = 1;
            else { o.tag = (uint64_t)(uintptr_t)(source == 1 ? v_cs : v_md); o.tag_len = (uint32_t)(source == 1 ? l_cs : l_md); }
        }
        outs[jb] = o;
    }
}

// ---- lcd_bam_nm_kernel: bam_get_NM (src/bam_utils.c:1632-1639) of a kept record, the third key of sort_chunk_reads (:1641).  One lane per record: tens of fields,
// about 1 000 records per chunk.  The fields are hopped exactly as lcd_bam_aux_kernel hops them -- a field that runs past the record ends the walk and what lies
// behind it does not exist -- and the first field named NM decides: types c C s S i I give their value (an I above 2^31 - 1 wraps, as the reference's int does),
// any other type gives 0 (bam_aux2i), no NM field gives 0. ----
namespace {
// offset of the first NUL in [p, end), or -1, one lane: aligned words (the stream buffer is padded behind its end), the bytes in front of p masked out
__device__ __forceinline__ long long lane_find_nul(const uint8_t *p, const uint8_t *end) {
    if (p >= end) return -1;
    const uintptr_t a = (uintptr_t)p;
    const unsigned *q = (const unsigned *)(a & ~(uintptr_t)3);
    const long long n = end - p;
    long long at = -(long long)(a & 3);                    // offset (relative to p) of the word's first byte
    unsigned w = *q | ((1u << (8 * (unsigned)(a & 3))) - 1u);   // (a & 3) low bytes forced non-zero
    for (;;) {
        const unsigned z = (w - 0x01010101u) & ~w & 0x80808080u;   // the lowest set bit marks the first zero byte
        if (z) { const long long i = at + ((__ffs((int)z) - 1) >> 3); return i < n ? i : -1; }
        at += 4;
        if (at >= n) return -1;
        w = *++q;
    }
}
} // namespace
__global__ void __launch_bounds__(64) lcd_bam_nm_kernel(const BamNmJob *jobs, int *nm, const int n_jobs) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_jobs) return;
    const BamNmJob j = jobs[i];
    const uint8_t *aux = (const uint8_t *)(uintptr_t)j.aux, *end = (const uint8_t *)(uintptr_t)j.end;
    int v = 0;
    while (aux + 3 <= end) {
        const unsigned h = ld32u(aux);
        const uint8_t t0 = (uint8_t)(h & 0xff), t1 = (uint8_t)((h >> 8) & 0xff), ty = (uint8_t)((h >> 16) & 0xff); aux += 3;
        size_t sz = 0; bool bad = false;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') { const long long zl = lane_find_nul(aux, end); if (zl < 0) bad = true; else sz = (size_t)zl + 1; }
        else if (ty == 'B') {
            if (aux + 5 > end) bad = true;
            else {
                const uint8_t sub = aux[0]; const unsigned cnt = ld32u(aux + 1);
                const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (!es || (size_t)(end - (aux + 5)) < (size_t)cnt * es) bad = true;
                else sz = 5 + (size_t)cnt * es;
            }
        } else bad = true;
        if (bad || (size_t)(end - aux) < sz) break;
        if (t0 == 'N' && t1 == 'M') {
            const unsigned w = ld32u(aux);
            if (ty == 'c') v = (int)(signed char)(w & 0xff);
            else if (ty == 'C') v = (int)(w & 0xff);
            else if (ty == 's') v = (int)(short)(w & 0xffff);
            else if (ty == 'S') v = (int)(w & 0xffff);
            else if (ty == 'i' || ty == 'I') v = (int)w;
            break;
        }
        aux += sz;
    }
    nm[i] = v;
}

// e = sum over the slice of 10^(-q / 10), in slice order, divided by the length: tab[q] is the host's pow(10.0, -q / 10.0)
__global__ void __launch_bounds__(64) lcd_errrate_kernel(const ErrJob *jobs, const double *tab, double *out, const int n_jobs) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_jobs) return;
    const ErrJob j = jobs[i];
    if (j.len <= 0) { out[i] = 0.0; return; }
    const uint8_t *q = (const uint8_t *)(uintptr_t)j.qual;
    double e = 0.0;
    int k = 0;
    for (; k < j.len && (((uintptr_t)(q + k)) & 3); ++k) e += tab[q[k]];
    for (; k + 4 <= j.len; k += 4) { const unsigned w = *(const unsigned *)(q + k); e += tab[w & 0xff]; e += tab[(w >> 8) & 0xff]; e += tab[(w >> 16) & 0xff]; e += tab[w >> 24]; }
    for (; k < j.len; ++k) e += tab[q[k]];
    out[i] = e / j.len;
}

void lcd_launch_bam_walk(const BamWalkJob *jobs, BamWalkOut *outs, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_walk_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs); }
void lcd_launch_bam_stat(const BamStatJob *jobs, BamStatOut *outs, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_stat_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs, n_jobs); }
void lcd_launch_bam_cigar(const GatherJob *jobs, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_cigar_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, n_jobs); }
void lcd_launch_bam_aux(const BamAuxJob *jobs, BamAuxOut *outs, int is_ont, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_aux_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, outs, is_ont, n_jobs); }
void lcd_launch_bam_nm(const BamNmJob *jobs, int *nm, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_bam_nm_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, st, jobs, nm, n_jobs); }
void lcd_launch_errrate(const ErrJob *jobs, const double *tab, double *out, int n_jobs, hipStream_t st) { if (n_jobs > 0) hipLaunchKernelGGL(lcd_errrate_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, st, jobs, tab, out, n_jobs); }
