// bam_aux_hop.h -- what the kernels that hop a record's auxiliary fields share (bam_tag_kernel.hip, bam_refine_kernel.hip, bam_sam_kernel.hip, mods_kernel.hip, bam_kernel.hip, depth_kernel.hip): the NUL search of a Z / H value,
// a field's value size with the walk's stop rule, bam_aux2i by the project's documented rule (types c C s S i I give their value, any other type 0), and the
// rule that reads a record with its CG field's operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_copy.h"

namespace lcd_aux {
// offset of the first NUL in [p, end), or -1, one lane: aligned words (the stream buffer is padded behind its end), the bytes in front of p masked out
__device__ __forceinline__ long long lane_find_nul(const uint8_t *p, const uint8_t *end) {
    if (p >= end) return -1;
    const uintptr_t a = (uintptr_t)p;
    const unsigned *q = (const unsigned *)(a & ~(uintptr_t)3);
    const long long n = end - p;
    long long at = -(long long)(a & 3);
    unsigned w = *q | ((1u << (8 * (unsigned)(a & 3))) - 1u);
    for (;;) {                                                            // ends at the record's end at the latest
        const unsigned z = (w - 0x01010101u) & ~w & 0x80808080u;
        if (z) { const long long i = at + ((__ffs((int)z) - 1) >> 3); return i < n ? i : -1; }
        at += 4;
        if (at >= n) return -1;
        w = *++q;
    }
}
__device__ __forceinline__ long long aux2i(const uint8_t ty, const unsigned w) {
    if (ty == 'c') return (long long)(signed char)(w & 0xff);
    if (ty == 'C') return (long long)(w & 0xff);
    if (ty == 's') return (long long)(short)(w & 0xffff);
    if (ty == 'S') return (long long)(w & 0xffff);
    if (ty == 'i') return (long long)(int)w;
    if (ty == 'I') return (long long)w;
    return 0;
}
// the size of the value of a field of type ty whose value starts at v; false: the field runs past `end` or its type is unknown (the walk ends there, what lies
// behind it does not exist)
__device__ __forceinline__ bool value_size(const uint8_t ty, const uint8_t *v, const uint8_t *end, size_t *size) {
    size_t sz = 0;
    if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
    else if (ty == 's' || ty == 'S') sz = 2;
    else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
    else if (ty == 'Z' || ty == 'H') { const long long zl = lane_find_nul(v, end); if (zl < 0) return false; sz = (size_t)zl + 1; }
    else if (ty == 'B') {
        if (v + 5 > end) return false;
        const uint8_t sub = v[0]; const unsigned cnt = lcd_wave::ld32u(v + 1);
        const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
        if (!es || (size_t)(end - (v + 5)) < (size_t)cnt * es) return false;
        sz = 5 + (size_t)cnt * es;
    } else return false;
    if ((size_t)(end - v) < sz) return false;
    *size = sz;
    return true;
}
// The operations a record is read with (lcd_bam_stat_kernel, lcd_depth_mark_kernel): its own CIGAR, or its CG field's.  htslib's bam_tag2cigar (behind the
// reference's sam_itr_next): a record with a reference and a position whose FIRST operation is `<l_seq>S` may carry its real operations in a CG:B,I (or B,i) tag
// with at least n_cigar and fewer than 2^29 entries; anything else -- no tag, another type, a shorter array, a broken auxiliary field -- leaves the record's own
// CIGAR in place, silently.  r: the record behind its block_size word, bs: that word; nc / lname / lseq: its n_cigar_op, l_read_name, l_seq.  One wavefront:
// lane 0 hops the fields one after the other.  true: *ops / *n_ops are the field's (inside the record), else they are left as they were
__device__ __forceinline__ bool cg_ops(const uint8_t *r, const unsigned lname, const int nc, const int lseq, const int bs, const int lane, const uint8_t **ops, int *n_ops) {
    const uint8_t *cg = r + 32 + lname;
    if (!(nc >= 1 && (int)lcd_wave::ld32u(r) >= 0 && (int)lcd_wave::ld32u(r + 4) >= 0)) return false;
    const unsigned c0 = lcd_wave::ld32u(cg);
    if (!((c0 & 0xf) == 4 && (int)(c0 >> 4) == lseq)) return false;
    unsigned long long found = 0; unsigned cnt_found = 0;
    if (lane == 0) { // the auxiliary fields, one after the other
        const uint8_t *aux = cg + 4 * (size_t)nc + ((size_t)lseq + 1) / 2 + (size_t)lseq, *end = r + bs;
        while (aux + 3 <= end) {
            const uint8_t t0 = aux[0], t1 = aux[1], ty = aux[2]; aux += 3;
            size_t sz = 0; bool bad = false;
            if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
            else if (ty == 's' || ty == 'S') sz = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
            else if (ty == 'Z' || ty == 'H') { const uint8_t *q = aux; while (q < end && *q) ++q; if (q >= end) bad = true; else sz = (size_t)(q - aux) + 1; }
            else if (ty == 'B') {
                if (aux + 5 > end) bad = true;
                else {
                    const uint8_t sub = aux[0]; const unsigned cnt = lcd_wave::ld32u(aux + 1);
                    const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                    if (!es || (size_t)(end - (aux + 5)) < (size_t)cnt * es) bad = true;
                    else if (t0 == 'C' && t1 == 'G') { if ((sub == 'I' || sub == 'i') && cnt >= (unsigned)nc && cnt < (1u << 29)) { found = (unsigned long long)(uintptr_t)(aux + 5); cnt_found = cnt; } break; } // (bam_aux_get: the first CG tag decides)
                    else sz = 5 + (size_t)cnt * es;
                }
            } else bad = true;
            if (t0 == 'C' && t1 == 'G') break; // a CG tag of another type: not a CIGAR
            if (bad || (size_t)(end - aux) < sz) break;
            aux += sz;
        }
    }
    found = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(found >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)found);
    cnt_found = (unsigned)__builtin_amdgcn_readfirstlane((int)cnt_found);
    if (!found) return false;
    *ops = (const uint8_t *)(uintptr_t)found; *n_ops = (int)cnt_found;
    return true;
}
} // namespace lcd_aux
