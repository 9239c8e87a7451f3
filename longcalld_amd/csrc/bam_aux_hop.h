// bam_aux_hop.h -- what the kernels that hop a record's auxiliary fields share (bam_tag_kernel.hip, bam_refine_kernel.hip, bam_sam_kernel.hip, mods_kernel.hip): the NUL search of a Z / H value,
// a field's value size with the walk's stop rule, and bam_aux2i by the project's documented rule (types c C s S i I give their value, any other type 0).
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
} // namespace lcd_aux
