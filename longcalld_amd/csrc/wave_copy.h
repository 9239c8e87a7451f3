// wave_copy.h -- n bytes from any byte offset to any byte offset by one wavefront: the destination is brought to a 4-byte boundary by single bytes, the body
// goes as coalesced dword stores whose source words are assembled from two aligned loads, the rest as single bytes.  The SOURCE buffer must be readable for 8
// bytes behind src + n (the library's stream buffers are padded by at least that much).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd_wave {
__device__ __forceinline__ unsigned ld32u(const uint8_t *p) { // four bytes at any alignment
    const uintptr_t a = (uintptr_t)p;
    const unsigned *q = (const unsigned *)(a & ~(uintptr_t)3);
    const unsigned lo = q[0], hi = q[1];
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(a & 3));
}
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, const long long n, const int lane) {
    if (n <= 0) return;
    long long h = (long long)((4 - ((uintptr_t)dst & 3)) & 3);
    if (h > n) h = n;
    if (lane < h) dst[lane] = src[lane];
    const long long nw = (n - h) >> 2;
    unsigned *d32 = (unsigned *)(dst + h);
    const uint8_t *s = src + h;
    for (long long k = lane; k < nw; k += 64) d32[k] = ld32u(s + 4 * k);
    const long long t = (n - h) & 3, o = h + 4 * nw;
    if (lane < t) dst[o + lane] = src[o + lane];
}
} // namespace lcd_wave
