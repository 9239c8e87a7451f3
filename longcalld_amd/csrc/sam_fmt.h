// sam_fmt.h -- the number formatters of the SAM text output (bam_sam_kernel.hip), as host + device code without a library call, so that the same text compiles into
// the kernel and into a CPU program that compares it with printf (tests/c/sam_float_check.cpp):
//   len_u / len_i / put_u / put_i    decimal integers;
//   fmt_g                            the text of a 32-bit float exactly as glibc's printf("%g", (double)x) prints it: 6 significant digits, rounded half-to-even on
//                                    the EXACT value, exponent form below 1e-4 or from 1e6, trailing zeros stripped, e+06 style exponents, -0, inf, -inf, nan, -nan.
// A float is m * 2^e with m < 2^24 and e in [-149, 104].  e >= 0: N = m << e (at most 128 bits), the value is N.  e < 0: N = m * 5^-e (at most 370 bits), the value
// is N * 10^e.  N lives in twelve 32-bit words; it is divided by 10^9 until nothing is left, and only the two highest base-10^9 limbs and whether any lower one is
// non-zero are kept: they hold the six digits, the digit behind them and the sticky bit the rounding needs.  No double is involved: its 53 bits get ties wrong.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LCD_SAM_HD __host__ __device__ inline
#else
#define LCD_SAM_HD inline
#endif

namespace sam_fmt {

LCD_SAM_HD int len_u(uint32_t v) { int n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
LCD_SAM_HD int len_u64(uint64_t v) { int n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
LCD_SAM_HD int len_i(long long v) { return v < 0 ? 1 + len_u64(0ull - (uint64_t)v) : len_u64((uint64_t)v); }
LCD_SAM_HD uint64_t pow10_u64(int k) { uint64_t p = 1; while (k-- > 0) p *= 10u; return p; }
// byte k (0 = first) of the decimal text of v, whose length is n = len_i(v): what lane k of a wavefront writes
LCD_SAM_HD char char_i(long long v, int n, int k) {
    if (v < 0) { if (k == 0) return '-'; return (char)('0' + (int)(((0ull - (uint64_t)v) / pow10_u64(n - 1 - k)) % 10u)); }
    return (char)('0' + (int)(((uint64_t)v / pow10_u64(n - 1 - k)) % 10u));
}
template <class Out> LCD_SAM_HD int put_u(Out out, uint32_t v) {
    const int n = len_u(v);
    for (int k = n - 1; k >= 0; --k) { out[k] = (char)('0' + v % 10u); v /= 10u; }
    return n;
}
template <class Out> LCD_SAM_HD int put_i(Out out, long long v) {
    const int n = len_i(v);
    for (int k = 0; k < n; ++k) out[k] = char_i(v, n, k);
    return n;
}

// at most 16 characters in two registers: filled front to back, read by index without an array in memory
struct Txt16 {
    uint64_t lo, hi; int n;
    LCD_SAM_HD void push(char c) {
        const uint64_t b = (uint64_t)(uint8_t)c;
        if (n < 8) lo |= b << (8 * n); else if (n < 16) hi |= b << (8 * (n - 8));
        ++n;
    }
    LCD_SAM_HD char at(int k) const { return (char)(uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xffu); }
};

LCD_SAM_HD Txt16 fmt_g(const uint32_t bits) {
    Txt16 t; t.lo = t.hi = 0; t.n = 0;
    const uint32_t ex = (bits >> 23) & 0xffu, fr = bits & 0x7fffffu;
    if (bits >> 31) t.push('-');
    if (ex == 255u) {
        if (fr) { t.push('n'); t.push('a'); t.push('n'); } else { t.push('i'); t.push('n'); t.push('f'); }
        return t;
    }
    if (ex == 0u && fr == 0u) { t.push('0'); return t; }
    const uint32_t m = ex ? (fr | 0x800000u) : fr;
    const int e = ex ? (int)ex - 150 : -149;
    // ---- N: twelve words, least significant first ----
    uint32_t w[12];
    int scale10 = 0;
    if (e >= 0) {
        const int wi = e >> 5, sh = e & 31;
        const uint64_t x = (uint64_t)m << sh;
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j] = j == wi ? (uint32_t)x : j == wi + 1 ? (uint32_t)(x >> 32) : 0u;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j] = j == 0 ? m : 0u;
        int k = -e;
        scale10 = e;
        while (k > 0) {
            const int step = k >= 13 ? 13 : k;
            uint32_t f = 1; for (int q = 0; q < step; ++q) f *= 5u;          // 5^13 = 1 220 703 125 < 2^32
            uint64_t carry = 0;
#pragma unroll
            for (int j = 0; j < 12; ++j) { const uint64_t p = (uint64_t)w[j] * f + carry; w[j] = (uint32_t)p; carry = p >> 32; }
            k -= step;
        }
    }
    // ---- the base-10^9 limbs from the lowest up: a = the latest, b = the one before, sticky = any older one non-zero ----
    uint32_t a = 0, b = 0; bool sticky = false; int n_limbs = 0;
    for (;;) {
        uint64_t r = 0; uint32_t any = 0;
#pragma unroll
        for (int j = 11; j >= 0; --j) { const uint64_t cur = (r << 32) | w[j]; const uint64_t q = cur / 1000000000u; r = cur - q * 1000000000u; w[j] = (uint32_t)q; any |= w[j]; }
        if (n_limbs >= 2 && b) sticky = true;
        b = a; a = (uint32_t)r; ++n_limbs;
        if (!any) break;
    }
    // ---- six digits, half to even on the exact value ----
    uint64_t lead = a; int nd = len_u(a); bool low = sticky;
    const int D0 = 9 * (n_limbs - 1) + nd;                                 // digits of N
    if (n_limbs >= 2) { lead = (uint64_t)a * 1000000000u + b; nd += 9; }
    uint32_t q6; int D = D0;
    if (nd <= 6) q6 = (uint32_t)(lead * pow10_u64(6 - nd));
    else {
        const uint64_t p = pow10_u64(nd - 6), q = lead / p, r = lead - q * p, half = p >> 1;
        q6 = (uint32_t)q;
        if (r > half || (r == half && (low || (q6 & 1u)))) ++q6;
        if (q6 == 1000000u) { q6 = 100000u; ++D; }
    }
    const int X = D - 1 + scale10;                                         // the decimal exponent of the first digit
    int nsig = 6; { uint32_t z = q6; while (nsig > 1 && z % 10u == 0u) { z /= 10u; --nsig; } }
    auto dig = [&](int k) -> char { return (char)('0' + (int)((q6 / (uint32_t)pow10_u64(5 - k)) % 10u)); };
    if (X < -4 || X >= 6) {
        t.push(dig(0));
        if (nsig > 1) { t.push('.'); for (int k = 1; k < nsig; ++k) t.push(dig(k)); }
        t.push('e'); t.push(X < 0 ? '-' : '+');
        const int ax = X < 0 ? -X : X;
        t.push((char)('0' + ax / 10)); t.push((char)('0' + ax % 10));
    } else if (X >= 0) {
        for (int k = 0; k <= X; ++k) t.push(dig(k));
        if (nsig > X + 1) { t.push('.'); for (int k = X + 1; k < nsig; ++k) t.push(dig(k)); }
    } else {
        t.push('0'); t.push('.');
        for (int k = 0; k < -X - 1; ++k) t.push('0');
        for (int k = 0; k < nsig; ++k) t.push(dig(k));
    }
    return t;
}
// the same text into a character buffer of at least 16 bytes (no terminator); returns its length
template <class Out> LCD_SAM_HD int put_g(Out out, const uint32_t bits) {
    const Txt16 t = fmt_g(bits);
    for (int k = 0; k < t.n; ++k) out[k] = t.at(k);
    return t.n;
}

} // namespace sam_fmt
