// crc32_gf2.h -- CRC-32 (RFC 1952) of a block by one wavefront, shared by inflate_kernel.hip (check) and deflate_kernel.hip (trailer): each lane takes a
// contiguous slice of the block through a byte table in LDS, the slices' CRCs are combined by multiplication with x^(8 * bytes behind the slice) mod P (the
// arithmetic of zlib's crc32_combine).  Every including file gets its own copy of the x^(2^k) table and fills it from the host once (lcd_crc_x2n_host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd_crc {
typedef unsigned crc_v4u __attribute__((ext_vector_type(4)));
typedef crc_v4u __attribute__((aligned(1))) crc_v4u_u;
typedef __attribute__((address_space(3))) unsigned crc_lds_u32;

// x^(2^k) mod P, k = 0..31 (bits, reflected representation): filled by the host once per including file
static __constant__ unsigned c_x2n[32];

__device__ __forceinline__ unsigned gf2_mulmod(unsigned a, unsigned b) { // a * b mod P, reflected CRC-32 polynomial
    unsigned m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
// the byte table (256 words of LDS at ct), by all lanes; the caller waits for the LDS writes before crc32_wave
__device__ __forceinline__ void crc32_fill_table(crc_lds_u32 *ct, const int lane) {
    for (int k = lane; k < 256; k += 64) { unsigned c = (unsigned)k; for (int b = 0; b < 8; ++b) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1; ct[k] = c; }
}
// CRC-32 of data[0, len): the same value in every lane
__device__ __forceinline__ unsigned crc32_wave(const uint8_t *data, const int len, const crc_lds_u32 *ct, const int lane) {
    const int per = ((len + 63) / 64 + 15) & ~15; // slice length: a multiple of 16 bytes
    const int b0 = lane * per < len ? lane * per : len, b1 = b0 + per < len ? b0 + per : len;
    unsigned c = 0xffffffffu;
    int k = b0;
    for (; k + 16 <= b1; k += 16) {
        const crc_v4u v = *(const crc_v4u_u *)(data + k);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned x = w[q];
#pragma unroll
            for (int b = 0; b < 4; ++b) { c = ct[(c ^ x) & 255] ^ (c >> 8); x >>= 8; }
        }
    }
    for (; k < b1; ++k) c = ct[(c ^ data[k]) & 255] ^ (c >> 8);
    c = b1 > b0 ? ~c : 0;
    // shift by the bytes behind this slice: c * x^(8 n) mod P
    unsigned n = (unsigned)(len - b1), p = 1u << 31; int kk = 3;
    while (n) { if (n & 1) p = gf2_mulmod(c_x2n[kk & 31], p); n >>= 1; ++kk; }
    c = b1 > b0 ? gf2_mulmod(p, c) : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c ^= __shfl_xor(c, o);
    return c;
}
} // namespace lcd_crc
