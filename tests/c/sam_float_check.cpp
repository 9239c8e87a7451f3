// sam_float_check.cpp -- longcalld_amd/csrc/sam_fmt.h against the C library on the CPU: fmt_g against snprintf("%g", (double)x), the integer formatters against
// snprintf("%lld").  A program of its own (tests/test_sam_float.py builds it with -fsanitize=address,undefined and runs it); `sam_float_check full [threads]` sweeps
// all 2^32 bit patterns (built without the sanitizers, by hand: the result stands in profiles/NOTES_sam_out.md).
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "sam_fmt.h"

static std::atomic<long long> g_bad{0}, g_n{0};

static bool check_bits(uint32_t bits) {
    float x; memcpy(&x, &bits, 4);
    char want[64], got[32];
    snprintf(want, sizeof(want), "%g", (double)x);
    const int n = sam_fmt::put_g(got, bits);
    got[n] = 0;
    ++g_n;
    if (n > 16 || strcmp(want, got) != 0) {
        if (g_bad++ < 20) fprintf(stderr, "fmt_g(0x%08x): \"%s\", printf gives \"%s\"\n", bits, got, want);
        return false;
    }
    return true;
}
static void check_int(long long v) {
    char want[64], got[32];
    snprintf(want, sizeof(want), "%lld", v);
    int n = sam_fmt::put_i(got, v); got[n] = 0;
    ++g_n;
    if (strcmp(want, got) != 0 || n != sam_fmt::len_i(v)) { if (g_bad++ < 20) fprintf(stderr, "put_i(%lld): \"%s\"\n", v, got); }
    for (int k = 0; k < n; ++k) if (sam_fmt::char_i(v, n, k) != want[k]) { if (g_bad++ < 20) fprintf(stderr, "char_i(%lld, %d)\n", v, k); }
    if (v >= 0 && v <= 0xffffffffll) {
        n = sam_fmt::put_u(got, (uint32_t)v); got[n] = 0;
        if (strcmp(want, got) != 0 || n != sam_fmt::len_u((uint32_t)v)) { if (g_bad++ < 20) fprintf(stderr, "put_u(%lld): \"%s\"\n", v, got); }
    }
}
static uint32_t bits_of(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "full")) {
        const int nt = argc > 2 ? atoi(argv[2]) : 8;
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t)
            th.emplace_back([t, nt]() { for (uint64_t b = (uint64_t)t; b < (1ull << 32); b += (uint64_t)nt) check_bits((uint32_t)b); });
        for (auto &x : th) x.join();
        printf("full sweep: %lld values, %lld differences\n", (long long)g_n, (long long)g_bad);
        return g_bad ? 1 : 0;
    }
    // every 1021st bit pattern
    for (uint64_t b = 0; b < (1ull << 32); b += 1021) check_bits((uint32_t)b);
    // for each sign and exponent, the 1024 lowest and highest mantissas
    for (uint32_t s = 0; s < 2; ++s)
        for (uint32_t ex = 0; ex < 256; ++ex)
            for (uint32_t k = 0; k < 1024; ++k) { check_bits((s << 31) | (ex << 23) | k); check_bits((s << 31) | (ex << 23) | (0x7fffffu - k)); }
    // the floats within 3 ulps of d * 10^k
    const double ds[4] = {1.0, 9.999994, 9.999995, 9.999996};
    for (int k = -45; k <= 38; ++k)
        for (const double d : ds) {
            const double v = d * pow(10.0, k);
            const float f = (float)v;                                     // (inf behind FLT_MAX: the bit patterns below it are walked all the same)
            const uint32_t c = bits_of(f);
            for (int u = -3; u <= 3; ++u) {
                const long long bb = (long long)c + u;
                if (bb < 0 || bb > 0x7fffffffll) continue;
                check_bits((uint32_t)bb); check_bits((uint32_t)bb | 0x80000000u);
            }
        }
    const uint32_t named[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x00000001u, 0x80000001u,
                              0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu, 0x3f800000u, 0x49742400u /* 1e6 */, 0x497423f0u /* 999999 */, 0x38d1b717u /* 1e-4 */};
    for (const uint32_t b : named) check_bits(b);
    // the integer formatters on each side of every digit-count step
    check_int(0);
    for (long long p = 10; p <= 10000000000ll; p *= 10) { check_int(p - 1); check_int(p); check_int(-(p - 1)); check_int(-p); }
    check_int(INT32_MIN); check_int(INT32_MAX); check_int(UINT32_MAX); check_int((long long)INT32_MAX + 1); check_int(-129); check_int(-128); check_int(32767); check_int(-32768);
    printf("%lld values, %lld differences\n", (long long)g_n, (long long)g_bad);
    return g_bad ? 1 : 0;
}
