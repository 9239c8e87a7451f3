// TEST ONLY, host code: cs_to_words / md_to_words (longcalld_amd/csrc/tag_words.h) on truncated and garbage tag bytes, built with -fsanitize=address,undefined
// by tests/test_tag_words_sanitized.py and run on the CPU.  Every tag lies in a heap block of exactly strlen + 1 bytes and every CIGAR in one of exactly its
// words, so a read behind either is an error the sanitizer reports.  Prints the number of cases and how many parsed; exit 0.
#include <cstdio>
#include <string>
#include "../../longcalld_amd/csrc/tag_words.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static long n_cases = 0, n_ok = 0;
static void run(const std::vector<uint32_t> &cig, const std::string &tag, bool is_cs) {
    uint32_t *c = (uint32_t *)malloc(cig.size() * 4 + (cig.empty() ? 1 : 0));
    if (!cig.empty()) memcpy(c, cig.data(), cig.size() * 4);
    char *t = (char *)malloc(tag.size() + 1);
    memcpy(t, tag.c_str(), tag.size() + 1);
    std::vector<uint32_t> w;
    const bool ok = is_cs ? lcd_tag_words::cs_to_words(c, (int)cig.size(), t, w) : lcd_tag_words::md_to_words(c, (int)cig.size(), t, w);
    ++n_cases; n_ok += ok;
    free(c); free(t);
}

int main() {
    const char alphabet[] = ":*+-=~^0123456789acgtnACGTN!; \t";
    for (int it = 0; it < 3000; ++it) {
        // an alignment: = runs, X, I, D between optional clips; its M CIGAR, cs and MD strings
        std::vector<uint32_t> eqx, mc; std::string cs, md; long md_cnt = 0;
        auto push_m = [&](uint32_t len, uint32_t op) { const uint32_t o = (op == 7 || op == 8) ? 0 : op; if (!mc.empty() && o == 0 && (mc.back() & 0xf) == 0) mc.back() += len << 4; else mc.push_back((len << 4) | o); };
        if (rnd() % 3 == 0) { const uint32_t l = 1 + rnd() % 50, op = rnd() % 2 ? 4 : 5; eqx.push_back((l << 4) | op); push_m(l, op); }
        const int n_ev = (int)(rnd() % 12);
        for (int e = 0; e <= n_ev; ++e) {
            const uint32_t l = 1 + rnd() % 300; eqx.push_back((l << 4) | 7); push_m(l, 7); cs += ":" + std::to_string(l); md_cnt += l;
            if (e == n_ev) break;
            const uint32_t k = rnd() % 3, el = 1 + rnd() % 6;
            if (k == 0) { eqx.push_back((1u << 4) | 8); push_m(1, 8); cs += "*ac"; md += std::to_string(md_cnt) + "A"; md_cnt = 0; }
            else if (k == 1) { eqx.push_back((el << 4) | 1); push_m(el, 1); cs += "+" + std::string(el, 'g'); }
            else { eqx.push_back((el << 4) | 2); push_m(el, 2); cs += "-" + std::string(el, 't'); md += std::to_string(md_cnt) + "^" + std::string(el, 'T'); md_cnt = 0; }
        }
        md += std::to_string(md_cnt);
        if (rnd() % 3 == 0) { const uint32_t l = 1 + rnd() % 50; eqx.push_back((l << 4) | 4); push_m(l, 4); }
        run(mc, cs, true); run(eqx, cs, true); run(mc, md, false); run(eqx, md, false);
        // truncated at every length (short tags) or at random lengths, and with one byte replaced
        for (int k = 0; k < 24; ++k) {
            const size_t a = cs.size() <= 24 ? (size_t)k % (cs.size() + 1) : rnd() % (cs.size() + 1), b = md.size() <= 24 ? (size_t)k % (md.size() + 1) : rnd() % (md.size() + 1);
            run(mc, cs.substr(0, a), true); run(mc, md.substr(0, b), false);
            std::string g = cs; if (!g.empty()) g[rnd() % g.size()] = alphabet[rnd() % (sizeof(alphabet) - 1)]; run(mc, g, true);
            g = md; if (!g.empty()) g[rnd() % g.size()] = alphabet[rnd() % (sizeof(alphabet) - 1)]; run(mc, g, false);
        }
        // garbage from the tags' alphabet and from all byte values, against this CIGAR, an empty one and a single huge operation
        for (int k = 0; k < 8; ++k) {
            std::string g; const int n = (int)(rnd() % 40);
            for (int i = 0; i < n; ++i) g += k < 6 ? alphabet[rnd() % (sizeof(alphabet) - 1)] : (char)(1 + rnd() % 255);
            run(mc, g, true); run(mc, g, false); run({}, g, true); run({}, g, false); run({0xfffffff0u}, g, false); run({0xfffffff4u, 0xfffffff0u}, g, true);
        }
    }
    printf("%ld cases, %ld parsed\n", n_cases, n_ok);
    return n_ok > 0 && n_ok < n_cases ? 0 : 1;
}
