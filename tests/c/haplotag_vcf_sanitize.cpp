// TEST ONLY: a stand-alone program around lcd_phased_vcf_read (longcalld_amd/csrc/lcd_phased_vcf.cpp), compiled together with that file by the host compiler under
// AddressSanitizer + UBSan (tests/test_haplotag_vcf_sanitized.py).  Usage: prog list.txt -- every line of the list is
//   <vcf path> <sample | -> <max_indel> <snvs_only> <contig name> ...
// and gives either `error <code>` or the dump tests/haplotag_common.py's dump() writes, each followed by `--end--`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "lcd_hotpath.h"

static const char NT16[] = "=ACMGRSVTWYHKDBN";

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream list(argv[1]);
    std::string line;
    int n_done = 0;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        std::string path, sample; lcd_hapvcf_opt_t opt; lcd_hapvcf_opt_default(&opt);
        if (!(is >> path >> sample >> opt.max_indel >> opt.snvs_only)) return 3;
        std::vector<std::string> names; std::string nm;
        while (is >> nm) names.push_back(nm);
        std::vector<const char *> np;
        for (const std::string &s : names) np.push_back(s.c_str());
        lcd_hapvcf_stats_t st;
        lcd_phased_vcf_t *v = lcd_phased_vcf_read(path.c_str(), sample == "-" ? nullptr : sample.c_str(), (int)np.size(), np.data(), &opt, &st);
        ++n_done;
        if (!v) {
            if (!lcd_phased_vcf_errno() || !lcd_phased_vcf_error()[0]) return 4;         // a failure names its reason
            printf("error %d\n--end--\n", lcd_phased_vcf_errno());
            continue;
        }
        const int64_t *s = &st.n_lines;
        printf("stats");
        for (int k = 0; k < 16; ++k) printf(" %lld", (long long)s[k]);
        printf("\n");
        if (lcd_phased_vcf_n_contigs(v) != (int)np.size() || lcd_phased_vcf_n_sites(v, (int)np.size()) != -4 || lcd_phased_vcf_n_sites(v, -1) != -4) return 5;
        for (int c = 0; c < (int)np.size(); ++c) {
            const size_t n = (size_t)lcd_phased_vcf_n_sites(v, c), nps = (size_t)lcd_phased_vcf_n_phase_sets(v, c), npool = (size_t)lcd_phased_vcf_pool_size(v, c);
            // exact-size heap arrays: a write past any of them is the sanitizer's to find
            std::vector<int64_t> pos(n), ins_off(n), psv(nps); std::vector<uint8_t> kind(n), hap(n), rc(n), ac(n), pool(npool); std::vector<int> len(n), psi(n);
            if (lcd_phased_vcf_sites_to_host(v, c, pos.data(), kind.data(), hap.data(), len.data(), rc.data(), ac.data(), ins_off.data(), psi.data(), psv.data(), pool.data())) return 6;
            printf("contig %d sites %zu sets %zu pool %zu max_footprint %d\n", c, n, nps, npool, lcd_phased_vcf_max_footprint(v, c));
            for (size_t i = 0; i < n; ++i)
                printf("%lld %d %d %d %d %d %lld %d\n", (long long)pos[i], kind[i], hap[i], len[i], rc[i], ac[i], (long long)ins_off[i], psi[i]);
            printf("ps");
            for (size_t i = 0; i < nps; ++i) printf(" %lld", (long long)psv[i]);
            printf("\npool ");
            for (size_t i = 0; i < npool; ++i) putchar(NT16[pool[i] & 15]);
            printf("\n");
        }
        printf("--end--\n");
        lcd_phased_vcf_free(v);
    }
    printf("%d files ok\n", n_done);
    return 0;
}
