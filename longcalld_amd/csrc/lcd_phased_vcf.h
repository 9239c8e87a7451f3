// lcd_phased_vcf.h -- the phased-site tables of lcd_phased_vcf_read as lcd_phased_vcf.cpp (the reader, host only) and lcd_haplotag.cpp (their upload) see them.
// No HIP header here: the reader is compiled stand-alone by the host compiler too (tests/c/haplotag_vcf_sanitize.cpp).
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

struct lcd_hapvcf_contig {
    std::vector<int64_t> pos, ins_off, ps_value;
    std::vector<uint8_t> kind, hap_of_alt, ref_code, alt_code, pool;
    std::vector<int> len, ps_idx;
    int max_footprint = 0;
};
struct lcd_phased_vcf_s {
    std::vector<std::string> names;
    std::vector<lcd_hapvcf_contig> contigs;
    // the tables in HBM, made by the first lcd_chunk_haplotag of a contig on a device and freed with the handle: owned by lcd_haplotag.cpp, which sets both
    std::mutex dev_lock;
    void *dev = nullptr;
    void (*dev_free)(void *) = nullptr;
};
