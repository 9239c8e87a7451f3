// lcd_bai_internal.h -- what the index builder (lcd_bai.cpp, device side) and its finisher (lcd_index_host.cpp, pure host code without a HIP call) share: the
// accumulated state of an index and its serialisation.  No HIP header is included here: lcd_index_host.cpp compiles with a plain host compiler.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace lcd_bai {
struct Chunk { int refid; uint32_t bin; uint64_t vbeg, vend; };              // one run of records with equal (refid, bin), in file order (BaiChunk of lcd_types.h)
struct Contig { int64_t n_mapped = 0, n_unmapped = 0; uint64_t first_vbeg = ~0ull, last_vend = 0; std::vector<uint64_t> win; };   // win: all-ones = unset
struct Accum { int n_ref = 0; std::vector<Chunk> chunks; std::vector<Contig> ctg; uint64_t n_no_coor = 0; };
// rules 6-9 of include/lcd_hotpath.h: the bytes of the .bai
void serialize(const Accum &a, std::vector<uint8_t> &out);
// lcd_last_error's string when the library is linked, a string of this file's own in a stand-alone program
int index_err(int code, const std::string &m);
const char *index_host_error();
inline uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
} // namespace lcd_bai
