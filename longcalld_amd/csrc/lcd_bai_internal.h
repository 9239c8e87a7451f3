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
// the BGZF members inside buf (file offset base) for the whole-file drivers (lcd_bai.cpp): whole members only, at most `want`; 0 or < 0.  *used: the bytes they take
struct BgzfMember { uint64_t coff; uint32_t bsize, ulen; };
int parse_members(const uint8_t *f, size_t n, uint64_t base, size_t want, bool at_eof, std::vector<BgzfMember> &out, size_t *used, const std::string &W);
// ---- the VCF indexes (.tbi / .csi; rules of the section "VCF indexes" of include/lcd_hotpath.h) ----
// A line's bin is kept as (level << 28) | index, level 0 = the 16 kb leaves: the pair does not depend on the depth the file ends up with (a CSI's depth is known
// only at the end when the header names no contig length).  VAccum's chunks carry that key in Chunk::bin; Contig::n_mapped counts the lines.
const int VIDX_MAX_DEPTH = 8;                                  // intervals up to 2^38
inline uint32_t vidx_key(int64_t beg, int64_t end) {
    --end;
    int l = 0;
    while (l < VIDX_MAX_DEPTH && (beg >> (14 + 3 * l)) != (end >> (14 + 3 * l))) ++l;
    return ((uint32_t)l << 28) | (uint32_t)(beg >> (14 + 3 * l));
}
inline uint32_t vidx_bin(uint32_t key, int depth) { const int l = (int)(key >> 28); return l >= depth ? 0u : (uint32_t)((((1ull << (3 * (depth - l))) - 1) / 7) + (key & 0xfffffffu)); }
struct VAccum { int format = 0; Accum a; std::vector<std::string> names; int64_t max_contig_len = 0, max_end = 0; };
// 0, or LCD_ERR_VIDX_CSI: TBI with an interval behind 2^29, or a CSI whose depth (from the header's contig lengths) does not hold the largest interval
int serialize_tbx(const VAccum &v, std::vector<uint8_t> &out);
} // namespace lcd_bai
