// lcd_io.cpp's helpers used by lcd_chunk.cpp (same library; not part of the C ABI)
#pragma once
#include <stdint.h>
#include <utility>
#include <vector>
// The BGZF blocks a region's records can lie in, through the .bai: `image` = those whole blocks back to back (a valid input of lcd_bgzf_inflate_dev), `ranges` = the
// merged index chunks as [begin, end) offsets of the image's INFLATED stream, in file order.  tid / tlen / n_ref from the BAM header.
// Over several files (lcd_io_region_images): the per-file images appended in file order, every file's ranges shifted by the inflated size of the members in front of
// it; `files` gives per file its segment [ubeg, uend) of the inflated stream, its ranges [range_first, range_first + range_n) and its own tid / tlen / n_ref (the contig
// is looked up by name in every header).  tid / tlen / n_ref of the image are file 0's.  One file through lcd_io_region_image leaves `files` empty.
struct LcdFileSeg { uint64_t ubeg = 0, uend = 0; size_t range_first = 0, range_n = 0; int tid = -1, n_ref = 0; int64_t tlen = 0; };
struct LcdRegionImage { std::vector<uint8_t> image; std::vector<std::pair<uint64_t, uint64_t>> ranges; int tid = -1, n_ref = 0; int64_t tlen = 0; std::vector<LcdFileSeg> files; };
int lcd_io_region_image(const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end, LcdRegionImage &out);
// The inflated size comes from the members' ISIZE footers: nothing is inflated to learn it.  On failure lcd_io_last_error names the file.
int lcd_io_region_images(int n, const char *const *bam_paths, const char *const *bai_paths, const char *chrom, int64_t reg_beg, int64_t reg_end, LcdRegionImage &out);
// The BAM header block (magic, l_text, text, n_ref, reference table) as it lies in the file's inflated stream (lcd_bam_writer_open copies it to the output).
int lcd_io_bam_header(const char *bam_path, std::vector<uint8_t> &hdr);
