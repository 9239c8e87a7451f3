// lcd_kernels.h -- launchers of the gfx950 kernels (internal to liblcd_hotpath.so)
#pragma once
#include <hip/hip_runtime.h>
#include "lcd_types.h"

void lcd_launch_poa(const PoaChain *chains, const PoaRead *reads, const uint8_t *pool, uint8_t *arena, uint8_t *outpool,
                    PoaChainOut *outs, LcdScoring sc, int n_chains, int threads, int lds_bytes, hipStream_t stream, int *gate = nullptr, PoaSpare *spare = nullptr);
void lcd_launch_cu_probe(int *seen /* int[4096], zeroed */, hipStream_t stream);
void lcd_launch_gate(int *ctr, int target0, int target1, hipStream_t stream);
// lds_bytes > 0: the jobs keep their value ring in that much dynamic LDS (one wavefront per job); 0: ring in HBM, 256 threads per job
void lcd_launch_wfa(const WfaJob *jobs, const uint8_t *pool, uint8_t *arena, uint8_t *outpool, WfaOut *outs, LcdScoring sc,
                    int n_jobs, int lds_bytes, hipStream_t stream, int wide = 0); // wide: the HBM-ring class's SV-size jobs (diagonals in flight, wfa_kernel.hip)
void lcd_launch_edlib(const EdJob *jobs, const uint8_t *pool, uint8_t *arena, EdOut *outs, int n_jobs, hipStream_t stream);
void lcd_launch_strings(const StrJob *jobs, uint8_t *pool, StrOut *outs, int n_jobs, hipStream_t stream);
void lcd_launch_gather(const GatherJob *jobs, int n_jobs, hipStream_t stream);
void lcd_launch_patch_reads(PoaRead *tab, const ReadPatch *patches, int n, hipStream_t stream);
void lcd_launch_anchor_ends(const AnchorEndsJob *jobs, AnchorEndsOut *outs, int n_jobs, hipStream_t stream);
void lcd_launch_bam_walk(const BamWalkJob *jobs, BamWalkOut *outs, int n_jobs, hipStream_t st);
void lcd_launch_bam_stat(const BamStatJob *jobs, BamStatOut *outs, int n_jobs, hipStream_t st);
void lcd_launch_bam_cigar(const GatherJob *jobs, int n_jobs, hipStream_t st);
void lcd_launch_bam_aux(const BamAuxJob *jobs, BamAuxOut *outs, int is_ont, int n_jobs, hipStream_t st);
void lcd_launch_bam_nm(const BamNmJob *jobs, int *nm, int n_jobs, hipStream_t st);
// deflate_kernel.hip: BGZF payloads -> raw deflate streams in per-payload slots (one wavefront per payload, `grid` workgroups stride over them; toks: grid x
// payload words of token workspace), then the members (header, stream, CRC-32, ISIZE) packed at offs[] of the file image
void lcd_deflate_set_x2n(const unsigned *t32, hipStream_t st);
void lcd_launch_deflate(const uint8_t *data, unsigned long long n, int payload, int n_blocks, uint8_t *slots, unsigned slot_stride, unsigned *toks, DeflateOut *outs,
                        int grid, hipStream_t st);
void lcd_launch_deflate_pack(const uint8_t *slots, unsigned slot_stride, const DeflateOut *outs, const unsigned long long *offs, uint8_t *image, unsigned long long n,
                             int payload, int n_blocks, hipStream_t st);
int lcd_deflate_lds_bytes();
// bam_tag_kernel.hip: HP / PS rewrite of records in the inflated stream: measure (one lane per record), emit (one wavefront per record)
void lcd_launch_bam_tag_measure(const BamTagJob *jobs, BamTagOut *outs, int n_jobs, hipStream_t st);
void lcd_launch_bam_tag_emit(const BamTagJob *jobs, const BamTagOut *outs, uint8_t *out, int n_jobs, hipStream_t st);
// bam_refine_kernel.hip: records rewritten with the alignment of their final digars (CIGAR, POS, bin, NM / MD / cs, then HP / PS): measure and emit, one wavefront
// per record each; ref: the chunk window's codes 0-4, ref[0] = position ref_beg, read where ref_beg <= pos < ref_end
void lcd_launch_bam_refine_measure(const BamRefineJob *jobs, BamRefineOut *outs, const uint8_t *ref, long long ref_beg, long long ref_end, int n_jobs, hipStream_t st);
void lcd_launch_bam_refine_emit(const BamRefineJob *jobs, const BamRefineOut *outs, const uint8_t *ref, long long ref_beg, long long ref_end, uint8_t *out, int n_jobs,
                                hipStream_t st);
// bam_sam_kernel.hip: records in HBM as SAM text lines: measure (the length, flags and float count of every line) and emit (the lines at text_off[]), one
// wavefront per record each
void lcd_launch_bam_sam_measure(const BamSamIn &in, BamSamOut *outs, hipStream_t st);
void lcd_launch_bam_sam_emit(const BamSamIn &in, const unsigned long long *text_off, uint8_t *text, hipStream_t st);
// mods_kernel.hip: the CpG sites of a region (flags; lcd_launch_cv_scan makes them indices), the pile-up of the records' MM / ML calls (one wavefront per record),
// the non-empty sites as rows (rows: one entry per site; *n_rows: zeroed device int)
void lcd_launch_mods_sites(const ModsIn &in, int *flag, long long n_pos, hipStream_t st);
void lcd_launch_mods_pileup(const ModsIn &in, hipStream_t st);
void lcd_launch_mods_compact(const ModsIn &in, long long n_pos, ModsRow *rows, int *n_rows, hipStream_t st);
// depth_kernel.hip: the cover intervals of the kept records as a difference array (one wavefront per record), then the maximal runs of equal depth as rows in
// position order: per tile the plane sums and run heads, the scan of those partials by one workgroup (*n_rows: the total), per tile again the rows
void lcd_launch_depth_mark(const DepthIn &in, hipStream_t st);
void lcd_launch_depth_tiles(const DepthIn &in, DepthPart *parts, hipStream_t st);
void lcd_launch_depth_scan(DepthPart *parts, long long n_tiles, int *n_rows, hipStream_t st);
// split_kernel.hip: the records of a plan as FASTQ entries per haplotype and haplotag list lines, one wavefront per record: the rows of the measure pass, then
// (with the host's offsets in the rows) the text; fq[stream] and list are the four output buffers
void lcd_launch_split_measure(const SplitIn &in, SplitRow *rows, hipStream_t st);
void lcd_launch_split_emit(const SplitIn &in, const SplitRow *rows, uint8_t *fq0, uint8_t *fq1, uint8_t *fq2, uint8_t *list, hipStream_t st);
void lcd_launch_depth_rows(const DepthIn &in, const DepthPart *parts, DepthRow *rows, int cap, hipStream_t st);     // cap: the entries of rows (*n_rows of the scan)
// haplotag_kernel.hip: measure (span, candidate range; one wavefront per record), scan (the exclusive prefix of the candidate counts; one wavefront), mark (every
// operation's bits into the pair bytes), reduce (verdict bytes, votes per phase set, the read's haplotype); in.bits must be zeroed between scan and mark
void lcd_launch_htag_measure(const HtagIn &in, hipStream_t st);
void lcd_launch_htag_scan(const HtagIn &in, hipStream_t st);
void lcd_launch_htag_mark(const HtagIn &in, hipStream_t st);
void lcd_launch_htag_reduce(const HtagIn &in, hipStream_t st);
// bai_kernel.hip: a batch of walked records -> index entries (prep: the stat kernel's jobs and the batch's contig range; entry: offsets, bins, order test, windows,
// counters; compact: scan of the workgroups' run heads + the dense chunk list)
void lcd_launch_bai_prep(const BaiJob &j, hipStream_t st);
void lcd_launch_bai_entry(const BaiJob &j, hipStream_t st);
void lcd_launch_bai_compact(const BaiJob &j, hipStream_t st);
// vcf_index_kernel.hip: VCF text in HBM -> line table, parsed data lines, contig runs, index entries (the stages are listed at the top of that file); scan: the
// exclusive prefix of nb workgroup counts (j.block_cnt -> j.block_off, the total at [nb])
void lcd_launch_vidx_scan(const VIdxJob &j, int nb, hipStream_t st);
void lcd_launch_vidx_nl_count(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_nl_compact(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_flag(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_rank(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_parse(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_head_count(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_head(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_names(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_entry(const VIdxJob &j, hipStream_t st);
void lcd_launch_vidx_compact(const VIdxJob &j, hipStream_t st);
void lcd_launch_errrate(const ErrJob *jobs, const double *tab, double *out, int n_jobs, hipStream_t st);
void lcd_launch_compose(const CmpJob *jobs, CmpOut *outs, const CmpSeg *segs, int n_jobs, int emit, hipStream_t stream);
void lcd_launch_vars_scan(const VarScanJob *jobs, VarScanOut *outs, int n_jobs, hipStream_t stream);
void lcd_launch_vars_profile(const VarRegJob *jobs, VarRegOut *outs, const StrJob *sjobs, const StrOut *souts, int n_jobs, hipStream_t stream);
void lcd_launch_digar(const DigarJob *jobs, DigarOut *outs, DigarOpt opt, int n_jobs, hipStream_t stream);
void lcd_launch_slices(const SliceJob *jobs, SliceOut *outs, const DigarRec *digars, int flank, int n_jobs, hipStream_t stream);
void lcd_launch_unpack(const UnpackJob *jobs, int n_jobs, const uint8_t *packed, uint8_t *pool, hipStream_t stream);
void lcd_launch_refcmp(bool emit, const RefCmpJob *jobs, RefCmpOut *outs, const char *ref, long long ref_beg, long long ref_end, int n_jobs, hipStream_t stream);
void lcd_launch_region_support(const IvRec *regs, int n_regs, const long long *read_beg, const long long *read_end, const unsigned long long *iv_off,
                               const IvRec *ivs, int n_reads, int *total, int *noisy, hipStream_t stream);
void lcd_launch_region_support_batch(const SupChunk *chunks, const SupReg *regs, int n_regs, int *total, int *noisy, hipStream_t stream);
void lcd_launch_sdust(const unsigned char *pool, const SdSeg *segs, int T, int W, int seg, int n_seg, int cap, int *n_out, int2 *out, int4 *pbuf, int pcap, hipStream_t stream);
void lcd_launch_hap(const HapProb *probs, int n, hipStream_t stream);
// clean_vars_kernel.hip: candidate sites, pile-up, classification, noisy-read ratios and the read x variant profile of a device-resident chunk
void lcd_launch_cv_count(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long reg_beg, long long reg_end, int *cnt, hipStream_t st);
void lcd_launch_cv_emit(const CvRead *reads, const int *order, int n, const DigarRec *dg, long long reg_beg, long long reg_end, const int *off, CvSite *sites,
                        int *hist, long long key0, hipStream_t st);
int lcd_launch_cv_scan(int *a, int n, int *total, hipStream_t st);   // exclusive prefix sum in place, *total = the sum (device int)
void lcd_launch_cv_sort(const CvSite *sites, int n_sites, const CvRead *reads, const int *bstart, int *fill, int *tmp, int *sorted, long long key0, int n_buckets,
                        int *keep, int min_sv_len, hipStream_t st);
void lcd_launch_cv_compact(const CvSite *sites, const int *sorted, const int *keep, const int *kidx, int n, CvSite *out, hipStream_t st);
void lcd_launch_cv_pileup(const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *sites, int n_sites, CvCov *cov, CvOpt opt, hipStream_t st);
void lcd_launch_cv_classify(const CvSite *sites, const CvRead *reads, const CvCov *cov, int n_sites, const unsigned char *ref, CvOpt opt, int *cate, hipStream_t st);
void lcd_launch_cv_err_ivs(const CvRead *reads, const int *order, int n, const DigarRec *dg, IvRec *err, int *n_err, hipStream_t st);
void lcd_launch_cv_ratio(const CvRead *reads, const int *order, int n, const IvRec *err, const int *n_err, const long long *q, int n_q, int *counts, hipStream_t st);
// pass 0: start / end index per read; pass 1: alleles / alt_qi at allele_off[read]
void lcd_launch_cv_profile(int pass, const CvRead *reads, const int *order, int n, const DigarRec *dg, const CvSite *vars, const int *cate, int n_vars,
                           const IvRec *ivs, int *start, int *end, const unsigned long long *allele_off, int *alleles, int *alt_qi, CvOpt opt, hipStream_t st);
void lcd_launch_cv_alt(const CvSite *vars, const CvRead *reads, const unsigned long long *alt_off, int n_vars, unsigned char *pool, hipStream_t st);
// merge_vars_kernel.hip: the read x variant profile after a pass's region variants are folded into the chunk (all chunks of a call in one set of launches)
void lcd_launch_mv_span(const MvSrc *srcs, int n_src, int *start, int *end, hipStream_t st);
// cells per read -> off[0 .. n_reads] (off[n_reads] = the total); reads without a cell get (-1, -2); bsum: one entry per 256 reads
void lcd_launch_mv_scan(int *start, int *end, int n_reads, unsigned long long *off, unsigned long long *bsum, hipStream_t st);
void lcd_launch_mv_fill(int *cells, unsigned long long n, hipStream_t st);
void lcd_launch_mv_scatter(const MvSrc *srcs, int n_src, unsigned long long n_cells, const int *start, const unsigned long long *off, int *alleles, int *alt_qi,
                           unsigned long long cap, int *flag, hipStream_t st);
// plan_kernel.hip: the plan of a noisy-region pass over device-resident chunks (all regions of all chunks of a call in one grid)
void lcd_launch_plan_count(const PlanChunk *chunks, const PlanReg *regs, int n_regs, int max_cov, int *cnt, int *status, hipStream_t st);
void lcd_launch_plan_scan(const int *cnt, int n_regs, unsigned long long *off, hipStream_t st);   // exclusive scan, off[n_regs] = the total
void lcd_launch_plan_fill(const PlanChunk *chunks, const PlanReg *regs, int n_regs, const int *status, const unsigned long long *off, int *read_ids, int *pair_reg,
                          hipStream_t st);
void lcd_launch_plan_slices(const PlanChunk *chunks, const PlanReg *regs, const int *read_ids, const int *pair_reg, unsigned long long n_pairs, int flank,
                            SliceOut *outs, hipStream_t st);
