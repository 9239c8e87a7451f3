"""ctypes loader for liblcd_hotpath.so (built in-tree by __graft_entry__.build / csrc/Makefile)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblcd_hotpath.so")


class LcdError(RuntimeError):
    pass


class LcdOpt(C.Structure):
    """lcd_opt_t == the call_var_opt_t fields the path reads (src/call_var_main.h:128-180)."""
    _fields_ = [(n, C.c_int) for n in ("match", "mismatch", "gap_open1", "gap_ext1", "gap_open2", "gap_ext2", "gap_aln")] + [
        ("min_af", C.c_double), ("min_dp", C.c_int), ("partial_aln_ratio", C.c_double)] + [
        (n, C.c_int) for n in ("min_noisy_reg_size_to_sample_reads", "max_noisy_reg_len", "noisy_reg_flank_len",
                               "min_hap_full_reads", "min_hap_reads", "collect_ref_read_aln_str", "is_ont", "collect_noisy_vars", "min_sv_len")]


class LcdAlnStr(C.Structure):
    """lcd_aln_str_t == aln_str_t (src/collect_var.h:106-112)."""
    _fields_ = [("target_aln", C.POINTER(C.c_uint8)), ("query_aln", C.POINTER(C.c_uint8)), ("aln_len", C.c_int),
                ("target_beg", C.c_int), ("target_end", C.c_int), ("query_beg", C.c_int), ("query_end", C.c_int)]


class LcdRegionResult(C.Structure):
    """lcd_region_result_t (include/lcd_hotpath.h): one region of lcd_batch_region_results_arena"""
    _fields_ = [("n_cons", C.c_int), ("n_aln_strs", C.c_int), ("clu_n_seqs", C.c_int * 2), ("clu_read_ids", C.POINTER(C.c_int) * 2), ("aln_strs", C.POINTER(LcdAlnStr) * 2)]


class LcdDigar1(C.Structure):
    _fields_ = [("pos", C.c_int64), ("type", C.c_int), ("len", C.c_int), ("qi", C.c_int)]


class LcdNoisyVar(C.Structure):
    """lcd_noisy_var_t (include/lcd_hotpath.h): the cand_var_t fields of a noisy-region variant"""
    _fields_ = [("pos", C.c_int64)] + [(n, C.c_int) for n in ("var_type", "ref_len", "alt_len", "cate", "from_cons", "is_homopolymer_indel",
                                                               "ref_base", "alt_ref_base", "total_cov")] + [("alle_covs", C.c_int * 2),
                                                                                                              ("alt_seq", C.POINTER(C.c_uint8))]


class LcdDigarOpt(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("min_bq", "noisy_reg_max_xgaps", "noisy_reg_slide_win", "end_clip_reg", "end_clip_reg_flank_win")] + [
        ("max_noisy_frac_per_read", C.c_double), ("max_var_ratio_per_read", C.c_double)]


class LcdDigar(C.Structure):
    _fields_ = [("pos", C.c_int64), ("type", C.c_int), ("len", C.c_int), ("qi", C.c_int), ("is_low_qual", C.c_int)]


class LcdNoisyIv(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("label", C.c_int), ("pad", C.c_int)]


class LcdBamReads(C.Structure):
    """lcd_bam_reads_t"""
    _fields_ = [("n_reads", C.c_int), ("tid", C.c_int), ("n_targets", C.c_int), ("target_len", C.c_int64), ("pos0", C.POINTER(C.c_int64)), ("end_pos", C.POINTER(C.c_int64)),
                ("mapq", C.POINTER(C.c_int)), ("flag", C.POINTER(C.c_int)), ("n_cigar", C.POINTER(C.c_int)), ("qlen", C.POINTER(C.c_int)), ("cigar_off", C.POINTER(C.c_uint64)),
                ("cigar_pool", C.POINTER(C.c_uint32)), ("seq_off", C.POINTER(C.c_uint64)), ("seq_pool", C.POINTER(C.c_uint8)), ("qual_off", C.POINTER(C.c_uint64)),
                ("qual_pool", C.POINTER(C.c_uint8)), ("name_off", C.POINTER(C.c_uint64)), ("name_pool", C.POINTER(C.c_char))]


class LcdChunkSrc(C.Structure):
    _fields_ = [("ref_seq", C.c_char_p), ("ref_beg", C.c_int64), ("ref_end", C.c_int64), ("is_ont", C.c_int)]


class LcdReadView(C.Structure):
    _fields_ = [("digars", C.POINTER(LcdDigar1)), ("n_digar", C.c_int), ("qlen", C.c_int), ("bseq", C.POINTER(C.c_uint8)),
                ("qual", C.POINTER(C.c_uint8)), ("hap", C.c_int), ("phase_set", C.c_int64)]


class LcdBatchStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_regions", "n_regions_resolved", "n_chains", "n_anchor_jobs", "n_wfa_jobs", "n_edlib_jobs")] + [
        (n, C.c_uint64) for n in ("poa_aligned_bases", "poa_cells", "wfa_offsets", "edlib_blocks", "poa_alg_bytes")] + [
        (n, C.c_double) for n in ("ms_total", "ms_anchor", "ms_poa", "ms_wfa", "ms_strings", "ms_upload", "ms_download", "ms_host", "ms_poa_kernel")] + [
        ("n_poa_launches", C.c_int), ("poa_retries", C.c_int), ("ms_vars", C.c_double), ("poa_cells_computed", C.c_uint64), ("poa_grown", C.c_int)]


class LcdHapProblem(C.Structure):
    """lcd_hap_problem_t: bam_chunk_t / cand_var_t / read_var_profile_t flattened for K5 (src/assign_hap.c:473)"""
    _i32p, _i64p, _u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    _fields_ = [("n_reads", C.c_int), ("n_vars", C.c_int), ("is_ont", C.c_int), ("var_pos", _i64p), ("var_type", _i32p), ("var_cate", _i32p),
                ("is_homopolymer_indel", _i32p), ("total_cov", _i32p), ("alle_off", _i32p), ("alle_covs", _i32p), ("start_var_idx", _i32p),
                ("end_var_idx", _i32p), ("allele_off", _i32p), ("alleles", _i32p), ("ordered_read_ids", _i32p), ("is_skipped", _u8p),
                ("n_cr", C.c_int), ("cr_read", _i32p), ("haps", _i32p), ("phase_sets", _i64p), ("n_clean_agree_snps", _i32p),
                ("n_clean_conflict_snps", _i32p), ("var_phase_set", _i64p), ("hap_to_cons_alle", _i32p), ("hap_to_alle_profile", _i32p)]


class LcdCleanOpt(C.Structure):
    """lcd_clean_opt_t: the call_var_opt_t fields the first round of collect_var_main reads"""
    _fields_ = [(n, C.c_int) for n in ("min_dp", "min_alt_dp", "min_bq", "min_sv_len", "noisy_reg_max_xgaps", "noisy_reg_flank_len", "noisy_reg_merge_dis",
                                       "is_ont", "out_somatic")] + [("min_af", C.c_double), ("max_af", C.c_double), ("strand_bias_pval", C.c_float)]


class LcdCleanVars(C.Structure):
    """lcd_clean_vars_t: candidate variants, noisy regions and the read x variant profile of one chunk (every array malloc()'d)"""
    _i32p, _i64p, _u64p, _u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    _fields_ = [("n_vars", C.c_int), ("pos", _i64p), ("var_type", _i32p), ("ref_len", _i32p), ("alt_len", _i32p), ("cate", _i32p), ("total_cov", _i32p),
                ("low_qual_cov", _i32p), ("alle_covs", _i32p), ("strand_alle_covs", _i32p), ("alt_off", _u64p), ("alt_pool", _u8p),
                ("is_homopolymer_indel", _i32p), ("n_regs", C.c_int), ("regs", C.POINTER(LcdNoisyIv)), ("n_reads", C.c_int), ("start_var_idx", _i32p),
                ("end_var_idx", _i32p), ("allele_off", _u64p), ("alleles", _i32p), ("alt_qi", _i32p), ("n_cr", C.c_int), ("cr_read", _i32p),
                ("qual_upload_bytes", C.c_uint64), ("alt_ref_base", _u8p)]


class LcdRegionVars(C.Structure):
    """lcd_region_vars_t: one region's lcd_batch_region_vars output as lcd_merge_region_vars borrows it"""
    _i32p = C.POINTER(C.c_int)
    _fields_ = [("n_vars", C.c_int), ("vars", C.POINTER(LcdNoisyVar)), ("n_rows", C.c_int), ("row_read_ids", _i32p), ("prof_start", _i32p), ("prof_end", _i32p),
                ("prof_alleles", _i32p)]


class LcdPassOpt(C.Structure):
    """lcd_pass_opt_t: the call_var_opt_t fields the plan of a noisy-region pass reads"""
    _fields_ = [(n, C.c_int) for n in ("max_noisy_reg_len", "max_noisy_reg_cov", "noisy_reg_flank_len")]


class LcdPassPlan(C.Structure):
    """lcd_pass_plan_t: per region status / clamped interval, CSR of (region, read) pairs with their slices (every array malloc()'d)"""
    _i32p = C.POINTER(C.c_int)
    _fields_ = [("n_regs", C.c_int), ("status", _i32p), ("beg", C.POINTER(C.c_int64)), ("end", C.POINTER(C.c_int64)), ("read_off", C.POINTER(C.c_uint64)),
                ("read_ids", _i32p), ("read_beg", _i32p), ("read_end", _i32p), ("cover", _i32p)]


class LcdHapState(C.Structure):
    """lcd_hap_state_t: the in/out arrays of K5"""
    _i32p, _i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    _fields_ = [("n_reads", C.c_int), ("n_vars", C.c_int), ("haps", _i32p), ("phase_sets", _i64p), ("n_clean_agree_snps", _i32p), ("n_clean_conflict_snps", _i32p),
                ("var_phase_set", _i64p), ("hap_to_cons_alle", _i32p), ("hap_to_alle_profile", _i32p)]


class LcdRoundsChunk(C.Structure):
    """lcd_rounds_chunk_t: one chunk of lcd_chunks_noisy_rounds"""
    _fields_ = [("chunk", C.c_void_p), ("vars", C.POINTER(LcdCleanVars)), ("state", C.POINTER(LcdHapState)), ("ordered_read_ids", C.POINTER(C.c_int)),
                ("is_skipped", C.POINTER(C.c_uint8)), ("ref_seq", C.POINTER(C.c_uint8)), ("ref_beg", C.c_int64), ("ref_end", C.c_int64), ("is_ont", C.c_int),
                ("done", C.POINTER(C.c_int)), ("n_passes", C.c_int), ("n_first_vars", C.c_int), ("first_to_final", C.POINTER(C.c_int))]


class LcdFirstChunk(C.Structure):
    """lcd_first_chunk_t: one chunk of lcd_chunks_first_round"""
    _fields_ = [("chunk", C.c_void_p), ("ref_seq", C.POINTER(C.c_uint8)), ("ref_beg", C.c_int64), ("ref_end", C.c_int64), ("reg_beg", C.c_int64), ("reg_end", C.c_int64),
                ("is_ont", C.c_int), ("ordered_read_ids", C.POINTER(C.c_int)), ("is_rev", C.POINTER(C.c_uint8)), ("meta", C.POINTER(LcdBamReads)),
                ("n_reads", C.c_int), ("order", C.POINTER(C.c_int)), ("is_skipped", C.POINTER(C.c_uint8)), ("n_low", C.c_int), ("low_comp", C.POINTER(C.c_int64)),
                ("n_pre_regs", C.c_int), ("pre_regs", C.POINTER(LcdNoisyIv)), ("vars", C.POINTER(LcdCleanVars)), ("state", C.POINTER(LcdHapState))]


class LcdCallOpt(C.Structure):
    """lcd_call_opt_t"""
    _fields_ = [("log_p", C.c_double), ("log_1p", C.c_double), ("log_2", C.c_double)] + [(n, C.c_int) for n in ("max_gq", "max_qual", "min_sv_len", "min_dp", "min_alt_dp",
                                                                                                                 "out_amb_base")]


class LcdCfg(C.Structure):
    """lcd_cfg_t: the option structs of the whole path"""
    _fields_ = [("clean", LcdCleanOpt), ("opt", LcdOpt), ("pass_", LcdPassOpt), ("call", LcdCallOpt)]


class LcdVar1(C.Structure):
    """lcd_var1_t: one genotype record"""
    _u8p = C.POINTER(C.c_uint8)
    _fields_ = [("pos", C.c_int64), ("PS", C.c_int64), ("type", C.c_int), ("ref_len", C.c_int), ("n_alt_allele", C.c_int), ("alt_len", C.c_int * 2),
                ("ref_bases", _u8p), ("alt_bases", _u8p * 2), ("GT", C.c_int * 2), ("DP", C.c_int), ("AD", C.c_int * 3), ("QUAL", C.c_int), ("GQ", C.c_int),
                ("is_sv", C.c_int), ("is_clean", C.c_int), ("n_alt_reads", C.c_int), ("alt_read_i", C.POINTER(C.c_int)),
                ("cand_i", C.c_int), ("tsd_len", C.c_int), ("polya_len", C.c_int), ("te_seq_i", C.c_int), ("te_is_rev", C.c_int), ("tsd_pos1", C.c_int64),
                ("tsd_pos2", C.c_int64), ("tsd_seq", _u8p)]


class LcdCallChunk(C.Structure):
    """lcd_call_chunk_t: one chunk of lcd_chunks_call / one region of lcd_call_bam_regions"""
    _fields_ = [("first", LcdFirstChunk), ("n_passes", C.c_int), ("flip_hap", C.c_int), ("flip_pre_PS", C.c_int64), ("flip_cur_PS", C.c_int64), ("n_records", C.c_int)]


class LcdBamOut(C.Structure):
    """lcd_bam_out_t: the phased alignment output of lcd_call_bam_regions / lcd_write_phased"""
    _fields_ = [("path", C.c_char_p), ("pg_line", C.c_char_p), ("block_payload", C.c_int)] + [(n, C.c_int64) for n in ("n_records_out", "n_filtered_out", "bytes_inflated", "bytes_file")] + [
        (n, C.c_double) for n in ("ms_tag", "ms_deflate", "ms_download_write")]


class LcdChunkPhase(C.Structure):
    """lcd_chunk_phase_t: one chunk of the cross-chunk stitch"""
    _i32p, _i64p, _u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    _fields_ = [("tid", C.c_int), ("n_reads", C.c_int), ("n_vars", C.c_int), ("ordered_read_ids", _i32p), ("is_skipped", _u8p), ("haps", _i32p), ("phase_sets", _i64p),
                ("var_phase_set", _i64p), ("hap_to_cons_alle", _i32p), ("n_up_ovlp", C.c_int), ("n_down_ovlp", C.c_int), ("up_ovlp_read_i", _i32p), ("down_ovlp_read_i", _i32p),
                ("flip_hap", C.c_int), ("flip_pre_PS", C.c_int64), ("flip_cur_PS", C.c_int64)]


class LcdStitchCarry(C.Structure):
    """lcd_stitch_carry_t: what the stitch of the next window reads of a window's last chunk"""
    _fields_ = [("valid", C.c_int), ("tid", C.c_int), ("reg_beg", C.c_int64), ("reg_end", C.c_int64), ("n_reads", C.c_int), ("n_vars", C.c_int), ("n_down_ovlp", C.c_int),
                ("is_skipped", C.POINTER(C.c_uint8)), ("haps", C.POINTER(C.c_int)), ("phase_sets", C.POINTER(C.c_int64)), ("down_ovlp_read_i", C.POINTER(C.c_int))]


class LcdChunkPlan(C.Structure):
    """lcd_chunk_plan_t: the (tid, reg_beg, reg_end) entries of lcd_plan_chunks"""
    _fields_ = [("n", C.c_int), ("tid", C.POINTER(C.c_int)), ("reg_beg", C.POINTER(C.c_int64)), ("reg_end", C.POINTER(C.c_int64)), ("fallback", C.c_int)]


class LcdFileJob(C.Structure):
    """lcd_file_job_t: one whole-file run of lcd_call_files"""
    _fields_ = [("bam_path", C.c_char_p), ("bai_path", C.c_char_p), ("fasta_path", C.c_char_p), ("contig_mode", C.c_int), ("n_exclude", C.c_int),
                ("exclude", C.POINTER(C.c_char_p)), ("n_regions", C.c_int), ("regions", C.POINTER(C.c_char_p)), ("region_bed_path", C.c_char_p), ("chunk_len", C.c_int64),
                ("window_chunks", C.c_int), ("overlap", C.c_int), ("loader_threads", C.c_int), ("min_mapq", C.c_int), ("vcf_path", C.c_char_p), ("vcf_bgzf", C.c_int),
                ("no_vcf_header", C.c_int), ("sample_name", C.c_char_p), ("source_version", C.c_char_p), ("cmdline", C.c_char_p), ("date_yyyymmdd", C.c_char_p),
                ("bam_out", C.POINTER(LcdBamOut)), ("keep_records", C.c_int)]


class LcdFileStats(C.Structure):
    """lcd_file_stats_t: the counters of lcd_call_files (and, with keep_records, the per-chunk results and the records)"""
    _i32p, _i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    _fields_ = [(n, C.c_int) for n in ("n_planned", "n_loaded", "n_empty", "n_windows", "plan_fallback")] + [
        (n, C.c_int64) for n in ("n_reads", "n_records", "n_vcf_lines", "n_region_loads")] + [(n, C.c_double) for n in ("ms_load", "ms_call", "ms_write", "ms_wall")] + [
        ("peak_device_bytes", C.c_int64), ("n_chunks", C.c_int), ("chunk_tid", _i32p), ("chunk_reg_beg", _i64p), ("chunk_reg_end", _i64p), ("chunk_n_reads", _i32p),
        ("chunk_n_passes", _i32p), ("chunk_flip_hap", _i32p), ("chunk_n_records", _i32p), ("chunk_flip_pre_PS", _i64p), ("chunk_flip_cur_PS", _i64p),
        ("records", C.POINTER(LcdVar1)), ("n_kept_records", C.c_int)]


class LcdBaiMember(C.Structure):
    """lcd_bai_member_t: one BGZF member of a stream handed to lcd_bai_builder_add_stream"""
    _fields_ = [("uoff", C.c_uint64), ("coff", C.c_uint64), ("ulen", C.c_uint32), ("pad", C.c_uint32)]


class LcdBaiOpt(C.Structure):
    _fields_ = [("slab_members", C.c_int), ("verify_crc", C.c_int)]


class LcdBaiStats(C.Structure):
    """lcd_bai_stats_t: the counters and per-stage times of lcd_bai_build"""
    _fields_ = [(n, C.c_int64) for n in ("n_records", "n_indexed", "n_mapped", "n_unmapped", "n_no_coor", "n_chunks", "n_slabs", "n_members", "bytes_in", "bytes_inflated",
                                         "bytes_index")] + [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_walk", "ms_stat", "ms_entry", "ms_finish", "ms_wall")]


class LcdIndexOpt(C.Structure):
    """lcd_index_opt_t: what lcd_call_files builds and writes (lcd_run_opt_t.idx)"""
    _fields_ = [("build_missing_bai", C.c_int), ("build_missing_fai", C.c_int), ("write_out_bai", C.c_int), ("out_bai_path", C.c_char_p), ("slab_members", C.c_int)]


class LcdIndexStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("built_bai", "built_fai", "wrote_out_bai", "out_bai_skipped")] + [("out_bai_skip_reason", C.c_char * 256)] + [
        (n, C.c_int64) for n in ("out_bai_bytes", "out_n_indexed", "out_n_no_coor")] + [(n, C.c_double) for n in ("ms_build_bai", "ms_build_fai", "ms_out_bai")]


class LcdInputs(C.Structure):
    """lcd_inputs_t: the alignment files of one sample (lcd_call_files)"""
    _fields_ = [("n", C.c_int), ("bam_paths", C.POINTER(C.c_char_p)), ("bai_paths", C.POINTER(C.c_char_p)), ("sort_output", C.c_int)]


class LcdVcfFields(C.Structure):
    """lcd_vcf_fields_t: the TE library (-T) and the supporting read names (--out-var-rnames / --out-sv-rnames) of a driver call"""
    _fields_ = [("te_fasta_path", C.c_char_p), ("te_kmer_len", C.c_int), ("rnames_mode", C.c_int)]


class LcdVcfFieldsOut(C.Structure):
    """lcd_vcf_fields_out_t: the library's names, the MEI lines written, the ALTREADS value per returned / kept record"""
    _fields_ = [("n_te_seqs", C.c_int), ("te_names", C.POINTER(C.c_char_p)), ("n_mei_lines", C.c_int64), ("n_rnames", C.c_int), ("rnames", C.POINTER(C.c_char_p))]


class LcdModsOpt(C.Structure):
    """lcd_mods_opt_t: the options of lcd_chunk_mod_pileup"""
    _fields_ = [("code", C.c_int), ("threshold", C.c_int), ("combine_strands", C.c_int), ("reserved", C.c_int), ("ref_seq", C.c_char_p), ("ref_beg", C.c_int64),
                ("ref_end", C.c_int64)]


MODS_STAT_COUNTERS = ("n_records", "n_no_mm", "n_no_group", "n_hard_clip", "n_mn_mismatch", "n_syntax", "n_overrun", "n_ml_short", "n_unaligned", "n_outside", "n_off_context",
                      "n_counted", "n_sites", "n_rows")


class LcdModsStats(C.Structure):
    """lcd_mods_stats_t: where the records and their calls went, and the wall-clock split of the call"""
    _fields_ = [(n, C.c_int64) for n in MODS_STAT_COUNTERS] + [(n, C.c_double) for n in ("ms_site_map", "ms_pileup", "ms_compact")]


HAPVCF_STAT_KEYS = ("n_lines", "n_sites", "n_unknown_contig", "n_filtered", "n_unphased", "n_hom", "n_other_gt", "n_both_alt", "n_symbolic", "n_complex", "n_long_indel",
                    "n_indel_off", "n_snv", "n_ins", "n_del", "n_phase_sets")


class LcdHapvcfOpt(C.Structure):
    """lcd_hapvcf_opt_t: the options of lcd_phased_vcf_read"""
    _fields_ = [("max_indel", C.c_int), ("snvs_only", C.c_int), ("reserved", C.c_int * 2)]


class LcdHapvcfStats(C.Structure):
    """lcd_hapvcf_stats_t: the data lines, the sites, and the lines every rule left out"""
    _fields_ = [(n, C.c_int64) for n in HAPVCF_STAT_KEYS]


class LcdHaplotagOpt(C.Structure):
    """lcd_haplotag_opt_t: the options of lcd_chunk_haplotag"""
    _fields_ = [("min_bq", C.c_int), ("min_diff", C.c_int), ("reserved", C.c_int * 2)]


class LcdHaplotagStats(C.Structure):
    """lcd_haplotag_stats_t: records, pairs, pairs per verdict (NONE REF ALT OTHER LOWQ), reads per haplotype, and the wall-clock split of the call"""
    _fields_ = [("n_records", C.c_int64), ("n_pairs", C.c_int64), ("n_verdict", C.c_int64 * 5), ("n_tagged", C.c_int64 * 3), ("n_multi_ps", C.c_int64), ("n_cg", C.c_int64),
                ("n_bad_record", C.c_int64), ("n_no_seq", C.c_int64), ("ms_measure", C.c_double), ("ms_mark", C.c_double), ("ms_reduce", C.c_double)]


class LcdHaplotagRun(C.Structure):
    """lcd_haplotag_run_t: lcd_haplotag_files' own options; the first member is the struct's size"""
    _fields_ = [("size", C.c_size_t), ("vcf_path", C.c_char_p), ("sample", C.c_char_p), ("max_indel", C.c_int), ("snvs_only", C.c_int), ("min_bq", C.c_int), ("min_diff", C.c_int),
                ("vcf_stats", C.POINTER(LcdHapvcfStats)), ("stats", C.POINTER(LcdHaplotagStats))]


class LcdDepthOpt(C.Structure):
    """lcd_depth_opt_t: the options of lcd_chunk_depth (window: the drivers' window rule, not read by the chunk call)"""
    _fields_ = [("skip_dels", C.c_int), ("window", C.c_int), ("reserved", C.c_int * 2)]


DEPTH_STAT_COUNTERS = ("n_records", "n_no_cigar", "n_cg", "n_no_overlap", "n_intervals")


class LcdDepthStats(C.Structure):
    """lcd_depth_stats_t: the records and their intervals, the covered bases per haplotype, the rows, and the wall-clock split of the call"""
    _fields_ = [(n, C.c_int64) for n in DEPTH_STAT_COUNTERS] + [("bases", C.c_int64 * 3), ("n_rows", C.c_int64), ("ms_mark", C.c_double), ("ms_rows", C.c_double)]


class LcdRefineStats(C.Structure):
    """lcd_refine_stats_t: what lcd_chunk_refine_records did to the records it wrote"""
    _fields_ = [(n, C.c_int64) for n in ("n_records", "n_kept", "n_refined", "n_identical", "n_unrefined", "n_pos_moved", "n_no_digars", "n_qlen_mismatch", "n_bad_pos",
                                         "n_too_many_ops", "n_cg_cigar", "n_nm_replaced", "n_md_replaced", "n_cs_replaced", "n_touched", "bytes_digars_up",
                                         "bytes_ref_up")] + [("ms_measure", C.c_double), ("ms_emit", C.c_double)] + [
                    (n, C.c_int64) for n in ("n_log_entries", "bytes_log_down", "n_log_rejected")]


class LcdSamStats(C.Structure):
    """lcd_sam_stats_t: what lcd_tagged_to_sam / lcd_records_to_sam formatted"""
    _fields_ = [(n, C.c_int64) for n in ("n_records", "bytes_records", "bytes_text", "n_float_values", "n_cg_cigar", "n_walk_stopped", "n_bad_layout")] + [
        (n, C.c_double) for n in ("ms_measure", "ms_emit", "ms_download_write")]


class LcdAlnOpt(C.Structure):
    """lcd_aln_opt_t: the alignment output's format (LCD_ALN_BAM / LCD_ALN_SAM) and whether its records are refined"""
    _fields_ = [("format", C.c_int), ("refine", C.c_int)]


class LcdVcfIndexStats(C.Structure):
    """lcd_vcf_index_stats_t: the counters and per-stage times of lcd_vcf_index_build / of the indexing VCF writer"""
    _fields_ = [(n, C.c_int64) for n in ("n_lines", "n_data_lines", "n_meta_lines", "n_contigs", "n_chunks", "n_slabs", "n_members", "bytes_in", "bytes_inflated", "bytes_index",
                                         "bytes_file")] + [(n, C.c_int) for n in ("depth", "wrote", "skipped", "pad")] + [("skip_reason", C.c_char * 256)] + [
                    (n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_lines", "ms_entry", "ms_finish", "ms_wall")]


class LcdVcfIndexOpt(C.Structure):
    """lcd_vcf_index_opt_t: the index of a BGZF-compressed VCF (lcd_vcf_index_build, lcd_vcf_writer_open_idx, lcd_run_ext_t.vcf_idx)"""
    _fields_ = [("format", C.c_int), ("index_path", C.c_char_p), ("slab_members", C.c_int), ("verify_crc", C.c_int), ("stats", C.POINTER(LcdVcfIndexStats))]


class LcdRunOpt(C.Structure):
    """lcd_run_opt_t: the optional features of lcd_call_files / lcd_call_bam_regions; a NULL member is off"""
    _fields_ = [("idx", C.POINTER(LcdIndexOpt)), ("fields", C.POINTER(LcdVcfFields)), ("aln", C.POINTER(LcdAlnOpt))]


class LcdRunOut(C.Structure):
    """lcd_run_out_t: what a driver reports beside its statistics; a NULL member is not reported"""
    _fields_ = [("idx_stats", C.POINTER(LcdIndexStats)), ("n_reads_per_file", C.POINTER(C.c_int64)), ("fields_out", C.POINTER(LcdVcfFieldsOut)),
                ("refine_stats", C.POINTER(LcdRefineStats)), ("sam_stats", C.POINTER(LcdSamStats))]


class LcdRunExt2(C.Structure):
    """lcd_run_ext2_t: the options of lcd_call_files_ext2; `size` comes first and is sizeof of the struct as the caller knows it"""
    _fields_ = [("size", C.c_size_t), ("mods_path", C.c_char_p), ("mods_code", C.c_int), ("mods_threshold", C.c_int), ("mods_combine_strands", C.c_int), ("reserved", C.c_int),
                ("mods_stats", C.POINTER(LcdModsStats)),
                ("depth_path", C.c_char_p), ("depth_window", C.c_int), ("depth_skip_dels", C.c_int), ("depth_stats", C.POINTER(LcdDepthStats))]


SPLIT_STAT_COUNTERS_HEAD = ("n_records", "n_selected")
SPLIT_STAT_COUNTERS_TAIL = ("n_not_primary", "n_filtered_primary", "n_reverse", "n_no_seq", "n_bad_layout")


class LcdSplitOpt(C.Structure):
    """lcd_split_opt_t: the options of lcd_chunk_split_reads (comment: HP / PS behind the name; list: the haplotag list's lines as stream 3)"""
    _fields_ = [("comment", C.c_int), ("list", C.c_int), ("reserved", C.c_int * 2)]


class LcdSplitStats(C.Structure):
    """lcd_split_stats_t: where the records of the plan went, the bytes per stream, and the wall-clock split of the call (the last two: the drivers' sink)"""
    _fields_ = [(n, C.c_int64) for n in SPLIT_STAT_COUNTERS_HEAD] + [("n_hap", C.c_int64 * 3)] + [(n, C.c_int64) for n in SPLIT_STAT_COUNTERS_TAIL] + [
        ("bytes_fastq", C.c_int64 * 3), ("bytes_list", C.c_int64)] + [(n, C.c_double) for n in ("ms_measure", "ms_emit", "ms_deflate", "ms_download_write")]


class LcdRunExt2Split(C.Structure):
    """lcd_run_ext2_split_t: lcd_run_ext2_t grown at its end by the read sets of the run; handed to the drivers as byref(s.x) with s.x.size = sizeof of this struct"""
    _fields_ = [("x", LcdRunExt2), ("split_prefix", C.c_char_p), ("split_gz", C.c_int), ("split_comment", C.c_int), ("haplotag_path", C.c_char_p),
                ("split_stats", C.POINTER(LcdSplitStats))]


class LcdRunExt(C.Structure):
    """lcd_run_ext_t: the options of lcd_call_files_ext that came after lcd_run_opt_t / lcd_run_out_t were laid out; a NULL member is off"""
    _fields_ = [("vcf_idx", C.POINTER(LcdVcfIndexOpt)), ("vcf_idx_stats", C.POINTER(LcdVcfIndexStats))]


class LcdWriterOpt(C.Structure):
    """lcd_writer_opt_t: the options of lcd_bam_writer_open / lcd_write_phased"""
    _fields_ = [("format", C.c_int), ("sort_output", C.c_int), ("write_index", C.c_int), ("index_path", C.c_char_p), ("idx_stats", C.POINTER(LcdIndexStats)),
                ("refine_stats", C.POINTER(LcdRefineStats)), ("sam_stats", C.POINTER(LcdSamStats))]


class LcdRefineEntry(C.Structure):
    """lcd_refine_entry_t: one (cluster, read) of a resolved noisy region -- what lcd_update_digars_from_msa1 takes"""
    _fields_ = [(n, C.c_int) for n in ("read_id", "cover", "read_beg", "read_end", "aln_len", "pass_")] + [("reg_beg", C.c_int64), ("reg_end", C.c_int64),
                                                                                                        ("target", C.POINTER(C.c_uint8)), ("query", C.POINTER(C.c_uint8))]


LCD_RNAMES_NONE, LCD_RNAMES_SV, LCD_RNAMES_ALL = 0, 1, 2
LCD_ERR_BAI_ORDER, LCD_ERR_BAI_CSI, LCD_ERR_FAI_FORMAT, LCD_ERR_BAI_CONTIG, LCD_ERR_INPUT_HEADERS = -50, -51, -52, -53, -54
LCD_ERR_VIDX_ORDER, LCD_ERR_VIDX_CSI, LCD_ERR_VCF_LINE = -55, -56, -57
LCD_VIDX_TBI, LCD_VIDX_CSI = 0, 1
LCD_MAX_INPUTS = 64
LCD_ALN_BAM, LCD_ALN_SAM = 0, 1
LCD_CTG_AUTOSOME_XY, LCD_CTG_AUTOSOME, LCD_CTG_ALL = 0, 1, 2

_lib = None

# every symbol include/lcd_hotpath.h declares (tests check the .so exports all of them)
EXPORTS = [
    "lcd_opt_default", "lcd_init", "lcd_device_count", "lcd_alloc_events", "lcd_device_bytes", "lcd_set_thread_device", "lcd_batch_create_on", "lcd_last_error", "lcd_host_threads", "lcd_version", "lcd_wfa_end2end_aln", "lcd_edlib_end2end_aln",
    "lcd_edlib_xgaps", "lcd_edlib_edit_distance", "lcd_end2end_aln", "lcd_wfa_collect_diff_ins_seq", "lcd_edlib_infix_aln", "lcd_wfa_heuristic_aln", "lcd_collect_noisy_reg_aln_strs", "lcd_batch_create", "lcd_batch_destroy",
    "lcd_batch_clear", "lcd_batch_region_vars", "lcd_digar_opt_default", "lcd_digar_batch", "lcd_digar_batch_tags", "lcd_digar_batch_ref", "lcd_region_read_slices_batch", "lcd_te_opt_default", "lcd_te_lib_create", "lcd_te_lib_destroy", "lcd_te_lib_n_seqs", "lcd_check_te_seq", "lcd_collect_te_info", "lcd_collect_te_info_from_cons", "lcd_annotate_te", "lcd_format_vcf_te", "lcd_pre_process_noisy_regs", "lcd_post_process_noisy_regs", "lcd_cr_merge", "lcd_sdust", "lcd_sdust_batch", "lcd_batch_add_region", "lcd_batch_add_region_from_chunk", "lcd_batch_add_region_from_chunk_packed", "lcd_batch_upload", "lcd_batch_run", "lcd_batch_run_many",
    "lcd_batch_download", "lcd_dispatch_create", "lcd_dispatch_destroy", "lcd_dispatch_n_devices", "lcd_dispatch_run", "lcd_dispatch_set_flags", "lcd_dispatch_busy", "lcd_batch_cost", "lcd_lpt_assign", "lcd_batch_region_result", "lcd_batch_region_sorted_ids", "lcd_batch_region_read_slices", "lcd_batch_get_stats", "lcd_batch_k4_jobs", "lcd_chunk_create", "lcd_chunk_create_from_bam", "lcd_chunk_create_from_bam_src", "lcd_chunk_read_sources", "lcd_chunk_stage_ms", "lcd_chunk_digars", "lcd_chunk_destroy", "lcd_chunk_n_reads", "lcd_chunk_read_info", "lcd_chunk_intervals", "lcd_chunk_region_slices", "lcd_batch_add_region_from_chunk_dev", "lcd_copy_counters", "lcd_batch_digest", "lcd_batch_materialize", "lcd_batch_region_results_arena",
    "lcd_edlib_batch", "lcd_edlib_batch_hw", "lcd_wfa_batch", "lcd_wfa_arena_bytes", "lcd_poa_batch", "lcd_assign_hap_germline", "lcd_assign_hap_batch", "lcd_flip_variant_hap", "lcd_stitch_chunks", "lcd_call_opt_default", "lcd_make_variants", "lcd_free_variants", "lcd_format_vcf", "lcd_read_tags", "lcd_update_digars_from_msa1", "lcd_bam_load_region", "lcd_bam_load_region_indexed", "lcd_bam_reads_free", "lcd_fasta_fetch", "lcd_vcf_header", "lcd_io_last_error",
    "lcd_region_job_cost", "lcd_region_jobs_pack", "lcd_batch_add_packed", "lcd_rebalance_plan", "lcd_rccl_unique_id", "lcd_comm_create", "lcd_comm_destroy", "lcd_comm_info", "lcd_rebalance_exchange", "lcd_rebalance_last_error",
    "lcd_clean_opt_default", "lcd_chunk_clean_vars", "lcd_chunk_clean_vars_batch", "lcd_clean_vars_free", "lcd_clean_vars_hap_problem",
    "lcd_merge_region_vars", "lcd_merge_region_vars_batch", "lcd_sort_noisy_regs",
    "lcd_pass_opt_default", "lcd_chunk_plan_pass", "lcd_chunk_plan_pass_batch", "lcd_pass_plan_free", "lcd_batch_region_n_cons", "lcd_batch_add_planned",
    "lcd_hap_state_init", "lcd_hap_state_carry", "lcd_hap_state_free", "lcd_chunks_noisy_rounds",
    "lcd_chunk_read_nm", "lcd_sort_chunk_reads", "lcd_chunks_first_round", "lcd_first_round_free",
    "lcd_cfg_default", "lcd_chunks_call", "lcd_call_bam_regions", "lcd_call_free",
    "lcd_bgzf_deflate_dev", "lcd_bgzf_deflate_dev_ptr", "lcd_deflated_size", "lcd_deflated_n_blocks", "lcd_deflated_kernel_ms", "lcd_deflated_block_info", "lcd_deflated_to_host", "lcd_deflated_free",
    "lcd_chunk_tag_records", "lcd_tagged_dev_ptr", "lcd_tagged_size", "lcd_tagged_n_records", "lcd_tagged_to_host", "lcd_tagged_free", "lcd_write_phased",
    "lcd_bam_contigs", "lcd_bam_contigs_free", "lcd_bam_sample_name", "lcd_plan_chunks", "lcd_chunk_plan_free", "lcd_stitch_chunks_carry", "lcd_stitch_carry_free",
    "lcd_chunk_open_from_bam", "lcd_chunk_resolve", "lcd_bam_writer_open", "lcd_bam_writer_append", "lcd_bam_writer_close", "lcd_bam_writer_abort",
    "lcd_vcf_writer_open", "lcd_vcf_writer_append", "lcd_vcf_writer_close", "lcd_vcf_writer_abort", "lcd_file_job_default", "lcd_file_stats_free",
    "lcd_bai_from_records", "lcd_bai_builder_create", "lcd_bai_builder_add_stream", "lcd_bai_builder_finish", "lcd_bai_builder_bytes", "lcd_bai_builder_destroy", "lcd_bai_build",
    "lcd_fai_build",
    "lcd_tbx_from_records", "lcd_vcf_index_builder_create", "lcd_vcf_index_builder_add_stream", "lcd_vcf_index_builder_finish", "lcd_vcf_index_builder_bytes",
    "lcd_vcf_index_builder_destroy", "lcd_vcf_index_build", "lcd_vcf_writer_open_idx", "lcd_call_files_ext",
    "lcd_chunk_open_from_bams", "lcd_chunk_n_files", "lcd_chunk_read_files", "lcd_merged_record_plan", "lcd_chunk_tag_records_sel", "lcd_call_files",
    "lcd_te_lib_from_fasta", "lcd_te_lib_from_fasta_free", "lcd_format_vcf_fields", "lcd_alt_read_names", "lcd_vcf_fields_out_free", "lcd_chunks_call_fields",
    "lcd_chunk_refine_records", "lcd_refine_log_create", "lcd_refine_log_free", "lcd_refine_log_n_entries", "lcd_refine_log_row_bytes", "lcd_refine_log_append",
    "lcd_refine_log_entry", "lcd_refine_log_apply", "lcd_chunks_noisy_rounds_log", "lcd_batch_region_ref_read_rows",
    "lcd_chunk_set_refine", "lcd_chunk_refine_log", "lcd_chunks_call_refine",
    "lcd_sam_names_create", "lcd_sam_names_free", "lcd_tagged_to_sam", "lcd_records_to_sam", "lcd_sam_text_size", "lcd_sam_text_dev_ptr", "lcd_sam_text_to_host", "lcd_sam_text_free",
    "lcd_bgzf_inflate_dev", "lcd_inflated_dev_ptr", "lcd_inflated_size", "lcd_inflated_n_blocks", "lcd_inflated_kernel_ms", "lcd_inflated_upload_ms", "lcd_inflated_to_host", "lcd_inflated_free",
    "lcd_mods_opt_default", "lcd_mods_opt_check", "lcd_chunk_mod_pileup", "lcd_mods_n_rows", "lcd_mods_rows_to_host", "lcd_mods_free", "lcd_mods_combine_rows", "lcd_mods_format", "lcd_call_files_ext2", "lcd_call_bam_regions_ext2",
    "lcd_depth_opt_default", "lcd_depth_opt_check", "lcd_chunk_depth", "lcd_depth_n_rows", "lcd_depth_rows_to_host", "lcd_depth_free", "lcd_depth_tile", "lcd_depth_windows", "lcd_depth_format",
    "lcd_split_opt_default", "lcd_split_opt_check", "lcd_split_paths", "lcd_split_offsets", "lcd_chunk_split_reads", "lcd_split_size", "lcd_split_dev_ptr", "lcd_split_to_host", "lcd_split_free",
    "lcd_hapvcf_opt_default", "lcd_phased_vcf_read", "lcd_phased_vcf_n_contigs", "lcd_phased_vcf_n_sites", "lcd_phased_vcf_n_phase_sets", "lcd_phased_vcf_pool_size",
    "lcd_phased_vcf_max_footprint", "lcd_phased_vcf_sites_to_host", "lcd_phased_vcf_free", "lcd_phased_vcf_errno", "lcd_phased_vcf_error",
    "lcd_haplotag_opt_default", "lcd_haplotag_opt_check", "lcd_chunk_haplotag", "lcd_haplotag_n_reads", "lcd_haplotag_n_records", "lcd_haplotag_to_host", "lcd_haplotag_n_candidates",
    "lcd_haplotag_pairs_to_host", "lcd_haplotag_free", "lcd_haplotag_files",
]


def load_library():
    """Load liblcd_hotpath.so; raises LcdError (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LcdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path.")
    lib = C.CDLL(LIB_PATH)
    u8p, i32p, u64p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.lcd_last_error.restype = C.c_char_p
    lib.lcd_version.restype = C.c_char_p
    lib.lcd_host_threads.argtypes = [i32p, i32p, i32p, i32p]
    lib.lcd_opt_default.argtypes = [C.POINTER(LcdOpt)]
    lib.lcd_init.argtypes = [C.c_int]
    lib.lcd_batch_create.restype = C.c_void_p
    lib.lcd_batch_create.argtypes = [C.POINTER(LcdOpt)]
    lib.lcd_dispatch_create.restype = C.c_void_p
    lib.lcd_dispatch_create.argtypes = [C.c_int, i32p, C.c_int]
    lib.lcd_dispatch_destroy.argtypes = [C.c_void_p]
    lib.lcd_dispatch_destroy.restype = None
    lib.lcd_dispatch_n_devices.argtypes = [C.c_void_p]
    lib.lcd_dispatch_run.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, i32p]
    lib.lcd_batch_cost.restype = C.c_double
    lib.lcd_batch_cost.argtypes = [C.c_void_p]
    lib.lcd_lpt_assign.restype = None
    lib.lcd_lpt_assign.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, i32p, C.POINTER(C.c_double)]
    lib.lcd_batch_region_read_slices.argtypes = [C.c_void_p, C.c_int, i32p, i32p, i32p, i32p]
    lib.lcd_batch_k4_jobs.argtypes = [C.c_void_p, C.c_int, u64p, i32p, u64p, i32p, C.POINTER(u8p), u64p]
    lib.lcd_end2end_aln.argtypes = [C.POINTER(LcdOpt), C.c_char_p, C.c_int, u8p, C.c_int, C.POINTER(u32p)]
    lib.lcd_wfa_collect_diff_ins_seq.argtypes = [C.POINTER(LcdOpt), u8p, C.c_int, u8p, C.c_int, C.POINTER(u8p)]
    lib.lcd_edlib_infix_aln.argtypes = [u8p, C.c_int, u8p, C.c_int, i32p, i32p]
    lib.lcd_wfa_heuristic_aln.argtypes = [u8p, C.c_int, u8p, C.c_int] + [C.c_int] * 6 + [i32p, i32p]
    lib.lcd_wfa_arena_bytes.restype = C.c_uint64
    lib.lcd_wfa_arena_bytes.argtypes = [C.c_int] * 8
    lib.lcd_batch_create_on.restype = C.c_void_p
    lib.lcd_batch_create_on.argtypes = [C.POINTER(LcdOpt), C.c_int]
    lib.lcd_set_thread_device.argtypes = [C.c_int]
    lib.lcd_alloc_events.restype = C.c_longlong
    lib.lcd_device_bytes.restype = C.c_longlong
    lib.lcd_device_bytes.argtypes = [C.c_int]
    lib.lcd_batch_destroy.argtypes = [C.c_void_p]
    lib.lcd_batch_destroy.restype = None
    lib.lcd_batch_clear.argtypes = [C.c_void_p]
    lib.lcd_batch_clear.restype = None
    lib.lcd_batch_add_region.argtypes = [C.c_void_p, C.c_int64, C.c_int, i32p, i32p, C.POINTER(u8p), C.POINTER(u8p), i32p, i32p,
                                         C.POINTER(C.c_int64), u8p, C.c_int]
    lib.lcd_batch_add_region_from_chunk.argtypes = [C.c_void_p, C.POINTER(LcdReadView), C.c_int64, C.c_int64, C.c_int, i32p, u8p, C.c_int]
    lib.lcd_batch_add_region_from_chunk_packed.argtypes = lib.lcd_batch_add_region_from_chunk.argtypes
    for f in ("lcd_batch_upload", "lcd_batch_run", "lcd_batch_download"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.lcd_batch_run_many.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.lcd_batch_region_result.argtypes = [C.c_void_p, C.c_int, i32p, C.POINTER(i32p), C.POINTER(C.POINTER(LcdAlnStr))]
    lib.lcd_batch_region_vars.argtypes = [C.c_void_p, C.c_int, C.c_int64, u8p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(LcdNoisyVar)), i32p,
                                          C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p)]
    i64p, u64p_ = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    lib.lcd_digar_opt_default.argtypes = [C.POINTER(LcdDigarOpt), C.c_int]
    lib.lcd_digar_opt_default.restype = None
    lib.lcd_digar_batch.argtypes = [C.POINTER(LcdDigarOpt), C.c_int, i64p, C.POINTER(C.c_uint32), u64p_, i32p, u8p, u64p_, i32p, u8p, C.c_int64, C.c_int64, C.c_int64,
                                    C.POINTER(u64p_), C.POINTER(C.POINTER(LcdDigar)), C.POINTER(u64p_), C.POINTER(C.POINTER(LcdNoisyIv)), C.POINTER(u8p), i32p, i64p, i64p, i32p]
    _dg_head = [C.POINTER(LcdDigarOpt), C.c_int, i64p, C.POINTER(C.c_uint32), u64p_, i32p]
    _dg_tail = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(u64p_), C.POINTER(C.POINTER(LcdDigar)), C.POINTER(u64p_), C.POINTER(C.POINTER(LcdNoisyIv)), C.POINTER(u8p), i32p, i64p, i64p, i32p]
    lib.lcd_digar_batch_tags.argtypes = [_dg_head[0], C.c_int] + _dg_head[1:] + [C.POINTER(C.c_char_p), u8p, u64p_, i32p, u8p] + _dg_tail
    lib.lcd_digar_batch_ref.argtypes = _dg_head + [u8p, u64p_, u8p, u64p_, i32p, u8p, C.c_char_p, C.c_int64, C.c_int64] + _dg_tail
    lib.lcd_region_read_slices_batch.argtypes = [C.c_int, i32p, i64p, i64p, C.c_int, u64p_, C.POINTER(LcdDigar), i32p, C.c_int, i32p, i32p, i32p]
    lib.lcd_pre_process_noisy_regs.argtypes = [C.POINTER(LcdNoisyIv), C.c_int, i64p, C.c_int, C.c_int, i64p, i64p, u64p_, C.POINTER(LcdNoisyIv), C.c_int, C.c_float,
                                               C.POINTER(C.POINTER(LcdNoisyIv))]
    lib.lcd_post_process_noisy_regs.argtypes = [C.POINTER(LcdNoisyIv), C.c_int, C.c_int, i64p, i32p, i32p, C.c_int, C.POINTER(C.POINTER(LcdNoisyIv))]
    lib.lcd_sdust.argtypes = [u8p, C.c_int64, C.c_int, C.c_int, C.POINTER(i64p)]
    lib.lcd_clean_opt_default.argtypes = [C.POINTER(LcdCleanOpt), C.c_int]
    lib.lcd_clean_opt_default.restype = None
    lib.lcd_chunk_clean_vars.argtypes = [C.c_void_p, C.POINTER(LcdCleanOpt), i32p, u8p, u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(LcdNoisyIv), C.c_int,
                                         i64p, C.c_int, C.POINTER(LcdCleanVars)]
    lib.lcd_chunk_clean_vars_batch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(LcdCleanOpt), C.POINTER(i32p), C.POINTER(u8p), C.POINTER(u8p), i64p, i64p, i64p,
                                               i64p, C.POINTER(C.POINTER(LcdNoisyIv)), i32p, C.POINTER(i64p), i32p, C.POINTER(LcdCleanVars)]
    lib.lcd_clean_vars_free.argtypes = [C.POINTER(LcdCleanVars)]
    lib.lcd_clean_vars_free.restype = None
    lib.lcd_clean_vars_hap_problem.argtypes = [C.POINTER(LcdCleanVars), C.c_int, i32p, u8p, i32p, i32p, C.POINTER(LcdHapProblem)]
    lib.lcd_merge_region_vars.argtypes = [C.POINTER(LcdCleanVars), C.c_int, C.POINTER(LcdRegionVars), i32p, u8p, C.POINTER(LcdCleanVars), i32p, C.POINTER(i32p)]
    lib.lcd_merge_region_vars_batch.argtypes = [C.c_int, C.POINTER(C.POINTER(LcdCleanVars)), i32p, C.POINTER(C.POINTER(LcdRegionVars)), C.POINTER(i32p), C.POINTER(u8p),
                                                C.POINTER(LcdCleanVars), C.POINTER(i32p), C.POINTER(C.POINTER(i32p))]
    lib.lcd_sort_noisy_regs.argtypes = [C.POINTER(LcdNoisyIv), C.c_int, i32p]
    lib.lcd_pass_opt_default.argtypes = [C.POINTER(LcdPassOpt)]
    lib.lcd_pass_opt_default.restype = None
    lib.lcd_chunk_plan_pass.argtypes = [C.c_void_p, C.POINTER(LcdPassOpt), C.c_int, C.POINTER(LcdNoisyIv), i32p, i32p, u8p, C.c_int64, C.c_int64, C.POINTER(LcdPassPlan)]
    lib.lcd_chunk_plan_pass_batch.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(LcdPassOpt), i32p, C.POINTER(C.POINTER(LcdNoisyIv)), C.POINTER(i32p), C.POINTER(i32p),
                                              C.POINTER(u8p), i64p, i64p, C.POINTER(LcdPassPlan)]
    lib.lcd_pass_plan_free.argtypes = [C.POINTER(LcdPassPlan)]
    lib.lcd_pass_plan_free.restype = None
    lib.lcd_batch_region_n_cons.argtypes = [C.c_void_p, C.c_int]
    lib.lcd_batch_add_planned.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LcdPassPlan), i32p, i64p, u8p, C.c_int64, i32p]
    lib.lcd_hap_state_init.argtypes = [C.c_int, C.c_int, C.POINTER(LcdHapState)]
    lib.lcd_hap_state_carry.argtypes = [C.POINTER(LcdHapState), C.c_int, i32p, C.POINTER(LcdHapState)]
    lib.lcd_hap_state_free.argtypes = [C.POINTER(LcdHapState)]
    lib.lcd_hap_state_free.restype = None
    lib.lcd_chunks_noisy_rounds.argtypes = [C.c_int, C.POINTER(LcdRoundsChunk), C.POINTER(LcdOpt), C.POINTER(LcdPassOpt)]
    lib.lcd_chunk_read_nm.argtypes = [C.c_void_p, i32p]
    lib.lcd_sort_chunk_reads.argtypes = [C.c_int, i64p, i64p, i32p, u64p_, C.c_char_p, i32p]
    lib.lcd_chunks_first_round.argtypes = [C.c_int, C.POINTER(LcdFirstChunk), C.POINTER(LcdCleanOpt)]
    lib.lcd_first_round_free.argtypes = [C.POINTER(LcdFirstChunk)]
    lib.lcd_first_round_free.restype = None
    lib.lcd_cfg_default.argtypes = [C.POINTER(LcdCfg), C.c_int]
    lib.lcd_cfg_default.restype = None
    lib.lcd_chunks_call.argtypes = [C.c_int, C.POINTER(LcdCallChunk), C.POINTER(LcdCfg), C.c_char_p, C.POINTER(C.POINTER(LcdVar1)), i32p, C.POINTER(C.c_void_p)]
    lib.lcd_call_bam_regions.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, i64p, i64p, C.c_int, C.POINTER(LcdCfg), C.POINTER(LcdCallChunk),
                                         C.POINTER(C.POINTER(LcdVar1)), i32p, C.POINTER(C.c_void_p), C.POINTER(LcdBamOut), C.POINTER(LcdRunOpt), C.POINTER(LcdRunOut)]
    lib.lcd_write_phased.argtypes = [C.c_char_p, C.c_int, C.POINTER(LcdCallChunk), C.POINTER(LcdBamOut), C.POINTER(LcdWriterOpt)]
    for f in ("lcd_bgzf_deflate_dev", "lcd_bgzf_deflate_dev_ptr", "lcd_chunk_tag_records"):
        getattr(lib, f).restype = C.c_void_p
    lib.lcd_bgzf_deflate_dev.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
    lib.lcd_bgzf_deflate_dev_ptr.argtypes = [C.c_uint64, C.c_size_t, C.c_int, C.c_int]
    lib.lcd_chunk_tag_records.argtypes = [C.c_void_p, i32p, i64p, C.c_int, C.c_int]
    for f in ("lcd_deflated_size", "lcd_deflated_n_blocks", "lcd_tagged_size"):
        getattr(lib, f).restype = C.c_size_t
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.lcd_deflated_kernel_ms.restype = C.c_double
    lib.lcd_deflated_kernel_ms.argtypes = [C.c_void_p]
    lib.lcd_deflated_block_info.argtypes = [C.c_void_p, C.c_size_t, u32p, u32p, i32p]
    lib.lcd_tagged_dev_ptr.restype = C.c_uint64
    lib.lcd_tagged_dev_ptr.argtypes = [C.c_void_p]
    lib.lcd_tagged_n_records.argtypes = [C.c_void_p]
    for f in ("lcd_deflated_to_host", "lcd_tagged_to_host"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_char_p]
    for f in ("lcd_deflated_free", "lcd_tagged_free"):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = None
    lib.lcd_call_free.argtypes = [C.c_int, C.POINTER(LcdCallChunk), C.POINTER(LcdVar1), C.c_int, C.c_void_p]
    strv, i64p_ = C.POINTER(C.c_char_p), C.POINTER(C.c_int64)
    lib.lcd_bam_contigs.argtypes = [C.c_char_p, i32p, C.POINTER(C.POINTER(C.c_void_p)), C.POINTER(i64p_)]
    lib.lcd_bam_contigs_free.argtypes = [C.c_int, C.POINTER(C.c_void_p), i64p_]
    lib.lcd_bam_contigs_free.restype = None
    lib.lcd_bam_sample_name.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.lcd_plan_chunks.argtypes = [C.c_int, strv, i64p_, C.c_int, C.c_int, strv, C.c_int, strv, C.c_char_p, C.c_int64, C.POINTER(LcdChunkPlan)]
    lib.lcd_chunk_plan_free.argtypes = [C.POINTER(LcdChunkPlan)]
    lib.lcd_chunk_plan_free.restype = None
    lib.lcd_stitch_chunks_carry.argtypes = [C.POINTER(LcdChunkPhase), C.c_int, C.c_int, C.POINTER(LcdStitchCarry), C.POINTER(LcdStitchCarry)]
    lib.lcd_stitch_carry_free.argtypes = [C.POINTER(LcdStitchCarry)]
    lib.lcd_stitch_carry_free.restype = None
    lib.lcd_chunk_open_from_bam.restype = C.c_void_p
    lib.lcd_chunk_open_from_bam.argtypes = [C.POINTER(LcdDigarOpt), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_chunk_resolve.argtypes = [C.c_void_p, C.POINTER(LcdChunkSrc)]
    lib.lcd_bam_writer_open.restype = C.c_void_p
    lib.lcd_bam_writer_open.argtypes = [C.c_char_p, C.POINTER(LcdBamOut), C.POINTER(LcdWriterOpt)]
    lib.lcd_bam_writer_append.argtypes = [C.c_void_p, C.c_int, C.POINTER(LcdCallChunk), i32p, C.POINTER(LcdStitchCarry)]
    lib.lcd_bam_writer_close.argtypes = [C.c_void_p]
    lib.lcd_bam_writer_abort.argtypes = [C.c_void_p]
    lib.lcd_bam_writer_abort.restype = None
    lib.lcd_vcf_writer_open.restype = C.c_void_p
    lib.lcd_vcf_writer_open.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    lib.lcd_vcf_writer_append.argtypes = [C.c_void_p, C.c_char_p]
    lib.lcd_vcf_writer_close.argtypes = [C.c_void_p]
    lib.lcd_vcf_writer_abort.argtypes = [C.c_void_p]
    lib.lcd_vcf_writer_abort.restype = None
    lib.lcd_file_job_default.argtypes = [C.POINTER(LcdFileJob)]
    lib.lcd_file_job_default.restype = None
    lib.lcd_call_files.argtypes = [C.POINTER(LcdInputs), C.POINTER(LcdFileJob), C.POINTER(LcdCfg), C.POINTER(LcdRunOpt), C.POINTER(LcdFileStats), C.POINTER(LcdRunOut)]
    lib.lcd_file_stats_free.argtypes = [C.POINTER(LcdFileStats)]
    lib.lcd_bai_from_records.argtypes = [C.c_int, C.c_int64, i32p, i64p, i64p, i32p, u64p_, u64p_, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.lcd_bai_builder_create.restype = C.c_void_p
    lib.lcd_bai_builder_create.argtypes = [C.c_int, i64p]
    lib.lcd_bai_builder_add_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(LcdBaiMember), C.c_uint64, C.POINTER(C.c_size_t)]
    lib.lcd_bai_builder_finish.argtypes = [C.c_void_p, C.c_char_p]
    lib.lcd_bai_builder_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.lcd_bai_builder_destroy.argtypes = [C.c_void_p]
    lib.lcd_bai_builder_destroy.restype = None
    lib.lcd_bai_build.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(LcdBaiOpt), C.POINTER(LcdBaiStats)]
    lib.lcd_tbx_from_records.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int64, C.c_int64, i32p, i64p, i64p, u64p_, u64p_, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.lcd_vcf_index_builder_create.restype = C.c_void_p
    lib.lcd_vcf_index_builder_create.argtypes = [C.c_int]
    lib.lcd_vcf_index_builder_add_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(LcdBaiMember), C.c_uint64, C.POINTER(C.c_size_t)]
    lib.lcd_vcf_index_builder_finish.argtypes = [C.c_void_p, C.c_char_p]
    lib.lcd_vcf_index_builder_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.lcd_vcf_index_builder_destroy.argtypes = [C.c_void_p]
    lib.lcd_vcf_index_builder_destroy.restype = None
    lib.lcd_vcf_index_build.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(LcdVcfIndexOpt), C.POINTER(LcdVcfIndexStats)]
    lib.lcd_call_files_ext.argtypes = [C.POINTER(LcdInputs), C.POINTER(LcdFileJob), C.POINTER(LcdCfg), C.POINTER(LcdRunOpt), C.POINTER(LcdFileStats), C.POINTER(LcdRunOut),
                                       C.POINTER(LcdRunExt)]
    lib.lcd_vcf_writer_open_idx.restype = C.c_void_p
    lib.lcd_vcf_writer_open_idx.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(LcdVcfIndexOpt)]
    lib.lcd_fai_build.argtypes = [C.c_char_p, C.c_char_p]
    lib.lcd_file_stats_free.restype = None
    lib.lcd_chunk_open_from_bams.restype = C.c_void_p
    lib.lcd_chunk_open_from_bams.argtypes = [C.POINTER(LcdDigarOpt), C.c_int, strv, strv, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_chunk_n_files.argtypes = [C.c_void_p]
    lib.lcd_chunk_read_files.argtypes = [C.c_void_p, i32p]
    lib.lcd_merged_record_plan.argtypes = [C.c_int, i32p, i64p, i64p, C.c_int, C.c_int64, C.c_int64, C.c_int, u8p, i32p]
    lib.lcd_chunk_tag_records_sel.restype = C.c_void_p
    lib.lcd_chunk_tag_records_sel.argtypes = [C.c_void_p, i32p, i64p, u8p, i32p]
    lib.lcd_refine_log_create.restype = C.c_void_p
    lib.lcd_refine_log_free.argtypes = [C.c_void_p]
    lib.lcd_refine_log_free.restype = None
    for f in ("lcd_refine_log_n_entries", "lcd_refine_log_row_bytes"):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_int64
    lib.lcd_refine_log_append.argtypes = [C.c_void_p, C.POINTER(LcdRefineEntry)]
    lib.lcd_refine_log_entry.argtypes = [C.c_void_p, C.c_int64, C.POINTER(LcdRefineEntry)]
    lib.lcd_refine_log_apply.argtypes = [C.c_void_p, C.c_int, u64p_, C.POINTER(LcdDigar), i32p, i32p, C.POINTER(i32p), C.POINTER(u64p_), C.POINTER(C.POINTER(LcdDigar)), i64p]
    lib.lcd_chunks_noisy_rounds_log.argtypes = [C.c_int, C.POINTER(LcdRoundsChunk), C.POINTER(LcdOpt), C.POINTER(LcdPassOpt), C.POINTER(C.c_void_p)]
    lib.lcd_batch_region_ref_read_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, C.POINTER(u8p), C.POINTER(u8p)]
    lib.lcd_chunk_refine_records.restype = C.c_void_p
    lib.lcd_chunk_refine_records.argtypes = [C.c_void_p, C.c_int, i32p, u64p_, C.POINTER(LcdDigar), C.c_char_p, C.c_int64, C.c_int64, i32p, i64p, u8p, i32p,
                                             C.POINTER(LcdRefineStats)]
    lib.lcd_call_free.restype = None
    fo = C.POINTER(LcdVcfFieldsOut)
    lib.lcd_te_lib_from_fasta.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(i32p), i32p]
    lib.lcd_te_lib_from_fasta_free.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), i32p, C.c_int]
    lib.lcd_te_lib_from_fasta_free.restype = None
    lib.lcd_format_vcf_fields.argtypes = [C.POINTER(LcdCallOpt), C.c_char_p, C.POINTER(LcdVar1), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, u64p_, C.c_char_p,
                                          C.POINTER(C.c_void_p), i32p]
    lib.lcd_alt_read_names.argtypes = [C.POINTER(LcdVar1), C.c_int, u64p_, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.lcd_vcf_fields_out_free.argtypes = [fo]
    lib.lcd_vcf_fields_out_free.restype = None
    lib.lcd_chunks_call_fields.argtypes = [C.c_int, C.POINTER(LcdCallChunk), C.POINTER(LcdCfg), C.c_char_p, C.POINTER(LcdVcfFields), C.POINTER(C.POINTER(LcdVar1)), i32p,
                                           C.POINTER(C.c_void_p), fo]
    lib.lcd_batch_region_sorted_ids.argtypes = [C.c_void_p, C.c_int, i32p]
    lib.lcd_batch_get_stats.argtypes = [C.c_void_p, C.POINTER(LcdBatchStats)]
    lib.lcd_batch_digest.argtypes = [C.c_void_p]
    lib.lcd_batch_digest.restype = C.c_uint64
    lib.lcd_batch_materialize.argtypes = [C.c_void_p]
    lib.lcd_batch_materialize.restype = C.c_uint64
    lib.lcd_edlib_batch.argtypes = [C.c_int, u8p, C.c_uint64, u64p, i32p, u64p, i32p, i32p, i32p, i32p, i32p]
    lib.lcd_edlib_batch_hw.argtypes = [C.c_int, u8p, C.c_uint64, u64p, i32p, u64p, i32p, i32p, i32p, i32p, i32p, i32p, i32p]
    lib.lcd_wfa_batch.argtypes = [C.c_int, u8p, C.c_uint64, u64p, i32p, u64p, i32p, i32p] + [C.c_int] * 6 + [i32p, u32p, C.c_int, i32p, u8p, C.c_int, i32p]
    lib.lcd_poa_batch.argtypes = [C.POINTER(LcdOpt), C.c_int, i32p, i32p, i32p, C.c_int, u64p, i32p, i32p, i32p, u8p, C.c_uint64, i32p,
                                  i32p, i32p, i32p, i32p, u8p, C.c_int, u8p, C.c_int, C.c_int, i32p]
    lib.lcd_assign_hap_germline.argtypes = [C.POINTER(LcdHapProblem), C.c_int]
    lib.lcd_assign_hap_batch.argtypes = [C.c_int, C.POINTER(LcdHapProblem), i32p]
    lib.lcd_wfa_end2end_aln.argtypes = [u8p, C.c_int, u8p, C.c_int] + [C.c_int] * 8 + [C.POINTER(u32p), i32p, C.POINTER(u8p), C.POINTER(u8p), i32p]
    lib.lcd_edlib_end2end_aln.argtypes = [u8p, C.c_int, u8p, C.c_int, i32p, i32p]
    lib.lcd_edlib_xgaps.argtypes = [u8p, C.c_int, u8p, C.c_int]
    lib.lcd_edlib_edit_distance.argtypes = [u8p, C.c_int, u8p, C.c_int]
    lib.lcd_collect_noisy_reg_aln_strs.argtypes = [C.POINTER(LcdOpt), C.POINTER(LcdReadView), C.c_int64, C.c_int64, C.c_int, C.c_int, i32p,
                                                   u8p, C.c_int, i32p, C.POINTER(i32p), C.POINTER(C.POINTER(LcdAlnStr))]
    lib.lcd_chunk_set_refine.argtypes = [C.c_void_p, C.c_int]
    lib.lcd_chunk_refine_log.restype = C.c_void_p
    lib.lcd_chunk_refine_log.argtypes = [C.c_void_p]
    lib.lcd_chunks_call_refine.argtypes = lib.lcd_chunks_call.argtypes
    ssp = C.POINTER(LcdSamStats)
    lib.lcd_sam_names_create.restype = C.c_void_p
    lib.lcd_sam_names_create.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    lib.lcd_sam_names_free.argtypes = [C.c_void_p]
    lib.lcd_sam_names_free.restype = None
    lib.lcd_tagged_to_sam.restype = C.c_void_p
    lib.lcd_tagged_to_sam.argtypes = [C.c_void_p, C.c_void_p, ssp]
    lib.lcd_records_to_sam.restype = C.c_void_p
    lib.lcd_records_to_sam.argtypes = [u8p, C.c_size_t, C.c_void_p, ssp]
    lib.lcd_sam_text_size.restype = C.c_size_t
    lib.lcd_sam_text_size.argtypes = [C.c_void_p]
    lib.lcd_sam_text_dev_ptr.restype = C.c_uint64
    lib.lcd_sam_text_dev_ptr.argtypes = [C.c_void_p]
    lib.lcd_sam_text_to_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, u8p]
    lib.lcd_sam_text_free.argtypes = [C.c_void_p]
    lib.lcd_sam_text_free.restype = None
    i64p_m = C.POINTER(C.c_int64)
    lib.lcd_mods_opt_default.argtypes = [C.POINTER(LcdModsOpt)]
    lib.lcd_mods_opt_default.restype = None
    lib.lcd_mods_opt_check.argtypes = [C.POINTER(LcdModsOpt)]
    lib.lcd_chunk_mod_pileup.restype = C.c_void_p
    lib.lcd_chunk_mod_pileup.argtypes = [C.c_void_p, i32p, C.POINTER(LcdModsOpt), C.POINTER(LcdModsStats)]
    lib.lcd_mods_n_rows.argtypes = [C.c_void_p]
    lib.lcd_mods_rows_to_host.argtypes = [C.c_void_p, i64p_m, C.c_char_p, u32p]
    lib.lcd_mods_free.argtypes = [C.c_void_p]
    lib.lcd_call_files_ext2.argtypes = list(lib.lcd_call_files_ext.argtypes) + [C.POINTER(LcdRunExt2)]
    lib.lcd_call_bam_regions_ext2.argtypes = list(lib.lcd_call_bam_regions.argtypes) + [C.POINTER(LcdRunExt2)]
    lib.lcd_mods_free.restype = None
    lib.lcd_depth_opt_default.argtypes = [C.POINTER(LcdDepthOpt)]
    lib.lcd_depth_opt_default.restype = None
    lib.lcd_depth_opt_check.argtypes = [C.POINTER(LcdDepthOpt)]
    lib.lcd_chunk_depth.argtypes = [C.c_void_p, i32p, C.POINTER(LcdDepthOpt), C.POINTER(LcdDepthStats)]
    lib.lcd_chunk_depth.restype = C.c_void_p
    lib.lcd_depth_n_rows.argtypes = [C.c_void_p]
    lib.lcd_depth_rows_to_host.argtypes = [C.c_void_p, i64p_m, i64p_m, u32p]
    lib.lcd_depth_free.argtypes = [C.c_void_p]
    lib.lcd_depth_free.restype = None
    lib.lcd_depth_tile.argtypes = []
    lib.lcd_depth_windows.argtypes = [C.c_int, i64p_m, i64p_m, u32p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.lcd_depth_format.argtypes = [C.c_int, i64p_m, i64p_m, u32p, C.POINTER(C.c_uint64), C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.lcd_split_opt_default.argtypes = [C.POINTER(LcdSplitOpt)]
    lib.lcd_split_opt_default.restype = None
    lib.lcd_split_opt_check.argtypes = [C.POINTER(LcdSplitOpt)]
    lib.lcd_split_paths.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
    lib.lcd_split_offsets.argtypes = [C.c_int, i32p, u64p, u64p, u64p, u64p, u64p]
    lib.lcd_chunk_split_reads.restype = C.c_void_p
    lib.lcd_chunk_split_reads.argtypes = [C.c_void_p, i32p, i64p_m, u8p, i32p, C.c_void_p, C.POINTER(LcdSplitOpt), C.POINTER(LcdSplitStats)]
    lib.lcd_split_size.restype = C.c_size_t
    lib.lcd_split_size.argtypes = [C.c_void_p, C.c_int]
    lib.lcd_split_dev_ptr.restype = C.c_uint64
    lib.lcd_split_dev_ptr.argtypes = [C.c_void_p, C.c_int]
    lib.lcd_split_to_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, u8p]
    lib.lcd_split_free.argtypes = [C.c_void_p]
    lib.lcd_split_free.restype = None
    lib.lcd_hapvcf_opt_default.argtypes = [C.POINTER(LcdHapvcfOpt)]
    lib.lcd_hapvcf_opt_default.restype = None
    lib.lcd_phased_vcf_read.restype = C.c_void_p
    lib.lcd_phased_vcf_read.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(LcdHapvcfOpt), C.POINTER(LcdHapvcfStats)]
    lib.lcd_phased_vcf_n_contigs.argtypes = [C.c_void_p]
    for f in (lib.lcd_phased_vcf_n_sites, lib.lcd_phased_vcf_n_phase_sets, lib.lcd_phased_vcf_pool_size, lib.lcd_phased_vcf_max_footprint):
        f.argtypes = [C.c_void_p, C.c_int]
    lib.lcd_phased_vcf_n_sites.restype = C.c_int64
    lib.lcd_phased_vcf_pool_size.restype = C.c_int64
    lib.lcd_phased_vcf_sites_to_host.argtypes = [C.c_void_p, C.c_int, i64p_m, u8p, u8p, i32p, u8p, u8p, i64p_m, i32p, i64p_m, u8p]
    lib.lcd_phased_vcf_free.argtypes = [C.c_void_p]
    lib.lcd_phased_vcf_free.restype = None
    lib.lcd_phased_vcf_errno.argtypes = []
    lib.lcd_phased_vcf_error.argtypes = []
    lib.lcd_phased_vcf_error.restype = C.c_char_p
    lib.lcd_haplotag_opt_default.argtypes = [C.POINTER(LcdHaplotagOpt)]
    lib.lcd_haplotag_opt_default.restype = None
    lib.lcd_haplotag_opt_check.argtypes = [C.POINTER(LcdHaplotagOpt)]
    lib.lcd_chunk_haplotag.restype = C.c_void_p
    lib.lcd_chunk_haplotag.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(LcdHaplotagOpt), C.POINTER(LcdHaplotagStats)]
    lib.lcd_haplotag_n_reads.argtypes = [C.c_void_p]
    lib.lcd_haplotag_n_records.argtypes = [C.c_void_p]
    lib.lcd_haplotag_to_host.argtypes = [C.c_void_p, i32p, i64p_m, i32p, i32p]
    lib.lcd_haplotag_n_candidates.argtypes = [C.c_void_p]
    lib.lcd_haplotag_n_candidates.restype = C.c_int64
    lib.lcd_haplotag_pairs_to_host.argtypes = [C.c_void_p, i64p_m, i64p_m, u8p]
    lib.lcd_haplotag_free.argtypes = [C.c_void_p]
    lib.lcd_haplotag_free.restype = None
    lib.lcd_mods_combine_rows.argtypes = [C.c_int, i64p_m, C.c_char_p, u32p]
    lib.lcd_mods_format.argtypes = [C.c_int, i64p_m, C.c_char_p, u32p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    _lib = lib
    return lib


def check(rc, lib=None):
    if rc < 0:
        lib = lib or load_library()
        raise LcdError(f"liblcd_hotpath error {rc}: {lib.lcd_last_error().decode()}")
    return rc
