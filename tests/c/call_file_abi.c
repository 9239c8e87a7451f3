/* TEST ONLY: sizes and field offsets of the whole-file structs of include/lcd_hotpath.h, one "struct.field offset" line each ("struct size" for the size):
 * tests/test_call_file_abi.py compiles this file and compares them with the ctypes mirrors of longcalld_amd/_lib.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"

#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
    SZ(lcd_chunk_plan_t);
    OFF(lcd_chunk_plan_t, n); OFF(lcd_chunk_plan_t, tid); OFF(lcd_chunk_plan_t, reg_beg); OFF(lcd_chunk_plan_t, reg_end); OFF(lcd_chunk_plan_t, fallback);
    SZ(lcd_stitch_carry_t);
    OFF(lcd_stitch_carry_t, valid); OFF(lcd_stitch_carry_t, tid); OFF(lcd_stitch_carry_t, reg_beg); OFF(lcd_stitch_carry_t, reg_end); OFF(lcd_stitch_carry_t, n_reads);
    OFF(lcd_stitch_carry_t, n_vars); OFF(lcd_stitch_carry_t, n_down_ovlp); OFF(lcd_stitch_carry_t, is_skipped); OFF(lcd_stitch_carry_t, haps);
    OFF(lcd_stitch_carry_t, phase_sets); OFF(lcd_stitch_carry_t, down_ovlp_read_i);
    SZ(lcd_chunk_phase_t);
    OFF(lcd_chunk_phase_t, tid); OFF(lcd_chunk_phase_t, n_reads); OFF(lcd_chunk_phase_t, n_vars); OFF(lcd_chunk_phase_t, ordered_read_ids); OFF(lcd_chunk_phase_t, is_skipped);
    OFF(lcd_chunk_phase_t, haps); OFF(lcd_chunk_phase_t, phase_sets); OFF(lcd_chunk_phase_t, var_phase_set); OFF(lcd_chunk_phase_t, hap_to_cons_alle);
    OFF(lcd_chunk_phase_t, n_up_ovlp); OFF(lcd_chunk_phase_t, n_down_ovlp); OFF(lcd_chunk_phase_t, up_ovlp_read_i); OFF(lcd_chunk_phase_t, down_ovlp_read_i);
    OFF(lcd_chunk_phase_t, flip_hap); OFF(lcd_chunk_phase_t, flip_pre_PS); OFF(lcd_chunk_phase_t, flip_cur_PS);
    SZ(lcd_bam_out_t);
    SZ(lcd_file_job_t);
    OFF(lcd_file_job_t, bam_path); OFF(lcd_file_job_t, bai_path); OFF(lcd_file_job_t, fasta_path); OFF(lcd_file_job_t, contig_mode); OFF(lcd_file_job_t, n_exclude);
    OFF(lcd_file_job_t, exclude); OFF(lcd_file_job_t, n_regions); OFF(lcd_file_job_t, regions); OFF(lcd_file_job_t, region_bed_path); OFF(lcd_file_job_t, chunk_len);
    OFF(lcd_file_job_t, window_chunks); OFF(lcd_file_job_t, overlap); OFF(lcd_file_job_t, loader_threads); OFF(lcd_file_job_t, min_mapq); OFF(lcd_file_job_t, vcf_path);
    OFF(lcd_file_job_t, vcf_bgzf); OFF(lcd_file_job_t, no_vcf_header); OFF(lcd_file_job_t, sample_name); OFF(lcd_file_job_t, source_version); OFF(lcd_file_job_t, cmdline);
    OFF(lcd_file_job_t, date_yyyymmdd); OFF(lcd_file_job_t, bam_out); OFF(lcd_file_job_t, keep_records);
    SZ(lcd_file_stats_t);
    OFF(lcd_file_stats_t, n_planned); OFF(lcd_file_stats_t, n_loaded); OFF(lcd_file_stats_t, n_empty); OFF(lcd_file_stats_t, n_windows); OFF(lcd_file_stats_t, plan_fallback);
    OFF(lcd_file_stats_t, n_reads); OFF(lcd_file_stats_t, n_records); OFF(lcd_file_stats_t, n_vcf_lines); OFF(lcd_file_stats_t, n_region_loads); OFF(lcd_file_stats_t, ms_load);
    OFF(lcd_file_stats_t, ms_call); OFF(lcd_file_stats_t, ms_write); OFF(lcd_file_stats_t, ms_wall); OFF(lcd_file_stats_t, peak_device_bytes); OFF(lcd_file_stats_t, n_chunks);
    OFF(lcd_file_stats_t, chunk_tid); OFF(lcd_file_stats_t, chunk_reg_beg); OFF(lcd_file_stats_t, chunk_reg_end); OFF(lcd_file_stats_t, chunk_n_reads);
    OFF(lcd_file_stats_t, chunk_n_passes); OFF(lcd_file_stats_t, chunk_flip_hap); OFF(lcd_file_stats_t, chunk_n_records); OFF(lcd_file_stats_t, chunk_flip_pre_PS);
    OFF(lcd_file_stats_t, chunk_flip_cur_PS); OFF(lcd_file_stats_t, records); OFF(lcd_file_stats_t, n_kept_records);
    printf("LCD_CTG_AUTOSOME_XY %d\nLCD_CTG_AUTOSOME %d\nLCD_CTG_ALL %d\n", LCD_CTG_AUTOSOME_XY, LCD_CTG_AUTOSOME, LCD_CTG_ALL);
    return 0;
}
