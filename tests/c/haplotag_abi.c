/* the haplotag structs as a C compiler lays them out: prints "name size" and "name.member offset" lines for tests/test_haplotag_abi.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
    SZ(lcd_hapvcf_opt_t); OFF(lcd_hapvcf_opt_t, max_indel); OFF(lcd_hapvcf_opt_t, snvs_only); OFF(lcd_hapvcf_opt_t, reserved);
    SZ(lcd_hapvcf_stats_t); OFF(lcd_hapvcf_stats_t, n_lines); OFF(lcd_hapvcf_stats_t, n_sites); OFF(lcd_hapvcf_stats_t, n_unknown_contig); OFF(lcd_hapvcf_stats_t, n_filtered);
    OFF(lcd_hapvcf_stats_t, n_unphased); OFF(lcd_hapvcf_stats_t, n_hom); OFF(lcd_hapvcf_stats_t, n_other_gt); OFF(lcd_hapvcf_stats_t, n_both_alt); OFF(lcd_hapvcf_stats_t, n_symbolic);
    OFF(lcd_hapvcf_stats_t, n_complex); OFF(lcd_hapvcf_stats_t, n_long_indel); OFF(lcd_hapvcf_stats_t, n_indel_off); OFF(lcd_hapvcf_stats_t, n_snv); OFF(lcd_hapvcf_stats_t, n_ins);
    OFF(lcd_hapvcf_stats_t, n_del); OFF(lcd_hapvcf_stats_t, n_phase_sets);
    SZ(lcd_haplotag_opt_t); OFF(lcd_haplotag_opt_t, min_bq); OFF(lcd_haplotag_opt_t, min_diff); OFF(lcd_haplotag_opt_t, reserved);
    SZ(lcd_haplotag_stats_t); OFF(lcd_haplotag_stats_t, n_records); OFF(lcd_haplotag_stats_t, n_pairs); OFF(lcd_haplotag_stats_t, n_verdict); OFF(lcd_haplotag_stats_t, n_tagged);
    OFF(lcd_haplotag_stats_t, n_multi_ps); OFF(lcd_haplotag_stats_t, n_cg); OFF(lcd_haplotag_stats_t, n_bad_record); OFF(lcd_haplotag_stats_t, n_no_seq);
    OFF(lcd_haplotag_stats_t, ms_measure); OFF(lcd_haplotag_stats_t, ms_mark); OFF(lcd_haplotag_stats_t, ms_reduce);
    SZ(lcd_haplotag_run_t); OFF(lcd_haplotag_run_t, size); OFF(lcd_haplotag_run_t, vcf_path); OFF(lcd_haplotag_run_t, sample); OFF(lcd_haplotag_run_t, max_indel);
    OFF(lcd_haplotag_run_t, snvs_only); OFF(lcd_haplotag_run_t, min_bq); OFF(lcd_haplotag_run_t, min_diff); OFF(lcd_haplotag_run_t, vcf_stats); OFF(lcd_haplotag_run_t, stats);
    return 0;
}
