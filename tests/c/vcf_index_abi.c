/* TEST ONLY: sizes and field offsets of the VCF index structs of include/lcd_hotpath.h of lcd_run_ext_t that carries them into a run and of the two older option structs (which stay as they were), one "struct.field offset"
 * line each ("struct size" for the size), and the new constants.  Plain C against the public header; no library is needed. */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
    S(lcd_vcf_index_stats_t); F(lcd_vcf_index_stats_t, n_lines); F(lcd_vcf_index_stats_t, n_data_lines); F(lcd_vcf_index_stats_t, n_meta_lines); F(lcd_vcf_index_stats_t, n_contigs);
    F(lcd_vcf_index_stats_t, n_chunks); F(lcd_vcf_index_stats_t, n_slabs); F(lcd_vcf_index_stats_t, n_members); F(lcd_vcf_index_stats_t, bytes_in); F(lcd_vcf_index_stats_t, bytes_inflated);
    F(lcd_vcf_index_stats_t, bytes_index); F(lcd_vcf_index_stats_t, bytes_file); F(lcd_vcf_index_stats_t, depth); F(lcd_vcf_index_stats_t, wrote); F(lcd_vcf_index_stats_t, skipped);
    F(lcd_vcf_index_stats_t, pad); F(lcd_vcf_index_stats_t, skip_reason); F(lcd_vcf_index_stats_t, ms_read); F(lcd_vcf_index_stats_t, ms_inflate); F(lcd_vcf_index_stats_t, ms_lines);
    F(lcd_vcf_index_stats_t, ms_entry); F(lcd_vcf_index_stats_t, ms_finish); F(lcd_vcf_index_stats_t, ms_wall);
    S(lcd_vcf_index_opt_t); F(lcd_vcf_index_opt_t, format); F(lcd_vcf_index_opt_t, index_path); F(lcd_vcf_index_opt_t, slab_members); F(lcd_vcf_index_opt_t, verify_crc);
    F(lcd_vcf_index_opt_t, stats);
    S(lcd_run_ext_t); F(lcd_run_ext_t, vcf_idx); F(lcd_run_ext_t, vcf_idx_stats);
    S(lcd_run_opt_t); F(lcd_run_opt_t, idx); F(lcd_run_opt_t, fields); F(lcd_run_opt_t, aln);
    S(lcd_run_out_t); F(lcd_run_out_t, idx_stats); F(lcd_run_out_t, n_reads_per_file); F(lcd_run_out_t, fields_out); F(lcd_run_out_t, refine_stats); F(lcd_run_out_t, sam_stats);
    printf("LCD_ERR_VIDX_ORDER %d\nLCD_ERR_VIDX_CSI %d\nLCD_ERR_VCF_LINE %d\nLCD_VIDX_TBI %d\nLCD_VIDX_CSI %d\nptr %zu\n", LCD_ERR_VIDX_ORDER, LCD_ERR_VIDX_CSI, LCD_ERR_VCF_LINE, LCD_VIDX_TBI,
           LCD_VIDX_CSI, sizeof(void *));
    return 0;
}
