/* TEST ONLY: size and field offsets of lcd_refine_stats_t and lcd_refine_entry_t (include/lcd_hotpath.h), in the format of call_file_abi.c: tests/test_refine_abi.py compiles this file and
 * compares them with the ctypes mirror of longcalld_amd/_lib.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"

#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
    SZ(lcd_refine_stats_t);
    OFF(lcd_refine_stats_t, n_records); OFF(lcd_refine_stats_t, n_kept); OFF(lcd_refine_stats_t, n_refined); OFF(lcd_refine_stats_t, n_identical);
    OFF(lcd_refine_stats_t, n_unrefined); OFF(lcd_refine_stats_t, n_pos_moved); OFF(lcd_refine_stats_t, n_no_digars); OFF(lcd_refine_stats_t, n_qlen_mismatch);
    OFF(lcd_refine_stats_t, n_bad_pos); OFF(lcd_refine_stats_t, n_too_many_ops); OFF(lcd_refine_stats_t, n_cg_cigar); OFF(lcd_refine_stats_t, n_nm_replaced);
    OFF(lcd_refine_stats_t, n_md_replaced); OFF(lcd_refine_stats_t, n_cs_replaced); OFF(lcd_refine_stats_t, n_touched); OFF(lcd_refine_stats_t, bytes_digars_up);
    OFF(lcd_refine_stats_t, bytes_ref_up); OFF(lcd_refine_stats_t, ms_measure); OFF(lcd_refine_stats_t, ms_emit);
    OFF(lcd_refine_stats_t, n_log_entries); OFF(lcd_refine_stats_t, bytes_log_down); OFF(lcd_refine_stats_t, n_log_rejected);
    SZ(lcd_digar_t);
    SZ(lcd_refine_entry_t);
    OFF(lcd_refine_entry_t, read_id); OFF(lcd_refine_entry_t, cover); OFF(lcd_refine_entry_t, read_beg); OFF(lcd_refine_entry_t, read_end); OFF(lcd_refine_entry_t, aln_len);
    OFF(lcd_refine_entry_t, pass); OFF(lcd_refine_entry_t, reg_beg); OFF(lcd_refine_entry_t, reg_end); OFF(lcd_refine_entry_t, target); OFF(lcd_refine_entry_t, query);
    return 0;
}
