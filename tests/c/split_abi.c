/* the read sets' structs as a C compiler lays them out: prints "name size" and "name.member offset" lines for tests/test_split_abi.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
    SZ(lcd_split_opt_t); OFF(lcd_split_opt_t, comment); OFF(lcd_split_opt_t, list); OFF(lcd_split_opt_t, reserved);
    SZ(lcd_split_stats_t); OFF(lcd_split_stats_t, n_records); OFF(lcd_split_stats_t, n_selected); OFF(lcd_split_stats_t, n_hap); OFF(lcd_split_stats_t, n_not_primary);
    OFF(lcd_split_stats_t, n_filtered_primary); OFF(lcd_split_stats_t, n_reverse); OFF(lcd_split_stats_t, n_no_seq); OFF(lcd_split_stats_t, n_bad_layout);
    OFF(lcd_split_stats_t, bytes_fastq); OFF(lcd_split_stats_t, bytes_list); OFF(lcd_split_stats_t, ms_measure); OFF(lcd_split_stats_t, ms_emit);
    OFF(lcd_split_stats_t, ms_deflate); OFF(lcd_split_stats_t, ms_download_write);
    SZ(lcd_run_ext2_t);
    SZ(lcd_run_ext2_split_t); OFF(lcd_run_ext2_split_t, x); OFF(lcd_run_ext2_split_t, split_prefix); OFF(lcd_run_ext2_split_t, split_gz); OFF(lcd_run_ext2_split_t, split_comment);
    OFF(lcd_run_ext2_split_t, haplotag_path); OFF(lcd_run_ext2_split_t, split_stats);
    return 0;
}
