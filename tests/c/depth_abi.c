/* the depth track's structs as a C compiler lays them out: prints "name size" and "name.member offset" lines for tests/test_depth_abi.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
    SZ(lcd_depth_opt_t); OFF(lcd_depth_opt_t, skip_dels); OFF(lcd_depth_opt_t, window); OFF(lcd_depth_opt_t, reserved);
    SZ(lcd_depth_stats_t); OFF(lcd_depth_stats_t, n_records); OFF(lcd_depth_stats_t, n_no_cigar); OFF(lcd_depth_stats_t, n_cg); OFF(lcd_depth_stats_t, n_no_overlap);
    OFF(lcd_depth_stats_t, n_intervals); OFF(lcd_depth_stats_t, bases); OFF(lcd_depth_stats_t, n_rows); OFF(lcd_depth_stats_t, ms_mark); OFF(lcd_depth_stats_t, ms_rows);
    SZ(lcd_run_ext2_t); OFF(lcd_run_ext2_t, size); OFF(lcd_run_ext2_t, mods_path); OFF(lcd_run_ext2_t, mods_code); OFF(lcd_run_ext2_t, mods_threshold);
    OFF(lcd_run_ext2_t, mods_combine_strands); OFF(lcd_run_ext2_t, reserved); OFF(lcd_run_ext2_t, mods_stats);
    OFF(lcd_run_ext2_t, depth_path); OFF(lcd_run_ext2_t, depth_window); OFF(lcd_run_ext2_t, depth_skip_dels); OFF(lcd_run_ext2_t, depth_stats);
    SZ(lcd_mods_stats_t); SZ(lcd_run_ext_t); SZ(lcd_run_opt_t); SZ(lcd_run_out_t);
    return 0;
}
