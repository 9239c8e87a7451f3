/* the methylation table's structs as a C compiler lays them out: prints "name size" and "name.member offset" lines for tests/test_mods_abi.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
    SZ(lcd_mods_opt_t); OFF(lcd_mods_opt_t, code); OFF(lcd_mods_opt_t, threshold); OFF(lcd_mods_opt_t, combine_strands); OFF(lcd_mods_opt_t, ref_seq); OFF(lcd_mods_opt_t, ref_beg);
    OFF(lcd_mods_opt_t, ref_end);
    SZ(lcd_mods_stats_t); OFF(lcd_mods_stats_t, n_records); OFF(lcd_mods_stats_t, n_counted); OFF(lcd_mods_stats_t, n_sites); OFF(lcd_mods_stats_t, n_rows); OFF(lcd_mods_stats_t, ms_site_map);
    OFF(lcd_mods_stats_t, ms_compact);
    SZ(lcd_run_ext2_t); OFF(lcd_run_ext2_t, size); OFF(lcd_run_ext2_t, mods_path); OFF(lcd_run_ext2_t, mods_code); OFF(lcd_run_ext2_t, mods_threshold);
    OFF(lcd_run_ext2_t, mods_combine_strands); OFF(lcd_run_ext2_t, mods_stats);
    SZ(lcd_run_ext_t); SZ(lcd_run_opt_t); SZ(lcd_run_out_t);
    return 0;
}
