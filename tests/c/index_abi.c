/* TEST ONLY: sizes and field offsets of the index structs of include/lcd_hotpath.h, one "struct.field offset" line each ("struct size" for the size), and the
 * error codes.  Plain C against the public header; no library is needed. */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
    S(lcd_bai_member_t); F(lcd_bai_member_t, uoff); F(lcd_bai_member_t, coff); F(lcd_bai_member_t, ulen); F(lcd_bai_member_t, pad);
    S(lcd_bai_opt_t); F(lcd_bai_opt_t, slab_members); F(lcd_bai_opt_t, verify_crc);
    S(lcd_bai_stats_t); F(lcd_bai_stats_t, n_records); F(lcd_bai_stats_t, n_indexed); F(lcd_bai_stats_t, n_mapped); F(lcd_bai_stats_t, n_unmapped); F(lcd_bai_stats_t, n_no_coor);
    F(lcd_bai_stats_t, n_chunks); F(lcd_bai_stats_t, n_slabs); F(lcd_bai_stats_t, n_members); F(lcd_bai_stats_t, bytes_in); F(lcd_bai_stats_t, bytes_inflated);
    F(lcd_bai_stats_t, bytes_index); F(lcd_bai_stats_t, ms_read); F(lcd_bai_stats_t, ms_inflate); F(lcd_bai_stats_t, ms_walk); F(lcd_bai_stats_t, ms_stat);
    F(lcd_bai_stats_t, ms_entry); F(lcd_bai_stats_t, ms_finish); F(lcd_bai_stats_t, ms_wall);
    S(lcd_index_opt_t); F(lcd_index_opt_t, build_missing_bai); F(lcd_index_opt_t, build_missing_fai); F(lcd_index_opt_t, write_out_bai); F(lcd_index_opt_t, out_bai_path);
    F(lcd_index_opt_t, slab_members);
    S(lcd_index_stats_t); F(lcd_index_stats_t, built_bai); F(lcd_index_stats_t, built_fai); F(lcd_index_stats_t, wrote_out_bai); F(lcd_index_stats_t, out_bai_skipped);
    F(lcd_index_stats_t, out_bai_skip_reason); F(lcd_index_stats_t, out_bai_bytes); F(lcd_index_stats_t, out_n_indexed); F(lcd_index_stats_t, out_n_no_coor);
    F(lcd_index_stats_t, ms_build_bai); F(lcd_index_stats_t, ms_build_fai); F(lcd_index_stats_t, ms_out_bai);
    printf("LCD_ERR_BAI_ORDER %d\nLCD_ERR_BAI_CSI %d\nLCD_ERR_FAI_FORMAT %d\nLCD_ERR_BAI_CONTIG %d\n", LCD_ERR_BAI_ORDER, LCD_ERR_BAI_CSI, LCD_ERR_FAI_FORMAT, LCD_ERR_BAI_CONTIG);
    return 0;
}
