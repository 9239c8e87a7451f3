/* TEST ONLY: size and field offsets of lcd_inputs_t and the constants of the several-input entry points of include/lcd_hotpath.h, in the format of call_file_abi.c:
 * tests/test_call_files_abi.py compiles this file and compares them with the ctypes mirror of longcalld_amd/_lib.py */
#include <stddef.h>
#include <stdio.h>
#include "lcd_hotpath.h"

#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
    SZ(lcd_inputs_t);
    OFF(lcd_inputs_t, n); OFF(lcd_inputs_t, bam_paths); OFF(lcd_inputs_t, bai_paths); OFF(lcd_inputs_t, sort_output);
    SZ(lcd_file_job_t); SZ(lcd_file_stats_t); SZ(lcd_index_opt_t); SZ(lcd_index_stats_t);
    printf("LCD_MAX_INPUTS %d\nLCD_ERR_INPUT_HEADERS %d\n", LCD_MAX_INPUTS, LCD_ERR_INPUT_HEADERS);
    return 0;
}
