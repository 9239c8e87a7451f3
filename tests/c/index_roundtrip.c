/* TEST ONLY: the host-side index exports called from plain C through the public header: two records of one contig -> the bytes of their .bai on stdout (hex), a
 * refused table -> its code and lcd_last_error, a FASTA path (argv[1]) -> lcd_fai_build's return value. */
#include <stdio.h>
#include <stdlib.h>
#include "lcd_hotpath.h"
int main(int argc, char **argv) {
    int refid[2] = {0, 0}, flag[2] = {0, 4};
    int64_t beg[2] = {100, 20000}, end[2] = {150, 20001};
    uint64_t vbeg[2] = {(98ull << 16) | 7, (98ull << 16) | 300}, vend[2] = {(98ull << 16) | 300, 400ull << 16};
    uint8_t *bytes = NULL; size_t n = 0;
    int rc = lcd_bai_from_records(2, 2, refid, beg, end, flag, vbeg, vend, &bytes, &n);
    printf("rc %d n %zu\nbytes ", rc, n);
    for (size_t i = 0; i < n; ++i) printf("%02x", bytes[i]);
    printf("\n");
    free(bytes);
    beg[1] = 50;
    rc = lcd_bai_from_records(2, 2, refid, beg, end, flag, vbeg, vend, &bytes, &n);
    printf("refused %d %s\n", rc, lcd_last_error());
    if (argc > 1) printf("fai %d\n", lcd_fai_build(argv[1], NULL));
    return 0;
}
