/* TEST ONLY: lcd_vcf_fields_t / lcd_vcf_fields_out_t and the drivers' option structs (lcd_run_opt_t, lcd_run_out_t, lcd_writer_opt_t) of include/lcd_hotpath.h.
 * Without arguments: sizes and field offsets in the format of call_file_abi.c (tests/test_vcf_fields.py compares them with the ctypes mirrors).  With <in.bam>
 * <ref.fa> <out prefix> [te.fa]: the whole-file run through lcd_call_files without options, and with lcd_run_opt_t whose fields member is NULL, a zeroed
 * lcd_vcf_fields_t and -- when te.fa is given -- that library; every run writes
 * <prefix>.<tag>.vcf and <prefix>.<tag>.bam and prints "<tag> rc <code> lines <VCF lines> mei <MEI lines> err <lcd_last_error>". */
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "lcd_hotpath.h"

#define SZ(T) printf(#T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

static void run(const char *tag, const char *bam, const char *fa, const char *prefix, int use_fields, const lcd_vcf_fields_t *fields) {
    char vcf[4096], out[4096];
    snprintf(vcf, sizeof(vcf), "%s.%s.vcf", prefix, tag); snprintf(out, sizeof(out), "%s.%s.bam", prefix, tag);
    lcd_cfg_t cfg; lcd_cfg_default(&cfg, 0);
    cfg.pass.max_noisy_reg_len = 600;
    lcd_bam_out_t bo; memset(&bo, 0, sizeof(bo)); bo.path = out; bo.pg_line = "@PG\tID:longcalld_amd\tPN:longcalld_amd";
    lcd_file_job_t job; lcd_file_job_default(&job);
    job.bam_path = bam; job.fasta_path = fa; job.chunk_len = 6000; job.vcf_path = vcf; job.bam_out = &bo;
    job.source_version = "test-1"; job.cmdline = "call ref.fa in.bam"; job.date_yyyymmdd = "20240102";
    lcd_file_stats_t st; lcd_vcf_fields_out_t fo; memset(&fo, 0, sizeof(fo));
    lcd_run_opt_t opt; memset(&opt, 0, sizeof(opt)); opt.fields = fields;
    lcd_run_out_t ro; memset(&ro, 0, sizeof(ro)); ro.fields_out = &fo;
    const int rc = use_fields ? lcd_call_files(NULL, &job, &cfg, &opt, &st, &ro) : lcd_call_files(NULL, &job, &cfg, NULL, &st, NULL);
    printf("%s rc %d lines %lld mei %lld err %s\n", tag, rc, (long long)st.n_vcf_lines, (long long)fo.n_mei_lines, rc < 0 ? lcd_last_error() : "");
    lcd_file_stats_free(&st); lcd_vcf_fields_out_free(&fo);
}

int main(int argc, char **argv) {
    if (argc < 4) {
        SZ(lcd_vcf_fields_t);
        OFF(lcd_vcf_fields_t, te_fasta_path); OFF(lcd_vcf_fields_t, te_kmer_len); OFF(lcd_vcf_fields_t, rnames_mode);
        SZ(lcd_vcf_fields_out_t);
        OFF(lcd_vcf_fields_out_t, n_te_seqs); OFF(lcd_vcf_fields_out_t, te_names); OFF(lcd_vcf_fields_out_t, n_mei_lines); OFF(lcd_vcf_fields_out_t, n_rnames);
        OFF(lcd_vcf_fields_out_t, rnames);
        SZ(lcd_run_opt_t);
        OFF(lcd_run_opt_t, idx); OFF(lcd_run_opt_t, fields); OFF(lcd_run_opt_t, aln);
        SZ(lcd_run_out_t);
        OFF(lcd_run_out_t, idx_stats); OFF(lcd_run_out_t, n_reads_per_file); OFF(lcd_run_out_t, fields_out); OFF(lcd_run_out_t, refine_stats); OFF(lcd_run_out_t, sam_stats);
        SZ(lcd_writer_opt_t);
        OFF(lcd_writer_opt_t, format); OFF(lcd_writer_opt_t, sort_output); OFF(lcd_writer_opt_t, write_index); OFF(lcd_writer_opt_t, index_path);
        OFF(lcd_writer_opt_t, idx_stats); OFF(lcd_writer_opt_t, refine_stats); OFF(lcd_writer_opt_t, sam_stats);
        printf("LCD_RNAMES_NONE %d\nLCD_RNAMES_SV %d\nLCD_RNAMES_ALL %d\n", LCD_RNAMES_NONE, LCD_RNAMES_SV, LCD_RNAMES_ALL);
        return 0;
    }
    lcd_vcf_fields_t zero; memset(&zero, 0, sizeof(zero));
    run("plain", argv[1], argv[2], argv[3], 0, NULL);
    run("null", argv[1], argv[2], argv[3], 1, NULL);
    run("zero", argv[1], argv[2], argv[3], 1, &zero);
    if (argc > 4) { lcd_vcf_fields_t te = zero; te.te_fasta_path = argv[4]; run("te", argv[1], argv[2], argv[3], 1, &te); }
    return 0;
}
