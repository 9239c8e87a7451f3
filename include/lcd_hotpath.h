/*
 * lcd_hotpath.h -- C ABI of liblcd_hotpath.so: the MI355X (gfx950) implementation of longcallD's
 * per-noisy-region alignment/phasing hot path.  Plain pointers and sizes only; no torch, no C++ types.
 *
 * Every entry point names the reference interface it replaces (paths relative to the longcallD tree).
 * INTEGRATION.md shows the few lines a longcallD maintainer adds to src/align.c / src/assign_hap.c /
 * src/collect_var.c to route the reference's own symbols here.
 *
 * PARITY STATUS (read before relying on byte identity with a real longcallD build):
 *   pinned to the reference's own code compiled in this project's container: K4 (edlib: distance, path, xgaps), the cgranges interval order, sdust;
 *   PARITY UNPINNED for K1/K2 (abPOA) and K3 (WFA2): the abPOA / WFA2-lib submodules are empty in the reference checkout, so consensus, MSA and CIGAR
 *   tie-breaks follow this project's restatement of the published algorithms (oracle/poa.c, oracle/wfa2p.c), pinned at score level only;
 *   K5, the align.c glue, f1 and f2 are line-by-line restatements of source that IS present, but no reference binary can be built here to confirm them.
 *   tests/test_replay_reference_dump.py replays `longcallD call -V 3` dumps of a real build once one is available (skipped until then).
 *
 * Conventions kept from the reference:
 *   - byte codes A0 C1 G2 T3 N4, gap 5 (src/seq.c:14-31, src/align.c:316,321);
 *   - buffers handed back are libc malloc()'d and owned by the caller, with the reference's interior
 *     pointer layout (aln_str_t: one block, target row first; only target_aln is free()d,
 *     src/collect_var.c:2718-2724);
 *   - return values: n_cons for the region call, distance/-1 for edlib, 0 for the WFA wrapper with
 *     failure signalled by *cigar_length == 0 (src/align.c:703);
 *   - unrecoverable states (no GPU, kernel error, arena exhaustion after retries) return a negative
 *     code and set lcd_last_error(); there is NO CPU fallback.
 *   - all entry points are thread-safe: each call (or each lcd_batch_t) owns its HIP stream and buffers.
 */
#ifndef LCD_HOTPATH_H
#define LCD_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the fields of call_var_opt_t (src/call_var_main.h:128-180) that the path reads */
typedef struct lcd_opt_t {
    int match, mismatch, gap_open1, gap_ext1, gap_open2, gap_ext2; /* src/align.h:21-26 */
    int gap_aln;                                                   /* LONGCALLD_GAP_LEFT_ALN = 1 */
    double min_af;
    int min_dp;
    double partial_aln_ratio;
    int min_noisy_reg_size_to_sample_reads, max_noisy_reg_len, noisy_reg_flank_len;
    int min_hap_full_reads, min_hap_reads;
    int collect_ref_read_aln_str; /* (refine_bam && out_aln_fp) || out_somatic, src/align.c:1785-1786 */
    int is_ont;
    /* additive: 1 = also run make_vars_from_msa_cons_aln (src/collect_var.c:2279) on the device after the strings are
     * built and return it through lcd_batch_region_vars; 2 = the same, and lcd_batch_download leaves the alignment strings in HBM
     * (lcd_batch_region_result then fails): only variants and alleles cross PCIe */
    int collect_noisy_vars;
    int min_sv_len;               /* call_var_opt_t.min_sv_len (LONGCALLD_MIN_SV_LEN 30, src/call_var_main.h:54,175) */
} lcd_opt_t;

/* == aln_str_t, src/collect_var.h:106-112 */
typedef struct lcd_aln_str_t {
    uint8_t *target_aln;
    uint8_t *query_aln;
    int aln_len;
    int target_beg, target_end, query_beg, query_end;
} lcd_aln_str_t;

/* digar1_t / digar_t views (src/bam_utils.h:27-43) for the read-slicing step (src/align.c:1377-1461) */
typedef struct lcd_digar1_t {
    int64_t pos;
    int type, len, qi;
} lcd_digar1_t;
typedef struct lcd_read_view_t {
    const lcd_digar1_t *digars;
    int n_digar;
    int qlen;            /* digar2qlen() */
    const uint8_t *bseq; /* BAM 4-bit packed bases (bam_get_seq) */
    const uint8_t *qual;
    int hap;             /* chunk->haps[read] */
    int64_t phase_set;   /* chunk->phase_sets[read] */
} lcd_read_view_t;

void lcd_opt_default(lcd_opt_t *opt);          /* src/call_var_main.c:140-224 */
int lcd_init(int device);                      /* process default device; 0 ok; <0: no usable gfx950 device */
/* One process, many GPUs (the reference's kt_for workers are threads of one process, src/call_var_main.c:773): a device belongs to an
 * lcd_batch_t (lcd_batch_create_on) or, for the per-call mirrors and K5, to the calling thread (lcd_set_thread_device; < 0 = process default). */
int lcd_device_count(void);
long long lcd_alloc_events(void);           /* device allocations made so far by the library's grow-only buffers (a steady state makes none) */
long long lcd_device_bytes(int device);     /* bytes those buffers hold on a device right now */
int lcd_set_thread_device(int device);
const char *lcd_last_error(void);
/* Host threads this process uses beside the calling thread: `team` = threads of a submission's short parallel loops (LCD_HOST_TEAM), `arena_threads` = threads that lay
 * results out on the host (LCD_ARENA_THREADS).  Their defaults are the CPUs this process may use (`cpus`: affinity mask cut by the cgroup's CPU quota) divided by the
 * processes of the job on this host (`local_world`: LOCAL_WORLD_SIZE, else WORLD_SIZE, else 1), at most 8 / 16 -- so N ranks on one host (one per GPU) share the host
 * instead of each taking what a lone process takes.  Additive (the reference sizes its one thread pool by -t, src/call_var_main.c:773).  Any pointer may be NULL; returns 0. */
int lcd_host_threads(int *team, int *arena_threads, int *cpus, int *local_world);
const char *lcd_version(void);

/* ---- drop-in mirrors of src/align.h:50-65 ---- */

/* replaces wfa_end2end_aln (definition src/align.c:374-376; parameter meaning follows the DEFINITION:
 * gap_aln, b, q, e, q2, e2, heuristic, affine_gap).  Only heuristic == 0 (none) and affine_gap == 1 (2-piece)
 * -- the germline-live configuration -- are implemented; others return -2. */
int lcd_wfa_end2end_aln(uint8_t *pattern, int plen, uint8_t *text, int tlen, int gap_aln, int b, int q, int e, int q2,
                        int e2, int heuristic, int affine_gap, uint32_t **cigar_buf, int *cigar_length,
                        uint8_t **pattern_alg, uint8_t **text_alg, int *alg_length);
/* replaces edlib_end2end_aln (src/align.c:234), edlib_xgaps (:222), edlib_edit_distance (:210) */
int lcd_edlib_end2end_aln(uint8_t *target, int tlen, uint8_t *query, int qlen, int *n_eq, int *n_xid);
int lcd_edlib_xgaps(uint8_t *target, int tlen, uint8_t *query, int qlen);
int lcd_edlib_edit_distance(uint8_t *target, int tlen, uint8_t *query, int qlen);

/* replaces end2end_aln (src/align.c:610; exported src/align.h:56, no caller in src) and wfa_collect_diff_ins_seq (src/align.c:463; callers
 * src/collect_var.c:203 and, with -s, src/assign_hap.c:1280): both are thin wrappers over the 2-piece WFA above */
int lcd_end2end_aln(const lcd_opt_t *opt, char *tseq, int tlen, uint8_t *qseq, int qlen, uint32_t **cigar_buf);
int lcd_wfa_collect_diff_ins_seq(const lcd_opt_t *opt, uint8_t *large_seq, int large_len, uint8_t *small_seq, int small_len, uint8_t **diff_seq);
/* replaces edlib_infix_aln (src/align.c:256-275, src/align.h:54; every caller is somatic-mode code): edlibAlign(query, target, {k = -1, EDLIB_MODE_HW,
 * EDLIB_TASK_PATH}) -- the query against the best-matching stretch of the target (free start and end in the target), the path on the first end position's
 * stretch (edlib/src/edlib.cpp:146-280).  Returns the edit distance (-1 on error); *n_eq / *n_xid as edlibAlignmentToXID counts the path (:164).  Byte-pinned to
 * the reference's own edlib (tests/golden/edlib_golden.json `hw_cases`). */
int lcd_edlib_infix_aln(uint8_t *target, int tlen, uint8_t *query, int qlen, int *n_eq, int *n_xid);
/* src/align.h:60: wfa_heuristic_aln (x-drop; NO caller in longcallD) is exported so that longcallD links against this library alone; it returns -2, sets
 * lcd_last_error() and prints to stderr -- never a silent result */
int lcd_wfa_heuristic_aln(uint8_t *pattern, int plen, uint8_t *text, int tlen, int a, int b, int q, int e, int q2, int e2, int *n_eq, int *n_xid);

/* replaces collect_noisy_reg_aln_strs (src/align.c:1760) with bam_chunk_t flattened to per-read views.
 * noisy_reads[] is permuted in place exactly as the reference does (src/align.c:1774). */
int lcd_collect_noisy_reg_aln_strs(const lcd_opt_t *opt, const lcd_read_view_t *chunk_reads, int64_t noisy_reg_beg,
                                   int64_t noisy_reg_end, int noisy_reg_i, int n_noisy_reg_reads, int *noisy_reads,
                                   const uint8_t *ref_seq, int ref_seq_len, int *clu_n_seqs, int **clu_read_ids,
                                   lcd_aln_str_t **aln_strs);

/* ---- K5: replaces assign_hap_based_on_germline_het_vars_kmeans (src/assign_hap.h:12, src/assign_hap.c:473-547) ----
 * bam_chunk_t / cand_var_t / read_var_profile_t flattened (src/collect_var.h:71-104, src/bam_utils.h:45-92). */
typedef struct lcd_hap_problem_t {
    int n_reads, n_vars, is_ont;
    const int64_t *var_pos;            /* cand_var_t.pos */
    const int *var_type;               /* BAM_CDIFF 8 / BAM_CINS 1 / BAM_CDEL 2 */
    const int *var_cate;               /* chunk->var_i_to_cate */
    const int *is_homopolymer_indel;
    const int *total_cov;
    const int *alle_off;               /* n_vars+1 CSR offsets into alle_covs and the three profile planes */
    const int *alle_covs;
    const int *start_var_idx, *end_var_idx; /* read_var_profile_t (-1 / -2: no variant) */
    const int *allele_off;             /* n_reads+1 CSR offsets into alleles */
    const int *alleles;
    const int *ordered_read_ids;
    const uint8_t *is_skipped;
    int n_cr;
    const int *cr_read;                /* labels of chunk->read_var_cr in its sorted interval order (cr->r[i].label) */
    int *haps;                         /* out: chunk->haps */
    int64_t *phase_sets;               /* out: chunk->phase_sets */
    int *n_clean_agree_snps, *n_clean_conflict_snps;
    int64_t *var_phase_set;            /* out: cand_var_t.phase_set */
    int *hap_to_cons_alle;             /* in/out n_vars*3 */
    int *hap_to_alle_profile;          /* in/out 3 planes of alle_off[n_vars] */
} lcd_hap_problem_t;
int lcd_assign_hap_germline(lcd_hap_problem_t *p, int target_var_cate);
int lcd_assign_hap_batch(int n, lcd_hap_problem_t *probs, const int *target_var_cates);

/* ---- batched form (additive; legal because regions of one pass are independent, SURVEY CS-2) ---- */
typedef struct lcd_batch_s lcd_batch_t;

typedef struct lcd_batch_stats_t {
    int n_regions, n_regions_resolved; /* regions reaching K1/K2 ; regions with n_cons > 0 */
    int n_chains, n_anchor_jobs, n_wfa_jobs, n_edlib_jobs;
    uint64_t poa_aligned_bases, poa_cells, wfa_offsets, edlib_blocks; /* poa_cells: DP cells of the reference's algorithm (K1: adaptive band, K2: full rows) */
    uint64_t poa_alg_bytes; /* SURVEY 8d B_poa summed over aligned reads (C = poa_cells) */
    double ms_total, ms_anchor, ms_poa, ms_wfa, ms_strings; /* HIP-event times on the batch stream */
    double ms_upload, ms_download, ms_host;
    double ms_poa_kernel;   /* HIP events tight around the POA chain kernel launch(es) only */
    int n_poa_launches;
    int poa_retries;
    double ms_vars;         /* stage S6 (opt.collect_noisy_vars) */
    uint64_t poa_cells_computed; /* cells the kernels actually computed: < poa_cells where K2 ran over a certified band (same alignments) */
    int poa_grown;               /* DP regions enlarged in place by a chain whose estimate was too small for a read (spare DP memory); such a chain is not re-run */
} lcd_batch_stats_t;

#define LCD_DEVICE_ANY (-2)
lcd_batch_t *lcd_batch_create(const lcd_opt_t *opt);                 /* on the calling thread's device */
/* device >= 0: that GPU; -1: the calling thread's; LCD_DEVICE_ANY: a host-only job buffer whose device is chosen at upload / dispatch time.
 * Batches of one lcd_batch_run_many call share a device. */
lcd_batch_t *lcd_batch_create_on(const lcd_opt_t *opt, int device);
void lcd_batch_destroy(lcd_batch_t *b);
void lcd_batch_clear(lcd_batch_t *b);
/* add one region AFTER read slicing (the outputs of collect_noisy_read_info, src/align.c:1377): returns region index */
int lcd_batch_add_region(lcd_batch_t *b, int64_t reg_len, int n_reads, const int *read_ids, const int *lens,
                         const uint8_t *const *seqs, const uint8_t *const *quals, const int *fully_covers, const int *haps,
                         const int64_t *phase_sets, const uint8_t *ref_seq, int ref_seq_len);
/* add one region from chunk views (does the digar walk of src/align.c:1392-1458 on the host) */
int lcd_batch_add_region_from_chunk(lcd_batch_t *b, const lcd_read_view_t *chunk_reads, int64_t noisy_reg_beg,
                                    int64_t noisy_reg_end, int n_noisy_reg_reads, const int *noisy_reads,
                                    const uint8_t *ref_seq, int ref_seq_len);
/* the same region with the reads' bases left as they are in their BAM records (4 bits per base): the host copies the slices' bytes, lcd_batch_upload unpacks them
 * on the device (seq_nt16_int[bam_seqi()], src/align.c:1445-1448) into the batch's input pool -- no per-base loop on the host, half the bytes over PCIe for the
 * reads.  Same results as lcd_batch_add_region_from_chunk. */
int lcd_batch_add_region_from_chunk_packed(lcd_batch_t *b, const lcd_read_view_t *chunk_reads, int64_t noisy_reg_beg,
                                    int64_t noisy_reg_end, int n_noisy_reg_reads, const int *noisy_reads,
                                    const uint8_t *ref_seq, int ref_seq_len);
int lcd_batch_upload(lcd_batch_t *b);  /* host -> HBM (not part of the timed hot path) */
int lcd_batch_run(lcd_batch_t *b);     /* anchors -> POA chains -> ref/cons WFA -> strings; inputs and outputs stay in HBM */
/* the same for n uploaded batches JOINTLY (one set of launches per stage over the jobs / chains of all of them: a chain is a
 * sequential object that occupies at most one CU, so several chunks' regions in flight are what fills 256 CUs -- the reference's
 * kt_for workers, src/call_var_main.c:321, are the natural source of such concurrent batches).  batches[0] lends its stream and work
 * buffers; every batch must be downloaded before batches[0] runs again or is destroyed.  Results are those of n separate lcd_batch_run calls.
 * Thread-safe for submissions with different batches[0]: two submitter threads with ~32 batches each is the measured optimum on one MI355X
 * (one submission's anchor / ref-cons / string stages run under the other's chains); a submission that exceeds the device
 * memory budget (LCD_MEM_FRACTION, default 0.92) is split in halves and retried. */
int lcd_batch_run_many(lcd_batch_t **batches, int n);
int lcd_batch_download(lcd_batch_t *b);/* HBM -> host */
/* ---- one process, all GPUs of the node (the GPU-side analogue of kt_for's work stealing, src/kthread.c:24-64, src/call_var_main.c:773) ----
 * lcd_dispatch_run orders the batches (job buffers created with LCD_DEVICE_ANY, regions added, not uploaded) by estimated DP work, longest first; one
 * submitter thread per device takes the next `coalesce` of them whenever its previous submission is done: bind + upload, lcd_batch_run_many, download.
 * Returns when every batch is downloaded (results through lcd_batch_region_result / _vars as usual); device_of[i] (optional) = the GPU batch i ran on.
 * Chunks are independent until stitch_var_main: no data-path exchange between devices. */
typedef struct lcd_dispatch_s lcd_dispatch_t;
lcd_dispatch_t *lcd_dispatch_create(int n_devices, const int *devices, int coalesce); /* n_devices <= 0: every visible GPU; coalesce <= 0: 16 */
void lcd_dispatch_destroy(lcd_dispatch_t *d);
int lcd_dispatch_n_devices(const lcd_dispatch_t *d);
int lcd_dispatch_run(lcd_dispatch_t *d, lcd_batch_t **batches, int n, int *device_of);
/* flags bit 0: no lcd_batch_download after a submission (results stay on the device) */
void lcd_dispatch_set_flags(lcd_dispatch_t *d, int flags);
/* per device (dispatcher order): ms its submitter thread spent inside submissions during the last lcd_dispatch_run, number of submissions; returns #devices */
int lcd_dispatch_busy(const lcd_dispatch_t *d, double *busy_ms, int *n_submissions);
double lcd_batch_cost(const lcd_batch_t *b);   /* the work estimate the queue is ordered by (DP cells of the batch's chains) */
/* longest-processing-time assignment of n costs to n_bins bins (static sharding across processes / ranks: bench.py --job-mb) */
void lcd_lpt_assign(int n, const double *cost, int n_bins, int *bin_of, double *bin_load);
/* ---- one process per GPU: cross-rank rebalancing of region queues (the reference's analogue inside one process is kt_for's work stealing,
 * src/kthread.c:24-64, called at src/call_var_main.c:773).  One epoch before the hot path: every rank packs its region jobs chunk by chunk
 * (lcd_region_jobs_pack: the arguments of lcd_batch_add_region, byte for byte) and prices them (lcd_region_job_cost); lcd_rebalance_exchange all-gathers the queue
 * depths and the (cost, bytes) tables over RCCL, computes the same plan on every rank (lcd_rebalance_plan) and moves WHOLE packed buffers with ncclSend / ncclRecv;
 * the receiver adds them to its batches with lcd_batch_add_packed.  No data-path collective (chunks are independent until stitch_var_main, src/collect_var.c:2983).
 * librccl is opened lazily by lcd_comm_create. */
typedef struct lcd_region_job_t {      /* the arguments of lcd_batch_add_region */
    int64_t reg_len; int n_reads;
    const int *read_ids, *lens; const uint8_t *const *seqs; const uint8_t *const *quals /* NULL, or NULL entries: zeros travel */;
    const int *fully_covers, *haps; const int64_t *phase_sets; const uint8_t *ref_seq; int ref_seq_len;
} lcd_region_job_t;
typedef struct lcd_move_t { int src, index /* in src's queue */, dst; } lcd_move_t;
typedef struct lcd_rebalance_stats_t { int n_moves, world; uint64_t moved_bytes; double imbalance_before, imbalance_after /* max load / mean load over the ranks */;
                                       double load_before_mine, load_after_mine; int jobs_before_mine, jobs_after_mine; } lcd_rebalance_stats_t;
typedef struct lcd_comm_s lcd_comm_t;
double lcd_region_job_cost(const lcd_region_job_t *job);                                  /* DP-cell estimate: banded K1 chains if any read is phased, else the unbanded K2 chain */
uint64_t lcd_region_jobs_pack(int n, const lcd_region_job_t *jobs, uint8_t *buf);         /* buf == NULL: the size; else fills buf (that many bytes) */
int lcd_batch_add_packed(lcd_batch_t *b, const uint8_t *buf, uint64_t nbytes);            /* -> regions added (lcd_batch_add_region each), < 0: malformed (lcd_rebalance_last_error) */
/* costs: every rank's job costs, rank after rank (n_jobs[r] each); moves: room for sum(n_jobs) entries.  From the most loaded rank to the least loaded one, the job
 * that brings the pair closest to equal -- or, when every job of the most loaded rank is at least as large as the gap (SV-heavy chunks), the swap of one job of
 * each whose difference does (two moves) -- until the most loaded rank is within tol of the mean or max_moves (< 0: no limit) are made; a job moves at most once.
 * Deterministic.  Returns the number of moves; load_before / load_after (world entries each, nullable). */
int lcd_rebalance_plan(int world, const int *n_jobs, const double *costs, double tol, int max_moves, lcd_move_t *moves, double *load_before, double *load_after);
int lcd_rccl_unique_id(uint8_t id[128]);                                                   /* ncclGetUniqueId on rank 0; the caller gives the bytes to the other ranks */
lcd_comm_t *lcd_comm_create(int world, int rank, const uint8_t id[128], int device);       /* ncclCommInitRank; NULL on failure */
void lcd_comm_destroy(lcd_comm_t *c);
int lcd_comm_info(lcd_comm_t *c, int *nccl_world, int *nccl_rank, int *nccl_device);      /* ncclCommCount / ncclCommUserRank / ncclCommCuDevice of the communicator: what RCCL itself sees */
/* One epoch.  In: this rank's queue.  Out (arrays malloc()'d): its new queue -- kept jobs (bufs_out[i] is the caller's pointer, owned_out[i] = 0) and received ones
 * (malloc()'d buffers, owned_out[i] = 1: the caller frees them). */
int lcd_rebalance_exchange(lcd_comm_t *c, int n_jobs, const double *cost, const uint64_t *nbytes, const uint8_t *const *bufs, double tol,
                           int *n_out, double **cost_out, uint64_t **nbytes_out, uint8_t ***bufs_out, uint8_t **owned_out, lcd_rebalance_stats_t *stats);
const char *lcd_rebalance_last_error(void);
/* region results; clu_read_ids[c] and aln_strs[c][j].target_aln are malloc()'d (aln_strs[c] must hold 1+2*n_reads zeroed entries) */
int lcd_batch_region_result(lcd_batch_t *b, int region, int *clu_n_seqs, int **clu_read_ids, lcd_aln_str_t **aln_strs);
/* ---- candidate variants of a region + the read x variant allele profile (opt.collect_noisy_vars) ----
 * == make_vars_from_msa_cons_aln (src/collect_var.c:2279-2347: make_cand_vars_from_msa :1855, update_cand_var_profile_from_cons_aln_str1/2
 * :2164/:2206) computed on the device from the strings of lcd_batch_run.  What stays with the caller, as host code in the reference too:
 * TSD / polyA / TE annotation of gaps >= min_sv_len (collect_te_info_from_cons, :1815/:1834, SURVEY a14: lcd_collect_te_info_from_cons below, applied by the
 * caller to the INS / DEL records it gets) and merge_var_profile (:2712; lcd_merge_region_vars below does it on the library's flat chunk state). */
typedef struct lcd_noisy_var_t {   /* the cand_var_t fields make_cand_vars0 (src/collect_var.c:1746) and the profile update fill */
    int64_t pos;
    int var_type, ref_len, alt_len; /* BAM_CDIFF 8 / BAM_CINS 1 / BAM_CDEL 2 */
    int cate;                       /* LONGCALLD_NOISY_CAND_HET_VAR 0x100 / LONGCALLD_NOISY_CAND_HOM_VAR 0x200 */
    int from_cons;                  /* var_from_cons_idx: 1 | 2 | 3 (:2216-2226) */
    int is_homopolymer_indel;       /* var_is_homopolymer_indel (:1720), from chunk_ref_seq; 0 for gaps >= min_sv_len */
    int ref_base, alt_ref_base;
    int total_cov, alle_covs[2];
    uint8_t *alt_seq;               /* malloc()'d alt_len bytes, NULL for deletions */
} lcd_noisy_var_t;
/* returns n_vars (>= 0) or < 0.  Rows of the profile = the reads of cluster 0 then cluster 1 in clu_read_ids order (row_read_ids);
 * prof_start/prof_end = read_var_profile_t.start_var_idx/end_var_idx (-1/-2: none); prof_alleles = n_rows x n_vars, -1 where unset.
 * chunk_ref_seq[k] = base code at reference position chunk_ref_beg + k (chunk->ref_seq / ref_beg); may be NULL (flag stays 0).
 * Every output array is malloc()'d (free vars[i].alt_seq, vars, row_read_ids, prof_*). */
int lcd_batch_region_vars(lcd_batch_t *b, int region, int64_t noisy_reg_beg, const uint8_t *chunk_ref_seq, int64_t chunk_ref_beg,
                          int64_t chunk_ref_len, lcd_noisy_var_t **vars, int *n_rows, int **row_read_ids, int **prof_start,
                          int **prof_end, int **prof_alleles);
int lcd_batch_region_sorted_ids(lcd_batch_t *b, int region, int *read_ids_out); /* the in-place permutation of noisy_reads */
/* per read of a region in its sorted order: chunk read id, cover flag and the read's slice read_reg_beg / read_reg_end as collect_noisy_read_info computed
 * them (src/align.c:1392-1458; -1 / -2 for regions added after slicing): what update_digars_from_aln_str (:1745) hands to lcd_update_digars_from_msa1 */
int lcd_batch_region_read_slices(lcd_batch_t *b, int region, int *read_ids, int *covers, int *read_beg, int *read_end);
int lcd_batch_get_stats(lcd_batch_t *b, lcd_batch_stats_t *st);
/* the K4 job set of the batch's anchor stage (edlib_xgaps calls of src/align.c:694,698,722): offsets into the batch's host pool (valid until the
 * batch is cleared); returns the number of jobs, fills at most cap of them.  bench.py times the reference's own edlib on it. */
int lcd_batch_k4_jobs(lcd_batch_t *b, int cap, uint64_t *t_off, int *tlen, uint64_t *q_off, int *qlen, const uint8_t **pool, uint64_t *pool_len);
/* a 64-bit FNV-1a digest over every region's results (n_cons, clusters, all alignment rows) -- cheap whole-batch parity check */
uint64_t lcd_batch_digest(lcd_batch_t *b);
/* lcd_batch_region_result for every region of a downloaded batch, results freed again: the host-side cost of holding every result the way the per-call
 * mirror hands it over (malloc()'d rows), without the digest's hashing; returns the bytes of alignment rows handed out */
uint64_t lcd_batch_materialize(lcd_batch_t *b);
/* Every region's results of a downloaded batch in ONE host block (additive entry; the reference's contract -- one malloc() per row, freed row by row,
 * src/collect_var.c:2670-2724 -- stays with lcd_batch_region_result).  *results_out[r] describes region r exactly as lcd_batch_region_result fills the caller's
 * arrays: n_cons, clu_n_seqs[2], clu_read_ids[2], aln_strs[2] (each an array of n_aln_strs = 1 + 2 * n_reads zero-initialised lcd_aln_str_t: [0] ref<->cons,
 * [2i+1] cons<->read i, [2i+2] ref<->read i).  The table, the id lists, the aln_str_t arrays and every row are INTERIOR pointers into *arena_out:
 * free(*arena_out) releases everything and nothing inside may be freed on its own.  Filled by host threads.  Returns the number of regions, < 0 on error. */
typedef struct lcd_region_result_t { int n_cons, n_aln_strs; int clu_n_seqs[2]; int *clu_read_ids[2]; lcd_aln_str_t *aln_strs[2]; } lcd_region_result_t;
int lcd_batch_region_results_arena(lcd_batch_t *b, lcd_region_result_t **results_out, void **arena_out, uint64_t *arena_bytes);

/* ---- SURVEY 8(f) f2, first part: EQX CIGARs -> digar lists + each read's noisy windows (additive) ----
 * == collect_digar_from_eqx_cigar (src/bam_utils.c:701-842, with push_xid_size_queue_win :161-200) for all reads of a chunk in one launch.
 * Inputs are what bam1_t holds: 0-based position, CIGAR words (bam_get_cigar), qualities; pal_flags bit0 / bit1 = is_ont_palindrome_clip
 * for the left / right clip (the caller reads the SA tag; 0 for HiFi).  Outputs (all malloc()'d, CSR over the reads):
 *   digars[digar_off[r] .. digar_off[r+1])   digar1_t fields (alt_seq copies are not made: bases stay in the packed read);
 *   ivs[iv_off[r] .. iv_off[r+1])            the read's digar->noisy_regs in cr_index order: start (= first position - 1), end, label;
 *   iv_in_chunk[k]                           1 if interval k is added to chunk->chunk_noisy_regs (read not skipped, overlaps [reg_beg, reg_end]);
 *   status[r] 0 / -1 (the function's return value: read skipped as too noisy) / -2 ('M' operation); beg/end = digar->beg/end; n_cand_vars. */
typedef struct lcd_digar_opt_t {
    int min_bq, noisy_reg_max_xgaps, noisy_reg_slide_win, end_clip_reg, end_clip_reg_flank_win; /* src/call_var_main.h:19-38: 10, 5, 100 | 25, 30, 100 */
    double max_noisy_frac_per_read, max_var_ratio_per_read;                                     /* 0.5, 0.05 */
} lcd_digar_opt_t;
typedef struct lcd_digar_t { int64_t pos; int type, len, qi, is_low_qual; } lcd_digar_t;
typedef struct lcd_noisy_iv_t { int64_t start, end; int label, pad; } lcd_noisy_iv_t;
void lcd_digar_opt_default(lcd_digar_opt_t *o, int is_ont);
int lcd_digar_batch(const lcd_digar_opt_t *opt, int n_reads, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off,
                    const int *n_cigar, const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags,
                    int64_t reg_beg, int64_t reg_end, int64_t whole_ref_len, uint64_t **digar_off, lcd_digar_t **digars, uint64_t **iv_off,
                    lcd_noisy_iv_t **ivs, uint8_t **iv_in_chunk, int *status, int64_t *beg, int64_t *end, int *n_cand_vars);
/* the reference's three other digar sources (src/collect_var.c:1072-1079 picks one per read: EQX CIGAR, else cs tag, else MD tag, else the reference
 * bases); same outputs as lcd_digar_batch.
 *   lcd_digar_batch_tags, mode LCD_DIGAR_CS == collect_digar_from_cs_tag (src/bam_utils.c:844-1008): tags[r] = the read's cs:Z string (short or long
 *     form); clips come from the first / last CIGAR operation, with that function's own clip rule (:884-888, :969-972);
 *   lcd_digar_batch_tags, mode LCD_DIGAR_MD == collect_digar_from_MD_tag (:1010-1177): tags[r] = the MD:Z string, the CIGAR has 'M';
 *   lcd_digar_batch_ref == collect_digar_from_ref_seq (:1179-1328): seq_pool + seq_off[r] = bam_get_seq (4-bit bases), ref_seq[0] is reference position
 *     ref_beg (1-based), ref_end inclusive (chunk->ref_seq / ref_beg / ref_end); the base comparison runs on the device.
 * The tag strings are parsed on the host (they are as long as the read has events) into EQX-shaped operations for the same kernel.  A tag that does
 * not fit its CIGAR, an unknown cs character or '=' / 'X' next to an MD tag -- where the reference stops the program -- gives status[r] = -2. */
#define LCD_DIGAR_CS 1
#define LCD_DIGAR_MD 2
int lcd_digar_batch_tags(const lcd_digar_opt_t *opt, int mode, int n_reads, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off,
                         const int *n_cigar, const char *const *tags, const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen,
                         const uint8_t *pal_flags, int64_t reg_beg, int64_t reg_end, int64_t whole_ref_len, uint64_t **digar_off, lcd_digar_t **digars,
                         uint64_t **iv_off, lcd_noisy_iv_t **ivs, uint8_t **iv_in_chunk, int *status, int64_t *beg, int64_t *end, int *n_cand_vars);
int lcd_digar_batch_ref(const lcd_digar_opt_t *opt, int n_reads, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off,
                        const int *n_cigar, const uint8_t *seq_pool, const uint64_t *seq_off, const uint8_t *qual_pool, const uint64_t *qual_off,
                        const int *qlen, const uint8_t *pal_flags, const char *ref_seq, int64_t ref_beg, int64_t ref_end, int64_t reg_beg,
                        int64_t reg_end, int64_t whole_ref_len, uint64_t **digar_off, lcd_digar_t **digars, uint64_t **iv_off, lcd_noisy_iv_t **ivs,
                        uint8_t **iv_in_chunk, int *status, int64_t *beg, int64_t *end, int *n_cand_vars);

/* ---- retrotransposon annotation of SV-size gaps (host code in the reference: src/align.c:32-163, src/kmer.c; host code here) ----
 * The variant builder calls collect_te_info_from_cons for every INS / DEL of at least min_sv_len bases (src/collect_var.c:1817,1834; :801 for a candidate
 * variant through collect_te_info_from_var); its results are cand_var_t.tsd_len / tsd_seq / tsd_pos1 / tsd_pos2 / polya_len / te_seq_i / te_is_rev.
 *   lcd_te_lib_create      == make_te_kmer_idx (src/kmer.c:120-150) without the file reading: per TE sequence the set of its overlapping k-mers and the set of
 *                             their reverse complements (kmer_len = opt->te_kmer_len, 15; 1..15), "simple" k-mers left out by the reference's own rule (:16-24);
 *   lcd_check_te_seq       == check_te_seq (:218-253): index of the TE sequence sharing most of seq's non-overlapping k-mers (>= 3), -1 if none; *is_rev
 *                             untouched when seq yields no k-mer;
 *   lcd_collect_te_info    == collect_te_info (src/align.c:32-83): returns the target-site-duplication length (0: not a TE candidate) and, if > 0, its bases
 *                             in tsd_seq (caller's buffer of opt->max_tsd_len bytes), its positions, the poly-A (> 0) / poly-T (< 0) length and the TE hit;
 *                             bases are codes 0-4; var_type 1 = BAM_CINS, 2 = BAM_CDEL; lib may be NULL (opt->n_te_seqs == 0);
 *   lcd_collect_te_info_from_cons == collect_te_info_from_cons (:139-163): the gap and the reference behind it taken from the consensus row / the chunk's reference
 *                             (ref_seq[0] = position ref_beg, letters or codes; outside [ref_beg, ref_end] = N); with cons_msa_seq = alt_seq and
 *                             msa_gap_start = 0 it is collect_te_info_from_var (:87-131). */
typedef struct lcd_te_lib_t lcd_te_lib_t;
typedef struct lcd_te_opt_t { int min_tsd_len, max_tsd_len, min_polya_len; float min_polya_ratio; } lcd_te_opt_t;   /* 2, 100, 10, 0.8 (src/call_var_main.h:55-58) */
void lcd_te_opt_default(lcd_te_opt_t *o);
lcd_te_lib_t *lcd_te_lib_create(int n_seqs, const char *const *seqs, const int *lens, int kmer_len);
void lcd_te_lib_destroy(lcd_te_lib_t *lib);
int lcd_te_lib_n_seqs(const lcd_te_lib_t *lib);
int lcd_check_te_seq(const lcd_te_lib_t *lib, const uint8_t *seq, int len, int *is_rev);
int lcd_collect_te_info(const lcd_te_opt_t *opt, const lcd_te_lib_t *lib, int var_type, const uint8_t *gap_seq, const uint8_t *flank_ref_seq, int gap_len,
                        int64_t gap_pos, uint8_t *tsd_seq, int64_t *tsd_pos1, int64_t *tsd_pos2, int *tsd_polya_len, int *te_seq_i, int *te_is_rev);
int lcd_collect_te_info_from_cons(const lcd_te_opt_t *opt, const lcd_te_lib_t *lib, const char *ref_seq, int64_t ref_beg, int64_t ref_end, int64_t gap_ref_start,
                                  int msa_gap_start, int var_type, int gap_len, const uint8_t *cons_msa_seq, uint8_t *tsd_seq, int64_t *tsd_pos1, int64_t *tsd_pos2,
                                  int *tsd_polya_len, int *te_seq_i, int *te_is_rev);

/* ---- SURVEY 8(f) f2 -> region jobs: collect_noisy_read_info's digar walk (src/align.c:1392-1456) for many (region, read) pairs in one launch ----
 * pair i = read pair_read[i] (index into digar_off / qlen) against the region [pair_reg_beg[i], pair_reg_end[i]] (1-based, flanks included); digars as
 * lcd_digar_batch returns them.  Out per pair: read_reg_beg / read_reg_end (the read's query interval over the region, src/align.c:1458) and the cover flag
 * (LONGCALLD_NOISY_{LEFT,RIGHT}_{COVER,GAP}; a deletion longer than noisy_reg_flank_len at a region end makes that end a gap). */
int lcd_region_read_slices_batch(int n_pairs, const int *pair_read, const int64_t *pair_reg_beg, const int64_t *pair_reg_end, int n_reads,
                                 const uint64_t *digar_off, const lcd_digar_t *digars, const int *qlen, int noisy_reg_flank_len,
                                 int *read_beg, int *read_end, int *cover);

/* ---- a DEVICE-RESIDENT chunk: records -> digars -> region slices -> a batch's read bases without host round trips ----
 * lcd_chunk_create uploads a chunk's reads ONCE (CIGARs, qualities, the records' 4-bit bases: seq_pool / seq_off as lcd_bam_load_region returns them), makes the
 * digars (lcd_digar_batch's kernel) and KEEPS them in HBM.  The host gets what its glue needs: lcd_chunk_read_info (status / digar->beg / end / #candidates /
 * #digars per read), lcd_chunk_intervals (the noisy windows, pointers into the handle), lcd_chunk_region_slices (per (region, read) pair the query interval and the
 * cover flag, computed on the digars in HBM) and lcd_batch_add_region_from_chunk_dev (a region job whose read bases are unpacked on the device from the chunk at
 * lcd_batch_upload).  No digar and no base crosses PCIe after lcd_chunk_create (lcd_copy_counters: [0] digar bytes D2H, [1] digar bytes H2D, [2] read-base bytes H2D,
 * [3] read-base bytes D2H since process start).  Results == the host path (lcd_digar_batch -> lcd_region_read_slices_batch -> lcd_batch_add_region_from_chunk). */
typedef struct lcd_chunk_s lcd_chunk_t;
struct lcd_bam_reads_t; /* (below: f3) */
lcd_chunk_t *lcd_chunk_create(const lcd_digar_opt_t *opt, int n_reads, const int64_t *pos0, const uint32_t *cigar_pool, const uint64_t *cigar_off, const int *n_cigar,
                              const uint8_t *qual_pool, const uint64_t *qual_off, const int *qlen, const uint8_t *pal_flags, const uint8_t *seq_pool,
                              const uint64_t *seq_off, int64_t reg_beg, int64_t reg_end, int64_t whole_ref_len);
/* f3 on the device, in front of the chunk: sam_itr_queryi + sam_itr_next (htslib: bgzf_read_block + inflate + bam_read1) and the record loop of
 * collect_ref_seq_bam_main (src/bam_utils.c:1672-1706), then collect_digar_from_eqx_cigar (:701-842), for one region of an indexed BAM.  The region's BGZF blocks
 * (the .bai's bins + linear index) are read from the file and uploaded COMPRESSED, inflated on the device (lcd_bgzf_inflate_dev's kernel), the records are found,
 * measured and filtered in HBM (tid, overlap with (reg_beg - 1, reg_end], BAM_FUNMAP / FSECONDARY / FSUPPLEMENTARY, MAPQ >= min_mapq, CG-tag CIGARs of reads with more
 * than 65 535 operations; file order; the loader's stop rule) and their digars made and kept there.  Bases and qualities are never moved: the region jobs unpack
 * bases from the inflated stream, the sampling rule of long regions (calc_read_error_rate, src/seq.c:429) runs on the qualities in HBM.  The host receives 80 bytes
 * per record and, with `meta`, the per-read scalars of lcd_bam_reads_t and the read names (cigar_pool / seq_pool / qual_pool stay NULL; seq_off / qual_off are
 * offsets of the device stream; free with lcd_bam_reads_free).  whole_ref_len = the contig's length in the BAM header; pal_flags = 0 and only reads with an
 * EQX CIGAR (an 'M' operation: status -2, whatever tags the read carries) -- lcd_chunk_create_from_bam_src below lifts both.  Result == lcd_bam_load_region_indexed + lcd_chunk_create on the same region.  A region without reads gives a chunk of 0 reads.
 * NULL on failure (lcd_last_error()); no host path: without a HIP device the call fails. */
lcd_chunk_t *lcd_chunk_create_from_bam(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end,
                                       int min_mapq, int verify_crc, struct lcd_bam_reads_t *meta);
/* Chunks from ANY BAM: per read the digar source the reference chooses (collect_digars_from_bam, src/collect_var.c:1072-1079), and on ONT data the SA-tag palindrome
 * rule (is_ont_palindrome_clip + check_ont_palindrome, src/bam_utils.c:642-698).  minimap2 without --eqx and dorado's aligner write 'M' CIGARs: through
 * lcd_chunk_create_from_bam every such read is status -2; through this entry point it is a read like any other.
 *   Selection (has_equal_X_in_bam_cigar, :51-66): the FIRST operation among '=' / 'X' / 'M' decides -- '=' or 'X': LCD_SRC_EQX; 'M', or none of the three: the first
 *   auxiliary field named cs gives LCD_SRC_CS, else the first named MD gives LCD_SRC_MD, else LCD_SRC_REF.  The fields are walked as bam_aux_get walks them: a field
 *   that runs past the record ends the walk silently, the tags behind it do not exist.  A cs / MD field whose type is not Z: status -2 (the reference would read it as
 *   a string).  LCD_SRC_REF without a reference window (src->ref_seq NULL or ref_end < ref_beg), or with a CIGAR that does not consume exactly the record's l_seq
 *   bases (the comparison reads the 4-bit bases in place): status -2.  A cs / MD value that does not fit its CIGAR: status -2, as lcd_digar_batch_tags.
 *   Per read, digars / noisy windows / iv_in_chunk / status / beg / end / n_cand_vars == lcd_digar_batch, lcd_digar_batch_tags (LCD_DIGAR_CS with the cs function's
 *   own clip rule, LCD_DIGAR_MD; digar->end = bam_endpos) or lcd_digar_batch_ref on that read.  One chunk may mix all four sources; ONE digar launch covers them.
 *   SA rule (src->is_ont != 0 only): the first field named SA, of type Z (another type counts as no tag); its value split on ';', empty pieces skipped; an entry is
 *   `rname,pos,strand,cigar[,...]` with rname and cigar non-empty, pos a decimal integer (one optional sign), strand one character.  PROJECT RULE: an entry that does
 *   not give these four is skipped (the reference's sscanf leaves its variables uninitialised there).  sa_end = pos + the lengths of the M / D / = / X operations of the
 *   entry's CIGAR ('N' is not counted; an operation letter without digits counts 0); primary = [pos0 + 1, bam_endpos]; overlap as check_ont_palindrome's four cases;
 *   palindromic if (double)overlap >= (double)primary_len * 0.9 for any entry.  rname and strand are not consulted.  A palindromic read on the reverse strand (flag 16)
 *   gets the left-clip flag, any other the right-clip flag (pal_flags bit 0 / bit 1 of lcd_digar_batch).
 *   What crosses PCIe: the cs / MD tag VALUES of the CS / MD reads (with their CIGAR words; O(events) bytes, parsed on the host like lcd_digar_batch_tags does) and the
 *   operation words made from them going back -- never a base, a quality or a digar; the reference window goes up once per chunk.
 * src == NULL: lcd_chunk_create_from_bam.  The chunk is the same kind of chunk: every lcd_chunk_* / lcd_chunks_* call accepts it.
 * lcd_chunk_read_sources: per read LCD_SRC_* (what the reference would have chosen, whatever the outcome; LCD_SRC_EQX for a chunk made any other way), the
 * chunk->is_ont_palindrome flag, and the summed strlen of the cs / MD values brought to the host; any pointer may be NULL.  lcd_chunk_stage_ms: wall-clock
 * milliseconds of lcd_chunk_create_from_bam_src's stages [aux fields, reference comparison, tag download + host parse, digars] (zeros without src).
 * lcd_chunk_digars: a malloc()'d CSR copy of the digars ANY chunk holds in HBM (tests, debugging; counted in lcd_copy_counters[0]); free() both. */
#define LCD_SRC_EQX 0
#define LCD_SRC_CS  1
#define LCD_SRC_MD  2
#define LCD_SRC_REF 3
typedef struct lcd_chunk_src_t {
    const char *ref_seq; int64_t ref_beg, ref_end;  /* chunk->ref_seq window, letters or codes 0-4, 1-based inclusive; NULL: no reference */
    int is_ont;                                     /* != 0: apply the SA-tag palindrome rule */
} lcd_chunk_src_t;
lcd_chunk_t *lcd_chunk_create_from_bam_src(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom,
                                           int64_t reg_beg, int64_t reg_end, int min_mapq, int verify_crc,
                                           const lcd_chunk_src_t *src, struct lcd_bam_reads_t *meta);
int lcd_chunk_read_sources(const lcd_chunk_t *c, uint8_t *source, uint8_t *is_ont_palindrome, uint64_t *tag_bytes_d2h);
/* chunk->ordered_read_ids: sort_chunk_reads (src/bam_utils.c:1616-1656) orders a chunk's reads by position, then end DESCENDING, then the NM tag, then the read name;
 * a coordinate-sorted BAM fixes only the first key, and the pile-up, K5 and collect_noisy_reg_reads1 all walk the reads in this order.
 * lcd_chunk_read_nm: bam_get_NM (:1632-1639) per kept read of a chunk made from a BAM, computed on the records in the inflated stream in HBM (one lane per record;
 *   4 bytes per read come back).  The auxiliary fields are hopped as bam_aux_get hops them: a field that runs past the record ends the walk.  The first field named
 *   NM gives the value for the types c C s S i I (an I above 2^31 - 1 wraps: the reference stores bam_aux2i's result in an int).  PROJECT RULE: any other type
 *   gives 0 and no NM field gives 0 (htslib's bam_aux2i is not part of the reference checkout; this is its documented behaviour: 0 with errno EINVAL).
 *   Returns n_reads, or -4 for a chunk that was not made from a BAM (its records never existed on the device).
 * lcd_sort_chunk_reads: comp_bam_read_sort on flat arrays, pure host code (no device needed): pos0 ascending, end_pos descending, nm ascending, strcmp of
 *   name_pool + name_off[i] (lcd_bam_reads_t's fields).  PROJECT RULE: entries equal in all four keys keep file order (qsort leaves their order unspecified).
 *   order_out[k] = the read at rank k.  Returns n or < 0. */
int lcd_chunk_read_nm(const lcd_chunk_t *c, int *nm_out);
int lcd_sort_chunk_reads(int n, const int64_t *pos0, const int64_t *end_pos, const int *nm, const uint64_t *name_off, const char *name_pool, int *order_out);
void lcd_chunk_stage_ms(const lcd_chunk_t *c, double out[4]);
int lcd_chunk_digars(const lcd_chunk_t *c, uint64_t **digar_off, lcd_digar_t **digars);   /* malloc()'d CSR copy; counted in lcd_copy_counters[0] */
void lcd_chunk_destroy(lcd_chunk_t *c);
int lcd_chunk_n_reads(const lcd_chunk_t *c);
int lcd_chunk_read_info(const lcd_chunk_t *c, int *status, int64_t *beg, int64_t *end, int *n_cand_vars, int *n_digars);
int lcd_chunk_intervals(const lcd_chunk_t *c, const uint64_t **iv_off, const lcd_noisy_iv_t **ivs, const uint8_t **iv_in_chunk);
int lcd_chunk_region_slices(const lcd_chunk_t *c, int n_pairs, const int *pair_read, const int64_t *pair_reg_beg, const int64_t *pair_reg_end, int noisy_reg_flank_len,
                            int *read_beg, int *read_end, int *cover);
int lcd_batch_add_region_from_chunk_dev(lcd_batch_t *b, const lcd_chunk_t *c, int64_t reg_beg, int64_t reg_end, int n, const int *read_ids, const int *read_beg,
                                        const int *read_end, const int *cover, const int *haps, const int64_t *phase_sets, const uint8_t *ref_seq, int ref_seq_len);
void lcd_copy_counters(unsigned long long out[4]);

/* ---- SURVEY 8(f) f2, chunk level: pre_process_noisy_regs (src/collect_var.c:557-638) ----
 * chunk_noisy: the intervals cr_add()'ed to chunk->chunk_noisy_regs while the reads were loaded (lcd_digar_batch: ivs[k] with iv_in_chunk[k]), in
 * that order; low_comp: chunk->low_comp_cr as (start, end) pairs (sdust output, may be empty); reads in ordered_read_ids order with the skipped
 * ones left out: digar beg / end and each read's own noisy intervals (CSR, as lcd_digar_batch returns them).  Steps: cr_index, extension to the
 * overlapping low-complexity intervals (:538-553), cr_merge with the label-dependent distance (src/cgranges.c:225-300, twice as the reference
 * does), then per region the reads spanning it and the reads noisy in it (device), kept when noisy >= min_alt_dp and noisy / total >= min_af.
 * Returns the number of surviving regions; *regs_out is malloc()'d, in index order (start = first position - 1, end, label). */
int lcd_pre_process_noisy_regs(const lcd_noisy_iv_t *chunk_noisy, int n_noisy, const int64_t *low_comp, int n_low, int n_reads, const int64_t *read_beg,
                               const int64_t *read_end, const uint64_t *read_iv_off, const lcd_noisy_iv_t *read_ivs, int min_alt_dp, float min_af,
                               lcd_noisy_iv_t **regs_out);

/* cr_merge (src/cgranges.h:73, src/cgranges.c:289): the interval merge chunk_noisy_regs goes through (src/collect_var.c:552, :568 with a negative fixed window =
 * "the smaller of the two labels"; :657 with 0).  Pinned to the reference's own cgranges by tests/golden/cgranges_golden.json.  *out malloc()'d. */
int lcd_cr_merge(const lcd_noisy_iv_t *iv, int n, int fixed_merge_win, lcd_noisy_iv_t **out);

/* post_process_noisy_regs (src/collect_var.c:640-660, collect_noisy_reg_start_end :481-536): every region is grown by noisy_reg_flank_len and
 * further while a candidate variant (categories outside LONGCALLD_NOT_CAND_VAR_CATE, src/collect_var.h:28) sits within the flank, then overlapping /
 * touching regions are merged (cr_merge(cr, 0, -1, -1)).  Host code, as in the reference (a two-pointer walk over tens of regions); it closes the
 * region pipeline lcd_digar_batch -> lcd_pre_process_noisy_regs -> here.  regs in index order; vars in chunk order.  *regs_out malloc()'d. */
int lcd_post_process_noisy_regs(const lcd_noisy_iv_t *regs, int n_regs, int n_vars, const int64_t *var_pos, const int *var_ref_len, const int *var_cate,
                                int noisy_reg_flank_len, lcd_noisy_iv_t **regs_out);

/* ---- low-complexity intervals of a chunk's reference: sdust (src/sdust.c), as chunk->low_comp_cr is filled (src/bam_utils.c:1573-1581) ----
 * seq: raw codes 0..3 (4+ = N) or letters; T, W: LONGCALLD_SDUST_T 5 / LONGCALLD_SDUST_W 20 (src/call_var_main.h:82-83), W <= 64.
 * *intervals_out: malloc()'d (start, finish) pairs exactly as sdust() returns them (0-based, half-open); returns their number or < 0. */
int lcd_sdust(const uint8_t *seq, int64_t len, int T, int W, int64_t **intervals_out);
/* the same for the references of many chunks in ONE launch (the recommended form: a single sequence is latency-bound -- 21 ms per 500 kb chunk against 9 ms
 * for the reference's sdust() on one core -- while a pipeline step's worth of chunks shares that latency).  intervals_out[q] malloc()'d, n_out[q] pairs. */
int lcd_sdust_batch(int n_seqs, const uint8_t *const *seqs, const int64_t *lens, int T, int W, int64_t **intervals_out, int *n_out);

/* ---- cross-chunk stitching, genotype emission, tag values (host code in the reference and here: small and serial) ----
 * lcd_flip_variant_hap == flip_variant_hap + update_chunk_{var,read}_hap_phase_set1 (src/collect_var.c:1565-1680): the reads that overlap both chunks
 * vote (same haplotype in both: -1, different: +1); a non-zero score joins the phase sets (cur's smallest read PS becomes pre's largest) and, if
 * positive, swaps haplotypes 1 / 2 of the current chunk's variants (and reads, when update_reads: opt->out_aln_fp != NULL) in that phase set.
 * Overlap lists are the concatenation over the input BAMs of up_ovlp_read_i / down_ovlp_read_i (src/bam_utils.h:64-65). */
typedef struct lcd_chunk_phase_t {
    int tid, n_reads, n_vars;
    const int *ordered_read_ids;
    const uint8_t *is_skipped;
    int *haps; int64_t *phase_sets;                    /* in/out, n_reads */
    int64_t *var_phase_set; int *hap_to_cons_alle;     /* in/out, n_vars and n_vars*3 */
    int n_up_ovlp, n_down_ovlp;
    const int *up_ovlp_read_i, *down_ovlp_read_i;
    int flip_hap; int64_t flip_pre_PS, flip_cur_PS;    /* out (flip_hap starts at 0, src/bam_utils.c:1368) */
} lcd_chunk_phase_t;
int lcd_flip_variant_hap(lcd_chunk_phase_t *pre, lcd_chunk_phase_t *cur, int update_reads);  /* 0, or -6 when the overlap counts disagree (the reference exits) */
int lcd_stitch_chunks(lcd_chunk_phase_t *chunks, int n_chunks, int update_reads);            /* stitch_var_main, src/collect_var.c:2983-2989 */
/* lcd_make_variants == make_variants (src/collect_var.c:1465-1601), germline fields: candidate variants of the output categories inside [reg_beg, reg_end]
 * -> VCF-ready records.  p supplies the chunk state K5 works on (positions, types, categories, coverages, the read x variant profile, var_phase_set,
 * hap_to_cons_alle); var_ref_len / var_alt_len / alt_off + alt_pool / alt_ref_base are the remaining cand_var_t fields; ref_seq is chunk->ref_seq (letters
 * or codes, nst_nt4_table applies) starting at ref_beg.  Returns the number of records; *vars_out malloc()'d (free with lcd_free_variants). */
typedef struct lcd_call_opt_t { double log_p, log_1p, log_2; int max_gq, max_qual, min_sv_len, min_dp, min_alt_dp, out_amb_base; } lcd_call_opt_t;
typedef struct lcd_var1_t {          /* var1_t, src/call_var_main.h:108-121 (somatic fields left out) */
    int64_t pos, PS;
    int type, ref_len, n_alt_allele, alt_len[2];
    uint8_t *ref_bases, *alt_bases[2];
    int GT[2], DP, AD[3], QUAL, GQ, is_sv, is_clean, n_alt_reads; /* AD[2]: what the reference's formatter reads for a two-alt record -- var1_t has `int DP, AD[2]; uint8_t GT[2]`,
                                                                    * so its AD[2] is the third allele's coverage when there is one (the store at src/collect_var.c:1561 runs on), else the GT bytes */
    int *alt_read_i;
    int cand_i;                          /* the candidate (index into the lcd_hap_problem_t) the record was made from */
    int tsd_len, polya_len, te_seq_i, te_is_rev;   /* SURVEY a14 (var1_t's retrotransposon members): 0 / 0 / -1 / 0 from lcd_make_variants, filled by lcd_annotate_te */
    int64_t tsd_pos1, tsd_pos2;          /* -1 until then */
    uint8_t *tsd_seq;                    /* malloc()'d, tsd_len codes; freed by lcd_free_variants */
} lcd_var1_t;
void lcd_call_opt_default(lcd_call_opt_t *o);   /* src/call_var_main.c:156-157,209,217-219 */
int lcd_make_variants(const lcd_call_opt_t *opt, const lcd_hap_problem_t *p, const int *var_ref_len, const int *var_alt_len, const uint64_t *alt_off,
                      const uint8_t *alt_pool, const uint8_t *alt_ref_base, const char *ref_seq, int64_t ref_beg, int64_t reg_beg, int64_t reg_end,
                      lcd_var1_t **vars_out);
void lcd_free_variants(lcd_var1_t *vars, int n);
/* the VCF body lines write_var_to_vcf (src/vcf_utils.c:97-268) emits for these records (filters DP / AD / ambiguous bases applied); *text_out malloc()'d,
 * NUL-terminated; returns the number of lines */
int lcd_format_vcf(const lcd_call_opt_t *opt, const char *chrom, const lcd_var1_t *vars, int n_vars, char **text_out);
/* SURVEY a14 in the output records.  The reference computes the annotation when a candidate is made (collect_te_info_from_cons, src/collect_var.c:1817,1834) and copies
 * it into the record (:1504-1520); the values depend only on the candidate's own position, type, length and inserted bases, so here they are computed for the
 * finished records: every INS / DEL record whose gap (without the anchor base) has at least opt->min_sv_len bases.  te_lib may be NULL.  Returns the number of
 * records that got a target-site duplication.  lcd_format_vcf_te == lcd_format_vcf plus the INFO keys write_var_to_vcf adds for them (src/vcf_utils.c:184-195: MEI,
 * TSD, TSDLEN, POLYALEN, TSDPOS1, TSDPOS2, REPNAME = strand + te_names[te_seq_i]); te_names may be NULL (no REPNAME). */
int lcd_annotate_te(const lcd_call_opt_t *opt, const lcd_te_opt_t *te_opt, const lcd_te_lib_t *te_lib, const char *ref_seq, int64_t ref_beg, int64_t ref_end,
                    lcd_var1_t *vars, int n_vars);
int lcd_format_vcf_te(const lcd_call_opt_t *opt, const char *chrom, const lcd_var1_t *vars, int n_vars, const char *const *te_names, char **text_out);
/* HP / PS aux tags of write_processed_read_to_bam (src/bam_utils.c:1955-2006): HP:i is written iff hap != 0, PS:i iff phase set > 0 (an existing tag with
 * another value is replaced, one that should not be there is deleted): has_hp / has_ps say whether the record ends up carrying the tag */
void lcd_read_tags(int n_reads, const int *haps, const int64_t *phase_sets, uint8_t *has_hp, int *hp, uint8_t *has_ps, int64_t *ps);

/* ---- update_digars_from_msa1 (src/align.c:1701-1743; only with --refine-aln -b / -s, host code in the reference too) ----
 * rebuilds one read's digar list around a noisy region from its ref<->read alignment string (aln_strs[c][2k+2], opt.collect_ref_read_aln_str): the old
 * digars left / right of the region (collect_left_digars :1463, collect_right_digars :1500) around per-column digars of the string (collect_full / left /
 * right_msa_digars :1543-1699, by cover flag), joined with the reference's push rule (same_digar1, src/bam_utils.c:557).  digars as lcd_digar_batch returns
 * them (alt_seq is implicit: the read's bases [qi, qi + len)); read_beg / read_end = the read's slice of the region (collect_noisy_read_info's
 * read_reg_beg / read_reg_end).  Returns 0 and the new list (malloc()'d; *n_out may be 0), 1 when double_check_digar rejects the result (the read keeps its
 * old digars, as in the reference), 2 for a read that covers neither end (untouched). */
int lcd_update_digars_from_msa1(const lcd_digar_t *digars, int n_digar, int qlen, int msa_len, const uint8_t *ref_str, const uint8_t *read_str, int full_cover,
                                int64_t noisy_reg_beg, int64_t noisy_reg_end, int read_beg, int read_end, lcd_digar_t **out, int *n_out);

/* ---- the data formats in front of the path, without htslib (host code; lcd_io.cpp) ----
 * lcd_bam_load_region == the record loop of collect_ref_seq_bam_main (src/bam_utils.c:1672-1706) for one input BAM: reads of `chrom` overlapping
 * [reg_beg, reg_end] (1-based, i.e. sam_itr_queryi on (reg_beg - 1, reg_end]) that are mapped, primary (not BAM_FSECONDARY / BAM_FSUPPLEMENTARY) and of
 * MAPQ >= min_mapq (opt->min_mq, 30), in file order, as the flat arrays lcd_digar_batch (pos0, cigar_pool / cigar_off / n_cigar, qual_pool / qual_off, qlen)
 * and lcd_read_view_t (seq_pool + seq_off[r] = bam_get_seq: BAM 4-bit bases) take.  BGZF blocks are inflated in parallel on n_threads host threads
 * (0 = all); the region is a scan of the sorted file.  Returns n_reads or < 0 (lcd_io_last_error()); free with lcd_bam_reads_free. */
typedef struct lcd_bam_reads_t {
    int n_reads, tid, n_targets; int64_t target_len;
    int64_t *pos0, *end_pos;               /* bam1_core_t.pos ; bam_endpos (0-based, exclusive) */
    int *mapq, *flag, *n_cigar, *qlen;
    uint64_t *cigar_off; uint32_t *cigar_pool;   /* words, bam_get_cigar */
    uint64_t *seq_off; uint8_t *seq_pool;        /* bytes, bam_get_seq */
    uint64_t *qual_off; uint8_t *qual_pool;      /* bytes, bam_get_qual */
    uint64_t *name_off; char *name_pool;         /* NUL-terminated, bam_get_qname */
} lcd_bam_reads_t;
int lcd_bam_load_region(const char *bam_path, const char *chrom, int64_t reg_beg, int64_t reg_end, int min_mapq, int n_threads, lcd_bam_reads_t *out);
/* the same records through the BAM's .bai (bins of the region + the linear index's offset, SAM specification 5.2-5.3): only the BGZF blocks of the region's
 * chunks are read and inflated -- what sam_itr_queryi does for the reference (src/bam_utils.c:1673) */
int lcd_bam_load_region_indexed(const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end, int min_mapq, lcd_bam_reads_t *out);
void lcd_bam_reads_free(lcd_bam_reads_t *r);
/* BGZF blocks inflated ON THE DEVICE (inflate_kernel.hip) -- what bgzf_read_block + zlib's inflate do for the reference one block at a time on the calling thread
 * (htslib behind sam_itr_next, src/bam_utils.c:1673-1675).  `file` is an image of a BGZF file or of a run of whole blocks (e.g. a .bai chunk): the block table
 * comes from the BSIZE fields on the host (a hop per block), the compressed bytes are uploaded once, every block is one wavefront (dynamic / fixed / stored
 * deflate blocks, decode tables and the 32 KB history in LDS), and the inflated stream -- the blocks' outputs back to back, exactly the bytes bgzf_read
 * delivers -- stays in HBM: lcd_inflated_dev_ptr / lcd_inflated_size.  verify_crc != 0 checks every block's CRC-32 on the device (ISIZE is always checked).
 * Returns NULL on a malformed container / deflate stream / CRC mismatch (lcd_io_last_error() names the block) and when there is no HIP device: this entry
 * point has no host path (lcd_bam_load_region inflates on host threads).  lcd_inflated_to_host copies a range of the stream back (the record walk of a
 * loader, tests); lcd_inflated_kernel_ms / lcd_inflated_upload_ms: HIP-event times of the decode kernel and of the upload, for the measurement. */
typedef struct lcd_inflated_s lcd_inflated_t;
lcd_inflated_t *lcd_bgzf_inflate_dev(const uint8_t *file, size_t n, int verify_crc);
uint64_t lcd_inflated_dev_ptr(const lcd_inflated_t *h);
size_t lcd_inflated_size(const lcd_inflated_t *h);
size_t lcd_inflated_n_blocks(const lcd_inflated_t *h);
double lcd_inflated_kernel_ms(const lcd_inflated_t *h);
double lcd_inflated_upload_ms(const lcd_inflated_t *h);
int lcd_inflated_to_host(const lcd_inflated_t *h, size_t off, size_t n, uint8_t *out);
void lcd_inflated_free(lcd_inflated_t *h);

/* ---- the inverse: BGZF blocks COMPRESSED on the device (deflate_kernel.hip), one wavefront per block ----
 * The input (host bytes, or n bytes already in HBM at dev_ptr) is cut into payloads of block_payload bytes (0: 0xff00, htslib's size; 1 ... 0xff00); each becomes
 * one BGZF member (SAM specification 4.1: 18-byte header with the BC field and BSIZE, a raw deflate stream, CRC-32, ISIZE); add_eof appends the standard 28-byte
 * empty member; n == 0 gives that member alone, or an empty image.  LZ77 matches (distance <= 32 768, length 3 ... 258, one candidate per position from a hash table
 * in LDS), dynamic Huffman codes limited to 15 bits, or fixed codes, or -- when neither is smaller -- stored: a member is at most payload + 5 + 26 bytes.  The file
 * image is contiguous in HBM (the members are compacted by a second kernel); lcd_deflated_to_host copies a range of it.  lcd_deflated_block_info: a member's payload
 * bytes, its total size and its kind (0 stored, 1 fixed codes, 2 dynamic codes).  lcd_deflated_kernel_ms: HIP-event time from the compressor's launch to the end
 * of the compaction.  No host path: without a device the calls fail (NULL + lcd_last_error). */
typedef struct lcd_deflated_s lcd_deflated_t;
lcd_deflated_t *lcd_bgzf_deflate_dev(const uint8_t *data, size_t n, int block_payload, int add_eof);
lcd_deflated_t *lcd_bgzf_deflate_dev_ptr(uint64_t dev_ptr, size_t n, int block_payload, int add_eof);
size_t lcd_deflated_size(const lcd_deflated_t *h);
size_t lcd_deflated_n_blocks(const lcd_deflated_t *h);
double lcd_deflated_kernel_ms(const lcd_deflated_t *h);
int lcd_deflated_block_info(const lcd_deflated_t *h, size_t i, uint32_t *payload, uint32_t *bsize, int *kind);
int lcd_deflated_to_host(const lcd_deflated_t *h, size_t off, size_t n, uint8_t *out);
void lcd_deflated_free(lcd_deflated_t *h);
/* faidx_fetch_seq of chrom:[beg, end] (1-based inclusive, clipped to the contig) through <fa_path>.fai, as byte codes A0 C1 G2 T3 N4 (get_bam_chunk_reg_ref_seq0,
 * src/bam_utils.c:1558); returns the length, *codes_out malloc()'d */
int64_t lcd_fasta_fetch(const char *fa_path, const char *chrom, int64_t beg, int64_t end, uint8_t **codes_out);
/* the header lines write_vcf_header appends (src/vcf_utils.c:17-96) + the column line.  htslib's bcf_hdr_write decides the final order / ##fileformat line of
 * the real tool and is absent from the reference checkout: this text is not pinned (the body lines, lcd_format_vcf, are). */
int lcd_vcf_header(const char *source_version, const char *cmdline, const char *date_yyyymmdd, int n_contigs, const char *const *contig_names,
                   const int64_t *contig_lens, const char *sample_name, char **text_out);
const char *lcd_io_last_error(void);

/* ---- kernel-level batches (also what the per-call mirrors above run on) ---- */
int lcd_edlib_batch(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen,
                    const uint64_t *t_off, const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid);
/* the same in HW (infix) mode; start / end (nullable): the target stretch [start, end] the path was taken on = edlib's startLocations[0] / endLocations[0] */
int lcd_edlib_batch_hw(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *q_off, const int *qlen,
                       const uint64_t *t_off, const int *tlen, int *dist, int *xgaps, int *n_eq, int *n_xid, int *start, int *end);
/* want bit0: cigars into cigars[i*cigar_stride ..], bit1: rows into rows[i*2*row_stride ..] (pattern row, then text row at +row_stride) */
int lcd_wfa_batch(int n, const uint8_t *pool, uint64_t pool_len, const uint64_t *p_off, const int *plen, const uint64_t *t_off,
                  const int *tlen, const int *gap_aln, int b, int q, int e, int q2, int e2, int want, int *score,
                  uint32_t *cigars, int cigar_stride, int *n_cigar, uint8_t *rows, int row_stride, int *aln_len);
/* bytes of device work arena one alignment of optimal score <= score_bound occupies: the decision bytes of one block of scores (1 B per diagonal,
 * 16 MB blocks) + the snapshots of the value ring, instead of 20 B x score^2 of retained wavefronts */
uint64_t lcd_wfa_arena_bytes(int plen, int tlen, int score_bound, int b, int q, int e, int q2, int e2);
/* POA chains with the anchor results supplied by the caller: mode 0 = K1 (src/align.c:762), 1 = K2 (:872).
 * anchors: 4 ints per read (ref_beg, ref_end, read_beg, read_end; 1-based).  Outputs are copied into caller arrays:
 * cons (2*cons_stride per chain), msa ((max_reads+2)*msa_stride per chain, row r at r*msa_stride), clu_ids (2*max_reads per chain). */
int lcd_poa_batch(const lcd_opt_t *opt, int n_chains, const int *mode, const int *chain_read0, const int *chain_n_reads,
                  int n_reads_total, const uint64_t *seq_off, const int *len, const int *skip, const int *anchors,
                  const uint8_t *pool, uint64_t pool_len, int *status, int *n_cons, int *cons_len, int *msa_len, int *clu_n,
                  uint8_t *cons, int cons_stride, uint8_t *msa, int msa_stride, int max_reads, int *clu_ids);

/* ---- the first round of collect_var_main on a DEVICE-RESIDENT chunk (src/collect_var.c:2897-2980, steps 1.2 - 3.1; germline) ----
 * == collect_all_cand_var_sites (:1209) + collect_cand_vars (:238, update_cand_vars_from_digar src/bam_utils.c:287) + classify_cand_vars (:902: classify_var_cate,
 * the extra noisy regions of low-complexity / overlapping variants, cr_merge2, post_process_noisy_regs, the compaction :1007-1023) + collect_read_var_profile (:1389,
 * update_read_vs_all_var_profile_from_digar src/bam_utils.c:446) on the digars, bases and qualities the chunk keeps in HBM (clean_vars_kernel.hip).  No digar crosses
 * PCIe (lcd_copy_counters()[0] is unchanged); a chunk made by lcd_chunk_create keeps its qualities on the host until the first call uploads them once
 * (qual_upload_bytes).  Host code, as in the reference: the interval logic (var_pos_cr counts, cr_add_var_cr, cr_merge2, post_process_noisy_regs, cr_is_contained)
 * and the ONT strand-bias test (var_is_strand_bias :270, fisher_exact_test src/math_utils.c:119, double precision).
 * Inputs: ordered_read_ids (chunk->ordered_read_ids; a read with status -1 is skipped); is_rev[r] = bam_is_rev (NULL: all forward; only the strand counts read it);
 * ref_seq[0] = position ref_beg (1-based), ref_end inclusive (chunk->ref_seq; codes 0-4 or letters); [reg_beg, reg_end] = chunk->reg_beg / reg_end;
 * pre_regs = lcd_pre_process_noisy_regs' output (chunk->chunk_noisy_regs, index order); low_comp = chunk->low_comp_cr as (start, end) pairs (lcd_sdust).
 * out_somatic != 0 returns -2 (somatic mode is out of scope).  Every array of *out is malloc()'d (lcd_clean_vars_free).  Returns 0 or < 0 (lcd_last_error()). */
typedef struct lcd_clean_opt_t {
    int min_dp, min_alt_dp, min_bq, min_sv_len, noisy_reg_max_xgaps, noisy_reg_flank_len, noisy_reg_merge_dis, is_ont, out_somatic;
    double min_af, max_af; float strand_bias_pval;
} lcd_clean_opt_t;
void lcd_clean_opt_default(lcd_clean_opt_t *o, int is_ont);   /* src/call_var_main.c:113-224: 5, 2, 10, 30, 5, 10, 500, is_ont, 0, 0.2, 0.8, 0.01 */
typedef struct lcd_clean_vars_t {
    int n_vars;                                      /* candidate variants after the compaction of classify_cand_vars, in chunk order */
    int64_t *pos; int *var_type, *ref_len, *alt_len, *cate;  /* cand_var_t fields; cate = chunk->var_i_to_cate */
    int *total_cov, *low_qual_cov, *alle_covs /* 2 per variant: ref, alt */, *strand_alle_covs /* 4 per variant: [fwd ref, fwd alt, rev ref, rev alt] */;
    uint64_t *alt_off; uint8_t *alt_pool;            /* n_vars + 1 offsets; alt_seq codes 0-4 of X / INS variants (none for DEL) */
    int *is_homopolymer_indel;                       /* 0 for every clean-region variant (set by the noisy-region pass only, src/collect_var.c:1754) */
    int n_regs; lcd_noisy_iv_t *regs;                /* chunk->chunk_noisy_regs after cr_merge2 + post_process_noisy_regs, index order */
    int n_reads; int *start_var_idx, *end_var_idx;   /* read_var_profile_t per chunk read (-1 / -2: none) */
    uint64_t *allele_off; int *alleles, *alt_qi;     /* n_reads + 1 offsets; end - start + 1 entries per read with a profile */
    int n_cr; int *cr_read;                          /* chunk->read_var_cr labels in cr_index order */
    uint64_t qual_upload_bytes;                      /* quality bytes this call uploaded (a host-array chunk's first call; else 0) */
    uint8_t *alt_ref_base;                           /* cand_var_t.alt_ref_base per variant: the base make_variants writes in front of a gap record's ALT when it is not 4
                                                      * (src/collect_var.c:1544).  4 = unknown for every first-round variant (:44); see lcd_merge_region_vars.  Last member:
                                                      * a table built by an older caller (NULL here) counts as all 4 wherever the library reads it */
} lcd_clean_vars_t;
int lcd_chunk_clean_vars(const lcd_chunk_t *c, const lcd_clean_opt_t *opt, const int *ordered_read_ids, const uint8_t *is_rev, const uint8_t *ref_seq, int64_t ref_beg,
                         int64_t ref_end, int64_t reg_beg, int64_t reg_end, const lcd_noisy_iv_t *pre_regs, int n_pre_regs, const int64_t *low_comp, int n_low,
                         lcd_clean_vars_t *out);
/* the same for n chunks of a pipeline step, each argument an array of n (is_rev / low_comp entries may be NULL): the chunks run concurrently, each on a stream of
 * its own (one host thread per chunk, at most LCD_HOST_TEAM at a time).  Results == n single calls.  Returns 0 or the first failure. */
int lcd_chunk_clean_vars_batch(int n, const lcd_chunk_t *const *chunks, const lcd_clean_opt_t *opt, const int *const *ordered_read_ids, const uint8_t *const *is_rev,
                               const uint8_t *const *ref_seq, const int64_t *ref_beg, const int64_t *ref_end, const int64_t *reg_beg, const int64_t *reg_end,
                               const lcd_noisy_iv_t *const *pre_regs, const int *n_pre_regs, const int64_t *const *low_comp, const int *n_low, lcd_clean_vars_t *outs);
void lcd_clean_vars_free(lcd_clean_vars_t *v);
/* an lcd_hap_problem_t view over v for K5 (lcd_assign_hap_germline): pointers into v and the caller's arrays; alle_off (n_vars + 1) and allele_off (n_reads + 1)
 * are filled here; haps / phase_sets / ... (the outputs) stay the caller's to set.  Returns 0. */
int lcd_clean_vars_hap_problem(const lcd_clean_vars_t *v, int is_ont, const int *ordered_read_ids, const uint8_t *is_skipped, int *alle_off, int *allele_off,
                               lcd_hap_problem_t *p);

/* ---- a pass's noisy-region variants folded into the chunk: merge_var_profile (src/collect_var.c:1298-1387) as collect_noisy_vars1 (:2711) calls it per region ----
 * cur = the chunk's state (lcd_chunk_clean_vars' output, or an earlier merge's); regions[k] = what lcd_batch_region_vars returned for the k-th region the caller
 * processed (borrowed; the order matters: lcd_sort_noisy_regs below gives the reference's).  The result is the left fold of one merge per region; a region with
 * n_vars <= 0 changes nothing.
 *   variant table   a two-pointer walk of the current table with the region's list IN THE ORDER GIVEN (MSA column order; not sorted first), compared with
 *                   exact_comp_var_site (:1878: position key, type, ref_len, alt_len, alt bases of X / INS; no fuzzy insertion match): the smaller entry is
 *                   emitted, on equality the table's entry stays and the region's is dropped.  A kept table entry carries all its fields; a kept region entry
 *                   takes pos, var_type, ref_len, alt_len, cate, total_cov, alle_covs, is_homopolymer_indel and alt_seq from its lcd_noisy_var_t, and its
 *                   low_qual_cov and strand_alle_covs are 0: make_cand_vars0 (:1746) clears the whole cand_var_t and the noisy-region pass never counts them.
 *                   alt_ref_base: a kept table entry carries its value (all 4 when cur->alt_ref_base is NULL); a kept region entry follows make_cand_vars0's
 *                   rule (:1755-1756: `if (var_type == BAM_CDIFF) var->ref_base = ref_base; else var->alt_ref_base = alt_ref_base;` on the cleared struct):
 *                   0 for an X variant, lcd_noisy_var_t.alt_ref_base for an insertion / deletion.
 *   profile         per chunk read (skipped reads: (-1, -2), no cells): every cell of its current span moves to the merged index of its variant, every cell of
 *                   its row's span in a region (prof_start >= 0 and prof_end >= prof_start) to the merged index of that region variant with alt_qi = -1, unless
 *                   the variant was dropped (the old allele at the equal variant stays); start / end = min / max of the moved indices, cells nobody moved are
 *                   allele -1 / alt_qi -1, a read without a cell keeps (-1, -2).  Computed on the device (merge_vars_kernel.hip).
 *   cr_read / n_cr  rebuilt as in lcd_chunk_clean_vars; n_regs / regs are copied; qual_upload_bytes = 0.
 * out is freed with lcd_clean_vars_free and lcd_clean_vars_hap_problem works on it unchanged; cur->n_vars == 0 is legal.  cur_to_merged (cur->n_vars entries) and
 * region_to_merged[k] (regions[k].n_vars entries, -1 = dropped) are the maps through the whole fold: what a caller carries per-variant K5 state (var_phase_set,
 * hap_to_cons_alle, hap_to_alle_profile) across the merge with; both may be NULL.  Malformed input -- a row read id outside [0, n_reads), a span outside
 * [0, n_vars), a read twice in one region, n_regions < 0 -- returns < 0 (lcd_last_error()) before anything is launched.  The table walk is host code (sequential,
 * regions x table size); the batch form runs all chunks through one upload, one set of launches on one stream, one device allocation, one download and one
 * synchronisation (every argument an array of n_chunks; cur_to_merged / region_to_merged and their entries may be NULL).  Results == n_chunks single calls. */
typedef struct lcd_region_vars_t {   /* one region's lcd_batch_region_vars output, borrowed */
    int n_vars; const lcd_noisy_var_t *vars;
    int n_rows; const int *row_read_ids, *prof_start, *prof_end, *prof_alleles;
} lcd_region_vars_t;
int lcd_merge_region_vars(const lcd_clean_vars_t *cur, int n_regions, const lcd_region_vars_t *regions, const int *ordered_read_ids, const uint8_t *is_skipped,
                          lcd_clean_vars_t *out, int *cur_to_merged /* cur->n_vars, may be NULL */,
                          int **region_to_merged /* n_regions arrays of n_vars, may be NULL; -1 = dropped */);
int lcd_merge_region_vars_batch(int n_chunks, const lcd_clean_vars_t *const *cur, const int *n_regions, const lcd_region_vars_t *const *regions,
                                const int *const *ordered_read_ids, const uint8_t *const *is_skipped, lcd_clean_vars_t *outs, int *const *cur_to_merged,
                                int **const *region_to_merged);
/* sort_noisy_regs (src/collect_var.c:2745-2769), host code: the order in which collect_var_main processes the chunk's noisy regions -- by label, then by
 * end - start, as that function's exchange sort leaves them (NOT stable: regions with equal keys can change places).  order_out[i] = index of the i-th region. */
int lcd_sort_noisy_regs(const lcd_noisy_iv_t *regs, int n, int *order_out);

/* ---- the noisy-region rounds of collect_var_main (src/collect_var.c:2946-2977) on device-resident chunks (germline) ----
 * lcd_chunk_plan_pass: the plan of one pass -- per region of regs[] (lcd_clean_vars_t.regs) whose done[i] is 0 what collect_noisy_vars1 (:2650-2663) and
 * collect_noisy_read_info (src/align.c:1377-1461) work out before the alignment, computed on the chunk's reads in HBM (plan_kernel.hip):
 *   beg / end    [regs[i].start, regs[i].end] clamped to [ref_beg, ref_end] (collect_reg_ref_bseq, src/seq.c:415-426);
 *   status       LCD_PLAN_DONE_BEFORE (done[i] != 0) | LCD_PLAN_SKIP_LONG (clamped length > max_noisy_reg_len: the reference returns 0, the region is done without a
 *                variant) | LCD_PLAN_SKIP_DEEP (more than max_noisy_reg_cov reads: the same) | LCD_PLAN_NO_READS (collect_noisy_reg_aln_strs returns 0 for
 *                n <= 0, src/align.c:1763: not done, tried again in the next pass) | LCD_PLAN_SUBMIT;
 *   read list    collect_noisy_reg_reads1 (:1047-1061): every read of ordered_read_ids, in that order, that is not skipped (is_skipped[r], or the chunk's own status
 *                of the read is not 0) and satisfies !(read.beg > end || read.end <= beg) -- the reference's asymmetric test on the clamped interval;
 *   slices       per (region, read) pair read_beg / read_end / cover, as lcd_chunk_region_slices gives them for the pair with noisy_reg_flank_len.
 * read_off (n_regs + 1 entries) is the CSR into read_ids / read_beg / read_end / cover; only submitted regions have pairs.  Every array of *out is malloc()'d
 * (lcd_pass_plan_free).  The first plan of a chunk uploads its reads' beg / end / status / digar slots once (40 bytes per read, a blocking copy); after that a call
 * uploads the region tables, ordered_read_ids and is_skipped in one staged copy, allocates the pair area once (sized after the count launch), downloads once and
 * synchronises twice: after the counts and at the end.  No digar and no base crosses PCIe (lcd_copy_counters is unchanged).  The batch form takes all regions of
 * all chunks (one device) in one grid on one stream; every argument is an array of n_chunks; results == n_chunks single calls.  Malformed input -- n_regs < 0,
 * ref_end < ref_beg, a NULL chunk, an ordered_read_ids entry outside [0, n_reads) -- returns < 0 (lcd_last_error()) before any device call. */
typedef struct lcd_pass_opt_t { int max_noisy_reg_len, max_noisy_reg_cov, noisy_reg_flank_len; } lcd_pass_opt_t;
void lcd_pass_opt_default(lcd_pass_opt_t *o);   /* 50000, 1000, 10 (src/call_var_main.h:36-42) */
#define LCD_PLAN_DONE_BEFORE 0
#define LCD_PLAN_SKIP_LONG 1
#define LCD_PLAN_SKIP_DEEP 2
#define LCD_PLAN_NO_READS 3
#define LCD_PLAN_SUBMIT 4
typedef struct lcd_pass_plan_t {
    int n_regs; int *status; int64_t *beg, *end;    /* per region */
    uint64_t *read_off;                             /* n_regs + 1 */
    int *read_ids, *read_beg, *read_end, *cover;    /* per pair */
} lcd_pass_plan_t;
int lcd_chunk_plan_pass(const lcd_chunk_t *c, const lcd_pass_opt_t *opt, int n_regs, const lcd_noisy_iv_t *regs, const int *done, const int *ordered_read_ids,
                        const uint8_t *is_skipped, int64_t ref_beg, int64_t ref_end, lcd_pass_plan_t *out);
int lcd_chunk_plan_pass_batch(int n_chunks, const lcd_chunk_t *const *chunks, const lcd_pass_opt_t *opt, const int *n_regs, const lcd_noisy_iv_t *const *regs,
                              const int *const *done, const int *const *ordered_read_ids, const uint8_t *const *is_skipped, const int64_t *ref_beg,
                              const int64_t *ref_end, lcd_pass_plan_t *outs);
void lcd_pass_plan_free(lcd_pass_plan_t *p);
/* n_cons of a region of a downloaded batch (0: collect_noisy_reg_aln_strs could not resolve it; also with opt.collect_noisy_vars == 2, where
 * lcd_batch_region_result is not available): what tells "no consensus" from "resolved without a variant" for the done[] rule of the loop */
int lcd_batch_region_n_cons(lcd_batch_t *b, int region);
/* every LCD_PLAN_SUBMIT region of a plan into a batch through lcd_batch_add_region_from_chunk_dev, in region order: reference bases ref_seq[beg - ref_beg ..
 * end - ref_beg] (codes; ref_seq[0] = position ref_beg), haps / phase_sets (chunk->haps / phase_sets, indexed by read id) gathered by the region's read ids.
 * region_idx_out[i] (plan->n_regs entries, may be NULL) = the batch index of region i, or -1.  Returns the number of regions added or < 0.  Results ==
 * calling lcd_batch_add_region_from_chunk_dev region by region with the same arrays. */
int lcd_batch_add_planned(lcd_batch_t *b, const lcd_chunk_t *c, const lcd_pass_plan_t *plan, const int *haps, const int64_t *phase_sets, const uint8_t *ref_seq,
                          int64_t ref_beg, int *region_idx_out);
/* K5's state (the in/out arrays of lcd_hap_problem_t) on its own, and its way across a merge (host code).  lcd_hap_state_init: malloc()'d arrays with the values
 * the first K5 call starts from (haps 0, phase sets -1, counts 0, var_phase_set -1, hap_to_cons_alle -1, hap_to_alle_profile 0; two alleles per variant).
 * lcd_hap_state_carry: old state -> the merged table of lcd_merge_region_vars: per-read arrays unchanged; per-variant entries of old variant i at
 * cur_to_merged[i] (var_phase_set, hap_to_cons_alle[3i ..], the three hap_to_alle_profile planes through 2 i -> 2 cur_to_merged[i]); variants that came from a
 * region get the fresh values.  A map entry outside [0, n_merged_vars) or two old variants with one target return -4.  *out is malloc()'d (lcd_hap_state_free);
 * out may not alias old. */
typedef struct lcd_hap_state_t {
    int n_reads, n_vars;
    int *haps; int64_t *phase_sets; int *n_clean_agree_snps, *n_clean_conflict_snps;    /* n_reads */
    int64_t *var_phase_set; int *hap_to_cons_alle /* 3 n_vars */, *hap_to_alle_profile /* 3 planes of 2 n_vars */;
} lcd_hap_state_t;
int lcd_hap_state_init(int n_reads, int n_vars, lcd_hap_state_t *out);
int lcd_hap_state_carry(const lcd_hap_state_t *old, int n_merged_vars, const int *cur_to_merged, lcd_hap_state_t *out);
void lcd_hap_state_free(lcd_hap_state_t *s);
/* lcd_chunks_noisy_rounds: n_chunks device chunks (one device) from "first round done" (lcd_chunk_clean_vars + K5 over the clean categories) to the fixed point of
 * the loop at :2952-2975.  lcd_sort_noisy_regs once per chunk; then per pass: lcd_chunk_plan_pass_batch over the chunks that are still in the loop, one batch per
 * chunk (lcd_batch_add_planned) through ONE lcd_batch_run_many, lcd_batch_region_vars per submitted region in sorted-region order, done[] by the reference's rule
 * (a region whose call returned >= 0 variants is done, n_cons == 0 leaves it, long / deep regions are done), lcd_merge_region_vars_batch + lcd_hap_state_carry +
 * lcd_clean_vars_hap_problem + lcd_assign_hap_batch over LONGCALLD_CAND_GERMLINE_VAR_CATE for exactly the chunks that got a variant (new_var), and a chunk leaves
 * the loop after a pass in which none of its regions became done.  Regions of one pass are independent in germline mode (SURVEY CS-2); opt->collect_ref_read_aln_str
 * != 0 (out_somatic / refine) returns -2.  opt->collect_noisy_vars is forced to 2: only variants and alleles cross PCIe.
 * In per chunk: chunk, vars (lcd_chunk_clean_vars' output: owned by the driver from a successful return on, i.e. freed and replaced), state (after the clean-
 * category K5 call, arrays malloc()'d: freed and replaced), ordered_read_ids, is_skipped, ref_seq (codes 0-4, ref_seq[0] = position ref_beg) / ref_beg / ref_end,
 * is_ont.  Out per chunk: vars (final table + profile), state (final, arrays sized to the final table), done (malloc()'d, n_regs), n_passes, n_first_vars and
 * first_to_final (malloc()'d: first-round variant index -> final index).  On a failure of any stage everything the driver allocated is freed, vars / state are as
 * they were handed in, the out fields are NULL / 0 and the stage's error is returned. */
typedef struct lcd_rounds_chunk_t {
    const lcd_chunk_t *chunk;
    lcd_clean_vars_t *vars; lcd_hap_state_t *state;
    const int *ordered_read_ids; const uint8_t *is_skipped;
    const uint8_t *ref_seq; int64_t ref_beg, ref_end;
    int is_ont;
    int *done; int n_passes; int n_first_vars; int *first_to_final;   /* out */
} lcd_rounds_chunk_t;
int lcd_chunks_noisy_rounds(int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt);

/* ---- the head of collect_var_main (src/collect_var.c:2897-2945) for a pipeline step's device chunks (one device): from the chunk handles to "first round done",
 * i.e. to the lcd_rounds_chunk_t fields lcd_chunks_noisy_rounds takes.  Per chunk, in the reference's order:
 *   order        ordered_read_ids as given (copied), or -- NULL -- sort_chunk_reads from meta (pos0, end_pos, names) + lcd_chunk_read_nm + lcd_sort_chunk_reads:
 *                that needs a chunk made from a BAM and its meta, else -4;
 *   is_skipped   is_skipped[r] = the chunk's status of read r != 0.  The reference has ONE writer of is_skipped on this path, collect_digars_from_bam
 *                (src/collect_var.c:1081: `if (ret < 0)`), and every collect_digar_from_* failure is negative: status -1 (too noisy) and -2 (no usable source) both
 *                skip the read, everywhere from pre_process_noisy_regs (:586) on;
 *   low_comp     chunk->low_comp_cr (src/bam_utils.c:1573-1581): sdust (T 5, W 20) over the reference bases of [reg_beg, reg_end] -- NOT of the whole window -- as
 *                (reg_beg + start - 1, reg_beg + finish - 1) pairs; all chunks in one lcd_sdust_batch.  A region reaching outside [ref_beg, ref_end] is cut to it;
 *   pre_regs     pre_process_noisy_regs (:557-638) from the handle: the windows of the reads that are not skipped, in ordered_read_ids order (the order
 *                collect_digars_from_bam cr_add()s them in), filtered by iv_in_chunk; index, low-complexity extension and cr_merge on the host; the read support
 *                of ALL chunks' regions in one upload, one launch on one stream and one synchronisation; kept when noisy >= opt->min_alt_dp and
 *                noisy / total >= (float)opt->min_af;
 *   vars         lcd_chunk_clean_vars_batch (is_rev as given, or meta->flag & 16 when is_rev is NULL and meta is given, else all forward);
 *   state        lcd_hap_state_init; for the chunks with n_vars > 0 (:2934) lcd_clean_vars_hap_problem and ONE lcd_assign_hap_batch over
 *                LONGCALLD_CLEAN_HET_SNP | LONGCALLD_CLEAN_HET_INDEL | LONGCALLD_CLEAN_HOM_VAR (:2944).  A chunk without variants keeps the initial state; one
 *                without variants and regions (:2932) or without reads is legal and comes back empty.
 * Every out member is malloc()'d and released by lcd_first_round_free (vars and state are single malloc()'d structs: hand `vars` / `state` to lcd_rounds_chunk_t as
 * they are).  Malformed input -- a NULL chunk / reference, ref_end < ref_beg, a region outside [1, ..], an ordered_read_ids entry outside [0, n_reads) or twice,
 * chunks on different devices -- returns < 0 before anything is launched; opt->out_somatic returns -2.  On a failure of any stage everything allocated is freed,
 * the out members are NULL / 0 and the stage's error is returned.  No digar and no base crosses PCIe. */
typedef struct lcd_first_chunk_t {
    const lcd_chunk_t *chunk;                                        /* in */
    const uint8_t *ref_seq; int64_t ref_beg, ref_end;                /* codes 0-4 or letters, ref_seq[0] = position ref_beg (1-based), ref_end inclusive */
    int64_t reg_beg, reg_end; int is_ont;
    const int *ordered_read_ids; const uint8_t *is_rev;              /* both may be NULL */
    const struct lcd_bam_reads_t *meta;                              /* may be NULL when ordered_read_ids is given */
    int n_reads; int *order; uint8_t *is_skipped;                    /* out: chunk->ordered_read_ids, chunk->is_skipped */
    int n_low; int64_t *low_comp;                                    /* out: (start, end) pairs */
    int n_pre_regs; lcd_noisy_iv_t *pre_regs;                        /* out: pre_process_noisy_regs' regions, index order */
    lcd_clean_vars_t *vars; lcd_hap_state_t *state;                  /* out */
} lcd_first_chunk_t;
int lcd_chunks_first_round(int n_chunks, lcd_first_chunk_t *chunks, const lcd_clean_opt_t *opt);
void lcd_first_round_free(lcd_first_chunk_t *c);

/* ---- the whole germline path in one call: chunks -> stitched genotype records and VCF body lines ----
 * lcd_chunks_call: n chunks of ONE contig in genome order (one device).  Runs lcd_chunks_first_round, lcd_chunks_noisy_rounds, lcd_stitch_chunks
 * (stitch_var_main, src/collect_var.c:2983-2989), per chunk lcd_make_variants on its own [reg_beg, reg_end] + lcd_annotate_te without a TE library, and
 * lcd_format_vcf over the records concatenated in chunk order (merge_vars appends, :2996-2998).
 *   in           chunks[c].first's input members, as for lcd_chunks_first_round; ref_seq as CODES 0-4 (lcd_chunks_noisy_rounds reads them as codes);
 *   stitch       the overlap lists of chunk c are its reads, in file order, whose [beg, end] (digar beg / end = pos0 + 1, bam_endpos) overlaps the previous
 *                (up) / next (down) chunk's [reg_beg, reg_end] by the test of is_ovlp_with_prev_region / _next_region (src/bam_utils.c:1586-1614:
 *                !(read_end < reg_beg || read_beg > reg_end)).  Reads the loader's flag / MAPQ filter dropped never reach a chunk, so only the kept lists
 *                exist.  update_reads = 1: the reads' haplotypes and phase sets are final (what lcd_read_tags takes).  Two neighbours that do not hold the
 *                same number of shared reads return -6, as the reference exits;
 *   out          chunks[c].first's out members, with vars / state = the FINAL table and K5 state (state->haps / phase_sets after the stitch); n_passes of the
 *                noisy-region loop; flip_hap / flip_pre_PS / flip_cur_PS of the stitch (0 / -1 / -1 for a chunk that was not joined); n_records = how many
 *                of the records are this chunk's (they are consecutive).  *records (lcd_var1_t.cand_i indexes the chunk's final table), *vcf_body.
 * cfg->clean.out_somatic or cfg->opt.collect_ref_read_aln_str (somatic / refine) return -2.  On failure everything is freed and the outputs are NULL / 0.
 * lcd_call_free releases the chunks' out members, the records and the text (it does not destroy the chunk handles).
 * lcd_call_bam_regions: the file-level wrapper for n regions of one contig in genome order.  Per region: a first device pass (lcd_chunk_create_from_bam with
 * meta) gives the reads' span; the reference window is fetched around min(reg_beg, read begins) / max(reg_end, read ends) with get_bam_chunk_reg_ref_seq0's
 * 50 000-base padding (src/bam_utils.c:1558-1571) -- the reference, too, loads first and fetches then; when the pass left a read without a digar source (an 'M'
 * CIGAR: status -2) or the data is ONT (the SA-tag rule), the chunk is made again through lcd_chunk_create_from_bam_src with that window.  Then lcd_chunks_call;
 * the chunk handles are destroyed before the call returns (chunks[c].first.chunk / ref_seq / meta are NULL afterwards).  chunks: n caller-allocated entries.  It is
 * declared with the other drivers and their options at the end of this header. */
typedef struct lcd_cfg_t { lcd_clean_opt_t clean; lcd_opt_t opt; lcd_pass_opt_t pass; lcd_call_opt_t call; } lcd_cfg_t;
void lcd_cfg_default(lcd_cfg_t *cfg, int is_ont);   /* lcd_clean_opt_default(is_ont), lcd_opt_default + is_ont, lcd_pass_opt_default, lcd_call_opt_default */
typedef struct lcd_call_chunk_t {
    lcd_first_chunk_t first;
    int n_passes, flip_hap; int64_t flip_pre_PS, flip_cur_PS; int n_records;   /* out */
} lcd_call_chunk_t;
int lcd_chunks_call(int n_chunks, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, lcd_var1_t **records, int *n_records, char **vcf_body);
void lcd_call_free(int n_chunks, lcd_call_chunk_t *chunks, lcd_var1_t *records, int n_records, char *vcf_body);

/* ---- the phased alignment output (longcallD call -b): write_read_to_bam / write_processed_read_to_bam / write_unprocessed_read_to_bam, src/bam_utils.c:1944-2048 ----
 * A chunk made from a BAM remembers every record its region's iterator yields, in file order: kept records (the chunk's reads) and records the loader's flag / MAPQ
 * filter dropped.  The iterator's overlap test applies whatever the flags say; PROJECT RULE (htslib is not in the checkout): a record with the unmapped flag, or
 * whose CIGAR consumes no reference, spans one base (bam_endpos).
 * lcd_chunk_tag_records rewrites those records in HBM (bam_tag_kernel.hip) and leaves them back to back.  The auxiliary fields are hopped as lcd_chunk_read_nm hops
 * them (a field that runs past the record ends the walk); bam_aux2i: types c C s S i I give their value, any other type 0.  A kept record of read r, hap = haps[r],
 * ps = phase_sets[r]: HP first, then PS; a tag is wanted when hap != 0 / ps > 0.  Wanted and the first field of that name holds the value: it stays in place, byte
 * for byte.  Wanted otherwise: the first field (if any) is deleted and HP:i / PS:i (4 bytes, little endian; PS: the low 32 bits) is appended.  Not wanted: the first
 * field is deleted.  Later fields of the same name stay.  The record is its bytes without the deleted fields, the appended HP, the appended PS; only block_size
 * changes.  A filtered record loses its first HP and first PS field.  The first n_skip_kept kept and n_skip_filtered filtered records are not written (the region
 * before has written them).  NULL + lcd_last_error for a chunk that was not made from a BAM.
 * lcd_write_phased (after lcd_chunks_call, before lcd_call_free / the chunks' destruction): the input file's header block with pg_line (one finished @PG line
 * without a newline, or NULL) appended to its text, compressed into its own block(s); then region c's records in region order, the skip counts of region c being
 * its kept / filtered records that overlap region c - 1's [reg_beg, reg_end] (is_ovlp_with_prev_region, src/bam_utils.c:1684-1691); every region's stream through
 * lcd_bgzf_deflate_dev_ptr; the EOF member last.  Only compressed bytes cross PCIe; the file is written with fwrite.  htslib's sam_hdr_add_pg chooses ID / PP
 * itself and is not in the checkout: the @PG text is the caller's.  CRAM output is not supported.
 * lcd_call_bam_regions with bam_out: the alignment output is written after lcd_chunks_call succeeded (bam_out NULL: none).  A failure of the output
 * (unwritable path) returns < 0 with lcd_last_error and leaves *records / *vcf_body / the chunks' out members valid: free them with lcd_call_free as usual. */
typedef struct lcd_tagged_s lcd_tagged_t;
lcd_tagged_t *lcd_chunk_tag_records(const lcd_chunk_t *c, const int *haps, const int64_t *phase_sets, int n_skip_kept, int n_skip_filtered);
uint64_t lcd_tagged_dev_ptr(const lcd_tagged_t *h);
size_t lcd_tagged_size(const lcd_tagged_t *h);
int lcd_tagged_n_records(const lcd_tagged_t *h);
int lcd_tagged_to_host(const lcd_tagged_t *h, size_t off, size_t n, uint8_t *out);
void lcd_tagged_free(lcd_tagged_t *h);
typedef struct lcd_bam_out_t {
    const char *path; const char *pg_line; int block_payload;        /* in; pg_line may be NULL, block_payload 0 = 0xff00 */
    int64_t n_records_out, n_filtered_out, bytes_inflated, bytes_file; double ms_tag, ms_deflate, ms_download_write;   /* out */
} lcd_bam_out_t;

/* ---- a whole BAM in one call (longcallD call ref.fa in.bam -o out.vcf -b out.bam): call_var_worker_pipeline, src/call_var_main.c:762-815, germline path ----
 * lcd_bam_contigs: the reference table of the BAM header, in header order.  *names: n malloc()'d strings in a malloc()'d array, *lens malloc()'d; release with
 * lcd_bam_contigs_free.  Returns 0 or < 0 (lcd_last_error).
 * lcd_bam_sample_name == extract_sample_name_from_bam_header (src/bam_utils.c:2051-2070): the SM of the first @RG line that has one (a later, different SM does not
 * replace it); *name malloc()'d (free()), or NULL when no @RG line carries SM -- the caller then falls back to the BAM path (src/call_var_main.c:733-735). */
int lcd_bam_contigs(const char *bam_path, int *n_contigs, char ***names, int64_t **lens);
void lcd_bam_contigs_free(int n_contigs, char **names, int64_t *lens);
int lcd_bam_sample_name(const char *bam_path, char **name);
/* lcd_plan_chunks == collect_regions (src/call_var_main.c:404-634) + the fallback of :744-749, host code without a device: the (tid, reg_beg, reg_end) entries, 1-based
 * inclusive, in processing order.
 *   classes      classify_chromosome as written: an optional "chr" prefix is removed; X / Y are sex chromosomes; M / MT are other; a name strtol consumes completely
 *                with a value >= 1 is an autosome (no upper bound: chr23 is one, chr1_random is not).  LCD_CTG_AUTOSOME_XY keeps autosomes and sex chromosomes,
 *                LCD_CTG_AUTOSOME autosomes, LCD_CTG_ALL every contig.  `exclude` (-E) names are always left out;
 *   whole genome per kept contig ceil(len / chunk_len) chunks [i L + 1, min((i + 1) L, len)];
 *   regions      "chr", "chr:beg", "chr:beg-end" (commas in numbers ignored; a string that is a contig name as a whole is that contig), clamped to the contig
 *                (beg = max(1, beg), end = min(end, len)), each cut into chunks from its own beg.  Regions or a BED file switch the classes off, not `exclude`; with
 *                both, the strings win.  An unknown contig or an empty interval plans nothing;
 *   BED          '#' lines are skipped, an unknown contig is skipped, "chr" alone is the whole contig, column 2 is 0-based (+ 1), a missing column 3 is the contig's
 *                end, a line with beg > end or a non-positive bound is skipped; a last line without a newline counts;
 *   several      PROJECT RULE (the reference hands them to htslib's sam_itr_regarray, which is not in the checkout): regions are grouped by contig in header order,
 *                sorted by begin inside a contig, and regions that overlap (beg <= previous end) are merged;
 *   fallback     when nothing is planned, the whole file is planned with the classes off (`exclude` still applies) and out->fallback = 1.
 * chunk_len 0 = 500 000 (LONGCALLD_BAM_CHUNK_REG_SIZE).  The reference's steps (reg_chunks, min_reg_chunks_per_run) are not reproduced: a step boundary only falls
 * where the contig changes and neighbours of another contig are ignored, so they cannot change a result.  The neighbour of an entry is the previous / next entry
 * when it has the same tid.  Arrays malloc()'d; lcd_chunk_plan_free.  Returns the number of entries or < 0 (an unreadable BED file: -30). */
enum { LCD_CTG_AUTOSOME_XY = 0, LCD_CTG_AUTOSOME = 1, LCD_CTG_ALL = 2 };
typedef struct lcd_chunk_plan_t { int n; int *tid; int64_t *reg_beg, *reg_end; int fallback; } lcd_chunk_plan_t;
int lcd_plan_chunks(int n_contigs, const char *const *names, const int64_t *lens, int contig_mode, int n_exclude, const char *const *exclude, int n_regions,
                    const char *const *regions, const char *region_bed_path, int64_t chunk_len, lcd_chunk_plan_t *out);
void lcd_chunk_plan_free(lcd_chunk_plan_t *p);
/* The stitch carried across windows of chunks.  flip_variant_hap(pre, cur) reads pre's FINAL state (src/collect_var.c:1640-1695): its down overlap list, is_skipped,
 * haps, phase_sets and n_vars.  lcd_stitch_carry_t owns copies of those arrays of a window's last chunk (taken after that chunk's own join and swap) with the
 * chunk's tid and region.  lcd_stitch_chunks_carry: the first chunk is joined to carry_in (when given, valid and of the same tid), then lcd_stitch_chunks over the n
 * chunks, then carry_out (when given) is set from the last chunk (n == 0: carry_out becomes a copy of carry_in).  carry_in == carry_out is allowed.  The caller
 * sets carry_out->reg_beg / reg_end (lcd_chunk_phase_t has no region).  A zeroed struct is an empty carry; lcd_stitch_carry_free releases one.  Returns 0 or -6. */
typedef struct lcd_stitch_carry_t {
    int valid, tid; int64_t reg_beg, reg_end;
    int n_reads, n_vars, n_down_ovlp;
    uint8_t *is_skipped; int *haps; int64_t *phase_sets; int *down_ovlp_read_i;
} lcd_stitch_carry_t;
int lcd_stitch_chunks_carry(lcd_chunk_phase_t *chunks, int n_chunks, int update_reads, const lcd_stitch_carry_t *carry_in, lcd_stitch_carry_t *carry_out);
void lcd_stitch_carry_free(lcd_stitch_carry_t *c);
/* Two-phase chunk creation: a region is read and inflated ONCE for every kind of input.  lcd_chunk_open_from_bam does lcd_chunk_create_from_bam_src's region image,
 * inflate, record walk, CIGAR statistics, loader's rule and record table, and fills meta (so the reads' span is known); lcd_chunk_resolve(chunk, src or NULL) does
 * the sources, the comparison with the window, the cs / MD words and the digar launch.  What the second phase needs (the CIGAR words in HBM and their offsets, the
 * counts, the aux jobs, the true reference lengths) stays in the handle until lcd_chunk_resolve and is released there.  lcd_chunk_create_from_bam_src is open
 * followed by resolve.  A handle that was opened and not resolved is refused (-4) by every export that needs digars; lcd_chunk_destroy frees it.  lcd_chunk_resolve
 * on a resolved handle (or one not made by lcd_chunk_open_from_bam) is -4; on failure the handle stays unresolved and is only good for lcd_chunk_destroy. */
lcd_chunk_t *lcd_chunk_open_from_bam(const lcd_digar_opt_t *opt, const char *bam_path, const char *bai_path, const char *chrom, int64_t reg_beg, int64_t reg_end,
                                     int min_mapq, int verify_crc, struct lcd_bam_reads_t *meta);
int lcd_chunk_resolve(lcd_chunk_t *chunk, const lcd_chunk_src_t *src);
/* The appendable phased-BAM writer.  open: the input's header block with out->pg_line appended, in its own BGZF member(s); the counters of *out are zeroed and then
 * accumulate.  append: the records of n called chunks in order (lcd_chunk_tag_records + lcd_bgzf_deflate_dev_ptr per chunk); a chunk leaves out the records that
 * overlap the region of the chunk before it when both are on the same contig (tids[c] == tids[c - 1]; tids NULL: all the same) -- across a window border that chunk
 * is described by prev (NULL: none; prev->valid, tid, reg_beg, reg_end are read).  close: the one EOF member and fclose; lcd_bam_writer_abort closes the file as
 * it is, without the EOF member.  Both free the writer.  lcd_write_phased is open + one append + close.  *out must outlive the writer.  lcd_bam_writer_open and
 * lcd_write_phased are declared with their options (lcd_writer_opt_t) at the end of this header. */
typedef struct lcd_bam_writer_s lcd_bam_writer_t;
int lcd_bam_writer_append(lcd_bam_writer_t *w, int n_chunks, const lcd_call_chunk_t *chunks, const int *tids, const lcd_stitch_carry_t *prev);
int lcd_bam_writer_close(lcd_bam_writer_t *w);
void lcd_bam_writer_abort(lcd_bam_writer_t *w);
/* The VCF writer.  path NULL or "-": stdout.  bgzf 0: plain text through fwrite; 1 (-O z): every append is compressed by lcd_bgzf_deflate_dev into BGZF members
 * of its own and close adds the EOF member.  header_text NULL: no header (-H).  lcd_vcf_writer_abort closes without the EOF member. */
typedef struct lcd_vcf_writer_s lcd_vcf_writer_t;
lcd_vcf_writer_t *lcd_vcf_writer_open(const char *path, int bgzf, const char *header_text);
int lcd_vcf_writer_append(lcd_vcf_writer_t *w, const char *text);
int lcd_vcf_writer_close(lcd_vcf_writer_t *w);
void lcd_vcf_writer_abort(lcd_vcf_writer_t *w);
/* lcd_call_files: the whole-file run (declared with its options at the end of this header).  The plan (lcd_plan_chunks on the BAM header) is processed in windows of window_chunks consecutive entries (a window may span
 * contigs).  Per window -- load: every chunk is opened (lcd_chunk_open_from_bam, up to loader_threads host threads), its reference window fetched around the reads'
 * span with get_bam_chunk_reg_ref_seq0's padding, and resolved with that window (one file read and one inflate per chunk); a chunk without reads stays as an empty
 * entry: it yields nothing, but it is still the neighbour of the chunks beside it.  call: the body of lcd_chunks_call with a contig per chunk, the first chunk's up
 * list taken against the carried region, the last chunk's down list against the next PLANNED region, and lcd_stitch_chunks_carry (update_reads = 1).  write: the
 * text to the VCF writer, the window to the BAM writer; then the window is freed: nothing of it stays but the carry.  overlap 1: the three stages run on three host
 * threads joined by queues of depth one (at most three windows alive); 0: in turn on the calling thread.  Records, text, flips and the output BAM's record stream do
 * not depend on window_chunks, overlap or loader_threads.  The first error stops the pipeline, every thread is joined, both outputs are closed as they are (no EOF
 * member) and the failing stage's code and lcd_last_error are returned.  Somatic / refine settings: -2.  A missing .bai / .fai: -30 with the path in the message (lcd_run_opt_t.idx builds them on request).
 * Defaults: chunk_len 0 = 500 000; window_chunks 0 = 32 (HiFi) / 16 (ONT); overlap -1 = 0 (pipelining did not win reliably where it was measured, profiles/NOTES_call_file.md);
 * loader_threads 0 = 4, or the CPUs the process may use when fewer (an explicit value is cut to 16); bai_path NULL =
 * <bam>.bai; sample_name NULL = lcd_bam_sample_name, else the BAM path; vcf_path NULL or "-" = stdout.  The VCF header names every contig of the BAM header.
 * keep_records != 0: the records of all windows, the per-chunk flips and n_passes are also kept in *stats (tests).  Whatever the return code, release *stats with
 * lcd_file_stats_free (after an error it holds what the finished windows left). */
typedef struct lcd_file_job_t {
    const char *bam_path, *bai_path, *fasta_path;
    int contig_mode; int n_exclude; const char *const *exclude;
    int n_regions; const char *const *regions; const char *region_bed_path;
    int64_t chunk_len;
    int window_chunks, overlap, loader_threads, min_mapq;
    const char *vcf_path; int vcf_bgzf, no_vcf_header; const char *sample_name, *source_version, *cmdline, *date_yyyymmdd;
    lcd_bam_out_t *bam_out;
    int keep_records;
} lcd_file_job_t;
typedef struct lcd_file_stats_t {
    int n_planned, n_loaded, n_empty, n_windows, plan_fallback;
    int64_t n_reads, n_records, n_vcf_lines, n_region_loads;
    double ms_load, ms_call, ms_write, ms_wall;
    int64_t peak_device_bytes;                         /* the ledger of the library's device buffers, sampled after every stage */
    /* keep_records: */
    int n_chunks; int *chunk_tid; int64_t *chunk_reg_beg, *chunk_reg_end; int *chunk_n_reads, *chunk_n_passes, *chunk_flip_hap, *chunk_n_records;
    int64_t *chunk_flip_pre_PS, *chunk_flip_cur_PS;
    lcd_var1_t *records; int n_kept_records;
} lcd_file_stats_t;
void lcd_file_job_default(lcd_file_job_t *job);     /* zeroes; overlap = -1 */
void lcd_file_stats_free(lcd_file_stats_t *stats);

/* ---- indexes: .bai built on the device, .fai on the host (htslib's sam_index_build / fai_build are not in the checkout; src/call_var_main.c:675-686 builds a
 * missing alignment index and goes on).  The index content, SAM specification 5.2-5.3; any reader that follows it gets correct answers:
 *   1 interval     beg = pos (0-based), end = bam_endpos under the rule above (a record with the unmapped flag, or whose CIGAR consumes no reference, spans one base;
 *                  the CIGAR of a read with more than 65 535 operations comes from its CG tag).
 *   2 no coord.    a record with refid < 0 or pos < 0 is not indexed and counts in n_no_coor.
 *   3 order        indexed records are non-decreasing in (refid, pos) and none follows a no-coordinate record, else LCD_ERR_BAI_ORDER with the record number (0-based,
 *                  counted over all records of the file) in the message; end > 2^29 is LCD_ERR_BAI_CSI ("only BAI is supported, not CSI").  PROJECT RULE, made by the
 *                  device builder only (its window arrays are sized from the header's contig lengths, (len >> 14) + 1 words): a refid outside the header's table, or
 *                  a record that ends behind the last 16 kb window of its contig, is LCD_ERR_BAI_CONTIG; lcd_bai_from_records has no lengths and does not test it.
 *   4 bin          reg2bin(beg, end) of specification 5.3.
 *   5 offsets      (compressed file offset of the member << 16) | offset inside its payload.  PROJECT RULE: a position at the very end of a member's payload is written
 *                  as the immediately following member's start with offset 0 -- an empty member and the EOF member count as following members; if none follows, the
 *                  file size.  A record's begin and the end of the record before it are the same position and get the same offset.
 *   6 chunks       a maximal run of consecutive indexed records with equal (refid, bin) is one chunk [vbeg(first), vend(last)]; inside a bin chunks stay in file order.
 *                  PROJECT RULE: a chunk is merged into the one before it in its bin when prev.vend >> 16 >= next.vbeg >> 16 (no member is inflated twice for one
 *                  bin).  No bins are folded into parents.
 *   7 bins         ascending bin number; for a contig that has records the pseudo-bin 37450 comes last with two chunks: (vbeg of its first record, vend of its last)
 *                  and (n_mapped, n_unmapped); n_unmapped counts records with flag bit 4; n_bin includes the pseudo-bin.
 *   8 linear       windows beg >> 14 .. (end - 1) >> 14 take the smallest vbeg; n_intv = highest set window + 1; an unset window takes the previous window's value,
 *                  an unset window 0 is 0.
 *   9 trailer      a contig without records has n_bin = 0 and n_intv = 0; the trailing uint64 n_no_coor is always written.
 *  10 slabs        the bytes depend on nothing but the file: not on the slab size, the number of slabs, or where a slab border falls.
 * lcd_bai_from_records: the finisher on its own, pure host code -- rules 2-9 applied to a record table (flag bit 4 = unmapped; vbeg / vend as rule 5 gives them).
 * *bytes malloc()'d (free()).  Returns 0 or LCD_ERR_BAI_ORDER / LCD_ERR_BAI_CSI / -4.
 * lcd_bai_builder_*: the accumulating builder.  add_stream takes a stream of whole BAM records that already lies in HBM, from first_record_offset on (the stream
 * must be readable 64 bytes behind n_bytes), with the table of the BGZF members it was inflated from -- per member the inflated start offset inside the stream, the
 * compressed file offset and the payload length -- and end_coff, the file offset behind the last member (rule 5 for a position at the stream's end).  It runs the
 * record walk, the CIGAR statistics, lcd_bai_entry_kernel and lcd_bai_compact_kernel (bai_kernel.hip) and accumulates chunk lists, the per-contig window arrays in HBM
 * (allocated for a contig when its first record arrives) and the counters.  *next_record_offset = the offset of the first record that is not complete inside the
 * stream (== n_bytes when all were).  finish serialises (out_path NULL: nothing is written; the bytes are still available through lcd_bai_builder_bytes).  After an
 * error the builder only accepts destroy.
 * lcd_bai_build: the whole-file driver.  The file is read slab by slab (opt->slab_members BGZF members per slab; 0 = 4096, at most 256 MB inflated), every slab is
 * inflated by lcd_bgzf_inflate_dev and handed to add_stream; the next slab starts at the member that holds the first unfinished record (at most one record's worth
 * of members is inflated twice); a record larger than a slab doubles the slab for that step (a block_size below 32 is refused at once, -33, and the growth ends
 * at one maximal record).  The file is read in pieces of 16 MB; bytes read behind a slab's last member are kept for the next slab.  The BAM header and the reference table are skipped by parsing them.
 * Slabs run one after the other (no two in flight).  On an error nothing is left at out_path and no device buffer stays in the ledger.
 * lcd_fai_build: host code; one NAME\tLENGTH\tOFFSET\tLINEBASES\tLINEWIDTH line per sequence.  The name ends at the first whitespace; \n and \r\n line ends, a last
 * line without a newline, blank lines at the end of the file and a shorter last line per sequence are accepted; a sequence whose other lines differ in length
 * (LCD_ERR_FAI_FORMAT, the sequence's name in the message), a duplicate name, a file that does not start with '>' and a compressed FASTA are refused. */
#define LCD_ERR_BAI_ORDER (-50)
#define LCD_ERR_BAI_CSI (-51)
#define LCD_ERR_FAI_FORMAT (-52)
#define LCD_ERR_BAI_CONTIG (-53)
int lcd_bai_from_records(int n_ref, int64_t n_rec, const int *refid, const int64_t *beg, const int64_t *end, const int *flag, const uint64_t *vbeg, const uint64_t *vend,
                         uint8_t **bytes, size_t *n);
typedef struct lcd_bai_member_t { uint64_t uoff, coff; uint32_t ulen, pad; } lcd_bai_member_t;
typedef struct lcd_bai_builder_s lcd_bai_builder_t;
lcd_bai_builder_t *lcd_bai_builder_create(int n_ref, const int64_t *ref_lens);
int lcd_bai_builder_add_stream(lcd_bai_builder_t *b, uint64_t dev_ptr, size_t n_bytes, size_t first_record_offset, size_t n_members, const lcd_bai_member_t *members,
                               uint64_t end_coff, size_t *next_record_offset);
int lcd_bai_builder_finish(lcd_bai_builder_t *b, const char *out_path);
int lcd_bai_builder_bytes(const lcd_bai_builder_t *b, const uint8_t **bytes, size_t *n);   /* after finish; borrowed */
void lcd_bai_builder_destroy(lcd_bai_builder_t *b);
typedef struct lcd_bai_opt_t { int slab_members, verify_crc; } lcd_bai_opt_t;
typedef struct lcd_bai_stats_t {
    int64_t n_records, n_indexed, n_mapped, n_unmapped, n_no_coor, n_chunks, n_slabs, n_members, bytes_in, bytes_inflated, bytes_index;
    double ms_read, ms_inflate, ms_walk, ms_stat, ms_entry, ms_finish, ms_wall;
} lcd_bai_stats_t;
int lcd_bai_build(const char *bam_path, const char *out_path, const lcd_bai_opt_t *opt /* may be NULL */, lcd_bai_stats_t *stats /* may be NULL */);
int lcd_fai_build(const char *fasta_path, const char *out_path /* NULL: <fasta>.fai */);
/* The outputs with their indexes.  lcd_writer_opt_t.write_index: the writer owns a builder; after each append's tag rewrite and deflate the tagged stream in HBM goes
 * to add_stream with the member table the deflater reports and the writer's running file offset; close writes the index to index_path (NULL: <out.bam>.bai) after
 * the EOF member.  If the output violates rule 3 -- lcd_plan_chunks sorts and merges a contig's regions, so the plan cannot cause it; an input whose records are out
 * of order inside a region can, and so can a caller of lcd_bam_writer_append who hands chunks over out of order -- or names a position outside the header's contigs
 * (LCD_ERR_BAI_ORDER, LCD_ERR_BAI_CSI, LCD_ERR_BAI_CONTIG), the BAM is still completed, no index file is left behind and idx_stats says so: that is not an error of
 * the run.  Any other failure of the index (a malformed record in the writer's own stream, a device error) fails the append.  *idx_stats must outlive the writer.
 * lcd_index_opt_t (lcd_run_opt_t.idx of lcd_call_files; NULL: none of it).  build_missing_bai / build_missing_fai: a missing input index is built at the path the job
 * would have read (bai_path or <bam>.bai, <fasta>.fai) and the run goes on; an unwritable location is -30 with the path in the message; an index that exists is
 * never rebuilt or touched.  write_out_bai needs job->bam_out; out_bai_path NULL = <out.bam>.bai. */
typedef struct lcd_index_opt_t { int build_missing_bai, build_missing_fai, write_out_bai; const char *out_bai_path; int slab_members; } lcd_index_opt_t;
typedef struct lcd_index_stats_t {
    int built_bai, built_fai, wrote_out_bai, out_bai_skipped;      /* out_bai_skipped: the LCD_ERR_* code that kept the output's index from being written, or 0 */
    char out_bai_skip_reason[256];
    int64_t out_bai_bytes, out_n_indexed, out_n_no_coor; double ms_build_bai, ms_build_fai, ms_out_bai;
} lcd_index_stats_t;

/* ---- one sample from several alignment files (longcallD call ref.fa in.bam -X more.bam ... / -L list): src/call_var_main.c:361-400, 640-741 ----
 * The ordinary shape of a PacBio / ONT sample is one BAM per SMRT cell or flow cell.  A chunk is made from a region image (whole BGZF blocks plus ranges of the
 * inflated stream), so several files become ONE chunk by appending their region images in file order: one inflate launch, one record walk launch, and everything
 * behind the chunk (first round, noisy rounds, K5, stitch, records, VCF) runs unchanged on the concatenated reads.  No kernel knows about files.
 *   1 reads        collect_ref_seq_bam_main (src/bam_utils.c:1659-1716): for file 0, then file 1, ... the region iterator's records in file order with the flag / MAPQ
 *                  filter; kept reads are appended, so the chunk's read ids and its record table are file-major and the reference window (meta) spans all files'
 *                  reads.  The loader's stop rules ("a record at or behind reg_end", "records of a later contig") restart at each file, and a walk job ends at its own
 *                  file's segment of the stream.  lcd_sort_chunk_reads' last tie-break, file order, becomes file-major order.
 *   2 stitch       the reference keeps the overlap lists per file and pairs them per file (src/collect_var.c:1640-1660); here one list per chunk is built in chunk
 *                  order, as before.  Both agree whenever the per-file counts of neighbours agree, which holds for sorted files; the total-count check and its
 *                  error stay.
 *   3 headers      tids, the VCF header's contigs and the output BAM's header (plus the @PG line) come from file 0 (:733-741, :1018-1019); the sample name is file
 *                  0's lcd_bam_sample_name, else all input paths joined by ','.  The chunk level looks the contig up by name in every file's header.  PROJECT RULE
 *                  (the reference uses file 0's tids for every file unchecked): lcd_call_files demands of every further file the reference table of file 0 -- same
 *                  names, same lengths, same order -- else LCD_ERR_INPUT_HEADERS with the file and the first differing entry in the message, before any output file
 *                  is created.
 *   4 BAM output   write_read_to_bam (src/bam_utils.c:2009-2048): per chunk the records of file 0, then file 1, ...; each file leaves out what the chunk before has
 *                  written.  The reference counts those per file (n_up_ovlp_reads[i], n_up_ovlp_skip_reads[i]; in a sorted file that file's first ones).  PROJECT
 *                  RULE: per record -- a record, kept or filtered, is left out if and only if it overlaps the previous chunk's region on the same contig
 *                  (is_ovlp_with_prev_region on [pos0 + 1, bam_endpos]); identical for sorted inputs, no prefix assumption.  The merged output is therefore NOT
 *                  coordinate-sorted (the reference says several inputs "will be merged" and no more).
 *   5 sort_output  additive: within each chunk the records to be written are ordered by (pos0, file index, position in the file), stable, before the tag rewrite -- a
 *                  host sort of the job table.  A chunk only writes records that do not overlap its predecessor, so the file is non-decreasing in (refid, pos) and the
 *                  output's .bai can be written.  Without it interleaved inputs make the index builder give up with LCD_ERR_BAI_ORDER: the BAM is completed, no index
 *                  is left, out_bai_skipped says so (the indexing writer's rule, unchanged).
 * lcd_chunk_open_from_bams: lcd_chunk_open_from_bam over n_bams files (1 ... LCD_MAX_INPUTS; bai_paths NULL, or an entry NULL: <bam>.bai); n_bams = 1 is
 * lcd_chunk_open_from_bam.  meta->tid / n_targets / target_len are file 0's.  lcd_chunk_n_files; lcd_chunk_read_files: per kept read its file index (returns n_reads).
 * lcd_merged_record_plan (pure host code): rules 4 and 5 on a record table in file-major order -- skip[i] = 1 for a record left out; order[0 .. m) = the records to
 * write in output order, order[m .. n_rec) = -1; returns m.  rec_file NULL: one file.  has_prev 0: nothing is left out.  -4 for n_rec < 0 or a NULL table.
 * lcd_chunk_tag_records_sel: lcd_chunk_tag_records for the records with skip[i] == 0 (skip NULL: all), in the order `order` names them (as the plan gives it; NULL:
 * table order); an order that does not name every such record exactly once is -4.
 * lcd_writer_opt_t.sort_output: the writer's appends use the plan with sort_output (default 0).  With one sorted input and 0 an append writes the bytes it always wrote.
 * lcd_call_files over in->n files: in->sort_output is the writer's.  job->bam_path / bai_path must be NULL or equal entry 0 (-4).  Every file's
 * .bai is looked for (in->bai_paths NULL, or an entry NULL: <bam>.bai) and, with build_missing_bai, built at its own path; existing ones are never touched; a
 * missing one without the option is -30 with that path.  n_reads_per_file (in->n entries, or NULL): the kept reads each file contributed, summed over the chunks.
 * in == NULL is the job's one file (job->bam_path / bai_path), and in->n == 1 is that run byte for byte.  n < 1, n > LCD_MAX_INPUTS or a NULL path: -4. */
#define LCD_ERR_INPUT_HEADERS (-54)
#define LCD_MAX_INPUTS 64
typedef struct lcd_inputs_t { int n; const char *const *bam_paths; const char *const *bai_paths; int sort_output; } lcd_inputs_t;
lcd_chunk_t *lcd_chunk_open_from_bams(const lcd_digar_opt_t *opt, int n_bams, const char *const *bam_paths, const char *const *bai_paths /* NULL or entries NULL: <bam>.bai */,
                                      const char *chrom, int64_t reg_beg, int64_t reg_end, int min_mapq, int verify_crc, struct lcd_bam_reads_t *meta);
int lcd_chunk_n_files(const lcd_chunk_t *chunk);
int lcd_chunk_read_files(const lcd_chunk_t *chunk, int *file_of_read);
int lcd_merged_record_plan(int n_rec, const int *rec_file, const int64_t *rec_pos0, const int64_t *rec_endpos, int has_prev, int64_t prev_beg, int64_t prev_end,
                           int sort_output, uint8_t *skip, int *order);
lcd_tagged_t *lcd_chunk_tag_records_sel(const lcd_chunk_t *chunk, const int *haps, const int64_t *phase_sets, const uint8_t *skip, const int *order);

/* ---- VCF content: MEI annotation from a TE library (longcallD call -T FILE) and supporting read names (--out-var-rnames / --out-sv-rnames) ----
 * lcd_te_lib_from_fasta == make_te_kmer_idx (src/kmer.c:120-148) with its file reading: every record of a plain or gzip-compressed FASTA file (gzopen / gzread) as
 * kseq_read (src/kseq.h:175-215) yields it -- the name is the header up to the first whitespace, the sequence the letters as they are (any case, any number of
 * lines, \n or \r\n), records in file order: te_seq_i is the record's index -- handed to lcd_te_lib_create.  kmer_len 0 = 15 (src/call_var_main.c:215).  *names:
 * n malloc()'d strings in a malloc()'d array; *seq_lens (the pointer may be NULL): the sequences' lengths, malloc()'d; release everything with
 * lcd_te_lib_from_fasta_free.  A file that cannot be opened or read: -30 with the path in lcd_last_error.  A file without a record is valid (*n_seqs = 0: the
 * library matches nothing, as no library); a record with an empty sequence keeps its index and never matches.
 * lcd_format_vcf_fields == lcd_format_vcf_te plus write_var_to_vcf's ALTREADS (src/vcf_utils.c:205-253).  rnames_mode LCD_RNAMES_NONE: exactly lcd_format_vcf_te;
 * LCD_RNAMES_SV: records with is_sv; LCD_RNAMES_ALL: every record (the reference's `output_var_rnames || (is_sv && output_sv_rnames)`, :208).  A record that
 * qualifies gets ":ALTREADS" behind the FORMAT keys (after the optional ":PS") and, behind the sample's last value, ':' + the names of alt_read_i[0 .. AD[1]) joined
 * by ',' in the order lcd_make_variants stored them (ordered_read_ids order, skipped reads left out), or "." when AD[1] == 0; a two-alt record lists allele 1's
 * reads only, as the reference does.  alt_read_i indexes the reads of the chunk that made the record: name_pool + name_off[r] for r < n_reads are that chunk's names
 * (lcd_bam_reads_t's fields), so records are formatted chunk by chunk.  An index outside [0, n_reads), or AD[1] above n_alt_reads: -4 (nothing is read out of
 * bounds), *text_out NULL.  *n_mei (may be NULL): the lines written that carry MEI.  lcd_alt_read_names: the ALTREADS value of one record, malloc()'d.
 * lcd_vcf_fields_t: the options of the drivers below.  te_fasta_path NULL: no library; te_kmer_len 0 = 15; rnames_mode as above.  The library is read once per
 * call -- before any output file is created: an unreadable file fails the call like the other input checks -- and shared read-only by every window and host
 * thread; lcd_annotate_te gets it and the formatter its names.  With a names mode every chunk's records are formatted against chunks[c].first.meta's names (a chunk
 * without meta->name_off / name_pool: -4), whatever the number of chunks, contigs, windows or input files (several files: the reads, and so the names, are
 * file-major).  `fields` NULL or all zero: the text and every output file are byte-identical to the entry point without it.
 * lcd_vcf_fields_out_t (may be NULL; release with lcd_vcf_fields_out_free): the library's names, the MEI lines written, and -- with a names mode -- per returned /
 * kept record (*records of lcd_chunks_call_fields / lcd_call_bam_regions, stats->records with keep_records) its ALTREADS value, NULL for a record the mode
 * leaves out.  --out-som-var-rnames belongs to somatic mode and is not supported. */
#define LCD_RNAMES_NONE 0
#define LCD_RNAMES_SV 1
#define LCD_RNAMES_ALL 2
typedef struct lcd_vcf_fields_t { const char *te_fasta_path; int te_kmer_len; int rnames_mode; } lcd_vcf_fields_t;
typedef struct lcd_vcf_fields_out_t { int n_te_seqs; char **te_names; int64_t n_mei_lines; int n_rnames; char **rnames; } lcd_vcf_fields_out_t;
int lcd_te_lib_from_fasta(const char *path, int kmer_len, lcd_te_lib_t **lib, char ***names, int **seq_lens, int *n_seqs);
void lcd_te_lib_from_fasta_free(lcd_te_lib_t *lib, char **names, int *seq_lens, int n_seqs);
int lcd_format_vcf_fields(const lcd_call_opt_t *opt, const char *chrom, const lcd_var1_t *vars, int n_vars, const char *const *te_names, int rnames_mode, int n_reads,
                          const uint64_t *name_off, const char *name_pool, char **text_out, int *n_mei);
int lcd_alt_read_names(const lcd_var1_t *var, int n_reads, const uint64_t *name_off, const char *name_pool, char **out);
void lcd_vcf_fields_out_free(lcd_vcf_fields_out_t *out);
/* lcd_chunks_call is lcd_chunks_call_fields with fields == NULL and fields_out == NULL; the file drivers take both through lcd_run_opt_t / lcd_run_out_t */
int lcd_chunks_call_fields(int n_chunks, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, const lcd_vcf_fields_t *fields, lcd_var1_t **records,
                           int *n_records, char **vcf_body, lcd_vcf_fields_out_t *fields_out);

/* ---- refined alignments in the phased output (longcallD call --refine-aln -b): refine_bam1 + update_bam1_tags (src/bam_utils.c:1718-1942) in HBM ----
 * lcd_chunk_refine_records == lcd_chunk_tag_records_sel (same records, same skip / order selection, same handle) where every KEPT record is first rewritten with the
 * alignment of its read's FINAL digar list (bam_refine_kernel.hip, one wavefront per record; no record and no digar of an untouched read crosses PCIe):
 *   digars   read r's list is touched_digars[touched_off[k] .. touched_off[k + 1]) when touched_reads[k] == r (the reads a noisy region rewrote,
 *            lcd_update_digars_from_msa1 applied on the host in the reference's order; uploaded, counted in lcd_copy_counters[1]), else the chunk's own digars in
 *            HBM.  touched_reads names each read at most once; a digar with type outside 0 ... 8 or len < 0, or a list whose lengths reach 2^28 in all, is -4;
 *            qi is taken as it is (the reference's rewrite leaves '=' digars with qi -1): a base outside [0, l_seq) reads as n.
 *   R1 pos   core.pos = digars[0].pos - 1, also when the CIGAR turns out identical.
 *   R2 CIGAR one word per run of digars of equal type, in order (longcalld_push_cigar, :112-121: adjacent equal operations add up; a reference skip the input had
 *            is not in the digars and so not in the result); then a hard clip as the FIRST or LAST word becomes a soft clip (kept reads are never supplementary).
 *   R3       new words == the record's words: nothing else changes, no tag is touched (HP / PS excepted).
 *   R4       otherwise the record is name, new words, then bases, qualities and fields as they were, n_cigar updated, and
 *              NM  only if a first NM field exists and bam_aux2i of it (the project's rule: types c C s S i I give their value, any other type 0) differs from
 *                  the sum of len over X / I / D digars: the field is deleted and NM:i (4 bytes) appended;
 *              MD  only if a first MD field exists, has type Z and its string differs from get_md_from_digar (:1739-1771): deleted, MD:Z appended.  One number per
 *                  X / D digar (the '=' bases since the last X / D digar, "0" included), '^' in front of a deletion's bases, the rest at the end if > 0; an M digar
 *                  counts for nothing, as in the reference;
 *              cs  the same with get_cs_from_digar (:1773-1805): ":len" per '=' digar (so the text depends on how the list is cut), "*" + ref + read base per X base,
 *                  "+" bases, "-" ref bases.
 *            A first MD / cs field of another type than Z is left alone; later fields of a name are never looked at.
 *   R5       HP / PS then follow lcd_chunk_tag_records' rule on the record as it is: appended fields come in the order NM, MD, cs, HP, PS; every field that is not
 *            deleted keeps its place and bytes.
 * Project rules where the reference exits, is undefined, or htslib would decide:
 *   unrefined  a kept record gets HP / PS only -- byte for byte lcd_chunk_tag_records_sel's record -- and is counted under the FIRST reason that holds:
 *              n_no_digars (the read is skipped or has no digar); n_qlen_mismatch (digar2qlen != l_seq: the reference exits; hard-clipped primaries land here; also
 *              a record whose name, CIGAR, bases and qualities do not fit its block_size); n_bad_pos (digars[0].pos < 1: the reference exits); n_too_many_ops (more
 *              than 65 535 words in the result -- htslib would write a CG tag; the input's n_cigar is a 16-bit field); n_cg_cigar (the input's CIGAR lives in a CG
 *              tag: n_cigar == 2, first word <l_seq>S, second word N, a first CG field of type B).
 *   letters    MD letters are upper-case ACGTN and cs letters lower-case acgtn, from the codes 0-4 (the window's codes; seq_nt16_int of the record's 4-bit bases).
 *   window     ref_seq[0] = position ref_beg (1-based), codes 0-4 or letters, ref_end INCLUSIVE as everywhere in this header (get_bam_chunk_reg_ref_seq0 sets
 *              chunk->ref_end = ref_beg + len - 1 in these terms).  The reference's bounds test is `pos >= ref_beg && pos < ref_end` with that same number: a base
 *              ON ref_end -- the window's last base -- reads as N / n, as does every position outside; this is kept.  ref_seq NULL or ref_end < ref_beg: all N.
 *   bin        where pos or the CIGAR changed, bin = reg2bin(pos, pos + reference length of the new CIGAR), one base for a CIGAR without reference bases; else
 *              the record's bin is left as it is.
 *   order      a rewrite can move pos, so the stream may stop being sorted; nothing here sorts (the writer's index rule applies to the output as it is).
 * stats (may be NULL): counts over the records written; n_refined = CIGAR changed (R4), n_identical = R3, n_unrefined = the sum of the five reasons; n_pos_moved
 * counts refined or identical records whose pos changed; n_*_replaced the R4 fields; bytes_*_up what the call uploaded; ms_measure / ms_emit wall clock of the two
 * passes (each includes its copies and one synchronisation).  NULL on failure (lcd_last_error()); a chunk that was not made from a BAM, or opened and not resolved,
 * is -4.  Filtered records lose their first HP / PS as before. */
/* The refine log of a chunk: one entry per (cluster, read) of every noisy region that resolved with n_cons > 0, in the order update_digars_from_aln_str
 * (src/align.c:1745-1756, called at :1803-1806) walks them -- regions in the order the rounds resolve them, clusters 0 .. n_cons - 1, reads in clu_read_ids order.
 * An entry holds what lcd_update_digars_from_msa1 takes: the read, its cover flag and read_reg_beg / read_reg_end for the region (the pass plan's slices, computed
 * on the device), the region's bounds, and the read's ref<->read rows (stage S5, opt.collect_ref_read_aln_str); `pass` is the pass that resolved the region.
 * lcd_chunks_noisy_rounds_log == lcd_chunks_noisy_rounds with a sink per chunk (logs NULL, or an entry NULL: no sink for that chunk; with no sink at all the call IS
 * lcd_chunks_noisy_rounds, which still refuses opt->collect_ref_read_aln_str with -2).  With a sink the driver's batches run with collect_ref_read_aln_str = 1;
 * collect_noisy_vars stays 2: only the ref<->read rows come down beside the variants, every other string stays in HBM.  The chunk's digars in HBM are never
 * changed: a region is resolved at most once, noisy regions are disjoint, and a rewrite replaces digars inside its own region only, so vars / state / done come out
 * as without a sink (tests/test_gpu_refine_log.py compares them).  A call that fails leaves in the log what it had appended up to there.
 * lcd_refine_log_apply (pure host code): the log applied front to back with lcd_update_digars_from_msa1 on a running copy of the digars handed in (lcd_chunk_digars'
 * CSR; qlen[r] = the read's length) -- return code 1 keeps the read's list (counted in *n_rejected), 2 leaves it untouched -- and the FINAL lists of the reads the
 * log names as a CSR for lcd_chunk_refine_records (touched_reads ascending; malloc()'d, free() each).  Entries of one read are applied in log order: the cut of the
 * list decides the cs text.  lcd_refine_log_append copies an entry's rows (the driver's sink; tests); lcd_refine_log_entry's rows point into the log. */
typedef struct lcd_refine_log_s lcd_refine_log_t;
typedef struct lcd_refine_entry_t { int read_id, cover, read_beg, read_end, aln_len, pass; int64_t reg_beg, reg_end; const uint8_t *target, *query; } lcd_refine_entry_t;
lcd_refine_log_t *lcd_refine_log_create(void);
void lcd_refine_log_free(lcd_refine_log_t *log);
int64_t lcd_refine_log_n_entries(const lcd_refine_log_t *log);
int64_t lcd_refine_log_row_bytes(const lcd_refine_log_t *log);   /* the rows' bytes: what crossed PCIe for the log */
int lcd_refine_log_append(lcd_refine_log_t *log, const lcd_refine_entry_t *entry);
int lcd_refine_log_entry(const lcd_refine_log_t *log, int64_t i, lcd_refine_entry_t *out);
int lcd_refine_log_apply(const lcd_refine_log_t *log, int n_reads, const uint64_t *digar_off, const lcd_digar_t *digars, const int *qlen, int *n_touched,
                         int **touched_reads, uint64_t **touched_off, lcd_digar_t **touched_digars, int64_t *n_rejected /* may be NULL */);
int lcd_chunks_noisy_rounds_log(int n_chunks, lcd_rounds_chunk_t *chunks, const lcd_opt_t *opt, const lcd_pass_opt_t *pass_opt, lcd_refine_log_t *const *logs);
/* per row of lcd_batch_region_vars' row_read_ids (cluster 0's reads, then cluster 1's) the read's ref<->read rows of a resolved region, pointing into the batch's
 * download (valid until the batch runs or is cleared again); needs opt.collect_ref_read_aln_str (-5); returns the number of rows, 0 for an unresolved region */
int lcd_batch_region_ref_read_rows(lcd_batch_t *b, int region, int n_rows, int *aln_len, const uint8_t **target, const uint8_t **query);
typedef struct lcd_refine_stats_t {
    int64_t n_records, n_kept, n_refined, n_identical, n_unrefined, n_pos_moved, n_no_digars, n_qlen_mismatch, n_bad_pos, n_too_many_ops, n_cg_cigar;
    int64_t n_nm_replaced, n_md_replaced, n_cs_replaced, n_touched, bytes_digars_up, bytes_ref_up;
    double ms_measure, ms_emit;
    int64_t n_log_entries, bytes_log_down, n_log_rejected;   /* the drivers below: the refine logs of the chunks written (0 from lcd_chunk_refine_records itself) */
} lcd_refine_stats_t;
lcd_tagged_t *lcd_chunk_refine_records(const lcd_chunk_t *chunk, int n_touched, const int *touched_reads, const uint64_t *touched_off /* n_touched + 1 */,
                                       const lcd_digar_t *touched_digars, const uint8_t *ref_seq, int64_t ref_beg, int64_t ref_end, const int *haps,
                                       const int64_t *phase_sets, const uint8_t *skip, const int *order, lcd_refine_stats_t *stats);

/* The drivers with refined alignments (longcallD call --refine-aln -b; here --refine-bam).  A chunk handle carries its own sink: lcd_chunk_set_refine(chunk, 1)
 * gives it an empty refine log (0 takes it away; lcd_chunk_refine_log: the log, owned by the handle).  chunks_call's rounds then write that log
 * (lcd_chunks_noisy_rounds_log), and the alignment writer -- lcd_bam_writer_append / lcd_write_phased -- rewrites such a chunk's records with
 * lcd_chunk_refine_records instead of lcd_chunk_tag_records_sel: lcd_chunk_digars once and only if the log has entries, lcd_refine_log_apply, the touched reads'
 * final lists up, the window = the chunk's first.ref_seq / ref_beg / ref_end.  The VCF, HP and PS of a run are those of the run without it.  A several-file chunk
 * is one chunk with a selection and goes the same way.  A right-cover rewrite can move POS: the output may stop being sorted; the writer then completes without
 * <out.bam>.bai and says why (out_bai_skipped / out_bai_skip_reason), as for any unsorted stream; nothing is sorted here.
 * lcd_chunks_call_refine: lcd_chunk_set_refine on every chunk, then lcd_chunks_call.  lcd_writer_opt_t.refine_stats: the writer's sum of the refined chunks'
 * lcd_refine_stats_t (counters, times, and the logs: n_log_entries, bytes_log_down = the rows that came down, n_log_rejected = entries double_check_digar
 * rejected); NULL: no sum.  lcd_aln_opt_t.refine of the file drivers: every chunk is refined when an alignment output is asked for; without bam_out the option
 * has no effect, as in the reference. */
int lcd_chunk_set_refine(lcd_chunk_t *chunk, int on);
lcd_refine_log_t *lcd_chunk_refine_log(const lcd_chunk_t *chunk);
int lcd_chunks_call_refine(int n_chunks, lcd_call_chunk_t *chunks, const lcd_cfg_t *cfg, const char *chrom, lcd_var1_t **records, int *n_records, char **vcf_body);

/* ---- the alignment output as SAM text (the reference's -S FILE, src/call_var_main.c:961; here --sam FILE): records formatted in HBM (bam_sam_kernel.hip) ----
 * lcd_tagged_to_sam turns a tagged / refined stream where it lies into SAM lines (SAM specification 1.4), one wavefront per record: a measure pass, the host's
 * 64-bit prefix sum over the lines' lengths, an emit pass.  lcd_records_to_sam is the same for host bytes of back-to-back block_size-prefixed records (a stream
 * that ends inside a record, or a block_size below 32: -24).  NULL + lcd_last_error on failure; NULL arguments are refused (-4) before any HIP call.
 * A line is the eleven mandatory fields, one \tXX:T:value per auxiliary field, \n.  htslib's sam_format1 is not in the checkout; where it would decide, the rule
 * is marked PROJECT RULE.
 *   QNAME  the bytes of the name field in front of its first NUL; an empty name prints *.
 *   FLAG, MAPQ, POS = pos + 1, PNEXT = next_pos + 1, TLEN (signed): decimal.
 *   RNAME  * for refID < 0; PROJECT RULE: * for refID >= n_ref (and for a contig whose name is empty); else the contig's name.
 *   RNEXT  * for next_refID < 0 or >= n_ref; = when it equals the record's (valid) refID; else the name.
 *   CIGAR  * for n_cigar == 0; else <len><op> per word, MIDNSHP=XB for op 0-9 and ? above.  PROJECT RULE, a CIGAR that lives in a CG field (lcd_chunk_refine_records'
 *          test: n_cigar == 2, the first word <l_seq>S, the second N, and a first CG field of type B -- here with subtype I, the only one whose elements are
 *          words): the column is the CG array's words (* for an empty array) and that CG field is not printed among the auxiliary fields, as a BAM reader built on
 *          htslib shows the record.
 *   SEQ    * for l_seq == 0; else "=ACMGRSVTWYHKDBN"[nibble].   QUAL  * for l_seq == 0 or a first quality byte of 0xff; else byte + 33 (modulo 256).
 *   PROJECT RULE: a record whose name, CIGAR, bases and qualities do not fit its block_size (or whose l_seq is negative) prints the fields that can be read -- the
 *   name if it fits, else * -- with * for CIGAR / SEQ / QUAL and no auxiliary fields; it is counted in n_bad_layout.  Nothing outside the record is read.
 *   Auxiliary fields in record order, walked as lcd_chunk_read_nm walks them: a field that runs past the record or has an unknown type ends the walk, nothing behind
 *   it is printed, the record is counted in n_walk_stopped.  A: A:<char>; c C s S i I: i:<decimal>; f: f:<%g>; Z / H: the bytes in front of the NUL;
 *   B: B:<sub> then ,<value> per element (count 0: B:<sub> alone; subtype f: %g).
 *   A float prints exactly as glibc's printf("%g", (double)x): csrc/sam_fmt.h, exact on the value, no double arithmetic.
 * lcd_sam_names_create uploads the contigs' names once (n_ref == 0: none).  lcd_sam_stats_t: bytes_records in, bytes_text out; ms_measure includes the length
 * download, ms_download_write is the writer's.
 * lcd_writer_opt_t.format LCD_ALN_SAM gives the same writer object as LCD_ALN_BAM: append runs the same skip / order plan, the same tag / refine rewrite and then
 * lcd_tagged_to_sam instead of the deflate; only text comes down.  block_payload is ignored, ms_deflate stays 0, bytes_file counts text, close writes no EOF member,
 * path "-" is stdout.  sort_output, refine_stats and sam_stats (the sum over the appends; NULL: none) work on it.  The header is the input
 * header's text with trailing NULs dropped, pg_line appended as the BAM writer appends it, a newline at its end; PROJECT RULE: if no line starts with "@SQ\t" and
 * the binary table has contigs, @SQ\tSN:<name>\tLN:<len> lines in table order go straight behind a leading @HD line, or to the front when there is none.
 * lcd_aln_opt_t of lcd_call_files: the alignment output's format and whether its records are refined.  format SAM with idx->write_out_bai: -4; refine together
 * with fields: -2; a SAM output on stdout while the VCF goes to stdout: -4, before any file is created.  The records, the VCF, HP and PS of a run do not depend on
 * the format.  A several-file run uses file 0's header, as the BAM output does. */
typedef struct lcd_sam_names_s lcd_sam_names_t;
typedef struct lcd_sam_text_s lcd_sam_text_t;
typedef struct lcd_sam_stats_t {
    int64_t n_records, bytes_records, bytes_text, n_float_values, n_cg_cigar, n_walk_stopped, n_bad_layout;
    double ms_measure, ms_emit, ms_download_write;
} lcd_sam_stats_t;
lcd_sam_names_t *lcd_sam_names_create(int n_ref, const char *const *names);
void lcd_sam_names_free(lcd_sam_names_t *names);
lcd_sam_text_t *lcd_tagged_to_sam(const lcd_tagged_t *t, const lcd_sam_names_t *names, lcd_sam_stats_t *stats);
lcd_sam_text_t *lcd_records_to_sam(const uint8_t *records, size_t n_bytes, const lcd_sam_names_t *names, lcd_sam_stats_t *stats);
size_t lcd_sam_text_size(const lcd_sam_text_t *h);
uint64_t lcd_sam_text_dev_ptr(const lcd_sam_text_t *h);
int lcd_sam_text_to_host(const lcd_sam_text_t *h, size_t off, size_t n, uint8_t *out);
void lcd_sam_text_free(lcd_sam_text_t *h);
enum { LCD_ALN_BAM = 0, LCD_ALN_SAM = 1 };
typedef struct lcd_aln_opt_t { int format, refine; } lcd_aln_opt_t;

/* ---- VCF indexes: the .tbi / .csi of a BGZF-compressed VCF, built on the device (the tabix and CSI specifications; any reader that follows them gets correct
 * answers).  The input is VCF TEXT in HBM -- what the VCF writer is about to compress, or a slab inflated from an existing .vcf.gz -- with the table of the BGZF
 * members it lies in (lcd_bai_member_t) and end_coff, exactly as lcd_bai_builder_add_stream takes them.  vcf_index_kernel.hip finds the line starts (ballots over
 * bytes, per-workgroup counts, exclusive scan, compaction), parses every line with one wavefront (lanes striding 64 bytes) and then does for a line what
 * lcd_bai_entry_kernel does for a record.
 *   1 lines        a line ends at '\n'.  A line whose first byte is '#' is a meta line: counted, not indexed.  Every other line is a data line; data lines are numbered
 *                  from 0 over the whole file, and that number is in every message about a line.
 *   2 columns      a data line has at least 8 tab-separated columns (column 8 may end at the line end), a non-empty CHROM and a POS of decimal digits only, else
 *                  LCD_ERR_VCF_LINE.  PROJECT RULE: an empty line is a data line with too few columns.
 *   3 interval     beg = POS - 1 (POS 0: 0), end = beg + length of REF (PROJECT RULE: an empty REF spans one base).  END: if INFO begins with "END=", that value; else the
 *                  value behind the first ";END=" inside INFO (so CIEND= / SVEND= never match); a value that begins with '.' is ignored, and so is one that does not
 *                  begin with a decimal digit (PROJECT RULE: decimal digits only, where htslib's strtoll would also take a sign or a 0x prefix); if END > beg then
 *                  end = END, else it is ignored.  Only the first of the two keys decides: "END=.;...;END=5000" has no END.
 *   4 contigs      tids are given in order of first appearance; the lines of a contig are consecutive: a name that reappears after another contig is
 *                  LCD_ERR_VIDX_ORDER.  Inside a contig beg is non-decreasing, else LCD_ERR_VIDX_ORDER.  Of several refused lines the one with the smallest number is reported.
 *   5 offsets      rule 5 of the .bai section; a line's vbeg is its first byte's offset, its vend the offset of the byte behind its '\n' (the next line's vbeg).  A last
 *                  line without '\n' ends at the end of the file's last payload.
 *   6 bins         min_shift 14; TBI: depth 5, reg2bin of SAM specification 5.3, end > 2^29 is LCD_ERR_VIDX_CSI with a message that asks for CSI.  CSI: depth = max(5,
 *                  the smallest d with 2^(14 + 3d) >= the longest length of the header's contig lines); a contig line is a meta line that begins with "##contig=<" and has
 *                  "length=" directly behind a '<' or a ','.  With no such line the depth comes from the largest end seen.  An end behind 2^(14 + 3 depth) of a depth taken
 *                  from the header, or behind 2^38 (depth 8, the deepest this library writes), is LCD_ERR_VIDX_CSI.
 *   7 chunks       rules 6-7 of the .bai section: runs of equal (tid, bin), the merge rule, ascending bins, the pseudo-bin -- 37450 for TBI,
 *                  ((1 << (3 depth + 3)) - 1) / 7 + 1 for CSI -- last with (vbeg of the contig's first line, vend of its last) and (number of lines, 0).
 *   8 TBI          "TBI\1", n_ref, format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, the NUL-terminated names in tid order, per contig the bins and the
 *                  linear index of .bai rule 8, the trailing uint64 n_no_coor = 0.
 *   9 CSI          "CSI\1", min_shift 14, depth, l_aux, aux = the TBI header from format through the names, n_ref, per contig the bins, each with loffset in front of
 *                  n_chunk (the pseudo-bin's is 0), no linear index, the trailing n_no_coor = 0.  PROJECT RULE: a bin's loffset is the smallest vbeg of the contig's
 *                  lines that overlap the bin's interval; as beg never decreases inside a contig that is the value of the first set 16 kb window inside the bin's span.
 *                  Why a reader may use it: htslib's lookup for a region starts at the leaf bin of the region's first base and, while the bin it looks at is
 *                  absent from the index, goes to the bin on its left among its siblings or else to its parent; it takes the loffset of the first bin it finds
 *                  (0 if none) and skips every chunk that ends at or in front of it.  The bin B it finds is an ancestor of that leaf (or the leaf) or lies
 *                  wholly in front of it, so B ends behind the region's first base or in front of it -- never does B begin behind it.  Let W be a line that
 *                  overlaps the region: W ends behind the region's first base.  If W begins in front of B's end, W overlaps B's interval (it ends behind B's
 *                  begin), so loffset(B) <= vbeg(W) by the rule.  If W begins at or behind B's end: B is present, so a line lies inside B; that line begins in
 *                  front of W, file order is position order inside a contig, and it overlaps B: loffset(B) <= its vbeg <= vbeg(W).  The chunk that holds W ends
 *                  behind vbeg(W) and is kept.
 *  10 slabs        the bytes depend on nothing but the file: not on the slab size, not on where a slab or an append border falls.
 * lcd_tbx_from_records: the finisher on its own, pure host code -- rules 4 and 6-9 on a table of (tid, beg, end, vbeg, vend) with the names in tid order (tids never
 * decrease) and the header's longest contig length (0: none).  *bytes = the UNCOMPRESSED index, malloc()'d.  0, LCD_ERR_VIDX_ORDER, LCD_ERR_VIDX_CSI or -4.
 * lcd_vcf_index_builder_*: the accumulating builder, as lcd_bai_builder_*.  add_stream: the stream may begin inside a line; first_line_offset is where its first line
 * starts, *next_line_offset the offset of the first line that is not complete inside the stream (n_bytes when all were).  The stream must be readable 64 bytes behind
 * n_bytes.  Only the names of contig-run heads come to the host.  finish serialises, compresses the bytes with lcd_bgzf_deflate_dev(add_eof = 1) -- a .tbi / .csi is
 * itself BGZF -- and writes them to out_path (NULL: nothing is written); _bytes gives the uncompressed bytes.  After an error the builder only accepts destroy.
 * lcd_vcf_index_build: the whole-file driver, as lcd_bai_build (opt->slab_members members per slab, 0 = 4096; the next slab starts at the member that holds the first
 * unfinished line; a line larger than a slab doubles the slab for that step).  out_path NULL: <path>.tbi or <path>.csi by opt->format; opt NULL: TBI.  A last line
 * without '\n' is accepted.  A file that is not BGZF is refused with -33 and a message that says whether it is plain gzip or plain text.  On an error nothing is left at
 * out_path and no device buffer stays in the ledger.
 * lcd_vcf_writer_open_idx: lcd_vcf_writer_open with an index (vi NULL: without).  It needs bgzf = 1 and a real path (-4 otherwise).  Every append uploads its text
 * once, compresses it with lcd_bgzf_deflate_dev_ptr and hands the same buffer to the builder with the member table of lcd_deflated_block_info and the running file
 * offset; close writes the index to vi->index_path (NULL: <path>.tbi / .csi) after the EOF member, abort leaves none.  LCD_ERR_VIDX_ORDER / LCD_ERR_VIDX_CSI: the VCF
 * is still completed, no index is left behind, vi->stats->skipped / skip_reason say so; any other failure of the index fails the append.  *vi->stats (may be NULL)
 * must outlive the writer; it is zeroed at open.  The .vcf.gz bytes are those of lcd_vcf_writer_open. */
#define LCD_ERR_VIDX_ORDER (-55)
#define LCD_ERR_VIDX_CSI (-56)
#define LCD_ERR_VCF_LINE (-57)
enum { LCD_VIDX_TBI = 0, LCD_VIDX_CSI = 1 };
typedef struct lcd_vcf_index_stats_t {
    int64_t n_lines, n_data_lines, n_meta_lines, n_contigs, n_chunks, n_slabs, n_members, bytes_in, bytes_inflated, bytes_index, bytes_file;
    int depth, wrote, skipped, pad;        /* skipped: the LCD_ERR_* code that kept the writer's index from being written, or 0 */
    char skip_reason[256];
    double ms_read, ms_inflate, ms_lines, ms_entry, ms_finish, ms_wall;
} lcd_vcf_index_stats_t;
typedef struct lcd_vcf_index_opt_t { int format; const char *index_path; int slab_members, verify_crc; lcd_vcf_index_stats_t *stats; } lcd_vcf_index_opt_t;
int lcd_tbx_from_records(int format, int n_ref, const char *const *names, int64_t max_contig_len, int64_t n_rec, const int *tid, const int64_t *beg, const int64_t *end,
                         const uint64_t *vbeg, const uint64_t *vend, uint8_t **bytes, size_t *n);
typedef struct lcd_vcf_index_builder_s lcd_vcf_index_builder_t;
lcd_vcf_index_builder_t *lcd_vcf_index_builder_create(int format);
int lcd_vcf_index_builder_add_stream(lcd_vcf_index_builder_t *b, uint64_t dev_ptr, size_t n_bytes, size_t first_line_offset, size_t n_members, const lcd_bai_member_t *members,
                                     uint64_t end_coff, size_t *next_line_offset);
int lcd_vcf_index_builder_finish(lcd_vcf_index_builder_t *b, const char *out_path);
int lcd_vcf_index_builder_bytes(const lcd_vcf_index_builder_t *b, const uint8_t **bytes, size_t *n);   /* after finish; borrowed */
void lcd_vcf_index_builder_destroy(lcd_vcf_index_builder_t *b);
int lcd_vcf_index_build(const char *vcf_gz_path, const char *out_path, const lcd_vcf_index_opt_t *opt /* may be NULL */, lcd_vcf_index_stats_t *stats /* may be NULL */);
lcd_vcf_writer_t *lcd_vcf_writer_open_idx(const char *path, int bgzf, const char *header_text, const lcd_vcf_index_opt_t *vi);

/* ---- the four drivers and their options ----
 * Every optional feature of the sections above is a member of one of three structs; a NULL struct or a NULL / zero member means the feature is off, and a run
 * without options writes the bytes it always wrote.
 * lcd_run_opt_t (in): idx = the indexes (lcd_index_opt_t), fields = the VCF content (lcd_vcf_fields_t), aln = the alignment output's format and refinement
 * (lcd_aln_opt_t).  aln->format outside LCD_ALN_BAM / LCD_ALN_SAM: -4; aln->refine together with fields: -2.
 * lcd_run_ext_t (lcd_call_files_ext): the options that came after lcd_run_opt_t / lcd_run_out_t were laid out -- those two structs keep their size, so a caller
 * compiled against them goes on working; a NULL struct or member is off.  vcf_idx = the index of the compressed VCF (lcd_vcf_index_opt_t; its `stats` member is not
 * read: vcf_idx_stats, zeroed on entry, is where the run reports).  It needs job->vcf_bgzf and a vcf_path that names a file (-4, before any output is created); a VCF
 * that cannot be indexed (LCD_ERR_VIDX_ORDER, LCD_ERR_VIDX_CSI) is completed without an index and vcf_idx_stats->skipped / skip_reason say so.
 * lcd_call_files_ext(in, job, cfg, opt, stats, out, ext): lcd_call_files with those options; lcd_call_files is ext == NULL.
 * lcd_run_out_t (out): what the run reports beside *stats; NULL: not reported.  Every non-NULL member is zeroed on entry, on refusal paths too
 * (n_reads_per_file: in->n entries, 1 without `in`, zeroed once the inputs are accepted).  refine_stats / sam_stats are the writer's sums and stay zero when
 * the run does not refine / does not write SAM.
 * lcd_writer_opt_t: format (LCD_ALN_BAM / LCD_ALN_SAM, else -4), sort_output, write_index with index_path (NULL: <out>.bai) and idx_stats (not zeroed by the
 * writer: a run may have counted the input indexes it built there), refine_stats and sam_stats (zeroed at open, summed over the appends).  SAM with write_index: -4.
 * Everything named here must outlive the writer.
 * lcd_call_files(in, job, cfg, opt, stats, out): the whole-file run.  in == NULL: the one file job->bam_path / bai_path; neither `in` nor job->bam_path: -4.
 * Refusals come before an index is built or an output file is created.
 * lcd_call_bam_regions(..., bam_out, opt, out): the regions of one contig; bam_out NULL: no alignment output.  opt->fields, opt->aln->refine (with bam_out) and
 * out->fields_out / refine_stats as above.  This driver writes BAM only and builds no index: aln->format LCD_ALN_SAM is -2 and a non-NULL opt->idx is -4; it returns
 * its VCF body as text and writes no file, so there is no VCF index here (it takes no lcd_run_ext_t);
 * out->n_reads_per_file is not written.
 * lcd_bam_writer_open(in_bam_path, out, wopt): the appendable writer (lcd_bam_writer_append / _close / _abort above).  The index path is removed at open and by abort.
 * lcd_write_phased(in_bam_path, n_chunks, chunks, out, wopt): open + one append + close; the chunks are checked before the output is touched. */
typedef struct lcd_run_opt_t { const lcd_index_opt_t *idx; const lcd_vcf_fields_t *fields; const lcd_aln_opt_t *aln; } lcd_run_opt_t;
typedef struct lcd_run_out_t {
    lcd_index_stats_t *idx_stats; int64_t *n_reads_per_file; lcd_vcf_fields_out_t *fields_out; lcd_refine_stats_t *refine_stats; lcd_sam_stats_t *sam_stats;
} lcd_run_out_t;
typedef struct lcd_run_ext_t { const lcd_vcf_index_opt_t *vcf_idx; lcd_vcf_index_stats_t *vcf_idx_stats; } lcd_run_ext_t;
typedef struct lcd_writer_opt_t {
    int format, sort_output, write_index; const char *index_path; lcd_index_stats_t *idx_stats; lcd_refine_stats_t *refine_stats; lcd_sam_stats_t *sam_stats;
} lcd_writer_opt_t;
int lcd_call_files(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out);
int lcd_call_files_ext(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                       const lcd_run_ext_t *ext);
int lcd_call_bam_regions(const char *bam_path, const char *bai_path, const char *fasta_path, const char *chrom, int n_regions, const int64_t *reg_beg,
                         const int64_t *reg_end, int min_mapq, const lcd_cfg_t *cfg, lcd_call_chunk_t *chunks, lcd_var1_t **records, int *n_records, char **vcf_body,
                         lcd_bam_out_t *bam_out, const lcd_run_opt_t *opt, const lcd_run_out_t *out);
lcd_bam_writer_t *lcd_bam_writer_open(const char *in_bam_path, lcd_bam_out_t *out, const lcd_writer_opt_t *wopt);
int lcd_write_phased(const char *in_bam_path, int n_chunks, const lcd_call_chunk_t *chunks, lcd_bam_out_t *out, const lcd_writer_opt_t *wopt);

/* ---- the per-haplotype CpG methylation table of a chunk, from the MM / ML tags of its records (mods_kernel.hip) ----
 * The reference parses -m / --methylation and reads no tag; these are PROJECT RULES, restated in Python in tests/mods_common.py.  Positions are 1-based, as the
 * chunk's region [reg_beg, reg_end] and the window [ref_beg, ref_end] are.
 *   tags     MM: the first MM:Z, else the first Mm:Z.  ML: the first ML:B:C, else the first Ml:B:C.  MN: the first MN of an integer type.  The fields are hopped as
 *            lcd_chunk_tag_records hops them: a field that runs past the record ends the walk.
 *   MM       groups `B S codes [flag] (,delta)* ;` -- B one of ACGTUN, S + or -, codes lower-case letters (one modification each) or one decimal ChEBI id (one
 *            code), flag . or ? or none, a delta of 1 ... 10 digits.  Anything else is a syntax error; the empty text has no groups.  Delta d skips d occurrences of
 *            B in the read AS SEQUENCED; for a record with flag 0x10 those are the stored complements counted from the end of SEQ.  Only the exact 4-bit codes
 *            A C G T match.  ML holds one byte per (called occurrence, code), group after group, the codes of one occurrence side by side.
 *   wanted   the first group with B == C, S == +, and a letter list that holds opt->code; every group in front of it only moves the ML cursor.
 *   class    v = the wanted code's byte, s = the sum of the occurrence's bytes: mod if v >= threshold, else canon if 255 - min(s, 255) >= threshold, else
 *            filtered.  An occurrence the group does not list is canon under flag . or none and is not looked at under ?.
 *   record   a kept record (the loader's flag / MAPQ filter; n_records) falls into the first of: n_no_mm (no MM), n_hard_clip (an H op), n_mn_mismatch (MN differs
 *            from l_seq), n_syntax (anywhere in the text), n_no_group (no wanted group), n_overrun (a called ordinal at or behind the number of occurrences),
 *            n_ml_short (ML has fewer bytes than the groups up to and including the wanted one need; no ML: none) -- and then adds nothing.
 *   call     every other record's occurrences go, each, into the first of: n_unaligned (not in an M / = / X op), n_outside (p outside the region), n_off_context
 *            (no CpG site of the record's strand at p: '+' is C at p with G at p + 1 and takes records without 0x10, '-' is G at p with C at p - 1 and takes records
 *            with it; window codes 0-4, N and positions outside the window match nothing), else n_counted and the site's counter [3 * haps[read] + class].
 * A chunk counts a site of its region for ALL its kept records.  Planned regions are disjoint and a chunk holds every record that overlaps its region, so a run
 * counts every (record, site) pair once without the writer's skip plan.
 * rows: the sites with a counter above zero, by position.  combine_strands: a row's key is the position of the CpG's C (p of a '+' site, p - 1 of a '-' site),
 * its strand '.', and the chunk adds up what IT counted under the key; a CpG cut by the region's end gives one row in each of the two chunks, both with the key
 * reg_end, and whoever joins tables of several chunks adds rows of equal key.
 * lcd_chunk_mod_pileup: one site-map launch, one scan, one pile-up launch (a wavefront per kept record) and one compaction; only rows and statistics come down.
 * opt->ref_seq: the window as letters or codes 0-4, uploaded once per call.  -4: a chunk not made from a BAM or not resolved, a code outside m / h, a threshold
 * outside 128 ... 255, no window, a hap outside 0 ... 2.  lcd_mods_rows_to_host: pos[n], strand[n] ('+' '-' '.'), counts[9 n] (hap-major: mod, canon, filtered).
 * lcd_mods_format (host only, no device): the rows as text lines `chrom start end code strand n_all mod_all n_h1 mod_h1 n_h2 mod_h2 n_filtered` (tabs; start =
 * pos - 1, end = pos, or pos + 1 for '.'; n_* = mod + canon; integers only), behind the '#' header line when with_header; *text is malloc()'d. */
typedef struct lcd_mods_opt_t { int code /* 'm' or 'h' */, threshold, combine_strands, reserved; const char *ref_seq; int64_t ref_beg, ref_end; } lcd_mods_opt_t;
typedef struct lcd_mods_stats_t {
    int64_t n_records, n_no_mm, n_no_group, n_hard_clip, n_mn_mismatch, n_syntax, n_overrun, n_ml_short, n_unaligned, n_outside, n_off_context, n_counted;
    int64_t n_sites, n_rows;
    double ms_site_map, ms_pileup, ms_compact;
} lcd_mods_stats_t;
typedef struct lcd_mods_s lcd_mods_t;
void lcd_mods_opt_default(lcd_mods_opt_t *opt);
int lcd_mods_opt_check(const lcd_mods_opt_t *opt);                       /* 0, or -4 (host only) */
lcd_mods_t *lcd_chunk_mod_pileup(const lcd_chunk_t *chunk, const int *haps, const lcd_mods_opt_t *opt, lcd_mods_stats_t *stats);
int lcd_mods_n_rows(const lcd_mods_t *m);
int lcd_mods_rows_to_host(const lcd_mods_t *m, int64_t *pos, char *strand, uint32_t *counts);
void lcd_mods_free(lcd_mods_t *m);
/* host only: rows by position and strand -> combined rows in place (keys as above); returns their number, -4 for a NULL array or a strand outside + - */
int lcd_mods_combine_rows(int n_rows, int64_t *pos, char *strand, uint32_t *counts);
int lcd_mods_format(int n_rows, const int64_t *pos, const char *strand, const uint32_t *counts, const char *chrom, int code, int with_header, char **text);
/* ---- the per-haplotype depth track of a chunk, from the CIGARs of its kept records (depth_kernel.hip) ----
 * The reference has no such output; these are PROJECT RULES, restated in Python in tests/depth_common.py.  Positions are 1-based, as reg_beg / reg_end are.
 *   record     a kept record of the chunk: the set lcd_chunk_mod_pileup walks (the loader's flag / MAPQ filter).  Its haplotype is haps[read]: 0, 1 or 2.
 *   operations the record's own CIGAR, or those of its CG:B,I field by the rule of the loader (a placeholder `<l_seq>S<n>N` and a first CG field of subtype I / i
 *              with at least n_cigar and fewer than 2^29 entries; one wording for both: lcd_aux::cg_ops, csrc/bam_aux_hop.h).  n_cg counts the latter; a record
 *              with 0 operations, or whose fields run past its end, counts in n_no_cigar and adds nothing.
 *   cover      M, = and X cover their reference span; D covers it unless skip_dels; N never does; I, S, H, P and every other code consume no reference; an
 *              operation of length 0 does nothing.  Reference offsets are 64-bit: spans that sum past 2^31 are clipped, never wrapped.
 *   intervals  the record's covered positions inside [reg_beg, reg_end], joined where they touch: what lies between two covering operations and consumes no
 *              reference (I, S, P, a zero-length op; and D without skip_dels, which covers) does not break an interval.  A typical HiFi read is ONE interval.
 *              n_intervals counts them; a record with operations and no interval counts in n_no_overlap.
 *   depth      depth[h][p] = the kept records of haplotype h with p in an interval; bases[h] = its sum over the region.
 *   rows       the maximal runs of equal (depth[0], depth[1], depth[2]) in position order: they tile [reg_beg, reg_end], zero runs included; a chunk without
 *              records gives one zero row.  n_rows counts them.
 *   windows    (host rule, lcd_depth_windows) window k of width W is [kW + 1, (k + 1)W] on the contig; the rows are cut at the window bounds and every window
 *              that meets the rows gives one row: beg / end = the window cut to the rows' span, and per haplotype the 64-bit sum of depth x positions.
 *   source     the track describes the records AS STORED in the input: refined alignments (lcd_aln_opt_t.refine, --refine-bam) do not change it.
 * lcd_chunk_depth: one launch with a wavefront per kept record that adds +1 / -1 per interval to a three-plane difference array (32-bit integer atomics), then
 * three launches that turn it into rows without a depth array and without one workgroup waiting for another (tile partials; their scan; the rows).  Only rows and
 * statistics come down; `window` is not read here.  -4: a chunk not made from a BAM or not resolved, NULL haps with reads, a hap outside 0 ... 2, a region that
 * is empty or longer than 2^31 - 1024.  lcd_depth_rows_to_host: beg[n], end[n], depth[3 n] (h0 h1 h2 per row).  lcd_depth_tile: the positions per workgroup of
 * the row launches (host only; for tests that straddle it).
 * lcd_depth_windows (host only): rows that tile a span, in order -> the windows' rows; returns their number m and malloc()'d wbeg[m], wend[m], wsum[3 m]; -4 for
 * window < 1, NULL arrays, or rows that are not in order and contiguous; -11 without memory.
 * lcd_depth_format (host only): text lines `chrom start end all h1 h2 unassigned` (tabs; start = beg - 1, end = end: BED; all = h0 + h1 + h2, unassigned = h0;
 * integers only), from depth -- or from wsum when it is not NULL -- behind `#chrom start end depth_all depth_h1 depth_h2 depth_unassigned` (with wsum: bases_*)
 * when with_header; *text is malloc()'d. */
typedef struct lcd_depth_opt_t { int skip_dels, window, reserved[2]; } lcd_depth_opt_t;
typedef struct lcd_depth_stats_t {
    int64_t n_records, n_no_cigar, n_cg, n_no_overlap, n_intervals, bases[3], n_rows;
    double ms_mark, ms_rows;
} lcd_depth_stats_t;
typedef struct lcd_depth_s lcd_depth_t;
void lcd_depth_opt_default(lcd_depth_opt_t *opt);
int lcd_depth_opt_check(const lcd_depth_opt_t *opt);                     /* 0, or -4: window outside 0 ... 2^30 (host only) */
lcd_depth_t *lcd_chunk_depth(const lcd_chunk_t *chunk, const int *haps, const lcd_depth_opt_t *opt, lcd_depth_stats_t *stats);
int lcd_depth_n_rows(const lcd_depth_t *d);
int lcd_depth_rows_to_host(const lcd_depth_t *d, int64_t *beg, int64_t *end, uint32_t *depth);
void lcd_depth_free(lcd_depth_t *d);
int lcd_depth_tile(void);
int lcd_depth_windows(int n_rows, const int64_t *beg, const int64_t *end, const uint32_t *depth, int window, int64_t **wbeg, int64_t **wend, uint64_t **wsum);
int lcd_depth_format(int n_rows, const int64_t *beg, const int64_t *end, const uint32_t *depth, const uint64_t *wsum, const char *chrom, int with_header, char **text);
/* The track of a whole run: lcd_run_ext2_t.depth_path != NULL (below).  At the writer stage, chunk by chunk in plan order, every chunk's lcd_chunk_depth with its
 * final haplotypes; with depth_window = W > 0 its rows go through lcd_depth_windows.  The writer always holds a chunk's last row back: per base it and the next
 * chunk's first row become one row when the contig is equal, held.end + 1 == next.beg and the three depths are equal; window rows are added into one when the
 * contig and the window index are equal and held.end + 1 == next.beg; otherwise the held row is written as it is.  A track without rows still gets its header
 * line.  It works with or without an alignment output and beside mods_path.  Refused with -4 before any file is created: an empty path or "-", a window outside
 * 0 ... 2^30, depth_path equal to mods_path.  The file is removed when the run fails.  *depth_stats: the sums over the chunks (n_rows: the data lines
 * written), filled only by a run that succeeds. */
/* The table of a whole run: lcd_call_files_ext2 == lcd_call_files_ext with one more struct, lcd_run_ext2_t, whose FIRST member is its own size (sizeof as the
 * caller compiled it): members behind `size` bytes read as zero, so the struct can grow without another export; a size that does not reach `mods_path` is -4.
 * lcd_call_files_ext is the call with ext2 == NULL.  mods_path != NULL: at the writer stage, window by window and chunk by chunk in plan order, every chunk's
 * lcd_chunk_mod_pileup with its final haplotypes (the array the tag writer gets) and the window the chunk was resolved with; the rows go to mods_path as
 * lcd_mods_format writes them (the header line once), with or without an alignment output.  With mods_combine_strands the last row of a chunk is held back until
 * the next chunk's first row is known and added to it when their keys and contigs are equal.  mods_code 0: 'm'; mods_threshold 0: 204.  Refused with -4 before
 * any file is created: a code outside m / h, a threshold outside 128 ... 255, an empty path or "-".  The file is created after the refusals and removed when the
 * run fails -- at any stage, the close of the other outputs included; the table is finished last.  *mods_stats: the sums over the chunks (n_rows: the data lines
 * written), filled only by a run that succeeds. */
/* ---- the per-haplotype read sets of a chunk: FASTQ entries and the haplotag list, written on the device from the records where they lie (split_kernel.hip) ----
 * The reference has no such output; these are PROJECT RULES, restated in Python in tests/split_common.py.
 *   selection   the records of the chunk's table that `skip` / `order` name (the meaning they have for lcd_chunk_tag_records_sel; NULL: all, in table order), in
 *               that order: n_records.  A run hands in the plan of the alignment writer (lcd_merged_record_plan: rule 4's per-record overlap with the region
 *               before, rule 5's order under sort_output) whether or not an alignment output is written.  Of those, a record that carries 0x100 or 0x800 is
 *               left out (n_not_primary): every primary record a run visits appears exactly once in the run, in the order of the output BAM.
 *   layout      a primary record with l_seq < 0, or whose name, CIGAR words, packed bases and qualities (36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 +
 *               l_seq bytes) do not fit 4 + block_size or the table's entry, is left out of both outputs (n_bad_layout); nothing outside a record is read.
 *               What is left is selected: n_selected = n_hap[0] + n_hap[1] + n_hap[2].
 *   haplotype   a kept record of read r has haps[r] (0: none, 1, 2) and phase_sets[r] (NULL: 0), the arrays the tag writer gets; a record the loader filtered
 *               (low MAPQ, unmapped with a position) has 0 and 0 (n_filtered_primary counts the selected ones).  The record's stream is its haplotype.
 *   FASTQ entry `@` QNAME [comment] `\n` SEQ `\n+\n` QUAL `\n`.  QNAME: the bytes in front of the first NUL of the name, `*` when there are none.  SEQ:
 *               "=ACMGRSVTWYHKDBN"[nibble].  QUAL: min(byte, 93) + 33; a first quality byte of 0xff prints `!` at every position.  With flag 0x10 the entry is the
 *               read as sequenced (n_reverse): SEQ reversed and complemented through "=TGKCYSBAWRDMHVN", QUAL reversed.  The bases are the record's as stored
 *               (refined alignments change none).  comment (opt.comment): `\tHP:i:<h>` when h != 0, then `\tPS:i:<ps>` when ps > 0, the 64-bit value in decimal.
 *               A selected record with l_seq == 0 has no entry (n_no_seq) and keeps its line in the list.
 *   list line   (opt.list) QNAME `\t` H1 | H2 | none `\t` <ps> in decimal when ps > 0, else none `\t` chromosome `\n`; chromosome by the RNAME rule of the SAM
 *               output: `*` for a refID < 0, a refID >= n_ref or an empty name.  The header line `#readname haplotype phaseset chromosome` (tabs) is the file
 *               writer's, not the chunk call's.
 * lcd_chunk_split_reads: one wavefront per record in two launches, as lcd_tagged_to_sam: the measure pass gives one row per record (stream, the entry's and the
 * line's exact length, flag bits), lcd_split_offsets makes the four 64-bit exclusive prefix sums on the host, the emit pass writes into four device buffers
 * (stream 0 none, 1, 2: FASTQ; 3: the list).  A reverse record is walked from its far end: every step's loads and stores are contiguous across the wavefront.
 * Only the rows and the statistics come down; lcd_split_to_host copies a range of a stream, lcd_split_dev_ptr hands it to lcd_bgzf_deflate_dev_ptr.  NULL with
 * -4 before any HIP call: a NULL chunk or options, a chunk not made from a BAM or not resolved, NULL haps with reads, a hap outside 0 ... 2, list without names.
 * Host only (lcd_split_format.cpp): lcd_split_opt_check (0 / -4); lcd_split_paths: prefix + gz -> the malloc()'d paths PREFIX.none|h1|h2.fastq[.gz] in stream
 * order, -4 for an empty prefix or "-", or when two of them and the n_other paths are equal (NULL, empty and "-" entries name no file and are skipped; a NULL
 * prefix compares the others alone);
 * lcd_split_offsets: n rows' stream (-1 ... 2), fq_len and list_len -> fq_off[i] inside the record's stream, list_off[i], totals[4] (streams 0 1 2, the list);
 * a row with stream -1 adds nothing; -4 for a NULL array or a stream outside -1 ... 2.
 * The read sets of a whole run: lcd_run_ext2_split_t.split_prefix / haplotag_path (below).  At the writer stage, chunk by chunk in plan order, with the plan the
 * alignment writer uses for the chunk; split_gz: every append goes through the BGZF deflate in HBM and the EOF member is written at close.  A stream without
 * records still leaves its file.  Refused with -4 before any file is created: split_gz / split_comment without split_prefix, an empty prefix, "-", or one of the
 * four paths equal to another output of the run (VCF, alignment output, mods, depth, each other).  The files are removed when the run fails; *split_stats: the
 * sums over the chunks, filled only by a run that succeeds. */
typedef struct lcd_split_opt_t { int comment, list, reserved[2]; } lcd_split_opt_t;
typedef struct lcd_split_stats_t {
    int64_t n_records, n_selected, n_hap[3], n_not_primary, n_filtered_primary, n_reverse, n_no_seq, n_bad_layout, bytes_fastq[3], bytes_list;
    double ms_measure, ms_emit, ms_deflate, ms_download_write;
} lcd_split_stats_t;
typedef struct lcd_split_s lcd_split_t;
void lcd_split_opt_default(lcd_split_opt_t *opt);
int lcd_split_opt_check(const lcd_split_opt_t *opt);
int lcd_split_paths(const char *prefix, int gz, int n_other, const char *const *other, char *paths[3]);
int lcd_split_offsets(int n, const int *stream, const uint64_t *fq_len, const uint64_t *list_len, uint64_t *fq_off, uint64_t *list_off, uint64_t totals[4]);
lcd_split_t *lcd_chunk_split_reads(const lcd_chunk_t *chunk, const int *haps, const int64_t *phase_sets, const uint8_t *skip, const int *order,
                                   const lcd_sam_names_t *names /* list only; may be NULL when opt->list == 0 */, const lcd_split_opt_t *opt, lcd_split_stats_t *stats);
size_t lcd_split_size(const lcd_split_t *s, int stream /* 0 none, 1, 2, 3 = list */);
uint64_t lcd_split_dev_ptr(const lcd_split_t *s, int stream);
int lcd_split_to_host(const lcd_split_t *s, int stream, size_t off, size_t n, uint8_t *out);
void lcd_split_free(lcd_split_t *s);
typedef struct lcd_run_ext2_t {
    size_t size;
    const char *mods_path; int mods_code, mods_threshold, mods_combine_strands, reserved; lcd_mods_stats_t *mods_stats;
    const char *depth_path; int depth_window, depth_skip_dels; lcd_depth_stats_t *depth_stats;      /* the depth track of the run (below); added at the end */
} lcd_run_ext2_t;
/* lcd_run_ext2_t grown at its end by the read sets of the run (above): the same bytes under a name of their own, so that a caller compiled against the shorter
 * struct and the tests that pin its layout stay as they are.  It is handed to the two drivers as their ext2 with x.size = sizeof(lcd_run_ext2_split_t); by the
 * `size` rule a shorter struct reads as one without these members; a size beyond sizeof(lcd_run_ext2_split_t) is a layout this library does not know and reads
 * as lcd_run_ext2_t alone. */
typedef struct lcd_run_ext2_split_t {
    lcd_run_ext2_t x;
    const char *split_prefix; int split_gz, split_comment; const char *haplotag_path; lcd_split_stats_t *split_stats;
} lcd_run_ext2_split_t;
int lcd_call_files_ext2(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_run_opt_t *opt, lcd_file_stats_t *stats, const lcd_run_out_t *out,
                        const lcd_run_ext_t *ext, const lcd_run_ext2_t *ext2);
/* lcd_call_bam_regions_ext2 == lcd_call_bam_regions with the same struct: the table of the one contig, every region's chunk piled up with its final haplotypes (the
 * chunks[c].first.state->haps the call returns) in region order, by the same writer.  The file is created after the refusals and the call, and removed when the
 * table or the alignment output behind it fails.  lcd_call_bam_regions is the call with ext2 == NULL. */
int lcd_call_bam_regions_ext2(const char *bam_path, const char *bai_path, const char *fasta_path, const char *chrom, int n_regions, const int64_t *reg_beg,
                              const int64_t *reg_end, int min_mapq, const lcd_cfg_t *cfg, lcd_call_chunk_t *chunks, lcd_var1_t **records, int *n_records, char **vcf_body,
                              lcd_bam_out_t *bam_out, const lcd_run_opt_t *opt, const lcd_run_out_t *out, const lcd_run_ext2_t *ext2);

/* ---- haplotag: the reads of a chunk against the phased sites of a VCF (lcd_phased_vcf.cpp, haplotag_kernel.hip, lcd_haplotag.cpp) ----
 * The reference has no such command; these are PROJECT RULES, restated in Python in tests/haplotag_common.py.  They give the haps[read] / phase_sets[read]
 * arrays every per-haplotype output takes (tag rewrite, SAM text, mods, depth, read sets) without a calling run.  Positions are 1-based.
 *
 * The reader (host only, no HIP call; gzopen / gzread: plain, gzip and BGZF input).  The `#CHROM` line names the samples; `sample` NULL is the first one.  -4: an
 * unknown sample, a file without a sample column or without a `#CHROM` line, a data line with fewer columns than the header (the message names the line), a NULL
 * argument, max_indel < 1.  -30: the file cannot be opened or read (a gzip member cut short included).  Every data line is judged by the first rule that holds,
 * and that one is counted:
 *    1 CHROM is none of `names`                                          n_unknown_contig
 *    2 FILTER is neither PASS nor `.`                                     n_filtered
 *    3 the sample's GT (FORMAT's first key must be GT, else rule 3c): a '/' in it n_unphased; `a|b`, both numeric, a == b: n_hom; (3c) anything else --
 *      no GT, a `.`, haploid, more than two alleles, a number beyond the ALT list --  n_other_gt
 *    4 exactly one of a, b must be 0, else                                 n_both_alt.  The ALT allele is the non-zero one; hap_of_alt is 1 when it is a,
 *      2 when it is b
 *    5 REF or the ALT allele is empty or holds a byte outside ACGTNacgtn (symbolic alleles, `*`, breakends)    n_symbolic
 *    6 the pair is normalised in upper case: the longest common suffix is stripped while both are longer than 1, then common first bases while both are longer
 *      than 1, POS advancing.  SNV: lengths 1 and 1, bases differ.  INS: REF 1 long, ALT longer, first bases equal; len = the inserted bases.  DEL: ALT 1 long,
 *      REF longer, first bases equal; len = the deleted bases.  Anything else            n_complex
 *    7 an indel with len > max_indel (default 50)                          n_long_indel
 *    8 snvs_only and an indel                                              n_indel_off
 * What is left is a site (n_sites = n_snv + n_ins + n_del).  Its phase set is the integer value of the sample's PS key when that is > 0; the sites of a contig
 * without one share ONE set whose value is the POS of the first of them in table order.  Lines need not be sorted: a contig's table is its sites stable-sorted
 * by normalised POS (input order among equals; duplicates stay).  Per contig, a structure of arrays: pos (the anchor), kind (0 SNV, 1 INS, 2 DEL), hap_of_alt,
 * len (1 for an SNV), ref_code / alt_code (the nt16 codes of the SNV's bases, `=ACMGRSVTWYHKDBN`; 0 for indels), ins_off (into the contig's pool of the inserted
 * bases' nt16 codes, one per byte; 0 for others), ps_idx (dense, numbered by first appearance in table order), ps_value[ps_idx], and max_footprint.
 * A site's footprint: SNV [pos, pos], INS [pos, pos + 1], DEL [pos, pos + len]; max_footprint is the largest footprint length of the contig (0 without sites).
 *
 * lcd_chunk_haplotag works on a resolved chunk's KEPT records where the inflate left them in HBM: the operations (the record's own, or its CG field's by the
 * loader's rule), the packed bases and the qualities; no digars.  A record the loader filtered is no read and gets nothing.  `contig` is the index into the
 * reader's `names`.  The contig's table goes up once per device and is reused by every later call; only the four per-read arrays and the statistics come down
 * (the pair arrays on request, for the tests).
 *   span       [pos0 + 1, end]: end = pos0 + the lengths of the M / = / X / D / N operations.  A record's candidates are the table's sites with
 *              span.beg - (max_footprint - 1) <= pos <= span.end, a contiguous range; its PAIRS are those of them whose footprint intersects the span.
 *   verdict    of a pair, over the whole operation list, whatever the order the operations are visited in:
 *              disturbed   a D or N operation (length > 0) whose reference interval intersects the footprint, or an I operation (length > 0) at a boundary
 *                          r - 1 | r with pos < r <= the footprint's end -- unless that operation is the pair's own alt match;
 *              alt match   DEL: a D operation that starts at pos + 1 and has length len.  INS: an I operation at the boundary pos | pos + 1 of length len whose
 *                          read bases' nt16 codes equal the site's (all of them inside l_seq);
 *              base        (SNV) the M / = / X operation that contains pos gives the read's nt16 code there: alt_code ALT, ref_code REF, another one OTHER; a
 *                          quality byte below min_bq turns it into LOWQ (0xff, absent qualities, passes); a base index outside l_seq (l_seq == 0 included) OTHER.
 *              By the first that holds: the footprint is not inside the span NONE; disturbed OTHER; alt match ALT; an SNV: its base verdict; else (an indel
 *              site, covered and undisturbed) REF.  S, H, P, zero-length operations and unknown codes do nothing.  A record with l_seq == 0 (n_no_seq) can
 *              match no insertion: the I operation disturbs.
 *   votes      ALT votes for hap_of_alt, REF for the other haplotype; NONE, OTHER and LOWQ do not vote.  The record's phase set is the one with the most votes
 *              n1 + n2; among equals the one whose first voting site comes first in table order.  hap = 1 when n1 - n2 >= min_diff, 2 when n2 - n1 >= min_diff,
 *              else 0; phase_set = ps_value when hap != 0, else 0; n1 / n2 are the chosen set's, 0 / 0 when nothing voted.  n_multi_ps: records with votes in
 *              more than one set.
 *   layout     a record with l_seq < 0 or whose name, operation words, packed bases and qualities do not fit its block_size has hap 0, no candidates, and is
 *              counted in n_bad_record.  No lane reads outside the record or the tables.
 * The verdict depends on the record and the contig's table alone, so a record that two overlapping chunks hold gets the same answer in both: a run over many
 * chunks needs no stitch and no flip.
 * Four launches: measure (one wavefront per record: layout, span, candidate range by binary search), scan (one workgroup: the exclusive prefix of the candidate
 * counts), mark (one wavefront per record, 64 operations per step with carried 64-bit scans of the reference and query offsets; every lane ORs its own
 * operation's bits into the pair bytes, four to a 32-bit word), reduce (one wavefront per record: the verdict bytes and the votes per phase set by wave sums).
 * Integers only.  NULL with -4 before any HIP call: a NULL chunk / table, a chunk not made from a BAM or not resolved, a contig outside the table's, min_diff < 1,
 * min_bq outside 0 ... 254.
 * Verdict bytes: 0 NONE, 1 REF, 2 ALT, 3 OTHER, 4 LOWQ; 255: a candidate that is no pair. */
typedef struct lcd_hapvcf_opt_t { int max_indel, snvs_only, reserved[2]; } lcd_hapvcf_opt_t;
typedef struct lcd_hapvcf_stats_t {
    int64_t n_lines, n_sites, n_unknown_contig, n_filtered, n_unphased, n_hom, n_other_gt, n_both_alt, n_symbolic, n_complex, n_long_indel, n_indel_off,
            n_snv, n_ins, n_del, n_phase_sets;
} lcd_hapvcf_stats_t;
typedef struct lcd_phased_vcf_s lcd_phased_vcf_t;
void lcd_hapvcf_opt_default(lcd_hapvcf_opt_t *opt);
lcd_phased_vcf_t *lcd_phased_vcf_read(const char *path, const char *sample /* NULL: the first */, int n_contigs, const char *const *names, const lcd_hapvcf_opt_t *opt /* NULL: defaults */,
                                      lcd_hapvcf_stats_t *stats /* may be NULL */);
int lcd_phased_vcf_n_contigs(const lcd_phased_vcf_t *v);
int64_t lcd_phased_vcf_n_sites(const lcd_phased_vcf_t *v, int contig);        /* -4: contig outside the table's */
int lcd_phased_vcf_n_phase_sets(const lcd_phased_vcf_t *v, int contig);
int64_t lcd_phased_vcf_pool_size(const lcd_phased_vcf_t *v, int contig);
int lcd_phased_vcf_max_footprint(const lcd_phased_vcf_t *v, int contig);
/* any output may be NULL; pos / ins_off: n_sites 64-bit entries, kind / hap_of_alt / ref_code / alt_code: n_sites bytes, len / ps_idx: n_sites ints,
 * ps_value: n_phase_sets, pool: pool_size bytes */
int lcd_phased_vcf_sites_to_host(const lcd_phased_vcf_t *v, int contig, int64_t *pos, uint8_t *kind, uint8_t *hap_of_alt, int *len, uint8_t *ref_code, uint8_t *alt_code,
                                 int64_t *ins_off, int *ps_idx, int64_t *ps_value, uint8_t *pool);
void lcd_phased_vcf_free(lcd_phased_vcf_t *v);
int lcd_phased_vcf_errno(void);                                          /* of this thread's last lcd_phased_vcf_read: 0, -4 or -30 */
const char *lcd_phased_vcf_error(void);                                  /* its message (the reader is host-only code of its own and does not set lcd_last_error) */

typedef struct lcd_haplotag_opt_t { int min_bq, min_diff, reserved[2]; } lcd_haplotag_opt_t;
typedef struct lcd_haplotag_stats_t {
    int64_t n_records, n_pairs, n_verdict[5] /* NONE REF ALT OTHER LOWQ */, n_tagged[3] /* hap 0 1 2 */, n_multi_ps, n_cg, n_bad_record, n_no_seq;
    double ms_measure, ms_mark, ms_reduce;
} lcd_haplotag_stats_t;
typedef struct lcd_haplotag_s lcd_haplotag_t;
void lcd_haplotag_opt_default(lcd_haplotag_opt_t *opt);                    /* min_bq 0, min_diff 1 */
int lcd_haplotag_opt_check(const lcd_haplotag_opt_t *opt);                /* 0 / -4 (host only) */
lcd_haplotag_t *lcd_chunk_haplotag(const lcd_chunk_t *chunk, const lcd_phased_vcf_t *vcf, int contig, const lcd_haplotag_opt_t *opt /* NULL: defaults */,
                                   lcd_haplotag_stats_t *stats /* may be NULL */);
int lcd_haplotag_n_reads(const lcd_haplotag_t *h);
int lcd_haplotag_n_records(const lcd_haplotag_t *h);                       /* the kept records: one per read, in the reads' order */
int lcd_haplotag_to_host(const lcd_haplotag_t *h, int *haps, int64_t *phase_sets, int *n1, int *n2);      /* per kept read; any may be NULL */
/* for tests: per kept record the first candidate's index in the contig's table and the candidates' offsets (n_records + 1 entries, the last one the total), and one
 * verdict byte per candidate (copied from the device by this call) */
int64_t lcd_haplotag_n_candidates(const lcd_haplotag_t *h);
int lcd_haplotag_pairs_to_host(const lcd_haplotag_t *h, int64_t *first_site, int64_t *cand_off, uint8_t *verdict);
void lcd_haplotag_free(lcd_haplotag_t *h);
/* lcd_haplotag_files: a whole BAM (or the BAMs of one sample) against a phased VCF.  It IS lcd_call_files_ext2 with another middle stage: the plan, the windows,
 * the load stage, the write stage and the closing order are shared (one function in lcd_call_file.cpp takes the stage as a parameter).  The middle stage runs
 * lcd_chunk_haplotag on every chunk of the window (contig i of the BAM header is contig i of the site tables, read once with the header's names) and hands the
 * result on as the chunk's first.state (lcd_hap_state_init(n_reads, 0) with haps and phase_sets filled), so the alignment writer (BAM or SAM, HP / PS tags), the
 * methylation table, the depth track and the read sets run unchanged.  Because a record's answer depends on the record and its contig's table alone, two
 * overlapping chunks agree on a record they both hold: no stitch, no flip.  No VCF is written and nothing goes to stdout unless a SAM output to "-" asks for it.
 * hopt's FIRST member is its own size (members behind `size` read as zero; a size that does not reach vcf_path is -4): vcf_path, sample (NULL: the first),
 * max_indel (0: 50), snvs_only, min_bq, min_diff (0: 1), *vcf_stats (the reader's), *stats (the sums of lcd_haplotag_stats_t over the chunks; filled only by a
 * run that succeeds).  Refused with -4 before anything is created: job->vcf_path, opt->fields, opt->aln->refine, no vcf_path, negative max_indel / min_diff, min_bq
 * outside 0 ... 254, and a run without any output (no bam_out, mods_path, depth_path, split_prefix, haplotag_path).  Index handling (.bai / .fai, write_out_bai)
 * and every other refusal are those of a calling run; the reader's errors come back with its codes (-4 / -30).  stats->ms_call is the middle stage's time. */
typedef struct lcd_haplotag_run_t {
    size_t size;
    const char *vcf_path, *sample; int max_indel, snvs_only, min_bq, min_diff; lcd_hapvcf_stats_t *vcf_stats; lcd_haplotag_stats_t *stats;
} lcd_haplotag_run_t;
int lcd_haplotag_files(const lcd_inputs_t *in, const lcd_file_job_t *job, const lcd_cfg_t *cfg, const lcd_haplotag_run_t *hopt, const lcd_run_opt_t *opt,
                       lcd_file_stats_t *stats, const lcd_run_out_t *out, const lcd_run_ext2_t *ext2);

#ifdef __cplusplus
}
#endif
#endif