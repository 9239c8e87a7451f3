// lcd_plan.cpp -- how the host plans a POA chain and a WFA job: workgroup size, window, LDS bucket, ring slots and capacities of a chain (chain_caps, chain_class), the
// retry policy of the POA rounds, and class, decision-byte block and snapshots of a WFA job (wfa_plan, wfa_class).  Pure functions: the same chain or job, scoring,
// HostSwitches and PlanHints give the same PoaChain / WfaJob.  No HIP here -- nothing in this file touches a device, and tests/test_chain_plan.py runs it through
// lcd_plan_chain_probe / lcd_plan_wfa_probe (lcd_host.cpp) on a machine without one.  The learned levels behind PlanHints belong to the code that learns them
// (lcd_host.cpp: the POA rounds and the anchor WFA stage).
#include <algorithm>
#include <cstring>
#include "lcd_plan.h"

namespace lcd_internal __attribute__((visibility("hidden"))) {

// first score bound of a job (WfaJob.s_cap on entry of run_wfa_stage; overflow -> x4 + 64): the length difference as one long gap plus a little
// divergence.  Since the wavefront values live in a ring (wfa_kernel.hip) the bound no longer sizes a quadratic arena of retained wavefronts
// (20 B x s^2), only the decision bytes (1 B per diagonal, blocked and checkpointed above 16 MB) -- but a tight bound keeps the small jobs in
// the LDS class: a job of score <= ~100 holds its whole value ring in 16-32 KB of LDS.
int wfa_default_scap(int plen, int tlen, const int hint) {
    int d = plen > tlen ? plen - tlen : tlen - plen;
    int m = plen < tlen ? plen : tlen;
    static const double div[3] = {0.005, 0.06, 0.20};
    long long s = 24 + d + 40 + (long long)(m * div[hint]) * 6; // (ref<->cons and segment jobs are clean: hint 0; anchor jobs: the learned level, PlanHints.wfa.  Tried in round 4: twice / four times the slope -- 2 002 / 756 instead of 3 441 second-round jobs of 50 000, the stage within noise)
    return (int)std::min<long long>(s, 2000000);
}
// LDS classes of the value ring.  A class is one launch whose jobs-per-CU is 160 KB / bucket: until round 4 the buckets were 16 / 32 / 64 KB, and the 64 KB class (two
// jobs per CU) was the tail of both WFA stages -- 8 800 ref<->cons jobs of a 20-batch submission: 7.8 ms; in the HBM-ring class (256 threads, the ring in L2) the same
// jobs take 2 ms.  LCD_WFA_BUCKETS_KB="a,b,c" overrides (ascending; the last one is the largest ring that stays in LDS unless LCD_WFA_LDS_MAX_KB says otherwise).
// class (value ring in LDS or HBM), decision-byte block and snapshots of one job for the score bound s_want
void wfa_plan(WfaJob &j, const LcdScoring &sc, long long s_want, const HostSwitches &sw) {
    const uint64_t blk_target = sw.wfa_block_bytes(), lds_max = sw.wfa_lds_max(); // (LCD_WFA_BLOCK_KB is a test switch: tiny blocks)
    auto gap = [&](long long n) { return n <= 0 ? 0ll : std::min<long long>(sc.o1 + sc.e1 * n, sc.o2 + sc.e2 * n); };
    const long long ub = gap(j.plen) + gap(j.tlen); // delete the pattern, insert the text: no optimal score is above it
    s_want = std::max<long long>(8, std::min(s_want, ub));
    WfaLayout L = wfa_layout(j.plen, j.tlen, (int)s_want, (int)s_want + 1, 0, 1, sc.mismatch, sc.o1, sc.e1, sc.o2, sc.e2);
    if (L.ring_bytes <= lds_max && L.blk_bytes <= blk_target) { j.lds = 1; j.s_cap = (int)s_want; j.blk_rows = j.s_cap + 1; j.n_ckpt = 0; }
    else {
        j.lds = 0;
        if (L.blk_bytes <= blk_target) { j.s_cap = (int)s_want; j.blk_rows = j.s_cap + 1; j.n_ckpt = 0; }
        else {
            const long long w = L.w_cap - 2;
            j.blk_rows = (int)std::max<long long>(32, (long long)(blk_target / (uint64_t)w));
            j.n_ckpt = (int)((s_want + j.blk_rows) / j.blk_rows) - 1;
            j.s_cap = j.blk_rows * (j.n_ckpt + 1) - 1;
        }
        L = wfa_layout(j.plen, j.tlen, j.s_cap, j.blk_rows, j.n_ckpt, 0, sc.mismatch, sc.o1, sc.e1, sc.o2, sc.e2);
    }
    j.ws_bytes = lcd_align_up(L.total, 256);
}
int wfa_class(const WfaJob &j, const LcdScoring &sc, const HostSwitches &sw) { // 0: HBM ring, 1..: LDS bucket
    if (!j.lds) return 0;
    const WfaLayout L = wfa_layout(j.plen, j.tlen, j.s_cap, j.blk_rows, 0, 1, sc.mismatch, sc.o1, sc.e1, sc.o2, sc.e2);
    for (size_t b = 0; b < sw.wfa_buckets_kb.size(); ++b) if (L.ring_bytes <= (uint64_t)sw.wfa_buckets_kb[b] << 10) return (int)b + 1;
    return (int)sw.wfa_buckets_kb.size();
}
uint64_t ed_arena_bytes(int qlen, int tlen) { return ed_tb_cap(qlen, tlen) * 20 + (uint64_t)qlen * 8 + (uint64_t)tlen * 2 + 512; }
uint64_t wfa_out_bytes(const WfaJob &j) {
    uint64_t maxl = (uint64_t)j.plen + j.tlen + 1, o = 0;
    if (j.want & 1) o += lcd_align_up(maxl * 4, 16);
    if (j.want & 2) o += lcd_align_up(maxl * 2, 16);
    return o;
}

// where a K2 chain goes when its certified band outgrew the window: full rows.  (Tried: the band in multi-wavefront windowed rows of 512 / 1 024 columns first;
// their rows meet at a workgroup barrier twice per row and measured SLOWER than the systolic full rows they would replace -- configs[1]: 46.9 k instead of
// 52.5 k regions/s with three such chains per batch; ONT shape with every K2 chain there: 6.6 k instead of 13.1 k)
int cert_next_level(const PoaChain &) { return 0; }
// Capacities and class of one chain: a pure function of the chain's shape, the scoring, the switches, the learned levels and the number of chains in the
// submission at hand (lcd_plan_chain_probe shows its result without a device).
void chain_caps(const lcd_opt_t &opt, const ChainRec &C, const std::vector<PoaRead> &preads, int scale, const long long n_chains, const HostSwitches &sw, const PlanHints &hints, PoaChain &pc) {
    const int n = (int)C.members.size();
    long long sum = 0; int maxl = 0;
    for (int k = 0; k < n; ++k) { const PoaRead &r = preads[C.read0 + k]; sum += r.len; maxl = std::max(maxl, r.len); }
    pc.n_reads = n; pc.read0 = C.read0; pc.mode = C.mode;
    // K2 chains of clean reads run in the single-wavefront class with rows restricted to the CERTIFIED band (poa_kernel.hip align_certified: same
    // alignments as the full rows, ~20x fewer cells on HiFi-shape regions); noisy reads' bounds are too loose for a 256-column window (LCD_CERT=2 forces
    // them through it, 0 switches the path off).  A chain whose band outgrows the window comes back with LCD_ERR_CERT and is re-run with full rows.
    const int cert_mode = sw.cert; // (LCD_CERT: the tests switch it)
    int lvl = C.cert_level;
    // (Long chains are the critical path of a submission, and in a 64-thread workgroup a third to a half of such a chain is the per-read work around the rows --
    // graph update, re-sort, plan: parallel over the nodes.  LCD_CERT_SOLO_LEN=n gives chains of reads >= n bases a 256-thread workgroup whose wavefront 0 runs
    // the same rows (poa_kernel.hip align_windowed<.., SOLO>).  Measured slower at every threshold -- 20 batches: 36 - 42 k instead of 45 k regions/s, 2 x 32
    // batches: 52 k instead of 66 k -- so it is off by default.)
    const int solo_len = sw.cert_solo_len; // (LCD_CERT_SOLO_LEN: a test switches it)
    // Noisy reads (level 2): the band in the systolic rows of the class the reads' length asks for (poa_kernel.hip align_certified_sys); LCD_CERT_SYS=0: full rows
    const int cert_sys = sw.cert_sys; // (LCD_CERT_SYS: the tests switch it)
    if (lvl < 0) lvl = !(C.mode == 1 && maxl < 65535) ? 0 : (cert_mode == 2 || (cert_mode == 1 && !opt.is_ont)) ? 1 : (cert_mode == 1 && cert_sys && maxl >= 256) ? 2 : 0;
    pc.cert = C.mode == 1 ? lvl : 0; pc.ring_k = 0;
    // LONG chains -- the critical path of a submission, and of a single batch: 34 reads x 4 kb run 0.28 s on one wavefront, more than half of it the per-read phases around
    // the rows (row plan, graph update, re-sort, backtrack: latency chains through L2 with 64 loads in flight) -- get a 256-thread workgroup: wavefront 0 runs the same
    // lean rows, all four the phases around them (4x the loads in flight).  LCD_SOLO_RL: reads x longest read from which on (0 = off); LCD_CERT_SOLO_LEN: certified-band
    // chains by read length (test switch)
    {
        const long long solo_rl = sw.solo_rl; // (LCD_SOLO_RL: tests switch it)
        pc.solo = (C.solo >= 0 ? C.solo > 0 : (solo_rl > 0 && (long long)n * maxl >= solo_rl)) || (solo_len > 0 && pc.cert == 1 && maxl >= solo_len) ? 1 : 0;
        // LCD_SOLO_MW=1: long certified-band chains run their rows on all four wavefronts of the workgroup (poa_kernel.hip align_lean_mw) instead of wavefront 0 alone.
        // Same alignments (digest 0004c9ba86f18807 at the driver's flags), but measured SLOWER: 3 530 instead of 2 950 ticks per row of the longest chain, 80.6 k instead
        // of 88.4 k regions/s -- every wavefront pays the row's fixed cost (plan word, interval, predecessor loop, metadata: ~400 instructions in this version, which
        // reads every predecessor from the LDS ring) plus two LDS round trips and two barriers, and the cells it saves are ~75 instructions.  Off by default.
        if (pc.solo && pc.cert == 1 && sw.solo_mw > 0) pc.solo = 2;
        // Round 4: the rows of the long certified-band chains run as a PIPELINE over the four wavefronts (poa_kernel.hip align_cyc: mailboxes, no barrier, the row before in
        // registers) -- LCD_SOLO_CYC=0 keeps them on wavefront 0
        // (the four-wavefront pipeline pays on a CROWDED chip, where a lone wavefront of the long chain gets a quarter of its SIMD: 16 / 20 batches 173 / 200 ms with it,
        //  197 / 206 without.  A chain that has its CU to itself is faster on one wavefront -- a lone batch 117 ms instead of 128, four batches 152 instead of 154:
        //  the pipeline from LCD_SOLO_CYC_MIN chains per submission on)
        if (pc.solo == 1 && pc.cert == 1 && sw.solo_cyc != 0 && n_chains >= sw.solo_cyc_min) pc.solo = 3;
    }
    // graph capacity: the worst case is one node per base of every read (sum), the usual case a little more than the longest read.  Sized
    // from an estimate (a few per cent of new nodes per read on top of the backbone; hints.node: learned from noisier data); a chain that runs
    // out (LCD_ERR_NODES / LCD_ERR_EDGES) is re-run with 4x more per retry, up to the worst case.  The worst case for everybody was
    // 10 GB of arena per 1 250 regions, nearly all of it never touched.
    const long long node_worst = std::min<long long>(sum + 2, 2000000000ll), edge_worst = std::min<long long>(sum + n + 2, 2000000000ll);
    {
        static const double nf[3] = {1.25, 2.0, 4.0}, sf[3] = {0.03, 0.10, 0.30};
        const int nh = sw.node_hint >= 0 && sw.node_hint <= 2 ? sw.node_hint : hints.node; // (LCD_NODE_HINT, test switch: the learned level, fixed)
        long long est = (long long)(nf[nh] * maxl + sf[nh] * (double)sum) + 64;
        for (int sc2 = 1; sc2 < scale; sc2 *= 2) est *= 4;
        pc.node_cap = (int)std::min(node_worst, est);
        pc.edge_cap = (int)std::min(edge_worst, est + est / 4 + n);
    }
    pc.rid_words = (n + 63) / 64; pc.max_len = maxl;
    int mw = (int)(n * opt.min_af); if (mw < 2) mw = 2;
    pc.min_w = (uint32_t)mw;
    // rows actually visited ~ graph size ~ a small multiple of the backbone; band ~ 2w+1 plus drift.  Overflow is detected
    // in-kernel (LCD_ERR_CELLS) and the chain is re-run with `scale` x more, up to the worst case.
    const long long rows_worst = pc.node_cap;
    // hints.cell[mode]: learned from the overflow retries of earlier submissions (noisy reads: every read adds ~error-rate new nodes,
    // and the row-max columns that steer the adaptive band drift further) -- a chain that overflows is re-run from scratch, so data that
    // keeps overflowing is given the larger estimate up front
    const int hint = sw.cell_hint >= 0 && sw.cell_hint <= 2 ? sw.cell_hint : hints.cell[C.mode ? 1 : 0]; // (LCD_CELL_HINT: test switch)
    static const double rows_f[3] = {1.3, 2.2, 3.2}; static const int band_x[3] = {64, 128, 192};
    const long long rows_est = std::min<long long>(rows_worst, (long long)(rows_f[hint] * maxl) + 64);
    long long band;
    if (C.mode == 0) band = std::min<long long>(maxl + 1, 2ll * (10 + maxl / 100) + 1 + band_x[hint]);
    else if (pc.cert == 2) band = std::min<long long>(maxl + 1, std::max<long long>(1040, (long long)(0.6 * maxl))); // (noisy reads: intervals of a third to a half of the read)
    else if (pc.cert) { // windowed rows of <= 260 columns at 1 B of code per cell -- and room for a few reads through the generic rows (12 B per cell of intervals wider
        // than the window, poa_kernel.hip align_certified): LCD_CERT_BAND columns per row
        band = std::min<long long>(maxl + 1, sw.cert_band);
    }
    else band = maxl + 1;
    long long cells = rows_est * band;
    if (sw.cell_shrink > 0) cells = std::max<long long>(cells / sw.cell_shrink, 1); // test switch: estimates far too small, so that the chains have to grow their regions (tests/test_gpu_region.py)
    // (tried: the single-wavefront class compiled for 64 VGPRs (__launch_bounds__(64, 8): 32 instead of 16 wavefronts per CU, 4 - 8 KB pools): 34 - 37 k instead of
    // 51 k regions/s -- the row loops spill (40 - 170 B of scratch per lane inside align_windowed) and the graph phases' scratch grows from 924 to 1 336 B)
    // (tried: 3x the estimate up front for the long K1 chains of noisy reads, which overflow most -- 5 instead of 60 re-runs per 4 SV-shape batches, but
    // the POA stage got 20 % LONGER: an overflowing chain gives up early and its re-run shares the chip with ~50 others instead of 9 000)
    // K2 chains of noisy reads: at one code byte per worst-case cell EVERY such chain ran out of spilled value rows (a spilled row is 12 bytes
    // per window column; clean graphs spill a few per cent of their rows, but in the graphs of 5 %-error reads most rows have a successor more
    // than K rows away, and nearly every row has >= 2 usable predecessors, i.e. an ordinal word per cell) and was re-run with a 4x graph.
    // Once the hint says the K2 chains overflow, their region is code | 4 ordinal planes | 8 planes of spilled rows (13 x cell_cap, not 4 x)
    pc.spill_x = C.mode == 1 && hint >= 1 ? 8 : 2; // (a spilled row is 12 B per WINDOW column, 12-24x a code row: half of the rows spilled = 6-12x the code plane)
    if (C.mode == 1 && hint >= 1) pc.edge_cap = (int)std::min<long long>(edge_worst, 2ll * pc.edge_cap); // (and their graphs have more bubbles per node)
    // K1 chains of noisy reads: a dozen or two per ONT-shape submission ran out of EDGES (nothing grows those in place) and were re-run from their first read in a second
    // round that lasts as long as its slowest chain -- 0.29 s of a 1.9 s stage for 0.05 % of the chains; 28 bytes per edge
    if (C.mode == 0 && opt.is_ont) pc.edge_cap = (int)std::min<long long>(edge_worst, 2ll * pc.edge_cap);
    const long long worst = rows_worst * (long long)(maxl + 1);
    for (int s = 1; s < scale && cells < worst; s *= 2) cells *= 8;
    cells = std::min(cells, worst);
    pc.cell_cap = (uint64_t)std::max<long long>(cells, maxl + 64);
    // 16-bit ring values: wanted (LCD_RING16) and representable -- the same bounds the kernel checks per read (poa_kernel.hip align_lean, "int16 range"), here on the
    // chain's longest read with the scoring at hand: best case every base a match plus the heaviest bonus path (every traversed edge adds ilog2(weight) <= ilog2(reads),
    // a path has ~1.1 nodes per base), worst case a gap over all rows plus a gap over all columns.  A chain that fails this is laid out for a 32-bit ring from the
    // start (its pool and bucket are those of the 32-bit ring) instead of meeting the kernel's guard on every read and taking the generic rows
    {
        int lg = 0; while ((2 << lg) <= std::max(n, 1)) ++lg; // ilog2(n): the largest edge weight is the number of reads
        const long long rows = (long long)(1.1 * maxl) + 64;
        const long long o_max = std::max(opt.gap_open1, opt.gap_open2), e_min = std::min(opt.gap_ext1, opt.gap_ext2);
        const long long best = (long long)maxl * opt.match + rows * lg + 64;
        const long long worstv = 2 * (o_max + e_min * rows) + (opt.gap_open1 + opt.gap_open2) + 2ll * (opt.gap_ext1 + opt.gap_ext2) + 64;
        pc.ring16 = sw.ring16 == 2 ? 2 : sw.ring16 && best <= 32000 && worstv <= 32000 ? 1 : 0; // (chain_class keeps it for certified-band chains of the single-wavefront class)
    }
    chain_class(pc, opt.is_ont != 0, sw);
    // SMALL graphs of noisy reads: nearly every row has a successor further away than the ring and is spilled -- 12 bytes per WINDOW column (768 B for the narrowest
    // window) whatever the chain's width -- while their DP region, at the worst case of nodes x (length + 1) cells, is a few tens of KB: 45 of the 58 chains an
    // SV-shape submission sent to a second round were chains of 44 - 110 bases that had run out of spilled rows (LCD_RETRY_DEBUG=1), and a second round lasts as long
    // as its slowest chain.  Room for every row spilled, for graphs of up to 1 024 nodes (<= 1.5 MB per chain).
    if (opt.is_ont && pc.node_cap <= 1024) {
        const uint64_t win = (pc.threads == 64 || pc.solo) ? (uint64_t)pc.wmax : 4ull * pc.threads;
        const uint64_t floor_cells = ((uint64_t)pc.node_cap + 2) * (3 * win * 4) / (uint64_t)(pc.spill_x > 2 ? pc.spill_x : 2) + 64;
        if (pc.cell_cap < floor_cells) pc.cell_cap = floor_cells;
    }
}

// Workgroup size class + LDS budget of a chain (poa_kernel.hip): threads follow the DP row width; the dynamic LDS pool holds
// K ring slots of `wmax` columns + the query cache during the DP and the 16-bit graph copy of the re-sort (about 22 B per node)
// afterwards.  Chains are launched in groups of equal (threads, LDS bucket) so that short chains do not pay a long chain's LDS.
void chain_class(PoaChain &pc, bool noisy, const HostSwitches &sw) {
    // DP row width: K2 rows span the whole read (+2 guard columns of the window); K1 rows are the adaptive band plus drift
    const long long width = pc.cert == 1 ? 256 : pc.mode == 1 ? (long long)pc.max_len + 2 : 2ll * (10 + pc.max_len / 100) + 1 + 48;
    int threads, K, wmax; // wmax: window / ring-slot width in columns, a power of two <= 4 * threads (poa_kernel.hip align_windowed)
    if (width > 256) pc.solo = 0; // (the wide classes have their own rows)
    // one lane per four columns of the window: 64 / 128 / 256 / 512 / 1024 threads, so that no wavefront of a workgroup idles
    // (a 2 048-column chain in a 1 024-thread workgroup would hold a whole CU's registers with half of its wavefronts parked)
    if (width <= 256) { // single wavefront; banded chains prefer the narrowest window their band fits (1, 2 or 4 cells per lane, align_windowed)
        threads = 64; K = 2;
        const long long bw = 2ll * (10 + pc.max_len / 100) + 1 + sw.band_margin; // LCD_BAND_MARGIN: adaptive band + a little drift; a band that outgrows it is re-run wider
        wmax = pc.cert == 1 ? std::max(256, sw.cert_ring) /* LCD_CERT_RING: ring slots wide enough for the reads that take the generic rows */ : pc.mode == 1 ? 256 : bw <= 60 ? 64 : bw <= 124 ? 128 : 256;
        if (pc.solo) threads = 256; // (same rows, same ring layout: only the per-read phases see the other three wavefronts)
    }
    else if (width <= 512) { threads = 128; K = 2; wmax = 512; }
    else if (width <= 1024) { threads = 256; K = 2; wmax = 1024; }
    else if (width <= 2048) { threads = 512; K = 2; wmax = 2048; }
    else { threads = 1024; K = 2; wmax = 4096; } // wider rows take the generic (HBM) rows of the kernel
    const long long est_nodes = (long long)(pc.max_len * 1.15) + 64;
    const long long seq_bytes = lcd_align_up((long long)pc.max_len + 28, 16) + lcd_align_up(est_nodes + 16, 16); // query cache + first-predecessor distances
    // ring slots of the single-wavefront class: 2, except long K1 chains of noisy reads -- their graphs interleave the alternatives of every column, a row's
    // predecessors sit 3 - 6 rows back as often as not, and a predecessor that has left the ring costs the row two dependent trips to HBM (its metadata, then
    // its spilled values); those chains are few and they are the latency of an SV-shape submission, so they get LCD_RING_K (8) slots and the LDS that takes
    if ((threads == 64 || pc.solo) && pc.mode == 0 && noisy) {
        if (pc.max_len >= sw.ring_k_len && sw.ring_k) K = sw.ring_k; // (LCD_RING_K is 0 unless a power of two in 2..32)
    }
    // certified-band K2 chains of the single-wavefront class keep 16-bit ring values (H, E1, E2 of reads below 15 000 bases fit int16): their 512-column ring was 12 of
    // their 16 KB, and LDS x time is what a submission runs out of first ("Where the chain kernels' time goes now").  LCD_RING16=0 (read per submission): 32-bit, as before
    pc.ring16 = pc.ring16 /* wanted and representable: chain_caps, LCD_RING16 */ && threads == 64 && !pc.solo && pc.cert == 1 && (pc.ring16 == 2 || pc.max_len < 15000) ? 1 : 0; pc.pad3_ = 0;
    const long long dp_bytes = (long long)K * 3 * wmax * (pc.ring16 ? 2 : 4) + seq_bytes; // the ring holds `wmax` columns per slot (4 * threads, or the narrower preferred window of a single-wavefront banded chain)
    // the re-sort's LDS copy of the graph: 8 B per node + 4 B per edge (topo_sort_block); edges ~ nodes + a few per bubble
    long long need = std::max(dp_bytes, est_nodes * 8 + (est_nodes + est_nodes / 8) * 4 + 64);
    { // the single-wavefront class is kept to a small pool: 16 such chains per CU (8 KB each, the wavefront limit at 128 VGPRs) instead of 2-9
      // is worth more than a fast re-sort -- bigger graphs do their Kahn walk on the same packed words in HBM (16 KB: +17 % regions/s over
      // uncapped pools; 8 KB with the ring laid out for the preferred window: another +7 %).  Noisy reads (graphs twice the size, a re-sort after
      // nearly every read) preferred 16 KB while the Kahn walk was a serial pass over every node; since it jumps chains (v12) 8 KB is best for them
      // too (+6 % over 16 KB).  LCD_LDS_CAP_KB overrides.
        // (tried: certified-band K2 chains -- few, some long: 35 reads x 3.7 kb is the critical path of a submission, a quarter of it re-sorts -- with the pool
        //  the re-sort wants (32 / 64 KB instead of the cap): 42 k / 30 k instead of 43 k regions/s at 20 batches; the same for the long ones only (>= 1 000 /
        //  1 500 bases): 30 k / 28 k; again after the streams learned to count a group's longest chain, so that the extra launch group is not queued behind
        //  another: 41 k / 44 k / 48 k for chains >= 1 500 / 2 500 / 3 000 bases against 60.8 k -- it is the chains themselves that get slower with the
        //  re-sort's LDS path, not their place in the queue)
        const int cap_here = sw.lds_cap_kb;
        if (cap_here > 0 && threads == 64) need = std::max(dp_bytes, std::min<long long>(need, (long long)cap_here << 10));
        // (the long chains: what the re-sort would like beyond their bucket does not move them into the 148 KB bucket -- one workgroup per CU -- any more; LCD_SOLO_CAP=0: as before)
        if (sw.solo_cap && pc.solo) need = std::max(dp_bytes, std::min<long long>(need, (long long)sw.solo_kb << 10));
    }
    // LDS per workgroup decides how many single-wavefront chains share a CU (160 KB, 16 wavefronts at 128 VGPRs), and those chains are
    // most of the work: fine-grained buckets; every (threads, bucket) group is one launch, a few streams run the groups (launch_poa_grouped)
    static const int buckets[] = {8 << 10, 12 << 10, 16 << 10, 24 << 10, 32 << 10, 48 << 10, 64 << 10, 96 << 10, 148 << 10};
    int lds = buckets[8];
    for (int b : buckets) if (need <= b) { lds = b; break; }
    // the long chains of a submission are ONE launch group (one LDS size): kernels of a stream run one after the other, and every group of a few long chains lasts as
    // long as its longest chain -- four such groups on the four streams held everything else back for 0.2 s
    if (pc.solo) { const int solo_kb = sw.solo_kb; /* LCD_SOLO_KB, a bucket */ lds = std::max(std::min(lds, 148 << 10), solo_kb << 10); if (lds > (solo_kb << 10)) lds = 148 << 10; }
    // The longest single-wavefront chains are the critical path of a submission (34 reads x 4 kb: 0.28 s against 0.20 s of work for the whole chip), and next to 15
    // other chains of its CU such a wavefront issues one instruction per ~7 cycles.  Chains above LCD_ISO_RL read-bases ask for LCD_ISO_KB of LDS: three of them fill
    // a CU's LDS, so each has a SIMD (nearly) to itself -- and a pool its re-sort runs in.
    if (threads == 64) {
        const long long iso_rl = sw.iso_rl; const int iso_kb = sw.iso_kb; // (measured: the isolated chain is 8 % faster, the submission 10 % slower -- the extra launch group costs more than it gives; off)
        if (iso_kb > 0 && (long long)pc.n_reads * pc.max_len >= iso_rl) lds = std::max(lds, iso_kb << 10);
    }
    // (noisy K1 chains below that length: as many slots as the bucket they have anyway leaves room for -- LCD_RING_K_FREE=0 keeps them at 2.  Tried for the K1
    //  chains of clean reads too: no change at 2 x 32 batches, 47 k instead of 60 k regions/s at one submission of 20)
    if ((threads == 64 || pc.solo) && pc.mode == 0 && noisy && K == 2) {
        // (until round 4 only in the buckets the default pool cap produces: with LCD_LDS_CAP_KB=16 the rule gives eight slots of 64 columns whose next wider window --
        //  eight slots of 128 -- lies over the first-predecessor distances, and the rows that ran after it followed the overwritten distances for ever.  Root cause fixed
        //  in poa_kernel.hip (WinOut.clobber; tests/test_gpu_kernels.py::test_wider_window_after_a_ring_that_outgrew_the_pool_layout); the restriction is gone: same
        //  digest and rate on the ONT shape with and without it.  LCD_RING_K_MAXLDS_KB restores it)
        while (sw.ring_k_free && lds <= (sw.ring_k_maxlds_kb << 10) && K < 8 && (long long)(2 * K) * 3 * wmax * 4 + seq_bytes <= lds) K *= 2;
    }
    pc.threads = threads; pc.wmax = wmax; pc.lds_words = lds / 4; pc.ring_k = (threads == 64 || pc.solo) ? K : 0;
}
int chain_threads(const PoaChain &pc) { return pc.threads; }
long long chain_group_key(const PoaChain &pc) { return (long long)pc.threads * (1 << 20) + pc.lds_words; }
// Chains of one launch group that share a CU: 160 KiB of LDS over the chain's pool plus what a workgroup takes besides it, and 16 wavefronts at 128 VGPRs.
// The overhead exists with TWO sets of constants, and they are kept apart on purpose: the scheduling estimates (launch groups, LCD_PROFILE_CHAINS) say 1 KiB
// for the single-wavefront class and 6 KiB for the wider ones, the arena slots' count says 912 B and 6 096 B.  They decide launch groups and slot counts, so
// making them equal would change behaviour; nobody has measured which pair is right.
int chains_per_cu(const int lds, const int thr, const LdsOverhead &besides) { return std::max(1, std::min((160 * 1024) / (lds + (thr == 64 ? besides.wave64 : besides.wider)), 1024 / thr)); }
// The retry policy of the POA rounds, shared by a submission and lcd_poa_batch.  chain_goes_back: does a chain with this status run again in the next round?  A
// chain that ran out of DP cells, nodes or edges does, with larger capacities; a chain whose certified band outgrew its window does too, demoted
// (cert_next_level) and with the round remembered.  Anything else that is not LCD_OK is the caller's error.
bool chain_goes_back(const int status, const PoaChain &pc, ChainRec &CR, const int round) {
    if (status == LCD_ERR_CELLS || status == LCD_ERR_NODES || status == LCD_ERR_EDGES) return true;
    if (status != LCD_ERR_CERT || pc.cert <= 0) return false;
    CR.cert_fail_round = round; CR.cert_level = cert_next_level(pc); // one class up (512, 1 024 columns), then full rows
    return true;
}
// ... and the capacity scale it restarts with (`scale` doubles per round with retries): a chain sent back by the certified band starts its capacity ladder in the round after
int retry_scale(const ChainRec &CR, const int scale) { return CR.cert_fail_round < 0 ? scale : std::max(1, scale >> (CR.cert_fail_round + 1)); }

} // namespace lcd_internal
