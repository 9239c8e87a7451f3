// lcd_switches.h -- every LCD_* environment switch of the host library, in one table: a member of HostSwitches per switch, declared with its default and, in
// the comment behind it, `environment name | lifetime | default as INTEGRATION.md prints it | meaning` (tests/test_chain_plan.py reads these lines and holds the
// switch section of INTEGRATION.md to them).  HostSwitches::from_env() at the end of this file is the only place of the library that reads an LCD_* variable.
//
// LIFETIME, the one rule:
//   call     read at the entry of every exported call that plans work (lcd_batch_run_many, lcd_poa_batch, lcd_wfa_batch, lcd_dispatch_run and what calls
//            them begin with HostSwitches::from_env(); lcd_edlib_batch* would, but no switch bears on it) and handed down by const reference.  A caller that
//            changes the environment sees the change at its next call.
//   process  only what sizes something that outlives a call: from_env() keeps the values of its FIRST call in the process and gives them back ever after.
//            Each such entry says what it sizes.
// Launcher variables (LOCAL_RANK, WORLD_SIZE, LOCAL_WORLD_SIZE) are not ours and are read where they are used.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>

namespace lcd_internal __attribute__((visibility("hidden"))) {

constexpr int kSwitchUnset = INT_MIN;   // a switch whose default is not a number of its own range (it depends on the device, the host or the reads)
constexpr int kMaxStreams = 13;         // the caller's stream + the side streams of a batch (LCD_NSIDE + 1, lcd_host_internal.h)

struct HostSwitches {
    // ---- POA chains: capacities and class (lcd_plan.cpp chain_caps / chain_class) ----
    int cert = 1;                        // LCD_CERT | call | 1 | K2 chains over the certified band: 0 full rows everywhere, 1 clean reads, 2 noisy reads (is_ont) too
    int cert_solo_len = 0;               // LCD_CERT_SOLO_LEN | call | 0 | certified-band chains of reads at least this long run in a 256-thread workgroup (0: off)
    int cert_sys = 0;                    // LCD_CERT_SYS | call | 0 | 1: K2 chains of noisy reads run the band in the systolic rows of their class (0: full rows)
    long long cert_band = 1040;          // LCD_CERT_BAND | call | 1040 | columns per row the DP region of a certified-band chain is sized for
    int cert_ring = 512;                 // LCD_CERT_RING | call | 512 | width of a certified-band chain's LDS ring slots (at least 256)
    int band_margin = 12;                // LCD_BAND_MARGIN | call | 12 | drift columns added to a K1 chain's adaptive band when its window is chosen
    long long solo_rl = 100000;          // LCD_SOLO_RL | call | 100000 | reads x longest read from which a chain counts as long (0: off); set: the fixed cut replaces the longest-N choice
    bool solo_rl_set = false;            //   (whether LCD_SOLO_RL is set at all)
    int solo_mw = 0;                     // LCD_SOLO_MW | call | 0 | 1: long certified-band chains run their rows on all four wavefronts (measured slower)
    int solo_cyc = 1;                    // LCD_SOLO_CYC | call | 1 | long certified-band chains' rows as a pipeline over four wavefronts (0: wavefront 0 alone)
    long long solo_cyc_min = 16000;      // LCD_SOLO_CYC_MIN | call | 16000 | chains per submission from which on the pipeline is used
    bool solo_cap = true;                // LCD_SOLO_CAP | call | 1 | long chains keep to their bucket whatever the re-sort would like (0: they may move to 148 KB)
    int solo_kb = 64;                    // LCD_SOLO_KB | call | 64 | LDS bucket of the long chains, rounded up to a bucket
    long long iso_rl = 90000;            // LCD_ISO_RL | call | 90000 | reads x longest read from which a single-wavefront chain asks for LCD_ISO_KB
    int iso_kb = 0;                      // LCD_ISO_KB | call | 0 | LDS such a chain asks for, so that few share its CU (0: off; measured slower)
    int lds_cap_kb = 8;                  // LCD_LDS_CAP_KB | call | 8 | LDS pool of a single-wavefront chain (0: uncapped)
    int ring_k = 8;                      // LCD_RING_K | call | 8 | LDS ring slots of long K1 chains of noisy reads (a power of two in 2..32; anything else: 2 slots)
    int ring_k_len = 1500;               // LCD_RING_K_LEN | call | 1500 | read length from which such a chain counts as long
    bool ring_k_free = true;             // LCD_RING_K_FREE | call | 1 | shorter noisy K1 chains take the slots their bucket has room for (0: 2 slots)
    int ring_k_maxlds_kb = 148;          // LCD_RING_K_MAXLDS_KB | call | 148 | largest LDS bucket in which shorter noisy K1 chains take those extra ring slots
    int ring16 = 1;                      // LCD_RING16 | call | 1 | 16-bit LDS ring values for certified-band chains (0: 32-bit; 2: test switch, 16-bit whatever the bounds say)
    int cell_shrink = 0;                 // LCD_CELL_SHRINK | call | 0 | test switch: DP regions sized n times too small, so that chains have to grow them (0: off)
    int node_hint = -1;                  // LCD_NODE_HINT | call | -1 | test switch: the learned graph-capacity level fixed at 0..2 (-1: learned)
    int cell_hint = -1;                  // LCD_CELL_HINT | call | -1 | test switch: the learned DP-cell level fixed at 0..2 (-1: learned)
    // ---- WFA jobs (lcd_plan.cpp wfa_plan / wfa_class; run_wfa_stage) ----
    std::vector<int> wfa_buckets_kb{16, 32}; // LCD_WFA_BUCKETS_KB | process | "16,32" | LDS classes of the WFA value ring, ascending (process: one kernel launch configuration per bucket, and a stage's jobs are classed against the same list in every round)
    int wfa_lds_max_kb = kSwitchUnset;   // LCD_WFA_LDS_MAX_KB | call | the last bucket | largest value ring that stays in LDS; larger ones take the HBM-ring class
    int wfa_block_kb = 16 << 10;         // LCD_WFA_BLOCK_KB | call | 16384 | decision-byte block of a checkpointed WFA alignment
    long long wfa_wide_kb = 1024;        // LCD_WFA_WIDE_KB | call | 1024 | HBM-ring jobs with a workspace of at least this size run on the instantiation with four diagonals per thread (0: none)
    long long wfa_wide_min = 64;         // LCD_WFA_WIDE_MIN | call | 64 | ... as a launch of their own, and only when a stage has at least this many
    // ---- launch groups (lcd_host.cpp launch_poa_grouped) ----
    int streams = 4;                     // LCD_STREAMS | process | 4 | streams a submission deals its launch groups to, the caller's included, 1..13 (process: every submission of a process shares the runtime's hardware queues)
    double gate_frac = 0.80;             // LCD_GATE_FRAC | call | 0.80 | share of the CUs the wide classes may take before the narrow ones start
    int gate512_keep = kSwitchUnset;     // LCD_GATE512_KEEP | call | 2 x CUs | 512-thread workgroups that need not have started when the narrow launches begin
    double noisy_k1_weight = 3.0;        // LCD_NOISY_K1_WEIGHT | call | 3.0 | stream load model: weight of the longest K1 chain of noisy reads
    double noisy_k1_from = 150000.0;     // LCD_NOISY_K1_FROM | call | 150000 | ... from this many read-bases (reads x longest read) on
    bool group_debug = false;            // LCD_GROUP_DEBUG | call | unset | trace: the launch groups' stream assignment
    bool gate_debug = false;             // LCD_GATE_DEBUG | call | unset | trace: workgroups started behind the gates (synchronises the stream)
    // ---- a submission (lcd_host.cpp Submission) ----
    bool early = true;                   // LCD_EARLY | call | 1 | long certified-band K2 chains start before the anchor stage (0: never)
    bool no_prep_thread = false;         // LCD_NO_PREP_THREAD | call | unset | set: classes, order and arena layout on the calling thread
    bool anchor_seq = false;             // LCD_ANCHOR_SEQ | call | unset | set: K4 and K3 of the anchor stage one after the other in the shared arena
    bool strings_seq = false;            // LCD_STRINGS_SEQ | call | unset | set: the strings stage after the ref<->cons WFA stage on the leader's stream
    bool wfa_seq = false;                // LCD_WFA_SEQ | call | unset | set: the ref<->cons WFA classes on one stream
    bool spare_set = false; double spare_gb = 0.0; // LCD_SPARE_GB | call | 16 (32 for `is_ont`) | spare DP memory of a launch set; 0: a chain that runs out is re-run by the host
    int arena_slot_cus = 0;              // LCD_ARENA_SLOT_CUS | call | 0 | test switch: arena slots for this many CUs only, so that claims must wait (0: the device's CUs)
    long long solo_min = 20000;          // LCD_SOLO_MIN | process | 20000 | read-bases below which no chain is chosen as long (process: the long chains' output and arena blocks are kept between submissions)
    int solo_n = -1;                     // LCD_SOLO_N | process | CUs / 2 | the longest N chains of a submission count as long (process: as LCD_SOLO_MIN)
    bool arena_slots = true;             // LCD_ARENA_SLOTS | process | 1 | work arenas pooled per resident workgroup (0: one per chain) (process: the CU rank table and the slot flags are allocated once per device)
    bool anchor_wfa_seq = false;         // LCD_ANCHOR_WFA_SEQ | process | unset | set and not 0: K3's anchor classes on one stream (process: the side stream's buffers are grow-only)
    int dbg = 0;                         // LCD_DBG | call | 0 | test switches of the kernels (bit mask, LcdScoring.dbg); 32 with LCD_PROFILE_CHAINS: reads by widest interval
    int watchdog_s = 0;                  // LCD_WATCHDOG_S | call | 0 (30 s) | floor in seconds of the deadline after which a chain ends with LCD_ERR_WATCHDOG
    bool time_host = false;              // LCD_TIME_HOST | call | unset | trace: the host's timeline of a submission
    bool mem_debug = false;              // LCD_MEM_DEBUG | call | unset | trace: arenas and rounds of a submission
    bool cert_debug = false;             // LCD_CERT_DEBUG | call | unset | trace: chains sent back by the certified band
    bool retry_debug = false;            // LCD_RETRY_DEBUG | call | unset | trace: every chain that is run again, with its capacities
    bool placement = false;              // LCD_PLACEMENT | call | unset | trace: CU placement of the wide chains
    bool profile_chains = false;         // LCD_PROFILE_CHAINS | call | unset | trace: per-class phase ticks and the chains that end last
    const char *dump_chain = nullptr;    // LCD_DUMP_CHAIN | call | unset | file the reads of a failing chain are written to (tools/replay_chain.py)
    const char *chain_times = nullptr;   // LCD_CHAIN_TIMES | call | unset | file every chain's class, pool, start, end and ticks are written to (tools/occupancy.py)
    // ---- host threads, memory, input ----
    int host_team = kSwitchUnset;        // LCD_HOST_TEAM | call | min(8, CPUs / ranks on the host) | host threads per team of the short parallel loops, 1..32
    int arena_threads = kSwitchUnset;    // LCD_ARENA_THREADS | call | min(16, CPUs / ranks on the host) | host threads inside one lcd_batch_region_results_arena call
    double mem_fraction = 0.92;          // LCD_MEM_FRACTION | process | 0.92 | share of the device's HBM the grow-only buffers may take (process: the budget of a device is fixed when the device is first used)
    bool alloc_debug = false;            // LCD_ALLOC_DEBUG | call | unset | trace: every growth of a device buffer
    bool inflate_profile = false;        // LCD_INFLATE_PROFILE | call | unset | trace: tick counters of the device inflate

    uint64_t wfa_lds_max() const { return wfa_lds_max_kb == kSwitchUnset ? (uint64_t)wfa_buckets_kb.back() << 10 : (uint64_t)wfa_lds_max_kb << 10; }
    uint64_t wfa_block_bytes() const { return (uint64_t)wfa_block_kb << 10; }
    static HostSwitches from_env();
};

inline HostSwitches HostSwitches::from_env() {
    HostSwitches s;
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, auto &v) { if (const char *e = getenv(name)) v = (std::remove_reference_t<decltype(v)>)(sizeof(v) > 4 ? atoll(e) : atoi(e)); };
    auto real = [](const char *name, double &v) { if (const char *e = getenv(name)) v = atof(e); };
    auto not0 = [](const char *name, bool &v) { if (const char *e = getenv(name)) v = atoi(e) != 0; }; // on unless set to 0
    num("LCD_CERT", s.cert); num("LCD_CERT_SOLO_LEN", s.cert_solo_len); num("LCD_CERT_SYS", s.cert_sys); num("LCD_CERT_BAND", s.cert_band); num("LCD_CERT_RING", s.cert_ring);
    num("LCD_BAND_MARGIN", s.band_margin);
    num("LCD_SOLO_RL", s.solo_rl); s.solo_rl_set = set("LCD_SOLO_RL"); num("LCD_SOLO_MW", s.solo_mw); num("LCD_SOLO_CYC", s.solo_cyc); num("LCD_SOLO_CYC_MIN", s.solo_cyc_min);
    not0("LCD_SOLO_CAP", s.solo_cap);
    num("LCD_SOLO_KB", s.solo_kb); { int r = 148; for (int b : {8, 12, 16, 24, 32, 48, 64, 96, 148}) if (s.solo_kb <= b) { r = b; break; } s.solo_kb = r; } // (a value between two buckets -- 56 -- made the long chains' kernel end 3 s late: not understood, so not offered)
    num("LCD_ISO_RL", s.iso_rl); num("LCD_ISO_KB", s.iso_kb);
    num("LCD_LDS_CAP_KB", s.lds_cap_kb); if (s.lds_cap_kb < 0) s.lds_cap_kb = 8;
    num("LCD_RING_K", s.ring_k); if (!(s.ring_k >= 2 && (s.ring_k & (s.ring_k - 1)) == 0 && s.ring_k <= 32)) s.ring_k = 0;
    num("LCD_RING_K_LEN", s.ring_k_len); not0("LCD_RING_K_FREE", s.ring_k_free); num("LCD_RING_K_MAXLDS_KB", s.ring_k_maxlds_kb);
    num("LCD_RING16", s.ring16);
    if (set("LCD_CELL_SHRINK")) { num("LCD_CELL_SHRINK", s.cell_shrink); s.cell_shrink = std::max(1, s.cell_shrink); }
    num("LCD_NODE_HINT", s.node_hint); num("LCD_CELL_HINT", s.cell_hint);
    if (const char *e = getenv("LCD_WFA_BUCKETS_KB")) {
        std::vector<int> v;
        for (const char *p = e; *p;) { const int kb = atoi(p); if (kb > 0) v.push_back(kb); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        if (!v.empty()) { std::sort(v.begin(), v.end()); s.wfa_buckets_kb = v; }
    }
    num("LCD_WFA_LDS_MAX_KB", s.wfa_lds_max_kb); num("LCD_WFA_BLOCK_KB", s.wfa_block_kb); num("LCD_WFA_WIDE_KB", s.wfa_wide_kb); num("LCD_WFA_WIDE_MIN", s.wfa_wide_min);
    num("LCD_STREAMS", s.streams); s.streams = std::max(1, std::min(kMaxStreams, s.streams));
    real("LCD_GATE_FRAC", s.gate_frac); num("LCD_GATE512_KEEP", s.gate512_keep); real("LCD_NOISY_K1_WEIGHT", s.noisy_k1_weight); real("LCD_NOISY_K1_FROM", s.noisy_k1_from);
    s.group_debug = set("LCD_GROUP_DEBUG"); s.gate_debug = set("LCD_GATE_DEBUG");
    not0("LCD_EARLY", s.early);
    s.no_prep_thread = set("LCD_NO_PREP_THREAD"); s.anchor_seq = set("LCD_ANCHOR_SEQ"); s.strings_seq = set("LCD_STRINGS_SEQ"); s.wfa_seq = set("LCD_WFA_SEQ");
    s.spare_set = set("LCD_SPARE_GB"); real("LCD_SPARE_GB", s.spare_gb);
    if (set("LCD_ARENA_SLOT_CUS")) { num("LCD_ARENA_SLOT_CUS", s.arena_slot_cus); s.arena_slot_cus = std::max(1, s.arena_slot_cus); }
    num("LCD_SOLO_MIN", s.solo_min); num("LCD_SOLO_N", s.solo_n); not0("LCD_ARENA_SLOTS", s.arena_slots);
    if (const char *e = getenv("LCD_ANCHOR_WFA_SEQ")) s.anchor_wfa_seq = atoi(e) != 0;
    num("LCD_DBG", s.dbg); num("LCD_WATCHDOG_S", s.watchdog_s);
    s.time_host = set("LCD_TIME_HOST"); s.mem_debug = set("LCD_MEM_DEBUG"); s.cert_debug = set("LCD_CERT_DEBUG"); s.retry_debug = set("LCD_RETRY_DEBUG");
    s.placement = set("LCD_PLACEMENT"); s.profile_chains = set("LCD_PROFILE_CHAINS");
    s.dump_chain = getenv("LCD_DUMP_CHAIN"); s.chain_times = getenv("LCD_CHAIN_TIMES");
    num("LCD_HOST_TEAM", s.host_team); num("LCD_ARENA_THREADS", s.arena_threads);
    real("LCD_MEM_FRACTION", s.mem_fraction);
    s.alloc_debug = set("LCD_ALLOC_DEBUG"); s.inflate_profile = set("LCD_INFLATE_PROFILE");
    // the process-lifetime switches: what the first call of the process read
    static const HostSwitches first = s;
    s.wfa_buckets_kb = first.wfa_buckets_kb; s.streams = first.streams; s.solo_min = first.solo_min; s.solo_n = first.solo_n; s.arena_slots = first.arena_slots;
    s.anchor_wfa_seq = first.anchor_wfa_seq; s.mem_fraction = first.mem_fraction;
    return s;
}

} // namespace lcd_internal
