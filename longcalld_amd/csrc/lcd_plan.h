// lcd_plan.h -- the planner of lcd_plan.cpp as lcd_host_internal.h declares it (that header includes this one).  Kept apart from it for one reason: these
// declarations need no HIP header, so lcd_plan.cpp can be read -- and compiled -- without one.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/lcd_hotpath.h"
#include "lcd_types.h"
#include "lcd_switches.h"

namespace lcd_internal __attribute__((visibility("hidden"))) {

struct ChainRec {
    int region, clu;              // clu: hap-1 for K1, 0 for K2 (clusters come out of the kernel)
    int mode;
    std::vector<int> members;     // indices into the region's sorted read list
    int read0;                    // first PoaRead
    int cert_fail_round = -1;     // K2: the last round in which the certified band did not fit its class's window (the chain then moves one class up)
    int solo = -1;                // -1: by the fixed threshold (LCD_SOLO_RL); 0 / 1: decided for the submission at hand (lcd_host.cpp choose_long_chains: the longest chains of what is in flight)
    int cert_level = -1;          // -1: not chosen yet; 1: certified band in the single-wavefront rows; 2: in the systolic rows of the class the reads' length asks for (noisy reads); 0: full rows
};
// the learned levels (0..2 each) as the planner sees them: whoever calls it loads the global atomics of lcd_host.cpp into one of these (learned_hints())
struct PlanHints { int cell[2] = {0, 0}, node = 0, wfa = 0; }; // DP cells per mode (K1, K2); graph capacity; score bound of the anchor stage's WFA jobs

// POA chains
void chain_caps(const lcd_opt_t &opt, const ChainRec &C, const std::vector<PoaRead> &preads, int scale, long long n_chains, const HostSwitches &sw, const PlanHints &hints, PoaChain &pc);
void chain_class(PoaChain &pc, bool noisy, const HostSwitches &sw);
int chain_threads(const PoaChain &pc);
long long chain_group_key(const PoaChain &pc);
struct LdsOverhead { int wave64, wider; };
constexpr LdsOverhead kSchedOverhead{1 * 1024, 6 * 1024}, kSlotOverhead{912, 6096}; // (why there are two: lcd_plan.cpp chains_per_cu)
int chains_per_cu(int lds, int thr, const LdsOverhead &besides);
int cert_next_level(const PoaChain &pc);
bool chain_goes_back(int status, const PoaChain &pc, ChainRec &CR, int round);
int retry_scale(const ChainRec &CR, int scale);
// WFA and edlib jobs
int wfa_default_scap(int plen, int tlen, int hint = 0); // hint: PlanHints.wfa for a job of the anchor stage, 0 for the clean ones (ref<->cons, segments)
void wfa_plan(WfaJob &j, const LcdScoring &sc, long long s_want, const HostSwitches &sw);
int wfa_class(const WfaJob &j, const LcdScoring &sc, const HostSwitches &sw); // 0: HBM ring, 1..: LDS bucket sw.wfa_buckets_kb[class - 1]
uint64_t wfa_out_bytes(const WfaJob &j);
uint64_t ed_arena_bytes(int qlen, int tlen);

} // namespace lcd_internal
