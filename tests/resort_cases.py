"""Chains built for the RARE paths of the POA kernel's incremental re-sort (poa_kernel.hip topo_sort_incremental): graphs whose Kahn FIFO holds two live branches
for tens of rows, so that the walk it replays from a cut of the old order runs 13 - 64 rows, leaves its 64-row window, or finds no cut within 256 rows.

Every other input of the suite asks the walk for at most a dozen rows (the census of oracle/poa.c, pyoracle.poa_resort_census; tests/test_resort_cases_oracle.py
holds that converse).  The generators:

  divergent_chain  two haplotypes that differ over a stretch of d bases with NO base in common (h1 over {A, C}, h2 over {G, T}): from d = 8 on two gaps cost less
                   than d mismatches, the graph carries two parallel branches, and there is no cut for 2 d + 1 rows (the cut before the stretch to the last popped row of the stretch, both counted).  Late reads each add one small thing inside
                   the stretch, on either branch: a SNP, a third and a fourth allele, a deletion or an insertion of 1 - 3 bases, at its first base, its middle, its last
  feature_chain    one backbone with a 200-base stretch of that kind, nodes of five and six out-edges / in-edges, 100-base deletion edges whose far end is a plain
                   node and an aligned ring, insertions of 80 / 100 / 130 bases, rings of up to five nodes, an edges-only and a weights-only read
  over_ml_chain    a late read with more places than the kernel's `ml` list holds (INC_ML), from few enough new nodes to get that far
  over_seg_chain   a late read with more pieces than its pieces' table holds (INC_SEG) but fewer places than INC_ML

Everything is seeded, pure numpy, and returns reads only.  CASES is the table the CPU test (census minimums, planned class) and the GPU test
(tests/test_gpu_poa_resort.py: parity with the oracle under every environment of the row) share; oracle results are computed once per (reads, mode) and cached."""
import numpy as np

import tie_cases as T

_u8 = T._u8
_edit = T._edit


def _snp(h, pos, base):
    r = h.copy(); r[pos] = base
    return r


def _stretch(rng, h1, h2, s, d):
    """h1[s:s + d] over {A, C}, h2[s:s + d] over {G, T}; the base before the stretch differs from both branches' last base and the base behind it from both
    branches' first, so that neither gap can slide over a flank base (a slid gap puts matched bases between the two gaps: one branch after the other, no FIFO
    of two)"""
    h1[s:s + d] = rng.integers(0, 2, d)
    h2[s:s + d] = rng.integers(2, 4, d)
    h1[s - 1] = h2[s - 1] = min(set(range(4)) - {int(h1[s + d - 1]), int(h2[s + d - 1])})
    h1[s + d] = h2[s + d] = min(set(range(4)) - {int(h1[s]), int(h2[s])})


def divergent_pair(rng, L, d, snp_every=40):
    """h1, h2 and the stretch's first base: iid bases, h1[s:s + d] over {A, C}, h2[s:s + d] over {G, T}, a SNP every `snp_every` bases outside the stretch"""
    s = (L - d) // 2
    h1 = rng.integers(0, 4, L).astype(np.uint8)
    h2 = h1.copy()
    sites = [p for p in range(15, L - 15, snp_every) if p < s - 8 or p >= s + d + 8]
    h2[sites] = (h1[sites] + 1) % 4
    _stretch(rng, h1, h2, s, d)
    return h1, h2, s


def divergent_chain(rng, L, d, n_found=6):
    """n_found founding reads alternating h1 / h2, then per branch ten late reads with ONE change inside the stretch each -- SNPs at its first, its last and its
    middle base (there a third and a fourth allele), deletions of 1 / 2 / 3 bases at its start, its middle and its end, insertions of 1 / 2 / 3 bases likewise --
    and two reads that repeat an earlier change (weights only): n_found + 22 reads"""
    h1, h2, s = divergent_pair(rng, L, d)
    reads = [(h1 if i % 2 == 0 else h2).copy() for i in range(n_found)]
    first, mid, last = s, s + d // 2, s + d - 1
    for h, lo in ((h1, 0), (h2, 2)):
        other = lambda p: lo + (1 - (int(h[p]) - lo))          # the branch's own other base
        reads.append(_snp(h, first, other(first)))
        reads.append(_snp(h, last, other(last)))
        reads.append(_snp(h, mid, other(mid)))                # a third allele at the middle row ...
        reads.append(_snp(h, mid, 2 - lo))                     # ... and a fourth (a base of the other branch's alphabet)
        reads.append(_edit(h, dels=[(first, 1)]))
        reads.append(_edit(h, dels=[(mid, 2)]))
        reads.append(_edit(h, dels=[(last - 2, 3)]))
        reads.append(_edit(h, ins=[(first, rng.integers(lo, lo + 2, 1))]))
        reads.append(_edit(h, ins=[(mid, rng.integers(lo, lo + 2, 2))]))
        reads.append(_edit(h, ins=[(last + 1, rng.integers(lo, lo + 2, 3))]))
    reads += [reads[n_found + 2].copy(), reads[n_found + 15].copy()]
    return reads


# feature_chain's landmarks (backbone positions; L >= 870, and the longest read is L + 130 bases: 1 000 at L = 870 stays in the 256-thread class of the full rows)
F_STRETCH, F_D = 40, 200          # the divergent stretch
F_OUT, F_IN = 312, 387             # the node the deletions of 3 / 5 / 7 / 9 (and 11) bases start behind; the node those of 3 / 5 / 7 / 9 bases end at
F_DEL_PLAIN = (437, 100)           # a 100-base deletion whose far end (537) is a plain node
F_DEL_RING = (612, 88)             # ... and one whose far end (700) is a SNP site: an aligned ring
F_INS = (735, 765, 795, 830)       # a 100-base insertion; two 40-base insertions in one read; a 130-base insertion
F_DEL2 = 712                       # a 2-base deletion: the edges-only read


def feature_sites(L):
    return [p for p in range(250, L - 20, 25)]


def feature_chain(rng, L=870):
    """24 reads over one backbone, see the module docstring and the landmarks above"""
    assert L >= 870
    h1 = rng.integers(0, 4, L).astype(np.uint8)
    h2 = h1.copy()
    sites = feature_sites(L)
    h2[sites] = (h1[sites] + 1) % 4
    s, d = F_STRETCH, F_D
    _stretch(rng, h1, h2, s, d)
    for p, n in (F_DEL_PLAIN, F_DEL_RING):                     # (the long deletions cannot slide: their far end is the node meant)
        h1[p + n - 1] = h2[p + n - 1] = (h1[p - 1] + 1) % 4
        h1[p] = h2[p] = min(set(range(4)) - {int(h1[p + n]), int(h2[p + n])})
    third, fourth, withn = h1.copy(), h2.copy(), h1.copy()
    third[sites] = (h1[sites] + 2) % 4
    fourth[sites] = (h1[sites] + 3) % 4
    withn[sites] = 4
    A, B = F_OUT, F_IN
    new = lambda n: rng.integers(0, 4, n)
    alt = lambda h, p: (int(h[p]) + 2) % 4                     # (a base neither haplotype has at a plain position)
    reads = [h1.copy(), h2.copy(), h1.copy(), h2.copy()]
    # deletions that all start behind node A / all end at node B; the two 100-base deletions; the long insertions
    reads.append(_edit(h1, dels=[(A + 1, 3), (B - 3, 3), F_DEL_PLAIN]))
    reads.append(_edit(h2, dels=[(A + 1, 5), (B - 5, 5), F_DEL_RING]))
    reads.append(_edit(h1, dels=[(A + 1, 7), (B - 7, 7)], ins=[(F_INS[0], new(100))]))
    reads.append(_edit(h2, dels=[(A + 1, 9), (B - 9, 9)], ins=[(F_INS[1], new(40)), (F_INS[2], new(40))]))
    reads.append(_edit(h1, ins=[(F_INS[3], new(130))]))
    reads += [third, fourth, withn]                            # rings of three, four and five nodes at every SNP site
    reads.append(_edit(h1, dels=[(A + 1, 11)]))                # a sixth out-edge of A
    # late reads: one small thing each inside a span that holds the feature
    for h in (h1, h2):
        for off in (20, 180):
            reads.append(_snp(h, s + off, (0 if h is h2 else 2) + int(h[s + off]) % 2))     # a base of the other branch's alphabet, 20 and 180 bases into the stretch
    reads.append(_snp(_snp(h1, A + 1, alt(h1, A + 1)), B, alt(h1, B)))                      # a new edge out of A; a new member of B's ring (B itself in the span)
    reads.append(_snp(_snp(h2, A, alt(h2, A)), B - 1, alt(h2, B - 1)))                      # the row before each of the two
    reads.append(_snp(_snp(h1, B + 1, alt(h1, B + 1)), F_DEL_PLAIN[0], alt(h1, F_DEL_PLAIN[0])))     # a new edge out of B; one out of the row the plain 100-base deletion starts at
    reads.append(_snp(h2, F_DEL_RING[0], alt(h2, F_DEL_RING[0])))                           # ... and out of the row the other one starts at
    reads.append(_edit(h1, dels=[(F_DEL2, 2)]))                   # edges only
    reads.append(h1.copy())                                    # weights only
    reads.append(reads[13].copy())                             # an earlier change once more
    return reads


def inc_limits(lds_bytes):
    """the sizes of topo_sort_incremental's lists from the chain's LDS pool (poa_kernel.hip lines 953 - 954; the pool's words are lds_bytes / 4, INC_Q + 8 = 40 of
    them are the FIFO and its guard):
        inc_free = pool_words - INC_Q - 8
        INC_ML  = min(1024, inc_free / 8)
        INC_SEG = min(512, inc_free * 3 / 8 / 6)
        INC_EL  = min(4096, inc_free - INC_ML - 6 * INC_SEG)"""
    inc_free = lds_bytes // 4 - 40
    ml, seg = min(1024, inc_free // 8), min(512, inc_free * 3 // 8 // 6)
    return dict(INC_ML=ml, INC_SEG=seg, INC_EL=min(4096, inc_free - ml - 6 * seg))


def over_ml_chain(rng, inc_ml, n_found=4):
    """a late read with more places than INC_ML from at most 120 new nodes (128 are refused before the list is written): SNPs every third base, two places each (the
    new edge's source and the row before the ring that grew), and, while those are not enough, one-base deletions every third base behind them (one place each)"""
    n_snp = min(120, inc_ml // 2 + 4)
    n_del = max(0, inc_ml + 8 - 2 * n_snp)
    L = 20 + 3 * n_snp + 3 * n_del + 20
    h = rng.integers(0, 4, L).astype(np.uint8)
    at = 20 + 3 * np.arange(n_snp)
    same = np.flatnonzero(h[1:] == h[:-1]) + 1
    h[same] = (h[same] + 1) % 4; same = np.flatnonzero(h[1:] == h[:-1]) + 1; h[same] = (h[same] + 2) % 4     # (no two equal neighbours: a deleted base has one place)
    late = h.copy()
    late[at] = (h[at] + 1 + rng.integers(0, 3, n_snp)) % 4
    late = _edit(late, dels=[(21 + 3 * n_snp + 3 * i, 1) for i in range(n_del)])
    return [h.copy() for _ in range(n_found)] + [late, h.copy()]


def over_seg_chain(rng, inc_seg, n_found=4):
    """a late read of inc_seg + 8 isolated one-base deletions, 4 or 5 bases apart: one place and one piece each"""
    n_del = inc_seg + 8
    gaps = rng.integers(4, 6, n_del)
    pos = 20 + np.cumsum(gaps)
    L = int(pos[-1]) + 20
    h = rng.integers(0, 4, L).astype(np.uint8)
    same = np.flatnonzero(h[1:] == h[:-1]) + 1
    h[same] = (h[same] + 1) % 4; same = np.flatnonzero(h[1:] == h[:-1]) + 1; h[same] = (h[same] + 2) % 4     # (no two equal neighbours: a deleted base has one place)
    late = _edit(h, dels=[(int(p), 1) for p in pos])
    return [h.copy() for _ in range(n_found)] + [late, h.copy()]




# ---------------------------------------------------------------- the case table
FULL = {"LCD_CERT": "0"}
CERT = {"LCD_CERT": "1"}
SYS = {"LCD_CERT_SYS": "1"}
GENERATORS = {"divergent": divergent_chain, "feature": feature_chain, "over_ml": over_ml_chain, "over_seg": over_seg_chain}
LIMIT_OF = {"over_ml": "INC_ML", "over_seg": "INC_SEG"}


def _also(env, full=False):
    """the further environments of every row: the incremental re-sort off (LCD_DBG=1024), and the full re-sort's other layouts for the reads it refuses (64: never
    the compact LDS copy; 384: the compact copy wherever it fits, with a FIFO of three nodes); the full rows' generic variant (8) where the row has full rows"""
    out = [dict(env, LCD_DBG=v) for v in ("1024", "64", "384")]
    return out + ([dict(env, LCD_DBG="8")] if full else [])


def _case(name, mode, gen, args, planned, tag, seed=0, is_ont=0, env=None):
    """gen / args / seed: the generator call (a limit chain's size argument comes from the planner's probe, see limit_chain); planned: what the probe must report
    under `env`; tag: the census minimums of the row's class -- a third of what the census measures on the chain, rounded down, never below 1
    (profiles/NOTES_resort_cases.md has the measured values); seed: the smallest for which the minimums hold in that mode"""
    env = env or {}
    return dict(name=name, mode=mode, gen=gen, args=args, seed=seed, is_ont=is_ont, scoring={}, env=env, planned=planned, tag=tag, also=_also(env, full=env.get("LCD_CERT") == "0"))


K2C = dict(threads=64, wmax=512, cert=1, ring16=1, solo=0)      # K2, certified band, one wavefront
K2F = dict(threads=256, wmax=1024, cert=0)                      # K2, full rows, the 256-thread class (longest read 511 - 1 022 bases)
K1A = dict(threads=64, wmax=64, cert=0)                         # K1, 64-column window
K1B = dict(threads=64, wmax=128, cert=0)                        # K1, 128-column window (longest read from 1 400 bases)


ONT_A = dict(threads=128, cert=2)                               # K2, noisy reads, the band in the systolic rows (LCD_CERT_SYS=1), by the longest read
ONT_B = dict(threads=256, cert=2)
# census minimums of the feature chain (L = 870; ring_grew / fan_out4 / ring3_in_span grow with the number of SNP sites, so the row of L = 1 500 asks for twice as many)
FEATURE_TAG = dict(no_cut_256=1, span_over_64=2, fan_out4=34, fan_in4=1, far_target=2, far_target_ring=1, new_65_128=1, new_over_128=1, ring_grew=35, edges_only=1,
                   ring3_in_span=48)


def _cases():
    c = []
    # divergent stretches, K2 over the certified band: 2 d + 1 rows without a cut, more once late reads have added rows to the stretch
    #   d = 8, 12: every place inside the stretch in 13 - 52 rows; 24: both sides of 52; 26 - 31: the last rows of the 64-row window and beyond; 32, 40: beyond from
    #   the first late read on (the class that must refuse); 130: no cut within 256 rows for the places deep in the stretch, and one read of more than 128 new nodes
    div = {8: dict(span_13_52=8), 12: dict(span_13_52=9), 24: dict(span_13_52=3, span_53_64=5), 26: dict(span_53_64=8), 28: dict(span_53_64=6, span_over_64=2),
           30: dict(span_53_64=3, span_over_64=5), 31: dict(span_53_64=1, span_over_64=7), 32: dict(span_over_64=8), 40: dict(span_over_64=9),
           130: dict(span_over_64=8, no_cut_256=2, new_over_128=1)}
    for d, tag in div.items():
        c.append(_case(f"k2_cert_div_{d}", 1, "divergent", dict(L=400 if d < 100 else 500, d=d), K2C, dict(tag, ring_grew=5, edges_only=2), env=CERT))
    # ... K2 with full rows in the 256-thread class (600-base reads; the pool is 32 KB: lists four times as long)
    for d in (12, 30, 32, 130):
        c.append(_case(f"k2_full_div_{d}", 1, "divergent", dict(L=600, d=d), K2F, dict(div[d], ring_grew=6, edges_only=2), env=FULL))
    # ... noisy reads, and K1 with the 64- and the 128-column window
    c.append(_case("k2_ont_sys_div_28", 1, "divergent", dict(L=400, d=28), ONT_A, div[28], is_ont=1, env=SYS))
    for d in (12, 30, 40):
        c.append(_case(f"k1_w64_div_{d}", 0, "divergent", dict(L=400, d=d), K1A, div[d]))
    c.append(_case("k1_w128_div_24", 0, "divergent", dict(L=1500, d=24), K1B, div[24]))
    # the feature chain in every class
    c.append(_case("k2_cert_feature", 1, "feature", dict(L=870), K2C, FEATURE_TAG, env=CERT))
    c.append(_case("k2_full_feature", 1, "feature", dict(L=870), K2F, FEATURE_TAG, env=FULL))
    c.append(_case("k2_ont_sys_feature", 1, "feature", dict(L=870), ONT_B, FEATURE_TAG, is_ont=1, env=SYS))
    c.append(_case("k1_w64_feature", 0, "feature", dict(L=870), K1A, FEATURE_TAG))
    c.append(_case("k1_w128_feature", 0, "feature", dict(L=1500), K1B, dict(FEATURE_TAG, fan_out4=69, ring_grew=70, ring3_in_span=100)))
    # the two limit chains, in the two classes whose pool is small enough for a read of at most 128 new nodes to outgrow the lists (8 KB: INC_ML 251, INC_SEG 125;
    # the 32 KB pool of the 256-thread class holds 1 019 places, more than a read of that class's length has room for)
    c.append(_case("k2_cert_over_ml", 1, "over_ml", {}, K2C, dict(new_65_128=1), env=CERT))
    c.append(_case("k2_cert_over_seg", 1, "over_seg", {}, K2C, dict(edges_only=1), env=CERT))
    c.append(_case("k1_w64_over_ml", 0, "over_ml", {}, K1A, dict(new_65_128=1)))
    c.append(_case("k1_w64_over_seg", 0, "over_seg", {}, K1A, dict(edges_only=1)))
    return c


CASES = _cases()
_reads, _oracle, _plan_lib = {}, {}, []


class _environment:
    """the LCD_* environment is exactly `env` inside the block (the planner reads its switches per call)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        import os
        self.saved = {k: v for k, v in os.environ.items() if k.startswith("LCD_")}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.env)

    def __exit__(self, *exc):
        import os
        for k in [k for k in os.environ if k.startswith("LCD_")]:
            del os.environ[k]
        os.environ.update(self.saved)
        return False


def probe_plan(case, reads):
    """the planner's probe (chain_plan_cases.probe) for `reads` in the class of `case`, as a dict over CHAIN_OUT"""
    import chain_plan_cases as P
    if not _plan_lib:
        from longcalld_amd import _lib
        _plan_lib.append(P.open_lib(_lib.LIB_PATH))
    entry = P.chain(case["name"], case["mode"], 0, 0, lens=[len(r) for r in reads], ont=case["is_ont"], n_chains=1 << 40, env=case["env"])
    with _environment(case["env"]):
        return dict(zip(P.CHAIN_OUT, P.probe(_plan_lib[0], entry)))


def limit_chain(case):
    """the reads of a limit row: the generator is given the list size that follows from the pool the planner's probe reports FOR THE CHAIN IT RETURNS (the pool
    grows with the longest read, so: build for the smallest pool, probe, build again until the size stands)"""
    size = inc_limits(8192)[LIMIT_OF[case["gen"]]]
    for _ in range(6):
        reads = GENERATORS[case["gen"]](np.random.default_rng(case["seed"]), size, **case["args"])
        now = inc_limits(probe_plan(case, reads)["lds_bytes"])[LIMIT_OF[case["gen"]]]
        if now == size:
            return reads
        size = now
    raise AssertionError((case["name"], size))


def chain_reads(case):
    k = (case["gen"], tuple(sorted(case["args"].items())), case["seed"]) + ((case["mode"], case["is_ont"], tuple(sorted(case["env"].items()))) if case["gen"] in LIMIT_OF else ())
    if k not in _reads:
        _reads[k] = limit_chain(case) if case["gen"] in LIMIT_OF else GENERATORS[case["gen"]](np.random.default_rng(case["seed"]), **case["args"])
    return _reads[k]


def oracle_chain(reads, mode):
    """-> (the oracle's K1 (mode 0, every read full-cover) or K2 (mode 1) chain, its re-sort census)"""
    from oracle import pyoracle
    with pyoracle.poa_resort_census() as rc:
        res = pyoracle.poa_aln_msa_cons(reads, 2) if mode == 1 else pyoracle.poa_partial_aln_msa_cons(reads, [12] * len(reads))
    return res, rc.counts


def case_oracle(case):
    """-> (the oracle's chain for the case, its re-sort census), computed once per (reads, mode) and never changed"""
    reads = chain_reads(case)
    k = (id(reads), case["mode"])
    if k not in _oracle:
        _oracle[k] = oracle_chain(reads, case["mode"])
    return _oracle[k]


def plan_case(case):
    """the chain_plan_cases entry of a case: poa_batch plans without a submission around the chain (n_chains = 2^40)"""
    import chain_plan_cases as P
    return P.chain(case["name"], case["mode"], 0, 0, lens=[len(r) for r in chain_reads(case)], ont=case["is_ont"], n_chains=1 << 40, env=case["env"])


def census_line(census):
    from oracle import pyoracle
    return " ".join(f"{k}={census[k]}" for k in pyoracle.RESORT_KINDS)
