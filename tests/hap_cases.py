"""K5 test inputs (hap_kernel.hip vs oracle/assign_hap.c): a problem builder with explicit control of what jobs.make_hap_problem fixes -- span
lengths, the per-variant category mix, n_alle, an observed-allele alphabet that includes 2, depths derived from the reads or set by hand -- and the
named cases built with it.  tests/test_hap_cases_oracle.py proves on the CPU, from the oracle's branch counters, that every case reaches the branch
it is named for; tests/test_gpu_hap.py runs the same cases through the kernel.  Problems use the dict layout of jobs.make_hap_problem."""
import functools

import numpy as np

from longcalld_amd.jobs import CLEAN_HET_SNP, CLEAN_HET_INDEL, CLEAN_HOM_VAR, NOISY_HET, NOISY_HOM, NON_VAR, GERMLINE_CLEAN, GERMLINE_ALL

CATES = (CLEAN_HET_SNP, CLEAN_HET_INDEL, CLEAN_HOM_VAR, NOISY_HET, NOISY_HOM, NON_VAR)
DEFAULT_MIX = (0.55, 0.1, 0.1, 0.12, 0.05, 0.08)
STATE_KEYS = ("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps", "var_phase_set", "hap_to_cons_alle", "hap_to_alle_profile")
SNP, INS, DEL = 8, 1, 2  # var_type: BAM_CDIFF, BAM_CINS, BAM_CDEL


def build(cate, vtype, is_hp, n_alle, reads, is_ont=0, skipped=None, var_pos=None, alle_covs=None, total_cov=None):
    """a problem from explicit arrays.  reads: one entry per read, None (no variant in its span: start -1, end -2 as src/bam_utils.c:30-31 leaves it)
    or (start_var_idx, [observed allele per variant of the span]); alleles are -2, -1 or an index below the variant's n_alle.  alle_covs / total_cov
    are counted from the non-skipped reads unless given.  cr_read is built as make_hap_problem builds it: non-skipped reads with a span, by start."""
    cate = np.asarray(cate, np.int32); V = len(cate); R = len(reads)
    vtype = np.asarray(vtype, np.int32); is_hp = np.asarray(is_hp, np.int32); n_alle = np.asarray(n_alle, np.int32)
    assert len(vtype) == len(is_hp) == len(n_alle) == V
    alle_off = np.concatenate([[0], np.cumsum(n_alle)]).astype(np.int32)
    skipped = np.zeros(R, np.uint8) if skipped is None else np.asarray(skipped, np.uint8)
    start = np.full(R, -1, np.int32); end = np.full(R, -2, np.int32); allele_off = np.zeros(R + 1, np.int32); alleles = []
    counted = np.zeros(int(alle_off[-1]), np.int32)
    for r, rd in enumerate(reads):
        if rd is not None:
            s, a = int(rd[0]), np.asarray(rd[1], np.int32)
            assert len(a) >= 1 and 0 <= s and s + len(a) <= V
            assert (a >= -2).all() and (a < n_alle[s:s + len(a)]).all()  # an allele index past n_alle would land in the next variant's profile row
            start[r], end[r] = s, s + len(a) - 1
            alleles.append(a)
            if not skipped[r]:
                ok = a >= 0
                np.add.at(counted, alle_off[s:s + len(a)][ok] + a[ok], 1)
        allele_off[r + 1] = allele_off[r] + (0 if rd is None else len(rd[1]))
    alleles = np.concatenate(alleles).astype(np.int32) if alleles else np.zeros(0, np.int32)
    alle_covs = counted if alle_covs is None else np.asarray(alle_covs, np.int32)
    assert len(alle_covs) == alle_off[-1]
    if total_cov is None:
        total_cov = np.array([alle_covs[alle_off[v]:alle_off[v + 1]].sum() for v in range(V)], np.int32)
    total_cov = np.asarray(total_cov, np.int32)
    if var_pos is None:
        var_pos = 1000 + 100 * np.arange(V)
    var_pos = np.asarray(var_pos, np.int64)
    assert len(total_cov) == len(var_pos) == V
    with_span = np.array([r for r in range(R) if start[r] >= 0 and not skipped[r]], np.int64)
    cr_read = with_span[np.argsort(start[with_span], kind="stable")].astype(np.int32) if len(with_span) else np.zeros(0, np.int32)
    return dict(n_reads=R, n_vars=V, is_ont=int(is_ont), var_pos=var_pos, var_type=vtype, var_cate=cate, is_homopolymer_indel=is_hp, total_cov=total_cov,
                alle_off=alle_off, alle_covs=alle_covs, start_var_idx=start, end_var_idx=end, allele_off=allele_off, alleles=alleles,
                ordered_read_ids=np.arange(R, dtype=np.int32), is_skipped=skipped, cr_read=cr_read)


def random_case(rng, n_vars, n_reads, spans, cate=None, cate_p=DEFAULT_MIX, vtype=None, is_hp=None, n_alle=None, p3=0.05, p_true2=0.5, p_hp=0.15, err=0.02,
                p_lowq=0.02, p_minus2=0.01, p_switch=0.0, is_ont=0, p_skip=0.03, p_nospan=0.03, forced=(), total_cov=None):
    """a seeded two-haplotype problem.  spans: the span lengths (in variants) reads draw from, clipped to n_vars; forced: extra (start, span) reads.
    cate / vtype / is_hp / n_alle: explicit per-variant arrays, else drawn (cate from cate_p over CATES, 3 alleles with probability p3).  At a 3-allelic
    het variant allele 2 is the true allele of one haplotype with probability p_true2.  A read observes its haplotype's alleles with substitution errors
    inside the variant's own alphabet (err), low-quality (-1) and missing (-2) calls, and with probability p_switch changes haplotype once inside its span."""
    V = n_vars
    if cate is None:
        cate = rng.choice(CATES, V, p=cate_p)
    cate = np.asarray(cate, np.int32)
    if vtype is None:
        vtype = np.where(cate == CLEAN_HET_SNP, SNP, np.where(cate == CLEAN_HET_INDEL, rng.choice([INS, DEL], V), rng.choice([SNP, INS, DEL], V)))
    vtype = np.asarray(vtype, np.int32)
    if is_hp is None:
        is_hp = (vtype != SNP) & (rng.random(V) < p_hp)
    if n_alle is None:
        n_alle = np.where(rng.random(V) < p3, 3, 2)
    n_alle = np.asarray(n_alle, np.int32)
    hom = np.isin(cate, [CLEAN_HOM_VAR, NOISY_HOM])
    h1 = rng.integers(0, 2, V)
    truth = np.stack([np.where(hom, 1, h1), np.where(hom, 1, 1 - h1)])
    for v in np.flatnonzero((n_alle == 3) & ~hom & (rng.random(V) < p_true2)):
        truth[rng.integers(0, 2), v] = 2
    spans = np.atleast_1d(np.asarray(spans))
    todo = [(int(rng.integers(0, V)), int(rng.choice(spans))) for _ in range(n_reads - len(forced))] if V else [(0, 0)] * (n_reads - len(forced))
    todo = sorted(todo + [(int(s), int(n)) for s, n in forced])
    reads = []
    for s, n in todo:
        if V == 0 or rng.random() < p_nospan:
            reads.append(None); continue
        e = min(V, s + max(1, n))
        hap = int(rng.integers(0, 2))
        a = truth[hap, s:e].copy()
        if e - s > 1 and rng.random() < p_switch:
            k = int(rng.integers(1, e - s))
            a[k:] = truth[1 - hap, s + k:e]
        wrong = (a + 1 + rng.integers(0, 2, e - s) % (n_alle[s:e] - 1)) % n_alle[s:e]
        a = np.where(rng.random(e - s) < err, wrong, a)
        q = rng.random(e - s)
        a = np.where(q < p_lowq, -1, np.where(q < p_lowq + p_minus2, -2, a))
        reads.append((s, a))
    skipped = (rng.random(len(reads)) < p_skip).astype(np.uint8)
    pos = np.sort(rng.choice(np.arange(1000, 1000 + max(V, 1) * 400), V, replace=False))
    return build(cate, vtype, is_hp, n_alle, reads, is_ont=is_ont, skipped=skipped, var_pos=pos, total_cov=total_cov)


def default_state(prob):
    R, V, TA = prob["n_reads"], prob["n_vars"], int(prob["alle_off"][-1])
    return dict(haps=np.zeros(R, np.int32), phase_sets=np.full(R, -1, np.int64), n_clean_agree_snps=np.zeros(R, np.int32),
                n_clean_conflict_snps=np.zeros(R, np.int32), var_phase_set=np.full(V, -1, np.int64), hap_to_cons_alle=np.full(V * 3, -1, np.int32),
                hap_to_alle_profile=np.zeros(3 * TA, np.int32))


def poisoned_state(prob, target):
    """a state no call would leave behind: every array holds a sentinel, so whatever the reference does not write must come back as it went in.  Rows
    of variants outside `target` carry a value that also depends on the variant, so a write that lands on a neighbour's row shows as well."""
    R, V, TA = prob["n_reads"], prob["n_vars"], int(prob["alle_off"][-1])
    off_target = (np.asarray(prob["var_cate"]) & target) == 0
    v = np.arange(V)
    st = dict(haps=np.full(R, 7, np.int32), phase_sets=np.full(R, -77, np.int64), n_clean_agree_snps=np.full(R, 31, np.int32),
              n_clean_conflict_snps=np.full(R, 41, np.int32), var_phase_set=np.where(off_target, -5500 - v, -55).astype(np.int64),
              hap_to_cons_alle=np.repeat(np.where(off_target, -900 - v, -9), 3).astype(np.int32), hap_to_alle_profile=np.full(3 * TA, 1234, np.int32))
    return st


def copy_state(st):
    return {k: st[k].copy() for k in STATE_KEYS}


# ---------------------------------------------------------------- the named cases ----------------------------------------------------------------
HET_ONLY = (0.7, 0.15, 0.0, 0.15, 0.0, 0.0)          # every variant het and in GERMLINE_ALL
LONG_SPANS = (63, 64, 65, 127, 128, 129, 200)


def third_allele_literal():
    """4 variants, 3 reads, target GERMLINE_ALL.  v0 clean het SNP, v1 noisy het SNP (score 1), v2 and v3 clean het SNPs with three alleles.
    r0 = [0, 0, 2, 2] is seeded first and becomes haplotype 1 with consensus [0, 0, 2, 2]; haplotype 2 has no consensus yet.  r1 = [1, 1, 2, 2]:
    v0 and v1 fill haplotype 2 with 1 - 0 = 1 and score (-2, +2), (-1, +1); at v2 and v3 the fill gives 1 - 2 = -1, so haplotype 2 scores 0 there
    (src/assign_hap.c:145) and haplotype 1 scores +2 twice: (1, 3) -> haplotype 2.  With -var_score instead of 0 the sums are (1, -1) -> haplotype 1.
    r2 = [1, 1] on v0..v1 follows haplotype 2 either way."""
    return build([CLEAN_HET_SNP, NOISY_HET, CLEAN_HET_SNP, CLEAN_HET_SNP], [SNP] * 4, [0] * 4, [2, 2, 3, 3],
                 [(0, [0, 0, 2, 2]), (0, [1, 1, 2, 2]), (0, [1, 1])], var_pos=[100, 200, 300, 400])


# what oracle/assign_hap.c must return for third_allele_literal from a default state with GERMLINE_ALL, worked out by hand (see the docstring above):
# one iteration, no flip, every variant in the phase set of v0; v2 and v3 end hom 2/2; plane 0 of the profile is zeroed, planes 1 and 2 count r0 and r1 + r2
THIRD_ALLELE_LITERAL_EXPECTED = dict(
    haps=[1, 2, 2], phase_sets=[100, 100, 100], n_clean_agree_snps=[3, 3, 1], n_clean_conflict_snps=[0, 0, 0], var_phase_set=[100, 100, 100, 100],
    hap_to_cons_alle=[1, 0, 1, 1, 0, 1, 2, 2, 2, 2, 2, 2],
    hap_to_alle_profile=[0] * 10 + [1, 0, 1, 0, 0, 0, 1, 0, 0, 1] + [0, 2, 0, 2, 0, 0, 1, 0, 0, 1])


def _seed_classes(rng):
    V, R = 140, 150
    snp, ind = np.full(V, SNP), rng.choice([INS, DEL], V)
    kw = dict(spans=(8, 20, 30), p_skip=0.02, p_nospan=0.02)
    out = {}
    out["seed_clean_indel"] = (random_case(rng, V, R, cate=np.full(V, CLEAN_HET_INDEL), vtype=ind, **kw), GERMLINE_CLEAN)
    out["seed_noisy_snp"] = (random_case(rng, V, R, cate=np.full(V, NOISY_HET), vtype=snp, **kw), GERMLINE_ALL)
    out["seed_noisy_indel"] = (random_case(rng, V, R, cate=np.full(V, NOISY_HET), vtype=ind, is_hp=np.zeros(V, int), **kw), GERMLINE_ALL)
    cate = rng.choice([NOISY_HET, CLEAN_HOM_VAR, NOISY_HOM], V, p=[0.5, 0.3, 0.2])
    out["seed_none_iterates"] = (random_case(rng, V, R, cate=cate, vtype=ind, is_hp=(cate == NOISY_HET).astype(int), **kw), GERMLINE_ALL)
    cate = np.full(V, CLEAN_HET_SNP); cate[:2] = NON_VAR
    out["seed_depth0"] = (random_case(rng, V, R, cate=cate, total_cov=np.zeros(V, int), **kw), GERMLINE_CLEAN)
    # equal maximal depth at valid[] indices 3, 4, 67, 131 (variant 1 is outside the target, so valid index i is variant i + 1): lanes 3 and 4 of the
    # first stride of 64 and lane 3 of the second and third -- index 3 must win
    cate = np.full(V, CLEAN_HET_SNP); cate[1] = NON_VAR
    cov = rng.integers(5, 40, V); cov[[4, 5, 68, 132]] = 50
    out["seed_tie_first"] = (random_case(rng, V, R, cate=cate, total_cov=cov, **kw), GERMLINE_CLEAN)
    cate = rng.choice(CATES, V, p=DEFAULT_MIX); cate[[0, V - 1]] = CLEAN_HET_SNP
    cov = rng.integers(5, 40, V); cov[V - 1] = 90
    out["seed_last"] = (random_case(rng, V, R, cate=cate, total_cov=cov, **kw), GERMLINE_CLEAN)
    cov = rng.integers(5, 40, V); cov[0] = 90
    out["seed_first"] = (random_case(rng, V, R, cate=cate, total_cov=cov, **kw), GERMLINE_CLEAN)
    return out


def ont_hp_threshold():
    """is_ont = 1.  v0..v5 clean het SNPs phase 200 reads of haplotype 1 (alleles 0) and 100 of haplotype 2 (alleles 1); v6..v8 are homopolymer indels,
    which take no part in the scoring, so their per-haplotype profile counts are exactly what the reads carry:
        v6: haplotype 1 134/200, haplotype 2 67/100     v7: 2/3 (197 reads uncalled), 66/100 (rejected)     v8: 1/1, 67/100"""
    n1, n2 = 200, 100
    def col(n, major, k, called=None):
        a = np.full(n, -1 if called is not None else 1 - major)
        m = n if called is None else called
        a[:m] = 1 - major; a[:k] = major
        return a
    h1 = np.stack([col(n1, 1, 134), col(n1, 1, 2, called=3), col(n1, 1, 1, called=1)], 1)
    h2 = np.stack([col(n2, 0, 67), col(n2, 0, 66), col(n2, 0, 67)], 1)
    reads = [(0, [0] * 6 + h1[i].tolist()) for i in range(n1)] + [(0, [1] * 6 + h2[i].tolist()) for i in range(n2)]
    order = np.random.default_rng(77).permutation(len(reads))     # all reads start at variant 0: any order is a start order
    return build([CLEAN_HET_SNP] * 6 + [CLEAN_HET_INDEL] * 3, [SNP] * 6 + [DEL] * 3, [0] * 6 + [1] * 3, [2] * 9, [reads[i] for i in order], is_ont=1)


def phase_flip_break():
    """40 clean het SNPs in four blocks A = v0..v11, B = v12..v23, C = v24..v31, D = v32..v39; haplotype 1 carries 0 on every variant.  The seed is v14
    (hand-set depth).  W = v9..v14 with A's 0s and B's 1s is first in start order among the reads over the seed, so the seeding pass joins A's 0s to
    B's 1s.  The reads over v8..v13 that come later say the opposite (three all-0, two all-1): they are out-voted in the profile of B, follow their
    four A variants and conflict at the pair (v11, v12) -> conflict 5 > agree 1, flip == 1 from v12 on.  One read joins B to C and none joins C to D,
    so v24 and v32 start new phase sets.  The reference's double swap leaves the alleles as they were, so the flip repeats in every iteration:
    this input runs into the cap of 10 iterations."""
    V = 40
    reads = []
    def block(lo, hi, n, span):
        for k in range(n):
            s = lo + (k * 3) % max(1, hi - lo - span + 1)
            reads.append((s, [k % 2] * span))
    block(0, 12, 24, 5); block(12, 24, 24, 5); block(24, 32, 12, 4); block(32, 40, 12, 4)
    reads.append((9, [0, 0, 0, 1, 1, 1]))                                  # W
    reads += [(8, [0] * 6)] * 3 + [(8, [1] * 6)] * 2                        # the later majority over (v11, v12)
    reads.append((22, [0, 0, 0, 0]))                                       # the only read over (v23, v24)
    reads.sort(key=lambda rd: rd[0])
    # W must be the first read in start order that overlaps the seed v14: block-B reads start at 12 or later, the v8 reads end at v13
    cov = np.full(V, 10); cov[14] = 60
    return build([CLEAN_HET_SNP] * V, [SNP] * V, [0] * V, [2] * V, reads, total_cov=cov)


def _degenerate(rng):
    out = {}
    p = random_case(rng, 30, 0, spans=(5,))
    out["no_reads"] = (p, GERMLINE_CLEAN)
    out["no_vars"] = (random_case(rng, 0, 12, spans=(5,)), GERMLINE_CLEAN)
    out["all_skipped"] = (random_case(rng, 30, 20, spans=(5, 9), p_skip=1.0), GERMLINE_CLEAN)
    out["one_var_one_read"] = (build([CLEAN_HET_SNP], [SNP], [0], [2], [(0, [1])]), GERMLINE_CLEAN)
    for n in (64, 65):
        cate = np.full(130, NON_VAR); cate[rng.choice(130, n, replace=False)] = rng.choice([CLEAN_HET_SNP, CLEAN_HET_INDEL, CLEAN_HOM_VAR], n, p=[0.7, 0.2, 0.1])
        out[f"valid_{n}_of_130"] = (random_case(rng, 130, 120, spans=(10, 30, 70), cate=cate), GERMLINE_CLEAN)
        p = random_case(rng, 50, n + 5, spans=(6, 12), p_skip=0.0, p_nospan=0.0)
        p["is_skipped"][[3, n]] = 1                      # n + 5 reads: two skipped, three without a span -> exactly n in cr_read
        reads = [None if r in (7, 20, n + 2) else (int(p["start_var_idx"][r]), p["alleles"][p["allele_off"][r]:p["allele_off"][r + 1]]) for r in range(n + 5)]
        p = build(p["var_cate"], p["var_type"], p["is_homopolymer_indel"], np.diff(p["alle_off"]), reads, skipped=p["is_skipped"], var_pos=p["var_pos"])
        assert len(p["cr_read"]) == n
        out[f"cr_{n}"] = (p, GERMLINE_CLEAN)
    return out


CASE_NAMES = ("third_allele_literal", "third_allele_seeded", "long_spans", "long_spans_interleaved", "seed_clean_indel", "seed_noisy_snp", "seed_noisy_indel",
              "seed_none_iterates", "seed_depth0", "seed_tie_first", "seed_last", "seed_first", "ont_hp_threshold", "phase_flip_break", "no_reads", "no_vars",
              "all_skipped", "one_var_one_read", "valid_64_of_130", "cr_64", "valid_65_of_130", "cr_65")


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """name -> (problem, target of the run from a poisoned state); built once per process, never modified by a test"""
    rng = np.random.default_rng(20240521)
    out = {"third_allele_literal": (third_allele_literal(), GERMLINE_ALL)}
    # 120 variants, 30 % of them 3-allelic with allele 2 true on one haplotype of half of those; short reads and 30 % noisy het variants (score 1) leave
    # haplotypes without a consensus next to a partner at allele 2.  Scoring that state -var_score instead of 0 rarely changes the final arrays (a read
    # needs several such variants to outweigh the rest of its span): this seed is one where it does, in both passes -- haps[87] ends 2 instead of 1
    out["third_allele_seeded"] = (random_case(np.random.default_rng(50), 120, 120, spans=(4, 8, 15), cate_p=(0.5, 0.1, 0.05, 0.3, 0.05, 0.0), p3=0.3, p_true2=0.5),
                                  GERMLINE_CLEAN)
    V = 260
    forced = [(0, 200), (V - 129, 129), (0, 65), (V - 64, 64)]
    p = random_case(rng, V, 70, spans=LONG_SPANS, cate_p=HET_ONLY, forced=forced, p_nospan=0.0, p_skip=0.02)
    out["long_spans"] = (p, GERMLINE_ALL)
    cate = p["var_cate"].copy(); cate[1::2] = NON_VAR          # same reads, every other variant outside the target: target and non-target lanes interleave
    reads = [(int(p["start_var_idx"][r]), p["alleles"][p["allele_off"][r]:p["allele_off"][r + 1]]) for r in range(p["n_reads"])]
    out["long_spans_interleaved"] = (build(cate, p["var_type"], p["is_homopolymer_indel"], np.diff(p["alle_off"]), reads, skipped=p["is_skipped"],
                                           var_pos=p["var_pos"]), GERMLINE_ALL)
    out.update(_seed_classes(rng))
    out["ont_hp_threshold"] = (ont_hp_threshold(), GERMLINE_CLEAN)
    out["phase_flip_break"] = (phase_flip_break(), GERMLINE_CLEAN)
    out.update(_degenerate(rng))
    assert tuple(out) == CASE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """~40 problems for one lcd_assign_hap_batch call: every crafted case plus small seeded ones, shuffled, each with its own target.  Some targets
    leave a problem without a valid variant (the noisy-only and no-variant cases under GERMLINE_CLEAN): those blocks return at once."""
    rng = np.random.default_rng(4242)
    noisy_only = ("seed_noisy_snp", "seed_noisy_indel")     # nothing valid under GERMLINE_CLEAN
    probs = [(p, GERMLINE_CLEAN if name in noisy_only else None) for name, (p, _) in crafted_cases().items()]
    while len(probs) < 40:
        ont = int(rng.integers(0, 2))
        probs.append((random_case(rng, int(rng.integers(5, 90)), int(rng.integers(5, 90)), spans=np.arange(1, 40), is_ont=ont, p3=0.2, err=0.05 if ont else 0.02), None))
    probs.append((random_case(rng, 25, 30, spans=(4, 9), cate=np.full(25, NON_VAR)), None))       # no valid variant under either target
    probs = [probs[i] for i in rng.permutation(len(probs))]
    targets = [t if t is not None else (GERMLINE_CLEAN if rng.random() < 0.5 else GERMLINE_ALL) for _, t in probs]
    return [p for p, _ in probs], targets


SWEEP_SEED = 3
SWEEP_N = 256


@functools.lru_cache(maxsize=None)
def sweep():
    """256 small seeded problems for one launch: n_vars 1..140, n_reads 0..120, spans 1..130, alleles {-2, -1, 0, 1, 2}, a random category mix with the
    all-hom and all-non-target corners, random technology, 5 % skipped and 5 % span-less reads, a per-problem target"""
    rng = np.random.default_rng(SWEEP_SEED)
    probs, targets = [], []
    for i in range(SWEEP_N):
        V, R = int(rng.integers(1, 141)), int(rng.integers(0, 121))
        corner = rng.random()
        if corner < 0.04:
            mix = (0, 0, 0.6, 0, 0.4, 0)                # all hom
        elif corner < 0.08:
            mix = (0, 0, 0, 0, 0, 1)                    # all outside the target
        elif corner < 0.16:
            mix = (0, 0.3, 0.2, 0.4, 0.1, 0)            # no clean het SNP: the seed comes from a fallback class
        elif corner < 0.22:
            mix = (0, 0, 0.2, 0.7, 0.1, 0)              # noisy het only: class 2 or 3, or none
        else:
            mix = rng.dirichlet(np.ones(6))
        long_reads = rng.random() < 0.3
        vtype = rng.choice([INS, DEL], V) if 0.16 <= corner < 0.19 else None        # noisy het indels only: class 3, or no seed if all are homopolymer
        probs.append(random_case(rng, V, R, spans=np.arange(1, 131) if not long_reads else np.arange(60, 131), cate_p=mix, vtype=vtype, p3=float(rng.choice([0.05, 0.3])),
                                 err=float(rng.choice([0.02, 0.1, 0.3])), p_switch=float(rng.choice([0.0, 0.3])), is_ont=int(rng.integers(0, 2)),
                                 p_hp=float(rng.choice([0.15, 0.6])), p_skip=0.05, p_nospan=0.05))
        targets.append(GERMLINE_CLEAN if rng.random() < 0.4 else GERMLINE_ALL)
    return probs, targets
