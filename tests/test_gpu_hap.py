"""K5 on the GPU (hap_kernel.hip through lcd_assign_hap_germline and lcd_assign_hap_batch) vs the oracle: every output array bit-identical.
The crafted cases come from tests/hap_cases.py; tests/test_hap_cases_oracle.py shows on the CPU which branch each of them reaches."""
import numpy as np
import pytest

import hap_cases as hc

pytestmark = pytest.mark.gpu

KEYS = ("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps", "var_phase_set", "hap_to_cons_alle", "hap_to_alle_profile")


def _same(a, b):
    for k in KEYS:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if not (x == y).all():
            i = int(np.flatnonzero(x != y)[0])
            raise AssertionError(f"{k}[{i}]: oracle {x[i]}, kernel {y[i]} ({int((x != y).sum())} of {x.size} differ)")   # all three profile planes included


@pytest.mark.parametrize("seed,nv,nr,ont,gap", [(1, 300, 400, 0, 0), (2, 240, 500, 0, 60), (3, 120, 900, 1, 0), (4, 700, 1000, 0, 0), (5, 30, 40, 0, 0)])
def test_hap_assignment_matches_oracle(lcd, oracle, seed, nv, nr, ont, gap):
    from longcalld_amd import jobs
    rng = np.random.default_rng(seed)
    p = jobs.make_hap_problem(rng, nv, nr, is_ont=ont, gap_every=gap, err=0.05 if ont else 0.02)
    exp = oracle.assign_hap_germline(p, jobs.GERMLINE_CLEAN)
    got = lcd.assign_hap_germline(p, jobs.GERMLINE_CLEAN)
    _same(exp, got)
    # second call on the carried-over state with all germline categories (src/collect_var.c:2972)
    exp = oracle.assign_hap_germline(p, jobs.GERMLINE_ALL, exp)
    got = lcd.assign_hap_germline(p, jobs.GERMLINE_ALL, got)
    _same(exp, got)


def test_hap_no_valid_vars(lcd):
    from longcalld_amd import jobs
    rng = np.random.default_rng(9)
    p = jobs.make_hap_problem(rng, 40, 50)
    p["var_cate"][:] = jobs.NON_VAR
    st = lcd.assign_hap_germline(p, jobs.GERMLINE_CLEAN)
    assert (st["haps"] == 0).all() and (st["phase_sets"] == -1).all()


def test_k5_reference_side_binding_roundtrip(oracle):
    """the stub a longcallD maintainer adds for assign_hap_based_on_germline_het_vars_kmeans (longcalld_amd/binding/)
    compiled against a header with the reference's field names, run on array-of-structs chunk state (cand_var_t / read_var_profile_t / cgranges
    intervals / bam_chunk_t arrays): flatten -> lcd_assign_hap_germline on the GPU -> write-back, twice as collect_var_main calls it (clean
    categories, then all germline categories) == the oracle's two calls"""
    import ctypes as C
    import os
    import subprocess
    from conftest import ROOT
    from longcalld_amd import jobs
    so = os.path.join(ROOT, "tests", "c", "libk5_roundtrip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "c")])
    lib = C.CDLL(so)
    i32p, i64p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    for seed, nv, nr, ont in [(11, 260, 420, 0), (12, 90, 300, 1)]:
        rng = np.random.default_rng(seed)
        p = jobs.make_hap_problem(rng, nv, nr, is_ont=ont, err=0.05 if ont else 0.02)
        exp = oracle.assign_hap_germline(p, jobs.GERMLINE_CLEAN)
        exp = oracle.assign_hap_germline(p, jobs.GERMLINE_ALL, exp)
        R, V, TA = p["n_reads"], p["n_vars"], int(p["alle_off"][-1])
        keep = {k: np.ascontiguousarray(p[k], np.int64 if k == "var_pos" else np.uint8 if k == "is_skipped" else np.int32)
                for k in ("var_pos", "var_type", "var_cate", "is_homopolymer_indel", "total_cov", "alle_off", "alle_covs", "start_var_idx", "end_var_idx",
                          "allele_off", "alleles", "ordered_read_ids", "is_skipped", "cr_read")}
        out = dict(haps=np.zeros(R, np.int32), phase_sets=np.full(R, -1, np.int64), agree=np.zeros(R, np.int32), conflict=np.zeros(R, np.int32),
                   var_ps=np.full(V, -1, np.int64), cons=np.full(3 * V, -1, np.int32), prof=np.zeros(3 * TA, np.int32))
        targets = np.array([jobs.GERMLINE_CLEAN, jobs.GERMLINE_ALL], np.int32)
        P = lambda a, t: a.ctypes.data_as(t)
        rc = lib.k5_roundtrip(R, V, int(p["is_ont"]), P(keep["var_pos"], i64p), P(keep["var_type"], i32p), P(keep["var_cate"], i32p),
                              P(keep["is_homopolymer_indel"], i32p), P(keep["total_cov"], i32p), P(keep["alle_off"], i32p), P(keep["alle_covs"], i32p),
                              P(keep["start_var_idx"], i32p), P(keep["end_var_idx"], i32p), P(keep["allele_off"], i32p), P(keep["alleles"], i32p),
                              P(keep["ordered_read_ids"], i32p), P(keep["is_skipped"], u8p), len(keep["cr_read"]), P(keep["cr_read"], i32p), 2, P(targets, i32p),
                              P(out["haps"], i32p), P(out["phase_sets"], i64p), P(out["agree"], i32p), P(out["conflict"], i32p), P(out["var_ps"], i64p),
                              P(out["cons"], i32p), P(out["prof"], i32p))
        assert rc == 0
        assert (out["haps"] == exp["haps"]).all() and (out["phase_sets"] == exp["phase_sets"]).all()
        assert (out["agree"] == exp["n_clean_agree_snps"]).all() and (out["conflict"] == exp["n_clean_conflict_snps"]).all()
        tgt = (keep["var_cate"] & jobs.GERMLINE_ALL) != 0     # variants outside the target categories keep NULL arrays in the reference
        assert (out["var_ps"][tgt] == exp["var_phase_set"][tgt]).all()
        assert (out["cons"].reshape(V, 3)[tgt] == exp["hap_to_cons_alle"].reshape(V, 3)[tgt]).all()
        assert (out["prof"][TA:] == exp["hap_to_alle_profile"][TA:]).all()


# ---------------- crafted cases (tests/hap_cases.py): long spans, third alleles, seed classes, thresholds, flips, degenerate sizes ----------------
@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_case_two_passes_from_default_state(lcd, oracle, name):
    """GERMLINE_CLEAN from the default state, then GERMLINE_ALL on the carried state, as collect_var_main calls it"""
    from longcalld_amd import jobs
    p, _ = hc.crafted_cases()[name]
    exp = oracle.assign_hap_germline(p, jobs.GERMLINE_CLEAN, hc.default_state(p))
    got = lcd.assign_hap_germline(p, jobs.GERMLINE_CLEAN, hc.default_state(p))
    _same(exp, got)
    exp = oracle.assign_hap_germline(p, jobs.GERMLINE_ALL, exp)
    got = lcd.assign_hap_germline(p, jobs.GERMLINE_ALL, got)
    _same(exp, got)


@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_case_from_poisoned_state(lcd, oracle, name):
    """every array starts as a sentinel: what the reference leaves untouched (rows of variants outside the target, skipped reads, everything if no
    variant is valid) must come back untouched from the device, and what it initialises must not depend on what was there"""
    p, target = hc.crafted_cases()[name]
    exp = oracle.assign_hap_germline(p, target, hc.poisoned_state(p, target))
    got = lcd.assign_hap_germline(p, target, hc.poisoned_state(p, target))
    _same(exp, got)


def test_third_allele_literal_by_hand(lcd):
    """4 variants, 3 reads (hap_cases.third_allele_literal): the first seeded read puts allele 2 on haplotype 1 at two 3-allelic SNPs; the second read
    goes to haplotype 2 only if haplotype 2, still without a consensus after the 1 - 2 = -1 fill, scores 0 there and not -var_score.  The expected
    arrays are written out by hand; with -var_score the kernel returns haps = [1, 1, 2]"""
    from longcalld_amd import jobs
    p = hc.third_allele_literal()
    got = lcd.assign_hap_germline(p, jobs.GERMLINE_ALL, hc.default_state(p))
    for k in KEYS:
        assert got[k].tolist() == hc.THIRD_ALLELE_LITERAL_EXPECTED[k], (k, got[k].tolist())


# ---------------- lcd_assign_hap_batch ----------------
def _oracle_states(oracle, probs, targets, states):
    return [oracle.assign_hap_germline(p, t, st) for p, t, st in zip(probs, targets, states)]


def test_batch_mixed_equals_single_calls_equals_oracle(lcd, oracle):
    """~40 problems of different sizes, technologies and targets in one launch, from poisoned states; problems without a valid variant for their target
    come back untouched while their neighbours are written; then a second batch call (GERMLINE_ALL) on the carried states"""
    from longcalld_amd import jobs
    probs, targets = hc.mixed_batch()
    poison = [hc.poisoned_state(p, t) for p, t in zip(probs, targets)]
    exp = _oracle_states(oracle, probs, targets, [hc.copy_state(s) for s in poison])
    got = lcd.assign_hap_batch(probs, targets, [hc.copy_state(s) for s in poison])
    single = [lcd.assign_hap_germline(p, t, hc.copy_state(s)) for p, t, s in zip(probs, targets, poison)]
    n_untouched = 0
    for i, (p, t) in enumerate(zip(probs, targets)):
        _same(exp[i], got[i])
        _same(exp[i], single[i])
        if ((p["var_cate"] & t) != 0).sum() == 0:
            _same(poison[i], got[i])
            n_untouched += 1
    assert n_untouched >= 3
    all_t = [jobs.GERMLINE_ALL] * len(probs)
    exp = _oracle_states(oracle, probs, all_t, exp)
    got = lcd.assign_hap_batch(probs, all_t, got)
    for i in range(len(probs)):
        _same(exp[i], got[i])


def test_batch_seeded_sweep_in_one_launch(lcd, oracle):
    """256 small seeded problems (hap_cases.sweep) as one batch, each compared with the oracle"""
    probs, targets = hc.sweep()
    exp = _oracle_states(oracle, probs, targets, [hc.default_state(p) for p in probs])
    got = lcd.assign_hap_batch(probs, targets, [hc.default_state(p) for p in probs])
    bad = []
    for i in range(len(probs)):
        try:
            _same(exp[i], got[i])
        except AssertionError as e:
            bad.append((i, str(e)))
    assert not bad, (len(bad), bad[:5])


def test_batch_is_deterministic(lcd):
    """the same mixed batch twice gives identical bytes: the kernel's atomics are integer adds, so any difference is a race"""
    probs, targets = hc.mixed_batch()
    runs = [lcd.assign_hap_batch(probs, targets, [hc.poisoned_state(p, t) for p, t in zip(probs, targets)]) for _ in range(2)]
    for a, b in zip(*runs):
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k
