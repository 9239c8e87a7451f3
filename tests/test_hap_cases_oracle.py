"""Are the K5 GPU cases aimed correctly?  Every case of tests/hap_cases.py is run through oracle/assign_hap.c with its branch counters switched on
(lcdo_hap_trace_t), and each case must reach the branch it is named for.  No GPU needed: this file says what tests/test_gpu_hap.py exercises."""
import numpy as np
import pytest

import hap_cases as hc
from longcalld_amd import jobs


def _trace(oracle, prob, target, state=None):
    return oracle.assign_hap_germline(prob, target, state or hc.default_state(prob), trace=True)


# case -> what its trace (default state, the case's target) must show
REACHES = {
    "third_allele_literal": lambda t, p: t["n_zero_after_fill"] >= 1 and t["n_cons_ge2"] >= 1,
    "third_allele_seeded": lambda t, p: t["n_cons_ge2"] >= 1 and t["n_zero_after_fill"] >= 1,
    "long_spans": lambda t, p: t["n_seed_gt64"] >= 5 and t["n_seed_gt128"] >= 3 and t["n_valid"] == p["n_vars"],
    "long_spans_interleaved": lambda t, p: t["n_seed_gt64"] >= 5 and t["n_seed_gt128"] >= 3 and t["n_valid"] == p["n_vars"] // 2,
    "seed_clean_indel": lambda t, p: t["seed_class"] == 1,
    "seed_noisy_snp": lambda t, p: t["seed_class"] == 2,
    "seed_noisy_indel": lambda t, p: t["seed_class"] == 3,
    "seed_none_iterates": lambda t, p: t["seed_class"] == -1 and t["seed_index"] == -1 and t["n_valid"] > 0 and t["n_iters"] >= 1
    and t["n_hap0_unused"] == int((p["is_skipped"] == 0).sum()) > 0,          # every read that is not skipped ends at hap 0 through "nothing used"
    "seed_depth0": lambda t, p: t["seed_class"] == 0 and t["seed_index"] == 0 and (p["total_cov"] == 0).all(),
    "seed_tie_first": lambda t, p: t["seed_class"] == 0 and t["seed_index"] == 3 and t["n_valid"] > 131,
    "seed_last": lambda t, p: t["seed_class"] == 0 and t["seed_index"] == t["n_valid"] - 1 and t["n_valid"] > 64,
    "seed_first": lambda t, p: t["seed_class"] == 0 and t["seed_index"] == 0 and t["n_valid"] > 64,
    # the two counters also count the intermediate ratios of the seeding pass, so they alone do not show that the final 134/200, 67/100, 2/3, 66/100 and
    # 1/1 evaluations happen: test_ont_threshold_counts_are_what_the_case_claims below pins the final profile and consensus of the three indels
    "ont_hp_threshold": lambda t, p: t["n_ont_hp_near"] >= 4 and t["n_ont_hp_reject"] >= 1,
    # the only case that ends on the cap of 10 iterations (test_only_phase_flip_break_reaches_the_cap)
    "phase_flip_break": lambda t, p: t["n_flip_visits"] >= 1 and t["n_ps_breaks"] >= 2 and t["hit_cap"] == 1 and t["n_iters"] == 10,
    "no_reads": lambda t, p: p["n_reads"] == 0 and t["n_valid"] > 0 and t["n_iters"] >= 1,
    "no_vars": lambda t, p: p["n_vars"] == 0 and p["n_reads"] > 0 and (p["start_var_idx"] == -1).all() and t["n_valid"] == 0,
    "all_skipped": lambda t, p: len(p["cr_read"]) == 0 and p["is_skipped"].all() and t["n_valid"] > 0,
    "one_var_one_read": lambda t, p: p["n_vars"] == 1 and p["n_reads"] == 1 and t["n_valid"] == 1,
    "valid_64_of_130": lambda t, p: t["n_valid"] == 64 and p["n_vars"] == 130,
    "valid_65_of_130": lambda t, p: t["n_valid"] == 65 and p["n_vars"] == 130,
    "cr_64": lambda t, p: len(p["cr_read"]) == 64 and p["n_reads"] > 64 and t["n_valid"] > 0,
    "cr_65": lambda t, p: len(p["cr_read"]) == 65 and p["n_reads"] > 65 and t["n_valid"] > 0,
}


def test_every_case_has_a_reached_branch_condition():
    assert set(REACHES) == set(hc.CASE_NAMES) == set(hc.crafted_cases())


@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_case_reaches_its_branch(oracle, name):
    prob, target = hc.crafted_cases()[name]
    assert prob["n_vars"] <= 300 and prob["n_reads"] <= 300
    _, t = _trace(oracle, prob, target)
    assert REACHES[name](t, prob), t


def test_only_phase_flip_break_reaches_the_cap(oracle):
    """which inputs end on the cap of 10 iterations: phase_flip_break, in both passes, and no other crafted case in either pass"""
    for name, (prob, _) in hc.crafted_cases().items():
        st, t1 = _trace(oracle, prob, jobs.GERMLINE_CLEAN)
        _, t2 = _trace(oracle, prob, jobs.GERMLINE_ALL, st)
        assert (t1["hit_cap"], t2["hit_cap"]) == ((1, 1) if name == "phase_flip_break" else (0, 0)), (name, t1, t2)


def test_trace_does_not_change_the_result(oracle):
    prob, target = hc.crafted_cases()["third_allele_seeded"]
    a = oracle.assign_hap_germline(prob, target, hc.poisoned_state(prob, target))
    b, _ = oracle.assign_hap_germline(prob, target, hc.poisoned_state(prob, target), trace=True)
    for k in hc.STATE_KEYS:
        assert (a[k] == b[k]).all(), k


def test_third_allele_literal_by_hand(oracle):
    """the expected arrays written out in hap_cases.py are what the oracle computes, and the second read's haplotype hangs on the zero score"""
    prob, target = hc.crafted_cases()["third_allele_literal"]
    st, t = _trace(oracle, prob, target)
    for k, v in hc.THIRD_ALLELE_LITERAL_EXPECTED.items():
        assert st[k].tolist() == v, k
    assert t["seed_class"] == 0 and t["seed_index"] == 0 and t["n_iters"] == 1 and t["n_zero_after_fill"] >= 2


def test_long_span_set_is_covered():
    """the long-span cases hold a read of every length in {63, 64, 65, 127, 128, 129, 200}, one that starts at variant 0 and one that ends at the last"""
    for name in ("long_spans", "long_spans_interleaved"):
        p, _ = hc.crafted_cases()[name]
        keep = (p["start_var_idx"] >= 0) & (p["is_skipped"] == 0)
        n = (p["end_var_idx"] - p["start_var_idx"] + 1)[keep]
        assert set(hc.LONG_SPANS) <= set(n.tolist())
        assert (p["start_var_idx"][keep] == 0).any() and (p["end_var_idx"][keep] == p["n_vars"] - 1).any()


def test_ont_threshold_counts_are_what_the_case_claims(oracle):
    """the per-haplotype profile counts at the three homopolymer indels are 134/200 and 67/100, 2/3 and 66/100, 1/1 and 67/100; 67/100 and 134/200 sit on
    the threshold and pass, 2/3 and 66/100 fall below it"""
    prob, target = hc.crafted_cases()["ont_hp_threshold"]
    st = oracle.assign_hap_germline(prob, target)
    prof = st["hap_to_alle_profile"].reshape(3, -1)[:, 12:]
    assert prof.tolist() == [[0] * 6, [66, 134, 1, 2, 0, 1], [67, 33, 66, 34, 67, 33]]
    assert st["hap_to_cons_alle"].reshape(-1, 3)[6:, 1:].tolist() == [[1, 0], [-1, -1], [1, 0]]


def test_mixed_batch_composition(oracle):
    """the mixed batch holds both technologies, both targets, and problems with no valid variant for their target next to ones that have some"""
    probs, targets = hc.mixed_batch()
    assert 38 <= len(probs) <= 45
    assert {p["is_ont"] for p in probs} == {0, 1} and set(targets) == {jobs.GERMLINE_CLEAN, jobs.GERMLINE_ALL}
    n_valid = [int(((p["var_cate"] & t) != 0).sum()) for p, t in zip(probs, targets)]
    assert sum(n == 0 for n in n_valid) >= 3 and sum(n > 0 for n in n_valid) >= 30
    for p, t in zip(probs, targets):
        if ((p["var_cate"] & t) != 0).sum() == 0:
            st = hc.poisoned_state(p, t)
            out = oracle.assign_hap_germline(p, t, hc.copy_state(st))
            for k in hc.STATE_KEYS:
                assert (out[k] == st[k]).all(), k          # src/assign_hap.c:482-485: nothing is touched


def test_sweep_reaches_every_counter(oracle):
    """over the 256 problems of the one-launch sweep every branch counter is non-zero (the iteration cap aside) and every seed outcome occurs"""
    probs, targets = hc.sweep()
    assert len(probs) == 256
    total, classes, unused_with_span = {}, set(), 0
    for p, tg in zip(probs, targets):
        assert 1 <= p["n_vars"] <= 140 and 0 <= p["n_reads"] <= 120
        _, t = _trace(oracle, p, tg)
        unused_with_span += t["n_hap0_unused"] - (int(((p["start_var_idx"] < 0) & (p["is_skipped"] == 0)).sum()) if t["n_valid"] else 0)
        classes.add(t["seed_class"])
        for k, v in t.items():
            total[k] = total.get(k, 0) + v
    assert classes == {-1, 0, 1, 2, 3}, classes
    for k in ("n_valid", "n_scored_gt64", "n_scored_gt128", "n_seed_gt64", "n_seed_gt128", "n_zero_after_fill", "n_cons_ge2", "n_ont_hp_reject", "n_ont_hp_near",
              "n_flip_visits", "n_ps_breaks", "n_iters", "n_hap0_both_zero", "n_hap0_unused"):
        assert total[k] > 0, (k, total)
    assert unused_with_span > 0         # "nothing used" is reached by reads that have a span too, not only by the span-less ones
    alphabet = set(np.concatenate([p["alleles"] for p in probs]).tolist())
    assert alphabet == {-2, -1, 0, 1, 2}
    assert any(p["n_reads"] == 0 for p in probs) and any(p["is_skipped"].any() for p in probs) and any((p["start_var_idx"] == -1).any() for p in probs)
