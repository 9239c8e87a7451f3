"""Conditions on the tie-dense inputs of tests/tie_cases.py, checked against the oracle alone (no GPU): the inputs are worth running only if the oracle's
backtrack really decides ties on them (the census of oracle/poa.c, by kind), if each chain lands in the kernel class its table row names (the planner's probe),
if left- and right-aligned WFA differ on the pairs, and if the edlib vectors (the reference's own edlib) equal the oracle.  The parity of the kernels on the same
inputs is tests/test_gpu_poa_ties.py and tests/test_gpu_wfa_edlib_ties.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import chain_plan_cases as P
import tie_cases as T
from conftest import ROOT

# census minimums per chain (ISSUE: the constructed chain reaches 38 / 19 / 37 / 5 / 3 at 230 bases and grows linearly)
BUBBLE_MIN = dict(cross_kind=30, multi_match=10, multi_e=10, multi_ext=3, multi_ins=2)
STR_MIN = dict(cross_kind=100)
OPEN_AND_EXT_MIN = 5      # over all POA cases together

_IDS = [c["name"] for c in T.POA_CASES]


def _line(census):
    return " ".join(f"{k}={census[k]}" for k in ("h_steps", "cross_kind", "multi_match", "multi_e", "multi_ins", "e_steps", "open_and_ext", "multi_ext"))


def test_census_changes_no_result_and_resets(oracle):
    """the census only evaluates the alternatives the backtrack does not take: K1 and K2 chains with it on == with it off; reading the counters resets them, and
    they stay at zero while it is off"""
    reads = T.read_set("b230")
    for mode in (0, 1):
        plain = oracle.poa_aln_msa_cons(reads, 2) if mode else oracle.poa_partial_aln_msa_cons(reads, [12] * len(reads))
        counted, census = T.oracle_chain(reads, mode)
        assert plain["n_cons"] == counted["n_cons"] and plain["msa_len"] == counted["msa_len"]
        assert all((a == b).all() for a, b in zip(plain["msa"], counted["msa"])) and all((a == b).all() for a, b in zip(plain["clu"], counted["clu"]))
        assert census["h_steps"] > 0 and census["e_steps"] > 0
    with oracle.poa_tie_census() as again:
        pass
    assert set(again.counts) == set(oracle.TIE_KINDS) and not any(again.counts.values())
    oracle.poa_aln_msa_cons(reads, 2)                      # (off: nothing is counted)
    with oracle.poa_tie_census() as again:
        pass
    assert not any(again.counts.values())


def test_census_counts_a_tie_of_each_kind_on_hand_made_chains(oracle):
    """what the counters mean, on chains small enough to read: an N against a two-allele bubble of equal weight ties the two predecessors of the next node
    (multi_match); an insertion of exactly the crossover length ties the two gap pieces at the same k (multi_ins); a deletion of that length ties E1 with E2
    (multi_e); a deletion that spans a bubble of equal weight ties the two predecessors of the extension (multi_ext)"""
    rng = np.random.default_rng(5)
    h1 = rng.integers(0, 4, 120).astype(np.uint8)
    h1[np.flatnonzero(h1[1:] == h1[:-1]) + 1] += 1; h1 %= 4; h1[np.flatnonzero(h1[1:] == h1[:-1]) + 1] += 2; h1 %= 4     # (no two equal neighbours: gap placements do not tie)
    h2 = h1.copy(); h2[60] = (h2[60] + 1) % 4
    base = [h1, h2, h1, h2]
    withn = h1.copy(); withn[60] = 4
    X = T.crossover()
    ins = np.concatenate([h1[:30], rng.integers(0, 4, X), h1[30:]]).astype(np.uint8)
    dele = np.concatenate([h1[:20], h1[20 + X:]])
    span = np.concatenate([h1[:55], h1[65:]])
    for extra, kind in ((withn, "multi_match"), (ins, "multi_ins"), (dele, "multi_e"), (span, "multi_ext")):
        _, none = T.oracle_chain(base, 1)
        _, census = T.oracle_chain(base + [extra], 1)
        assert none[kind] == 0 and census[kind] >= 1, (kind, _line(census))


@pytest.mark.parametrize("case", T.POA_CASES, ids=_IDS)
def test_poa_case_decides_ties(oracle, case, record_property):
    _, census = T.case_oracle(case)
    record_property("census", _line(census))
    print(f"{case['name']}: {_line(census)}")
    for kind, least in (BUBBLE_MIN if case["gen"] == "bubble" else STR_MIN).items():
        assert census[kind] >= least, (case["name"], kind, _line(census))


def test_poa_cases_together_decide_open_against_extend(oracle):
    """`H - oe == E` holds while a predecessor satisfies the extend equality: rare (one or two per tandem-repeat chain), so counted over the distinct chains of the table"""
    seen, total = set(), 0
    for case in T.POA_CASES:
        k = (case["reads"], case["mode"], tuple(sorted(case["scoring"].items())))
        if k not in seen:
            seen.add(k); total += T.case_oracle(case)[1]["open_and_ext"]
    assert total >= OPEN_AND_EXT_MIN, total


def test_iid_chain_stays_below_every_minimum(oracle):
    """why the new inputs exist: a chain of the kind the older kernel tests draw (iid bases, 300 bases, 12 reads, 2 % errors, two haplotypes) decides fewer ties of
    EVERY kind than the least a constructed chain must"""
    _, census = T.oracle_chain(T.iid_chain(np.random.default_rng(T.IID_SEED)), 1)
    print("iid chain:", _line(census))
    for kind, least in dict(BUBBLE_MIN, open_and_ext=OPEN_AND_EXT_MIN).items():
        assert census[kind] < least, (kind, _line(census))
    assert census["cross_kind"] < STR_MIN["cross_kind"]


@pytest.fixture(scope="module")
def plan_lib():
    from longcalld_amd import _lib
    return P.open_lib(_lib.LIB_PATH)


@pytest.mark.parametrize("case", T.POA_CASES, ids=_IDS)
def test_poa_case_lands_in_its_class(plan_lib, case, monkeypatch):
    """the planner's probe under the row's environment (the switches are read per call) reports the class the row names"""
    for k in [k for k in os.environ if k.startswith("LCD_")]:
        monkeypatch.delenv(k)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    assert not any(k in P.PROCESS_SWITCHES for k in case["env"])
    got = dict(zip(P.CHAIN_OUT, P.probe(plan_lib, T.plan_case(case))))
    assert {k: got[k] for k in case["planned"]} == case["planned"], (case["name"], max(len(r) for r in T.case_reads(case)))


def test_poa_table_covers_the_classes():
    """the path table of the GPU test: every full-row workgroup class, the three K1 windows and the 128-thread windowed rows, band levels 1 and 2, every `solo` kind"""
    plans = [c["planned"] for c in T.POA_CASES]
    assert {p["threads"] for p in plans if p.get("cert") == 0 and "wmax" in p and p["wmax"] >= 256 and p["wmax"] == 4 * p["threads"]} >= {64, 128, 256, 512, 1024}
    assert {(p["threads"], p["wmax"]) for c, p in zip(T.POA_CASES, plans) if c["mode"] == 0 and "wmax" in p} >= {(64, 64), (64, 128), (64, 256), (128, 512), (256, 128)}
    assert {p.get("cert") for p in plans} >= {0, 1, 2} and {p.get("solo") for p in plans} >= {0, 1, 2, 3} and {p.get("ring16") for p in plans} >= {0, 1}
    assert 4300 <= max(len(r) for r in T.read_set("s4400")) <= 4500 and len(T.read_set("s4400")) == 6


def test_certified_band_widths_of_the_band_cases(oracle, monkeypatch):
    """oracle/poa.c's checker of the certified band (LCDO_CERT_STATS: the product's intervals and its guessing policy, replayed on the CPU) on the chains of the
    band cases: the tandem-repeat chains and the 190-base bubble chain stay inside the 256-column window with every read (their ties are decided in the lean rows),
    the 300-base one with all but three, and the 150-base indels do outgrow it (the generic rows, or the re-run with full rows)"""
    monkeypatch.setenv("LCDO_CERT_STATS", "1")
    def delta(name):
        before = oracle.poa_cert_stats()
        oracle.poa_aln_msa_cons(T.read_set(name), 2)
        after = oracle.poa_cert_stats()
        return {k: after[k] - before[k] for k in ("reads", "wide_rows", "policy_wide_reads", "true_wide_reads", "path_violations", "prefix_violations")}
    for name in ("s300", "s900", "b190"):
        d = delta(name)
        assert d["reads"] == len(T.read_set(name)) - 1 and d["wide_rows"] == d["policy_wide_reads"] == d["true_wide_reads"] == 0, (name, d)
    d = delta("b300")
    assert d["policy_wide_reads"] <= 3 and d["true_wide_reads"] <= 1, d
    d = delta("b900_150")
    assert d["wide_rows"] > 0 and d["true_wide_reads"] >= 4 and d["path_violations"] == d["prefix_violations"] == 0, d


def test_generators_are_deterministic_and_shaped():
    a, b = T.bubble_chain(np.random.default_rng(3), 230), T.bubble_chain(np.random.default_rng(3), 230)
    assert len(a) == 17 and all((x == y).all() for x, y in zip(a, b))
    assert all((a[i] == a[i % 2]).all() for i in range(8)) and not (a[0] == a[1]).all()          # 4 + 4 exact copies, alternating
    sites = T.bubble_sites(230)
    assert (a[9][sites] == 4).all() and (a[8][sites] != a[0][sites]).all() and (a[8][sites] != a[1][sites]).all()     # N and a third allele at every site
    X = T.crossover()
    assert X == 18 and T.crossover(T.ALT_SCORING) == 22
    assert [len(r) - 230 for r in a[10:]] == [-3 * X, -3 * X, 3 * X, 3 * (X + 1), 3 * (X - 1), -9, -9]
    long_ = T.read_set("b900_150")
    assert max(len(r) for r in long_) - 900 >= 2 * 150 and 900 - min(len(r) for r in long_) >= 2 * 150
    s = T.str_chain(np.random.default_rng(4), 400, 6, 0.03)
    assert len(s) == 6 and all(abs(len(r) - 400) < 40 for r in s) and all((x == y).all() for x, y in zip(s, T.str_chain(np.random.default_rng(4), 400, 6, 0.03)))


# ---------------------------------------------------------------- WFA pairs
@pytest.mark.parametrize("pen", T.WFA_PENALTIES, ids=lambda p: "_".join(map(str, p)))
def test_wfa_pairs_left_and_right_aligned_rows_differ(oracle, pen):
    """on at least three quarters of the pairs the oracle's rows with gap_aln = 1 differ from those with gap_aln = 2: the kernel's left / right rule is decided"""
    b, q, e, q2, e2 = pen
    pairs = T.wfa_pairs(pen)
    differ = 0
    for p, t in pairs:
        l, r = (oracle.wfa_end2end_aln(p, t, ga, b, q, e, q2, e2) for ga in (1, 2))
        assert l["score"] == r["score"] == oracle.gotoh2p_score(p, t, b, q, e, q2, e2)
        differ += len(l["pattern_alg"]) != len(r["pattern_alg"]) or bool((l["pattern_alg"] != r["pattern_alg"]).any() or (l["text_alg"] != r["text_alg"]).any())
    print(f"{pen}: {differ} of {len(pairs)} pairs differ")
    assert 4 * differ >= 3 * len(pairs), (differ, len(pairs))


def test_wfa_crossover_pairs_have_indels_of_the_crossover_length():
    for pen in T.WFA_PENALTIES:
        X = T.crossover(dict(gap_open1=pen[1], gap_ext1=pen[2], gap_open2=pen[3], gap_ext2=pen[4]))
        assert sorted({abs(len(p) - len(t)) for p, t in T.tie_pairs("crossover", penalties=pen)}) == [X - 1, X, X + 1]
    for p, t in T.tie_pairs("wide"):
        assert min(len(p), len(t)) == 1000 and 1500 <= abs(len(p) - len(t)) <= 2900


# ---------------------------------------------------------------- edlib vectors
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "edlib_tie_golden.json")) as f:
        return json.load(f)


def _arr(s):
    return np.frombuffer(s.encode(), np.uint8) - ord("0")


def test_edlib_tie_vectors_are_the_generators_pairs():
    g = _golden()
    pairs = T.tie_pairs("edlib")
    assert len(g["tie_cases"]) == len(g["tie_hw_cases"]) == len(pairs) >= 16
    for (t, q), c, h in zip(pairs, g["tie_cases"], g["tie_hw_cases"]):
        assert (_arr(c["target"]) == t).all() and (_arr(c["query"]) == q).all() and c["target"] == h["target"] and c["query"] == h["query"]
    assert sorted({len(t) for t, _ in pairs}) == sorted(T.EDLIB_LENS) and sum(len(t) >= 4300 for t, _ in pairs) <= 3


def test_oracle_edlib_equals_the_reference_on_tie_vectors(oracle):
    """oracle/edlib_nw.c == the reference's own edlib (tests/golden/make_edlib_golden.py) where nearly every traceback step is a tie: NW and HW"""
    g = _golden()
    for c in g["tie_cases"]:
        t, q = _arr(c["target"]), _arr(c["query"])
        d, ops = oracle.edlib_nw(q, t)
        assert d == c["dist"] and hashlib.sha1(ops.tobytes()).hexdigest() == c["path_sha1"], len(t)
        assert oracle.edlib_xgaps(t, q) == c["xgaps"] and oracle.edlib_end2end_aln(t, q) == (c["dist"], c["n_eq"], c["n_xid"]), len(t)
    for c in g["tie_hw_cases"]:
        t, q = _arr(c["target"]), _arr(c["query"])
        d, s0, e0, ops = oracle.edlib_hw(q, t)
        assert (d, s0, e0) == (c["dist"], c["start"], c["end"]) and hashlib.sha1(ops.tobytes()).hexdigest() == c["path_sha1"], len(t)
        assert (int(oracle.ops_to_xgaps(ops)), int((ops == 0).sum()), int((ops != 0).sum())) == (c["xgaps"], c["n_eq"], c["n_xid"]), len(t)
        assert oracle.edlib_infix_aln(t, q) == (c["dist"], c["n_eq"], c["n_xid"]), len(t)
