"""Conditions on the inputs of tests/resort_cases.py, checked against the oracle alone (no GPU): the chains are worth running only if they really ask the
incremental re-sort (poa_kernel.hip topo_sort_incremental) for its rare paths -- the re-sort census of oracle/poa.c, by class -- and if each chain lands in the
kernel class its table row names (the planner's probe).  The converse is why the file exists: no earlier input of the suite asks the walk for more than a dozen
rows.  The census holds properties of the input graph, not a replay of the kernel; the parity of the kernel on the same inputs, with the incremental re-sort on
and off, is tests/test_gpu_poa_resort.py."""
import os

import numpy as np
import pytest

import chain_plan_cases as P
import resort_cases as R
import tie_cases as T

_IDS = [c["name"] for c in R.CASES]
CLASSES = ("span_13_52", "span_53_64", "span_over_64", "no_cut_256", "fan_in4", "fan_out4", "far_target", "far_target_ring", "new_65_128", "new_over_128", "edges_only")
# what every input the suite had before stays below (measured: the longest span any of them has is five rows, profiles/NOTES_resort_cases.md)
EARLIER_MAX_SPAN = 12


def _k2(oracle, reads):
    return R.oracle_chain(reads, 1)[1]


def test_census_changes_no_result_and_resets(oracle):
    """the census reads the graph and the old order, nothing else: K1 and K2 chains with it on == with it off; reading the counters resets them, and they stay at
    zero while it is off"""
    reads = R.chain_reads(R.CASES[0])
    for mode in (0, 1):
        plain = oracle.poa_aln_msa_cons(reads, 2) if mode else oracle.poa_partial_aln_msa_cons(reads, [12] * len(reads))
        counted, census = R.oracle_chain(reads, mode)
        assert plain["n_cons"] == counted["n_cons"] and plain["msa_len"] == counted["msa_len"]
        assert all((a == b).all() for a, b in zip(plain["msa"], counted["msa"])) and all((a == b).all() for a, b in zip(plain["clu"], counted["clu"]))
        assert census["topo_reads"] > 0 and census["places"] > 0
        assert census["places"] == census["span_le_12"] + census["span_13_52"] + census["span_53_64"] + census["span_over_64"]
        assert census["topo_reads"] == census["edges_only"] + census["new_1_64"] + census["new_65_128"] + census["new_over_128"]
    with oracle.poa_resort_census() as again:
        pass
    assert set(again.counts) == set(oracle.RESORT_KINDS) and not any(again.counts.values())
    oracle.poa_aln_msa_cons(reads, 2)                      # (off: nothing is counted)
    with oracle.poa_resort_census() as again:
        pass
    assert not any(again.counts.values())


def _plain(rng, L):
    """iid bases, no two equal neighbours (a deleted or substituted base has one placement)"""
    h = rng.integers(0, 4, L).astype(np.uint8)
    for add in (1, 2):
        same = np.flatnonzero(h[1:] == h[:-1]) + 1
        h[same] = (h[same] + add) % 4
    return h


def test_census_counts_each_class_on_hand_made_chains(oracle):
    """what the counters mean, on chains small enough to read: for every counter one chain that lacks the feature (0) and one that has it (>= 1)"""
    rng = np.random.default_rng(11)
    h = _plain(rng, 120)
    # (a deletion of n bases at p slides unless h[p - 1] != h[p + n - 1] and h[p] != h[p + n]: the bases around the deletions below are set so that none can)
    h[39:47] = [3, 0, 1, 2, 3, 2, 3, 1]; h[54:62] = [0, 2, 3, 2, 3, 1, 0, 2]; h[18:22] = [3, 0, 1, 2]; h[48:52] = [1, 2, 3, 0]; h[88:92] = [1, 2, 3, 0]
    alt = lambda p: (int(h[p]) + 2) % 4
    dele = lambda p, n: R._edit(h, dels=[(p, n)])
    ins = lambda p, n: R._edit(h, ins=[(p, rng.integers(0, 4, n))])
    pairs = {
        # a read that adds nothing but weight is no topology read; a 2-base deletion adds one edge and no node
        "topo_reads": ([h, h], [h, h, dele(50, 2)]),
        "edges_only": ([h, h, R._snp(h, 50, alt(50))], [h, h, dele(50, 2)]),
        # a SNP: one new node aligned to an old one (its ring grew); inserted stretches of 70 and 140 bases
        "new_1_64": ([h, h, dele(50, 2)], [h, h, R._snp(h, 50, alt(50))]),
        "ring_grew": ([h, h, ins(50, 3)], [h, h, R._snp(h, 50, alt(50))]),
        "new_65_128": ([h, h, ins(50, 64)], [h, h, ins(50, 70)]),
        "new_over_128": ([h, h, ins(50, 128)], [h, h, ins(50, 140)]),
        # the read that makes a ring of two a ring of three
        "ring3_in_span": ([h, h, R._snp(h, 50, alt(50))], [h, h, R._snp(h, 50, alt(50)), R._snp(h, 50, (alt(50) + 1) % 4)]),
        # node 40's fourth out-edge is counted by the read that adds it (the place is node 40's own row)
        "fan_out4": ([h, h, dele(41, 2), dele(41, 3)], [h, h, dele(41, 2), dele(41, 3), dele(41, 4)]),
        # node 60's in-edges are counted by a read that changes the row before it: a SNP at 60 (three deletions that end there: four in-edges with the backbone's)
        "fan_in4": ([h, h, dele(58, 2), dele(57, 3), R._snp(h, 60, alt(60))], [h, h, dele(58, 2), dele(57, 3), dele(56, 4), R._snp(h, 60, alt(60))]),
        # a deletion edge out of row 19 seen by a read that changes row 19: 30 rows long, 70 rows long (beyond the 64-row window)
        "far_target": ([h, h, dele(20, 30), R._snp(h, 20, alt(20))], [h, h, dele(20, 70), R._snp(h, 20, alt(20))]),
        # ... the same with an aligned ring at its far end (a SNP at base 90)
        "far_target_ring": ([h, h, dele(20, 70), R._snp(h, 20, alt(20))], [h, R._snp(h, 90, alt(90)), h, dele(20, 70), R._snp(h, 20, alt(20))]),
    }
    # two branches of d bases with no base in common: 2 d + 1 rows without a cut around a SNP in the middle of one of them; one branch alone has a cut at every row
    for kind, d, L in (("span_13_52", 8, 120), ("span_53_64", 27, 120), ("span_over_64", 32, 140), ("no_cut_256", 130, 300)):
        h1, h2, s = R.divergent_pair(np.random.default_rng(d), L, d)
        at = s + d - 1 if kind == "no_cut_256" else s + d // 2        # (no cut within 256 rows: the branches' rows alternate, so the last base of 130 is 257 rows in)
        late = R._snp(h1, at, 1 - int(h1[at]))
        pairs[kind] = ([h1, h1, late], [h1, h2, h1, h2, late])
    assert set(pairs) >= set(CLASSES)
    for kind, (lack, have) in pairs.items():
        a, b = _k2(oracle, lack), _k2(oracle, have)
        assert a[kind] == 0 and b[kind] >= 1, (kind, R.census_line(a), R.census_line(b))
    # the two maxima, on the last pair: one place, one piece; and a read with two SNPs 40 bases apart: four places (two each), two pieces
    two = _k2(oracle, [h, h, R._snp(R._snp(h, 30, alt(30)), 70, alt(70))])
    assert (two["max_places"], two["max_pieces"], two["places"], two["max_span"]) == (4, 2, 4, 2), R.census_line(two)
    # span = c - q + 1 exactly: the cut before the stretch, 2 x 8 rows of which the last popped is a cut again (the FIFO is empty before the node behind it goes in)
    assert _k2(oracle, pairs["span_13_52"][1])["max_span"] == 17


@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_case_reaches_the_minimums_of_its_class(oracle, case, record_property):
    """every row on the oracle alone: the census minimums of its tag; the limit rows outgrow the list they are named after -- whose size follows from the pool the
    planner reports, by the kernel's own formulas (R.inc_limits: poa_kernel.hip lines 953 - 954) -- from a read the kernel does not refuse beforehand (at most 128
    new nodes), the seg row with fewer places than INC_ML; every other row stays below both lists"""
    _, census = R.case_oracle(case)
    record_property("census", R.census_line(census))
    print(f"{case['name']}: {R.census_line(census)}")
    for kind, least in case["tag"].items():
        assert least >= 1 and census[kind] >= least, (case["name"], kind, R.census_line(census))
    lim = R.inc_limits(R.probe_plan(case, R.chain_reads(case))["lds_bytes"])
    assert lim["INC_ML"] >= 32 and lim["INC_SEG"] >= 16 and lim["INC_EL"] >= 128          # (below these the kernel never tries: line 955)
    if case["gen"] == "over_ml":
        assert census["max_places"] > lim["INC_ML"] and census["new_over_128"] == 0, (lim, R.census_line(census))
    elif case["gen"] == "over_seg":
        assert census["max_pieces"] > lim["INC_SEG"] and census["max_places"] < lim["INC_ML"] and census["new_over_128"] == 0, (lim, R.census_line(census))
    else:
        assert census["max_places"] <= lim["INC_ML"] and census["max_pieces"] <= lim["INC_SEG"], (lim, R.census_line(census))


def _earlier(census, what):
    print(f"{what}: {R.census_line(census)}")
    assert census["topo_reads"] > 0, what
    assert census["max_span"] <= EARLIER_MAX_SPAN and census["no_cut_256"] == 0 and census["span_over_64"] == 0 and census["span_53_64"] == 0 and census["span_13_52"] == 0, (what, R.census_line(census))


def test_earlier_chains_never_ask_for_more_than_a_dozen_rows(oracle):
    """why the new inputs exist: the iid chain of the older kernel tests and the tie-dense sets, K1 and K2, have a cut within 12 rows of every place"""
    _earlier(_k2(oracle, T.iid_chain(np.random.default_rng(T.IID_SEED))), "iid")
    for name in ("b300", "b900", "s900"):
        for mode in (0, 1):
            _earlier(R.oracle_chain(T.read_set(name), mode)[1], (name, mode))


@pytest.mark.parametrize("shape,n", [("hifi", 8), ("ont", 4), ("sv", 2)])
def test_earlier_regions_never_ask_for_more_than_a_dozen_rows(oracle, shape, n):
    """... and so do regions of the seeded workload every end-to-end test and the benchmark draw from (all chains of a region: K1, K2)"""
    from longcalld_amd import jobs
    regs = jobs.make_regions(777, n, {"hifi": jobs.HIFI, "ont": jobs.ONT, "sv": jobs.SV}[shape])
    with oracle.poa_resort_census() as rc:
        for r in regs:
            oracle.collect_noisy_reg_aln_strs(r)
    _earlier(rc.counts, shape)


@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_case_lands_in_its_class(case, monkeypatch):
    """the planner's probe under the row's environment (the switches are read per call) reports the class the row names; every further environment of the row
    changes LCD_DBG only (no planning switch: the same class)"""
    for k in [k for k in os.environ if k.startswith("LCD_")]:
        monkeypatch.delenv(k)
    assert not any(k in P.PROCESS_SWITCHES for k in case["env"])
    got = R.probe_plan(case, R.chain_reads(case))
    assert {k: got[k] for k in case["planned"]} == case["planned"], (case["name"], max(len(r) for r in R.chain_reads(case)))
    for env in case["also"]:
        assert {k: v for k, v in env.items() if k != "LCD_DBG"} == case["env"] and env["LCD_DBG"] in ("1024", "64", "384", "8")
    assert [e["LCD_DBG"] for e in case["also"]][:3] == ["1024", "64", "384"] and (len(case["also"]) == 4) == (case["env"].get("LCD_CERT") == "0")
    assert len(R.chain_reads(case)) <= 30 and max(len(r) for r in R.chain_reads(case)) <= 1700


def test_table_covers_the_classes(oracle):
    """64- and 256-thread pools, K1 and K2, both K1 windows, noisy reads; every census class in at least two rows (by the rows' own minimums), both limits"""
    plans = [c["planned"] for c in R.CASES]
    assert {p["threads"] for p in plans} >= {64, 256} and {c["mode"] for c in R.CASES} == {0, 1} and {p.get("cert") for p in plans} >= {0, 1, 2}
    assert {p["wmax"] for c, p in zip(R.CASES, plans) if c["mode"] == 0} >= {64, 128} and any(c["is_ont"] for c in R.CASES)
    for kind in CLASSES:
        assert sum(kind in c["tag"] for c in R.CASES) >= 2, kind
    assert sum(c["gen"] == "over_ml" for c in R.CASES) >= 2 and sum(c["gen"] == "over_seg" for c in R.CASES) >= 2
    assert sorted({c["args"]["d"] for c in R.CASES if c["gen"] == "divergent"}) == [8, 12, 24, 26, 28, 30, 31, 32, 40, 130]


def test_generators_are_deterministic_and_shaped():
    a, b = R.divergent_chain(np.random.default_rng(3), 400, 30), R.divergent_chain(np.random.default_rng(3), 400, 30)
    assert len(a) == 28 and all((x == y).all() for x, y in zip(a, b))
    h1, h2, s = R.divergent_pair(np.random.default_rng(3), 400, 30)
    assert (a[0] == h1).all() and (a[1] == h2).all() and (h1[s:s + 30] < 2).all() and (h2[s:s + 30] >= 2).all() and h1[s - 1] == h2[s - 1] and h1[s + 30] == h2[s + 30]
    assert h1[s - 1] not in (h1[s + 29], h2[s + 29]) and h1[s + 30] not in (h1[s], h2[s])
    assert all(abs(len(r) - 400) <= 3 for r in a) and (a[26] == a[8]).all() and (a[27] == a[21]).all()     # the two repeats
    assert all(int((r[:s - 1] != (h1, h2)[(i - 6) // 10][:s - 1]).sum()) == 0 for i, r in enumerate(a[6:26], 6))     # every late read: its branch up to the stretch
    f = R.feature_chain(np.random.default_rng(0))
    assert len(f) == 24 and max(len(r) for r in f) == 870 + 130 and all((x == y).all() for x, y in zip(f, R.feature_chain(np.random.default_rng(0))))
    assert [len(r) - 870 for r in f[4:9]] == [-106, -98, 86, 62, 130] and (f[11][R.feature_sites(870)] == 4).all() and (f[22] == f[0]).all() and (f[23] == f[13]).all()
    assert R.inc_limits(8192) == dict(INC_ML=251, INC_SEG=125, INC_EL=1007) and R.inc_limits(32768) == dict(INC_ML=1019, INC_SEG=509, INC_EL=4079)
    assert R.inc_limits(1 << 20) == dict(INC_ML=1024, INC_SEG=512, INC_EL=4096)
    m, g = R.over_ml_chain(np.random.default_rng(0), 251), R.over_seg_chain(np.random.default_rng(0), 125)
    assert len(m) == len(g) == 6 and int((m[4][:380] != m[0][:380]).sum()) == 120 and len(g[0]) - len(g[4]) == 133
