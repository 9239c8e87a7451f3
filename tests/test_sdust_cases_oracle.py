"""The N-dense sdust cases (tests/sdust_cases.py) on the CPU: every case reaches the census it names, the suite as a whole reaches every key, the sequential
model (tests/sdust_model.py) equals the reference's own sdust() where oracle/_ref is built -- which is what licenses it as the oracle of
tests/test_gpu_sdust_seams.py -- and the model of the device's decomposition equals the sequential model on every case.  No GPU."""
import numpy as np
import pytest

import sdust_cases as SC
import sdust_model as M


@pytest.fixture(scope="module")
def runs():
    """per case name: (sdust_full's intervals, its census with sdust_segmented's max_back, sdust_segmented's intervals, its census), computed once"""
    out = {}
    for c in SC.cases():
        cs = {}
        full, cf = SC.full_runs()[c["name"]]
        segd = M.sdust_segmented(c["seq"], c["T"], c["W"], cs)
        out[c["name"]] = (full, dict(cf, max_back=cs.get("max_back", 0)), segd, cs)
    return out


def test_every_case_reaches_its_census(runs):
    for c in SC.cases():
        cen = runs[c["name"]][1]
        for key, least in c["reach"].items():
            assert cen.get(key, 0) >= least, (c["name"], key, cen)


def test_suite_reaches_every_key(runs):
    groups = SC.by_params()
    assert set(groups) == set(SC.PARAMS)
    top = {tw: {k: max(runs[c["name"]][1].get(k, 0) for c in cs) for k in ("displaced", "past_end", "order_inversions", "max_pn", "seam_crossers", "max_back")}
           for tw, cs in groups.items()}
    for tw in ((5, 20), (10, 33), (20, 64)):
        t = top[tw]
        assert t["displaced"] > 0 and t["past_end"] > 0 and t["order_inversions"] > 0 and t["max_pn"] > 32 and t["seam_crossers"] > 0, (tw, t)
        assert t["max_back"] > 2 * M.seg_of(tw[1]), (tw, t)
    assert top[(1, 4)]["seam_crossers"] > 0
    # the list P: pcap = W W + 8 is the device's bound (lcd_sdust_batch); the model has to stay inside it, and the named peak cases come close to the longest
    for (T, W), cs in groups.items():
        for c in cs:
            assert max(runs[c["name"]][1]["max_pn"], runs[c["name"]][3]["max_pn"]) <= W * W + 8, c["name"]
            assert runs[c["name"]][3]["max_lane"] <= M.seg_of(W) // 4 + W + 1 <= M.seg_of(W) + 8, c["name"]     # (the bound of the kernel's header; cap = seg + 8)
    for tw in ((5, 20), (10, 33)):
        peak = runs[f"T{tw[0]}W{tw[1]}:spill:peak"][1]["max_pn"]
        assert peak * 10 >= top[tw]["max_pn"] * 9, (tw, peak, top[tw]["max_pn"])
    assert top[(5, 20)]["max_pn"] > 300 and top[(10, 33)]["max_pn"] > 800
    # the families are all there at the caller's setting, every kind of failure of the old ownership rule has a case, and letters cover R, Y, -
    names = [c["name"] for c in groups[(5, 20)]]
    for fam in ("periodic", "random", "seam:one", "seam:pair", "end", "spill", "letters0", "letters1", "letters2"):
        assert any(fam in n for n in names), fam
    assert {c["kind"] for c in SC.cases()} == {None, "past_end", "order", "start", "cap"}
    assert any(ch in c["seq"] for c in SC.cases() if isinstance(c["seq"], bytes) for ch in b"RY-")


def test_sequential_model_is_the_reference(oracle, runs):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")
    for c in SC.cases():
        codes = np.array(M.codes_of(c["seq"]), np.uint8)
        exp = [tuple(x) for x in oracle.ref_sdust(codes, c["T"], c["W"]).tolist()]
        assert runs[c["name"]][0] == exp, c["name"]
        if isinstance(c["seq"], bytes):       # the reference maps the letters itself
            assert [tuple(x) for x in oracle.ref_sdust(np.frombuffer(c["seq"], np.uint8), c["T"], c["W"]).tolist()] == exp, c["name"]


def test_segmented_model_equals_sequential(runs):
    """the decomposition the device runs (ownership by step) on every case, with its census: the saves chain in the reference's order (same inversions by
    start), every save is reported once (same past_end count)"""
    for c in SC.cases():
        full, cen, segd, cs = runs[c["name"]]
        assert segd == full, (c["name"], [x for x in full if x not in segd], [x for x in segd if x not in full])
        assert cs.get("past_end", 0) == cen.get("past_end", 0) and cs.get("order_inversions", 0) == cen.get("order_inversions", 0), c["name"]


def test_kind_cases_tell_the_ownership_rules_apart(runs):
    """the cases kept for the three failures of ownership by start: that rule (sdust_model's rule="start") differs from the reference on each of them in the
    way the case names -- so a kernel that went back to it would fail these cases"""
    n = 0
    for c in SC.cases():
        if c["kind"] is None or isinstance(c["seq"], bytes):
            continue
        n += 1
        full = runs[c["name"]][0]
        cen = {}
        old = M.sdust_segmented(c["seq"], c["T"], c["W"], cen, rule="start")
        if c["kind"] == "cap":           # more reports from one lane than its slots
            assert cen["max_lane"] > M.seg_of(c["W"]) + 8, (c["name"], cen)
            continue
        lost, extra = [x for x in full if x not in old], [x for x in old if x not in full]
        assert lost, c["name"]
        ln = len(c["seq"])
        if c["kind"] == "past_end":      # an interval at or past len is missing, or the last one ends short
            assert any(s >= ln for s, f in lost) or any(f > ln and any(s2 == s and f2 < f for s2, f2 in extra) for s, f in lost), (c["name"], lost, extra)
        elif c["kind"] == "order":       # two of the reference's intervals come back as one
            assert any(sum(1 for s, f in lost if s2 <= s and f <= f2) >= 2 for s2, f2 in extra), (c["name"], lost, extra)
        else:                            # same finish, another start
            assert any(f == f2 and s != s2 for s, f in lost for s2, f2 in extra), (c["name"], lost, extra)
    assert n >= 6
