"""The methylation table's Python oracle (tests/mods_common.py) against tables worked out by hand: every named case of the case table adds the rows and the
statistics written beside it, its predicate proves from the oracle's trace that the condition it is named after is reached, and the table's text is as specified."""
import pytest

import mods_common as mc


@pytest.fixture(scope="module")
def table():
    return mc.build_cases()


def _run(t, code="m", T=204, combine=False, reg=None, trace=None):
    rb, re_ = reg or (t["reg_beg"], t["reg_end"])
    haps = t["haps"] if reg is None else _haps(t, rb, re_)
    return mc.pileup(t["bodies"], t["ref"], 1, rb, re_, haps, code=code, T=T, combine=combine, trace=trace)


def _haps(t, rb, re_):
    """the cases' haps for the kept reads of a sub-region"""
    import bam_out_common as bo
    by_body = {id(r["body"]): c["hap"] for r, c in zip(t["recs"], t["cases"])}
    return [by_body[id(b)] for b, r in bo.region_records(t["bodies"], rb, re_, 30) if r >= 0]


def test_the_cases_add_up_to_the_hand_written_table(table):
    rows, st = _run(table)
    want_rows, want_st = mc.expected_by_hand(table["cases"])
    assert rows == want_rows
    assert st == want_st
    assert st["n_records"] == len(table["haps"]) == len(table["cases"]) - 2            # (two records fail the flag / MAPQ filter)
    for k in mc.STAT_KEYS:
        assert st[k] > 0, k


def test_every_predicate_holds(table):
    trace = []
    _run(table, trace=trace)
    by_body = {id(e["body"]): e for e in trace}
    names = set()
    for c, r in zip(table["cases"], table["recs"]):
        assert c["name"] not in names
        names.add(c["name"])
        if c["pred"] is None:
            assert id(r["body"]) not in by_body, c["name"]                              # filtered: never looked at
            continue
        assert c["pred"](by_body[id(r["body"])]), c["name"]
    assert len(names) >= 70


@pytest.mark.parametrize("code,T", [("h", 204), ("m", 128), ("m", 255)])
def test_other_options_on_the_cases_that_name_them(table, code, T):
    rows, _ = _run(table, code=code, T=T)
    want, spans = mc.expected_alt(table["cases"], code, T)
    assert len(spans) >= 2
    got = [r for r in rows if any(a <= r[0] <= b for a, b in spans)]
    assert got == want


def test_combine_strands_inside_and_across_a_region_end(table):
    """a row's key is the position of the CpG's C; a CpG cut by a region's end gives one row per chunk, and the join of the chunks adds rows of equal key"""
    plain, _ = _run(table)
    comb, _ = _run(table, combine=True)
    assert comb == mc.combine_rows(plain) and all(s == "." for _, s, _ in comb)
    c = next(c for c in table["cases"] if c["name"] == "both_strands_forward")
    p = c["slot0"] + 9                                                                  # the C of a CpG that a forward and a reverse read cover
    row = dict((k, v) for k, _, v in comb)[p]
    assert row == (0, 0, 0, 1, 0, 0, 0, 1, 0)                                           # hap 1 mod from the '+' site, hap 2 canon from the '-' site at p + 1
    assert comb[0][0] == table["reg_beg"] - 1 and comb[-1][0] == table["reg_end"]       # keys may lie one base in front of the region
    # the same contig as two chunks that meet between that C and its G
    left, right = (table["reg_beg"], p), (p + 1, table["reg_end"])
    for combine in (False, True):
        a, sa = _run(table, combine=combine, reg=left)
        b, sb = _run(table, combine=combine, reg=right)
        whole, sw = _run(table, combine=combine)
        assert mc.merge_rows([a, b]) == whole
        if combine:
            assert a[-1][0] == b[0][0] == p                                             # one row in each chunk, the same key
        else:
            assert len({(r[0], r[1]) for r in a + b}) == len(a) + len(b)                # no site twice
        # every (record, site) pair is counted by exactly one chunk
        assert sa["n_counted"] + sb["n_counted"] == sw["n_counted"]


def test_text(table):
    rows = [(1001, "-", (0, 0, 0, 1, 0, 0, 0, 0, 0)), (1200, "+", (1, 2, 3, 4, 5, 6, 7, 8, 9))]
    assert mc.format_rows(rows, "chrS") == "chrS\t1000\t1001\tm\t-\t1\t1\t1\t1\t0\t0\t0\n" "chrS\t1199\t1200\tm\t+\t27\t12\t9\t4\t15\t7\t18\n"
    assert mc.format_rows([(7, ".", (0,) * 8 + (1,))], "c", "h") == "c\t6\t8\th\t.\t0\t0\t0\t0\t0\t0\t1\n"
    assert mc.HEADER.split("\t") == "#chrom start end code strand n_all mod_all n_h1 mod_h1 n_h2 mod_h2 n_filtered\n".split(" ")


def test_mm_syntax():
    g = mc.parse_mm(b"C+mh?,0,12;G-76792.;N+n;")
    assert [(x["base"], x["strand"], x["codes"], x["chebi"], x["flag"], x["deltas"]) for x in g] == [
        ("C", "+", ["m", "h"], False, "?", [0, 12]), ("G", "-", ["76792"], True, ".", []), ("N", "+", ["n"], False, "", [])]
    assert mc.parse_mm(b"") == []
    assert mc.parse_mm(b"C+m,9999999999;")[0]["deltas"] == [9999999999] and mc.parse_mm(b"C+m,10000000000;") is None
    assert mc.classify(204, 204, 204) == mc.MOD and mc.classify(0, 51, 204) == mc.CANON and mc.classify(0, 52, 204) == mc.FILT and mc.classify(200, 400, 204) == mc.FILT


def test_the_seeded_chunk_has_what_the_gpu_test_needs():
    s = mc.seeded()
    rb, re_ = s["first"] + 1, s["first"] + s["span"]
    haps = mc.haps_for(s["bodies"], rb, re_, 1)
    rows, st = mc.pileup(s["bodies"], s["ref"], 1, rb, re_, haps)
    assert any(v[3] + v[4] > 0 and v[6] + v[7] > 0 for _, _, v in rows) and any(v[2] + v[5] + v[8] > 0 for _, _, v in rows)
    assert {s_ for _, s_, _ in rows} == {"+", "-"}
    for k in mc.STAT_KEYS:
        assert st[k] > 0 or k in ("n_hard_clip", "n_no_group"), k
