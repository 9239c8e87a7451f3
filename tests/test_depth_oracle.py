"""The depth track's two Python oracles (tests/depth_common.py) against each other and against the rules' invariants, the window and seam rules, the text, and the
host-only exports lcd_depth_windows / lcd_depth_format of the built library against the Python rules, byte for byte.  Every named case proves from the oracle's
trace that the condition it is named after is reached."""
import numpy as np
import pytest

import depth_common as dc


@pytest.fixture(scope="module")
def table():
    return dc.build_cases()


@pytest.fixture(scope="module")
def lcd_host():
    from longcalld_amd import align
    return align


def _both(t, skip_dels, trace=None):
    got = dc.depth_rows(t["bodies"], t["reg_beg"], t["reg_end"], t["haps"], skip_dels=skip_dels, trace=trace)
    assert got == dc.depth_rows_naive(t["bodies"], t["reg_beg"], t["reg_end"], t["haps"], skip_dels=skip_dels)
    return got


@pytest.mark.parametrize("skip_dels", [False, True])
def test_the_oracles_agree_on_the_case_table(table, skip_dels):
    rows, st = _both(table, skip_dels)
    dc.check_tiling(rows, table["reg_beg"], table["reg_end"], st)
    assert st["n_records"] == len(table["recs"]) == len(table["haps"])
    assert st["n_no_cigar"] == 1 and st["n_cg"] == 2 and st["n_no_overlap"] == (3 if skip_dels else 2) and all(b > 0 for b in st["bases"])
    assert st["n_intervals"] > st["n_records"] and max(max(d) for _, _, d in rows) >= 300


@pytest.mark.parametrize("skip_dels", [False, True])
def test_every_predicate_holds(table, skip_dels):
    trace = []
    _both(table, skip_dels, trace=trace)
    by_body = {id(e["body"]): e for e in trace}
    names = set()
    for c in table["cases"]:
        assert c["name"] not in names
        names.add(c["name"])
        assert c["pred"]([by_body[id(r["body"])] for r in c["recs"]], skip_dels), c["name"]
    assert len(names) >= 30


def test_the_oracles_agree_on_200_seeded_chunks():
    seen = dict(n_no_cigar=0, n_no_overlap=0, n_intervals=0, empty=0, multi=0)
    for seed in range(200):
        recs, rb, re_ = dc.seeded_chunk(seed)
        bodies, haps = [r["body"] for r in recs], dc.haps_of(recs, rb, re_)
        for sd in (False, True):
            rows, st = dc.depth_rows(bodies, rb, re_, haps, skip_dels=sd)
            assert (rows, st) == dc.depth_rows_naive(bodies, rb, re_, haps, skip_dels=sd), seed
            dc.check_tiling(rows, rb, re_, st)
        for k in ("n_no_cigar", "n_no_overlap", "n_intervals"):
            seen[k] += st[k]
        seen["empty"] += st["n_records"] == 0
        seen["multi"] += st["n_intervals"] > st["n_records"]
    assert all(v > 0 for v in seen.values()), seen


def test_a_chunk_without_records_is_one_zero_row():
    rows, st = dc.depth_rows([], 10, 500, [])
    assert rows == [(10, 500, (0, 0, 0))] and st["n_rows"] == 1 and st["bases"] == [0, 0, 0] and st["n_records"] == 0


def test_offsets_are_64_bit():
    r = dc.make_record(b"far", 100, [(dc.M, 10)] + [(dc.N, 268435455)] * 9 + [(dc.M, 10)])
    _, ops, _ = dc.record_ops(r["body"])
    runs = dc.cover_runs(100, ops, False)
    assert runs == [(100, 109), (100 + 10 + 9 * 268435455, 100 + 19 + 9 * 268435455)] and runs[1][0] > 1 << 31
    # wrapped to 32 bits the second run would fall at 100 + 10 + 9 * 268435455 - 2^32 < 0, or -- with a region there -- inside it
    rows, st = dc.depth_rows([r["body"]], 50, 400, [1])
    assert st["n_intervals"] == 1 and st["bases"] == [0, 10, 0]


def test_windows(table):
    rows, st = dc.depth_rows(table["bodies"], table["reg_beg"], table["reg_end"], table["haps"])
    rb, re_ = table["reg_beg"], table["reg_end"]
    w1 = dc.windows(rows, 1)
    assert [(b, e) for b, e, _ in w1] == [(p, p) for p in range(rb, re_ + 1)]
    per_base = [d for b, e, d in rows for _ in range(b, e + 1)]
    assert [v for _, _, v in w1] == per_base
    for W in (re_, re_ + 1, 1 << 30):
        assert dc.windows(rows, W) == [(rb, re_, tuple(st["bases"]))]
    w = dc.windows(rows, 1000)                                  # the region starts at 2001 and does not end on a bound: the last window is cut
    assert w[0][0] == rb and w[0][1] == 3000 and w[-1][1] == re_ and all((b - 1) // 1000 == (e - 1) // 1000 for b, e, _ in w)
    assert [sum(v[h] for _, _, v in w) for h in range(3)] == st["bases"]
    w7 = dc.windows(rows, 7)
    assert all(e - b + 1 == 7 for b, e, _ in w7[1:-1]) and [sum(v[h] for _, _, v in w7) for h in range(3)] == st["bases"]


def test_the_seam_rule():
    a = ("c1", [(1, 10, (1, 0, 0)), (11, 20, (2, 0, 0))])
    b = ("c1", [(21, 25, (2, 0, 0)), (26, 30, (0, 0, 1))])
    c = ("c1", [(31, 40, (0, 1, 1))])
    d = ("c1", [(51, 60, (0, 1, 1))])                          # a gap in front of it
    e = ("c2", [(61, 70, (0, 1, 1))])                          # another contig
    assert dc.sink_rows([a, b, c, d, e]) == [("c1", 1, 10, (1, 0, 0)), ("c1", 11, 25, (2, 0, 0)), ("c1", 26, 30, (0, 0, 1)), ("c1", 31, 40, (0, 1, 1)),
                                            ("c1", 51, 60, (0, 1, 1)), ("c2", 61, 70, (0, 1, 1))]
    one = ("c1", [(41, 50, (0, 1, 1))])                        # a chunk of ONE row joins on both sides
    assert dc.sink_rows([c, one, d]) == [("c1", 31, 60, (0, 1, 1))]
    # windows of 8: [17, 24] is cut by the seam at 20 | 21 and added up; equal depths do not join across a window bound
    got = dc.sink_rows([a, b], W=8)
    assert got == [("c1", 1, 8, (8, 0, 0)), ("c1", 9, 16, (2 + 2 * 6, 0, 0)), ("c1", 17, 24, (16, 0, 0)), ("c1", 25, 30, (2, 0, 5))]
    assert dc.sink_rows([a, d], W=8)[2:] == [("c1", 17, 20, (8, 0, 0)), ("c1", 51, 56, (0, 6, 6)), ("c1", 57, 60, (0, 4, 4))]      # a gap: written as it is
    assert dc.sink_rows([], W=0) == []


def test_text():
    rows = [(1001, 1010, (3, 2, 1)), (1011, 1011, (0, 0, 0))]
    assert dc.format_rows(rows, "chrS") == "chrS\t1000\t1010\t6\t2\t1\t3\n" "chrS\t1010\t1011\t0\t0\t0\t0\n"
    assert dc.HEADER.split("\t") == "#chrom start end depth_all depth_h1 depth_h2 depth_unassigned\n".split(" ")
    assert dc.HEADER_W.split("\t") == "#chrom start end bases_all bases_h1 bases_h2 bases_unassigned\n".split(" ")


def test_the_library_windows_and_text_equal_the_python_rules(table, lcd_host):
    rows, _ = dc.depth_rows(table["bodies"], table["reg_beg"], table["reg_end"], table["haps"])
    assert lcd_host.depth_format(rows, "chrS", with_header=True) == dc.HEADER + dc.format_rows(rows, "chrS")
    assert lcd_host.depth_format([], "chrS", with_header=True) == dc.HEADER and lcd_host.depth_format([], "chrS") == ""
    for W in (1, 7, 64, 1000, table["reg_end"], 1 << 30):
        w = dc.windows(rows, W)
        assert lcd_host.depth_windows(rows, W) == w
        assert lcd_host.depth_format(w, "chr1", windows=True, with_header=True) == dc.HEADER_W + dc.format_rows(w, "chr1")
    for seed in range(20):
        recs, rb, re_ = dc.seeded_chunk(seed)
        r, _ = dc.depth_rows([x["body"] for x in recs], rb, re_, dc.haps_of(recs, rb, re_))
        W = 1 + seed * 3
        assert lcd_host.depth_windows(r, W) == dc.windows(r, W) and lcd_host.depth_format(r, "c") == dc.format_rows(r, "c")
    big = [(1, 1 << 31, (0xffffffff, 7, 0)), ((1 << 31) + 1, 1 << 32, (1, 0xffffffff, 2))]
    assert lcd_host.depth_windows(big, 1 << 30) == dc.windows(big, 1 << 30)
    with pytest.raises(lcd_host.LcdError):
        lcd_host.depth_windows(rows, 0)
    with pytest.raises(lcd_host.LcdError):
        lcd_host.depth_windows([rows[0], rows[2]], 5)           # not contiguous
    with pytest.raises(lcd_host.LcdError):
        lcd_host.depth_format([(0, 5, (1, 1, 1))], "c")
    assert lcd_host.depth_tile() >= 64 and lcd_host.depth_tile() % 64 == 0
