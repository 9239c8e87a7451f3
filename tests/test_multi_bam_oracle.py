"""lcd_merged_record_plan (pure host code) against the Python statement of rules 1, 4 and 5 (tests/multi_bam_common.py): on the record tables of the seeded
contigs dealt out to two files, and on hand-made tables.  The test proves from the Python side alone that the conditions it is about are reached: records left out
that are not a prefix of the file-major table, per-file counts that differ, a tie on pos0 between two files."""
import ctypes as C

import pytest

import multi_bam_common as mb


@pytest.fixture(scope="module")
def tables():
    """per contig and region: the file-major record table of files A (even reads) and B (odd reads) with the filtered records over every border"""
    out = []
    for name, ch in mb.seeded_contigs().items():
        L = len(ch["ref"])
        regs = mb.regions_of(L)
        files = mb.deal(ch["reads"], name, 2, borders=[e for _, e in regs[:-1]])
        for c, (rb, re_) in enumerate(regs):
            rows, reads = mb.chunk_table(files, rb, re_)
            out.append(dict(contig=name, c=c, rows=rows, reads=reads, prev=regs[c - 1] if c > 0 else None))
    return out


def test_the_data_reaches_the_conditions(tables):
    seen = dict(non_prefix=0, counts_differ=0, filtered_left_out=0, both_files=0)
    for t in tables:
        if t["prev"] is None:
            continue
        skip, _ = mb.python_plan(t["rows"], 1, *t["prev"], 0)
        per_file = [sum(1 for r, s in zip(t["rows"], skip) if s and r["file"] == f) for f in (0, 1)]
        first_kept = min(i for i, s in enumerate(skip) if not s)
        seen["non_prefix"] += any(skip[first_kept:])                       # a record behind the first written one is left out: not a prefix of the table
        seen["counts_differ"] += per_file[0] != per_file[1]
        seen["both_files"] += per_file[0] > 0 and per_file[1] > 0
        seen["filtered_left_out"] += any(s and r["read"] < 0 for r, s in zip(t["rows"], skip))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    # positions inside a file are sorted, and the kept reads' positions are distinct over both files
    for t in tables:
        for f in (0, 1):
            p = [r["pos0"] for r in t["rows"] if r["file"] == f]
            assert p == sorted(p)
        kept = [r["pos0"] for r in t["rows"] if r["read"] >= 0]
        assert len(set(kept)) == len(kept)
        assert [r["read"] for r in t["rows"] if r["read"] >= 0] == list(range(len(t["reads"])))     # read ids are file-major


@pytest.mark.parametrize("sort_output", [0, 1])
def test_plan_equals_the_rules_on_the_seeded_tables(lcd, tables, sort_output):
    for t in tables:
        prev = t["prev"] or (0, 0)
        want = mb.python_plan(t["rows"], t["prev"] is not None, *prev, sort_output)
        got = mb.plan_of(lcd, t["rows"], int(t["prev"] is not None), *prev, sort_output)
        assert got == ([bool(s) for s in want[0]], want[1]), (t["contig"], t["c"])
        if sort_output:
            p = [t["rows"][i]["pos0"] for i in got[1]]
            assert p == sorted(p)
        else:
            assert got[1] == sorted(got[1])                                # table order


def row(file, idx, pos0, end, read=0):
    return dict(file=file, idx=idx, pos0=pos0, end=end, read=read)


HAND = {
    "one_file": [row(0, 0, 10, 50), row(0, 1, 20, 60), row(0, 2, 120, 150), row(0, 3, 130, 131, -1)],
    "a_file_with_no_record": [row(0, 0, 10, 50), row(0, 1, 150, 160), row(2, 0, 5, 40), row(2, 1, 101, 140)],                     # file 1 contributes nothing
    "every_record_left_out": [row(0, 0, 10, 50), row(1, 0, 20, 99), row(1, 1, 99, 100, -1)],
    "equal_pos0_in_two_files": [row(0, 0, 110, 150), row(0, 1, 130, 160), row(1, 0, 110, 140), row(1, 1, 110, 120, -1), row(1, 2, 130, 170)],
    "ends_touch_the_border": [row(0, 0, 50, 99), row(0, 1, 50, 100), row(0, 2, 100, 140), row(1, 0, 99, 101), row(1, 1, 100, 101)],    # [pos0 + 1, end] against [1, 100]
}


@pytest.mark.parametrize("name", sorted(HAND))
@pytest.mark.parametrize("has_prev,sort_output", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_plan_equals_the_rules_on_hand_made_tables(lcd, name, has_prev, sort_output):
    rows = HAND[name]
    want = mb.python_plan(rows, has_prev, 1, 100, sort_output)
    got = mb.plan_of(lcd, rows, has_prev, 1, 100, sort_output, with_files=name != "one_file")
    assert got == want
    if not has_prev:
        assert not any(got[0]) and sorted(got[1]) == list(range(len(rows)))           # has_prev 0: nothing is left out
    if name == "every_record_left_out" and has_prev:
        assert all(got[0]) and got[1] == []
    if name == "equal_pos0_in_two_files" and sort_output:
        assert got[1] == [0, 2, 3, 1, 4]                                              # the tie on 110: file 0 first, then file 1's records in file order
    if name == "ends_touch_the_border" and has_prev:
        assert got[0] == [True, True, False, True, False]                             # pos0 + 1 == 100 overlaps, pos0 + 1 == 101 does not


def test_one_file_unsorted_plan_is_the_prefix_rule(lcd, tables):
    """one sorted file, sort_output 0: "skip the first nsk kept and nsf filtered records, keep table order" -- what lcd_chunk_tag_records' counts say"""
    n_with_skips = 0
    for t in tables:
        if t["prev"] is None:
            continue
        for f in (0, 1):
            rows = [r for r in t["rows"] if r["file"] == f]
            skip, order = mb.plan_of(lcd, rows, 1, *t["prev"], 0, with_files=False)
            nsk = sum(1 for r, s in zip(rows, skip) if s and r["read"] >= 0); nsf = sum(1 for r, s in zip(rows, skip) if s and r["read"] < 0)
            want, sk, sf = [], nsk, nsf
            for i, r in enumerate(rows):
                if r["read"] >= 0 and sk > 0:
                    sk -= 1; continue
                if r["read"] < 0 and sf > 0:
                    sf -= 1; continue
                want.append(i)
            assert order == want
            n_with_skips += nsk > 0 and nsf > 0
    assert n_with_skips > 0


def test_plan_argument_errors(lcd):
    lib = lcd.load_library()
    one = (C.c_int64 * 1)(5); sk = (C.c_uint8 * 1)(); od = (C.c_int * 1)()
    assert lib.lcd_merged_record_plan(-1, None, one, one, 0, 0, 0, 0, sk, od) == -4
    for args in ((None, one, sk, od), (one, None, sk, od), (one, one, None, od), (one, one, sk, None)):
        assert lib.lcd_merged_record_plan(1, None, args[0], args[1], 0, 0, 0, 0, args[2], args[3]) == -4
    assert b"lcd_merged_record_plan" in lib.lcd_last_error()
    assert lib.lcd_merged_record_plan(0, None, None, None, 1, 1, 2, 1, None, None) == 0          # an empty table
