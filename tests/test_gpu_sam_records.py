"""lcd_records_to_sam on the MI355X: the case table of tests/sam_out_common.py formatted in HBM (bam_sam_kernel.hip), byte for byte against the oracle -- the whole
table in one call, rotated by one, two and three records (every record and every line starts at each offset modulo 4), every case alone, the large record, and the
statistics the oracle derives."""
import ctypes as C

import pytest

import sam_out_common as so

pytestmark = pytest.mark.gpu
TIMES = ("ms_measure", "ms_emit", "ms_download_write")


@pytest.fixture(scope="module")
def table():
    cs = so.cases()
    return cs, [so.sam_line(b, so.NAMES)[0] for _, b in cs]


def counters(st):
    return {k: v for k, v in st.items() if k not in TIMES}


def compare(cs, lines, got, st, rot=0):
    """line by line: a mismatch names its condition"""
    order = list(range(rot, len(cs))) + list(range(rot))
    o = 0
    for i in order:
        n = len(lines[i])
        assert got[o:o + n] == lines[i], (cs[i][0], rot)
        o += n
    assert o == len(got)
    assert counters(st) == so.sam_text([cs[i][1] for i in order], so.NAMES)[1]


def test_the_case_table_in_one_call(lcd, table):
    cs, lines = table
    got, st = lcd.records_to_sam(so.stream([b for _, b in cs]), so.NAMES)
    compare(cs, lines, got, st)
    starts = {sum(4 + len(b) for _, b in cs[:i]) % 4 for i in range(len(cs))}
    assert starts == {0, 1, 2, 3} and {sum(len(x) for x in lines[:i]) % 4 for i in range(len(cs))} == {0, 1, 2, 3}
    assert st["n_float_values"] > 200 and st["n_cg_cigar"] == 2 and st["n_walk_stopped"] == 5 and st["n_bad_layout"] == 6


@pytest.mark.parametrize("rot", [1, 2, 3])
def test_the_table_rotated(lcd, table, rot):
    cs, lines = table
    got, st = lcd.records_to_sam(so.stream([b for _, b in cs[rot:] + cs[:rot]]), so.NAMES)
    compare(cs, lines, got, st, rot)


def test_every_case_alone(lcd, table):
    cs, lines = table
    for (name, body), want in zip(cs, lines):
        got, st = lcd.records_to_sam(so.stream([body]), so.NAMES)
        assert got == want, name
        assert counters(st) == so.sam_text([body], so.NAMES)[1], name


def test_the_large_record(lcd):
    """l_seq 70 001, 40 000 CIGAR words, a B:C array of 70 001 elements; behind and in front of a short record"""
    big, small = so.big_record(), so.mk(b"s", qlen=3)
    want, wst = so.sam_text([small, big, small], so.NAMES)
    got, st = lcd.records_to_sam(so.stream([small, big, small]), so.NAMES)
    assert len(got) == len(want) > 500000 and got == want and counters(st) == wst


def test_names_and_the_empty_stream(lcd):
    got, st = lcd.records_to_sam(b"", so.NAMES)
    assert got == b"" and st["n_records"] == 0 and st["bytes_text"] == 0
    body = so.mk(b"n", refid=1, nrefid=0)
    assert lcd.records_to_sam(so.stream([body]), [])[0] == so.sam_line(body, [])[0] == b"n\t0\t*\t101\t60\t8M\t*\t0\t0\tACGTACGT\t!(/6=DKR\n"
    assert lcd.records_to_sam(so.stream([body]), [b"a", b""])[0] == so.sam_line(body, [b"a", b""])[0] == b"n\t0\t*\t101\t60\t8M\ta\t0\t0\tACGTACGT\t!(/6=DKR\n"


def test_a_stream_that_ends_inside_a_record_is_refused(lcd):
    s = so.stream([so.mk(b"a"), so.mk(b"b")])
    for cut in (s[:-1], s[:len(s) // 2 + 3], s + b"\x01\0", s + b"\x10\0\0\0" + b"\0" * 16):
        with pytest.raises(lcd.LcdError, match="ends inside a record|shorter than its fixed fields"):
            lcd.records_to_sam(cut, so.NAMES)
    lib = lcd.load_library()
    with lcd._SamNames(so.NAMES) as nm:
        assert not lib.lcd_records_to_sam((C.c_uint8 * 8)(*s[:8]), 8, nm.h, None)
        assert lib.lcd_last_error().startswith(b"lcd_records_to_sam") and lcd.records_to_sam(s, so.NAMES)[0].count(b"\n") == 2
