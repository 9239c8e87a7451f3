"""lcd_chunk_mod_pileup on the MI355X against the Python oracle of tests/mods_common.py: the whole case table as ONE chunk and one pile-up launch per option set,
and a seeded chunk of about 200 reads of 0.3 - 3 kb over a 6 kb window (both strands, three haplotypes, mixed flags, every kind of bad record).  Rows and
statistics must be equal, not close: the counters are integers."""
import numpy as np
import pytest

import mods_common as mc
from bam_src_common import CONTIG

pytestmark = pytest.mark.gpu


def _chunk(lcd, tmp, name, t, reg_beg, reg_end):
    path = str(tmp / name)
    mc.write_bam(path, t["recs"], block=9000, tlen=t["tlen"])
    return lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, reg_beg, reg_end, min_mapq=30, src=(t["ref"], 1, t["tlen"], 0))


def _same(got, want):
    rows, st = got
    want_rows, want_st = want
    assert {k: st[k] for k in mc.STAT_KEYS} == want_st
    assert rows == want_rows
    assert st["n_rows"] == len(rows)


@pytest.fixture(scope="module")
def table(lcd, tmp_path_factory):
    t = mc.build_cases()
    ch = _chunk(lcd, tmp_path_factory.mktemp("mods"), "cases.bam", t, t["reg_beg"], t["reg_end"])
    yield t, ch
    ch.close()


@pytest.mark.parametrize("code,T,combine", mc.OPTION_SETS)
def test_the_case_table_as_one_chunk(lcd, table, code, T, combine):
    t, ch = table
    assert ch.n == len(t["haps"])
    want = mc.pileup(t["bodies"], t["ref"], 1, t["reg_beg"], t["reg_end"], t["haps"], code=code, T=T, combine=combine)
    got = ch.mod_pileup(t["haps"], t["ref"], 1, t["tlen"], code=code, threshold=T, combine_strands=combine)
    _same(got, want)
    if (code, T, combine) == ("m", 204, False):
        assert got[0] == mc.expected_by_hand(t["cases"])[0]                      # ... which is the table worked out by hand
        assert lcd.mods_format(got[0], CONTIG, "m", with_header=True) == mc.HEADER + mc.format_rows(want[0], CONTIG, "m")
        assert lcd.mods_combine_rows(got[0]) == mc.combine_rows(want[0])


def test_a_window_that_ends_inside_the_region(lcd, table):
    """positions outside the reference window read as N: no site there, and a site whose partner base lies outside the window is none"""
    t, ch = table
    lo, hi = t["reg_beg"] + 1, t["reg_beg"] + 3000
    want = mc.pileup(t["bodies"], t["ref"][lo - 1:hi], lo, t["reg_beg"], t["reg_end"], t["haps"])
    assert want[1]["n_off_context"] > 10
    _same(ch.mod_pileup(t["haps"], t["ref"][lo - 1:hi], lo, hi), want)


def test_refusals(lcd, table):
    t, ch = table
    for kw in (dict(code="a"), dict(code="mh"), dict(threshold=127), dict(threshold=256)):
        with pytest.raises(lcd.LcdError, match="code outside m / h or a threshold"):
            ch.mod_pileup(t["haps"], t["ref"], 1, t["tlen"], **kw)
    with pytest.raises(lcd.LcdError, match="haplotype outside"):
        ch.mod_pileup([3] * ch.n, t["ref"], 1, t["tlen"])
    with pytest.raises(lcd.LcdError, match="no reference window"):
        ch.mod_pileup(t["haps"], b"", 5, 4)
    q = np.full(100, 30, np.uint8)
    host = lcd.DeviceChunk([10], [np.array([(100 << 4) | 7], np.uint32)], [q], [np.full(50, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="not made from a BAM"):
        host.mod_pileup([0], t["ref"], 1, t["tlen"])
    host.close()


def test_an_unresolved_chunk_is_refused(lcd, table, tmp_path):
    t, _ = table
    path = str(tmp_path / "open.bam")
    mc.write_bam(path, t["recs"], block=9000, tlen=t["tlen"])
    ch = lcd.DeviceChunk.open_from_bam(path, path + ".bai", CONTIG, t["reg_beg"], t["reg_end"])
    with pytest.raises(lcd.LcdError, match="not resolved"):
        ch.mod_pileup(t["haps"], t["ref"], 1, t["tlen"])
    ch.close()


def test_a_seeded_chunk(lcd, tmp_path):
    s = mc.seeded()
    rb, re_ = s["first"] + 1, s["first"] + s["span"]
    haps = mc.haps_for(s["bodies"], rb, re_, 1)
    ch = _chunk(lcd, tmp_path, "seeded.bam", s, rb, re_)
    assert ch.n == len(haps) > 150
    want = mc.pileup(s["bodies"], s["ref"], 1, rb, re_, haps)
    rows = want[0]
    # the fixture must have what the comparison is for
    assert any(v[3] + v[4] > 0 and v[6] + v[7] > 0 for _, _, v in rows), "no row with n_h1 > 0 and n_h2 > 0"
    assert any(v[2] + v[5] + v[8] > 0 for _, _, v in rows), "no filtered call"
    assert {x for _, x, _ in rows} == {"+", "-"} and {h for h in haps} == {0, 1, 2}
    _same(ch.mod_pileup(haps, s["ref"], 1, s["tlen"]), want)
    _same(ch.mod_pileup(haps, s["ref"], 1, s["tlen"], code="h", threshold=150, combine_strands=True), mc.pileup(s["bodies"], s["ref"], 1, rb, re_, haps, code="h", T=150, combine=True))
    ch.close()
