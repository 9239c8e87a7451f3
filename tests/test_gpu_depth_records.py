"""lcd_chunk_depth on the MI355X against the Python oracle of tests/depth_common.py: the whole case table as ONE chunk for both values of skip_dels, sub-regions of
it, regions whose lengths straddle the tile of the row launches with run heads on the first and the last position of a tile, a region without records, the
HiFi-like record alone, and a seeded chunk.  Rows and statistics must be equal, not close: the counters are integers."""
import pytest

import depth_common as dc
from bam_src_common import CONTIG

pytestmark = pytest.mark.gpu
INT_KEYS = tuple(k for k in dc.STAT_KEYS)


def _chunk(lcd, path, reg_beg, reg_end):
    return lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, reg_beg, reg_end, min_mapq=30, src=(dc.ref_codes(), 1, dc.TLEN, 0))


def _bam(tmp, name, recs):
    path = str(tmp / name)
    dc.write_bam(path, recs, block=9000, tlen=dc.TLEN)
    return path


def _same(got, want):
    rows, st = got
    want_rows, want_st = want
    print({k: st[k] for k in INT_KEYS}, want_st)
    assert {k: st[k] for k in INT_KEYS} == want_st
    assert rows == want_rows
    assert st["ms_mark"] >= 0 and st["ms_rows"] >= 0


def _check(lcd, path, recs, rb, re_, skip_dels=False):
    haps = dc.haps_of(recs, rb, re_)
    ch = _chunk(lcd, path, rb, re_)
    try:
        assert ch.n == len(haps)
        got = lcd.chunk_depth(ch, haps, skip_dels=skip_dels)
        _same(got, dc.depth_rows([r["body"] for r in recs], rb, re_, haps, skip_dels=skip_dels))
        return got
    finally:
        ch.close()


@pytest.fixture(scope="module")
def table(lcd, tmp_path_factory):
    t = dc.build_cases()
    t["path"] = _bam(tmp_path_factory.mktemp("depth"), "cases.bam", t["recs"])
    ch = _chunk(lcd, t["path"], t["reg_beg"], t["reg_end"])
    yield t, ch
    ch.close()


@pytest.mark.parametrize("skip_dels", [False, True])
def test_the_case_table_as_one_chunk(lcd, table, skip_dels):
    t, ch = table
    assert ch.n == len(t["haps"]) == len(t["recs"])
    want = dc.depth_rows(t["bodies"], t["reg_beg"], t["reg_end"], t["haps"], skip_dels=skip_dels)
    got = lcd.chunk_depth(ch, t["haps"], skip_dels=skip_dels)
    _same(got, want)
    dc.check_tiling(got[0], t["reg_beg"], t["reg_end"], got[1])
    assert lcd.depth_format(got[0], CONTIG, with_header=True) == dc.HEADER + dc.format_rows(want[0], CONTIG)
    assert lcd.depth_windows(got[0], 1000) == dc.windows(want[0], 1000)


@pytest.mark.parametrize("skip_dels", [False, True])
def test_sub_regions_cut_the_cases(lcd, table, skip_dels):
    """regions that begin and end inside records: in the staggered ladder, inside the operation-count cases, one position wide"""
    t, _ = table
    lad = next(c for c in t["cases"] if c["name"] == "staggered_130")["recs"][0]["pos0"] + 1
    o129 = next(c for c in t["cases"] if c["name"] == "ops_129")["recs"][0]["pos0"] + 1
    for rb, re_ in ((lad + 40, lad + 200), (o129 + 30, o129 + 131), (lad + 64, lad + 64), (t["reg_beg"], t["reg_beg"])):
        _check(lcd, t["path"], t["recs"], rb, re_, skip_dels)


def test_the_hifi_like_record_is_one_interval(lcd, tmp_path):
    c = next(c for c in dc.case_table()[0] if c["name"] == "hifi_like_200")
    pos1 = c["recs"][0]["pos0"] + 1
    path = _bam(tmp_path, "hifi.bam", c["recs"])
    _, st = _check(lcd, path, c["recs"], pos1 - 50, pos1 + 300)
    assert st["n_records"] == 1 and st["n_intervals"] == 1
    _, st = _check(lcd, path, c["recs"], pos1 - 50, pos1 + 300, skip_dels=True)
    assert st["n_intervals"] > 10


def test_region_lengths_around_the_tile(lcd, tmp_path):
    T = lcd.depth_tile()
    base = 4001
    recs = dc.tile_records(base, T)
    path = _bam(tmp_path, "tiles.bam", recs)
    for n in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        rows, _ = _check(lcd, path, recs, base, base + n - 1)
        begs = {b - base for b, _, _ in rows}
        if n >= T + 1:
            assert {T - 1, T} <= begs                       # a run head on the last position of a tile and on the first of the next
        if n == 2 * T + 1:
            assert {2 * T - 1, 2 * T} <= begs
    _check(lcd, path, recs, base + 1, base + T)              # the same records, the tile bounds one position further


def test_a_region_without_records(lcd, tmp_path):
    recs = [dc.make_record(b"elsewhere", 3000, [(dc.M, 100)])]
    path = _bam(tmp_path, "one.bam", recs)
    rb, re_ = 9000, 11000
    ch = _chunk(lcd, path, rb, re_)
    try:
        assert ch.n == 0
        rows, st = lcd.chunk_depth(ch, [])
        assert rows == [(rb, re_, (0, 0, 0))] and st["n_rows"] == 1 and st["n_records"] == 0 and st["bases"] == [0, 0, 0] and st["n_intervals"] == 0
    finally:
        ch.close()


def test_a_seeded_chunk(lcd, tmp_path):
    recs, rb, re_ = dc.seeded_chunk(1234, n_rec=150, reg_len=3000)
    path = _bam(tmp_path, "seeded.bam", recs)
    for sd in (False, True):
        _, st = _check(lcd, path, recs, rb, re_, sd)
    assert st["n_intervals"] > st["n_records"] > 50 and st["n_no_overlap"] > 0


def test_refusals(lcd, table, tmp_path):
    import numpy as np
    t, ch = table
    with pytest.raises(lcd.LcdError, match="haplotype outside"):
        lcd.chunk_depth(ch, [3] * ch.n)
    with pytest.raises(ValueError):
        lcd.chunk_depth(ch, t["haps"][:-1])
    q = np.full(100, 30, np.uint8)
    host = lcd.DeviceChunk([10], [np.array([(100 << 4) | 7], np.uint32)], [q], [np.full(50, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="not made from a BAM"):
        lcd.chunk_depth(host, [0])
    host.close()
    op = lcd.DeviceChunk.open_from_bam(t["path"], t["path"] + ".bai", CONTIG, t["reg_beg"], t["reg_end"])
    with pytest.raises(lcd.LcdError, match="not resolved"):
        lcd.chunk_depth(op, t["haps"])
    op.close()
