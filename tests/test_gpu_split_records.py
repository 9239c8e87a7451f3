"""lcd_chunk_split_reads on the MI355X against the Python oracle of tests/split_common.py: the whole case table as ONE chunk with the comment off and on, with and
without the list; a plan that skips every second record and reverses the rest; permuted haplotypes; the 20 000-base record alone on both strands; a seeded chunk.
The four streams and the integer statistics must be equal, not close.  The case table's record with a broken layout is not part of the chunk: the loader refuses
a file that holds one, so no chunk can (the oracle's own test covers the rule)."""
import numpy as np
import pytest

import split_common as sc
from bam_src_common import CONTIG

pytestmark = pytest.mark.gpu
NAMES = [CONTIG]


def _ref():
    return np.where(np.random.default_rng(7).integers(0, 2, sc.TLEN) == 0, 0, 3).astype(np.uint8)


def _chunk(lcd, path, reg_beg, reg_end):
    return lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, reg_beg, reg_end, min_mapq=30, src=(_ref(), 1, sc.TLEN, 0))


def _bam(tmp, name, recs):
    path = str(tmp / name)
    sc.write_bam(path, recs, block=9000, tlen=sc.TLEN)
    return path


def _same(got, want, with_list):
    streams, st = got
    fq, lst, want_st = want
    print({k: st[k] for k in sc.STAT_KEYS}, want_st)
    assert {k: st[k] for k in sc.STAT_KEYS} == want_st
    for s in range(3):
        assert streams[s] == fq[s], s
    assert streams[3] == (lst if with_list else b"")
    assert st["ms_measure"] >= 0 and st["ms_emit"] >= 0


@pytest.fixture(scope="module")
def table(lcd, tmp_path_factory):
    t = sc.build_cases(with_broken=False)
    t["path"] = _bam(tmp_path_factory.mktemp("split"), "cases.bam", t["recs"])
    ch = _chunk(lcd, t["path"], t["reg_beg"], t["reg_end"])
    yield t, ch
    ch.close()


@pytest.mark.parametrize("comment", [False, True])
@pytest.mark.parametrize("with_list", [False, True])
def test_the_case_table_as_one_chunk(lcd, table, comment, with_list):
    t, ch = table
    assert ch.n == len(t["haps"]) and len(t["table"]) == len(t["recs"])
    want = sc.split_text(t["table"], t["haps"], t["phase_sets"], names=NAMES if with_list else None, comment=comment)
    got = lcd.chunk_split_reads(ch, t["haps"], t["phase_sets"], names=NAMES if with_list else None, comment=comment, list=with_list)
    _same(got, want, with_list)
    st = got[1]
    assert st["n_not_primary"] == 2 and st["n_no_seq"] == 2 and st["n_filtered_primary"] == 3 and st["n_bad_layout"] == 0 and all(st["n_hap"]) and st["n_reverse"] > 10


def test_skip_every_second_record_and_reverse_the_rest(lcd, table):
    t, ch = table
    n = len(t["table"])
    skip = [i % 2 for i in range(n)]
    order = [i for i in range(n) if not skip[i]][::-1]
    order += [-1] * (n - len(order))
    want = sc.split_text(t["table"], t["haps"], t["phase_sets"], skip=skip, order=order, names=NAMES, comment=True)
    _same(lcd.chunk_split_reads(ch, t["haps"], t["phase_sets"], skip=skip, order=order, names=NAMES, comment=True, list=True), want, True)
    want = sc.split_text(t["table"], t["haps"], t["phase_sets"], skip=skip, names=NAMES)
    _same(lcd.chunk_split_reads(ch, t["haps"], t["phase_sets"], skip=skip, names=NAMES, list=True), want, True)


def test_permuted_haplotypes_and_an_empty_stream(lcd, table):
    t, ch = table
    rng = np.random.default_rng(9)
    haps = [int(h) for h in rng.permutation(t["haps"])]
    pss = [int(p) for p in rng.permutation(t["phase_sets"])]
    _same(lcd.chunk_split_reads(ch, haps, pss, names=NAMES, comment=True, list=True), sc.split_text(t["table"], haps, pss, names=NAMES, comment=True), True)
    # a stream that ends up empty: nobody is on haplotype 2, and the plan leaves every filtered record out
    haps = [1 if h == 2 else h for h in t["haps"]]
    skip = [int(r < 0) for _, r in t["table"]]
    got = lcd.chunk_split_reads(ch, haps, t["phase_sets"], skip=skip, names=NAMES, list=True)
    _same(got, sc.split_text(t["table"], haps, t["phase_sets"], skip=skip, names=NAMES), True)
    assert got[0][2] == b"" and got[1]["n_hap"][2] == 0 and got[1]["n_filtered_primary"] == 0


@pytest.mark.parametrize("strand", ["fwd", "rev"])
def test_the_long_record_alone(lcd, tmp_path, strand):
    rec = next(c["rec"] for c in sc.case_table() if c["name"] == "len_20000_" + strand)
    path = _bam(tmp_path, "long.bam", [rec])
    rb, re_ = rec["pos0"] + 1, rec["pos0"] + 500
    x = sc.table_of([rec], rb, re_)
    ch = _chunk(lcd, path, rb, re_)
    try:
        assert ch.n == 1
        got = lcd.chunk_split_reads(ch, x["haps"], x["phase_sets"], names=NAMES, comment=True, list=True)
        _same(got, sc.split_text(x["table"], x["haps"], x["phase_sets"], names=NAMES, comment=True), True)
        assert got[1]["n_reverse"] == (strand == "rev") and sum(got[1]["bytes_fastq"]) > 40000
    finally:
        ch.close()


def test_a_seeded_chunk(lcd, tmp_path):
    recs, rb, re_ = sc.seeded_chunk(4321, n_rec=200)
    path = _bam(tmp_path, "seeded.bam", recs)
    x = sc.table_of(recs, rb, re_)
    ch = _chunk(lcd, path, rb, re_)
    try:
        assert ch.n == len(x["haps"])
        for comment in (False, True):
            got = lcd.chunk_split_reads(ch, x["haps"], x["phase_sets"], names=NAMES, comment=comment, list=True)
            _same(got, sc.split_text(x["table"], x["haps"], x["phase_sets"], names=NAMES, comment=comment), True)
        st = got[1]
        assert st["n_records"] > 150 and st["n_not_primary"] > 10 and st["n_filtered_primary"] > 10 and st["n_reverse"] > 20 and st["n_no_seq"] > 3
    finally:
        ch.close()


def test_refusals(lcd, table):
    t, ch = table
    with pytest.raises(lcd.LcdError, match="haplotype outside"):
        lcd.chunk_split_reads(ch, [3] * ch.n, t["phase_sets"])
    with pytest.raises(ValueError):
        lcd.chunk_split_reads(ch, t["haps"][:-1], t["phase_sets"])
    with pytest.raises(ValueError):
        lcd.chunk_split_reads(ch, t["haps"], t["phase_sets"], list=True)
    with pytest.raises(lcd.LcdError, match="exactly once"):
        lcd.chunk_split_reads(ch, t["haps"], t["phase_sets"], order=[0] * len(t["table"]))
    op = lcd.DeviceChunk.open_from_bam(t["path"], t["path"] + ".bai", CONTIG, t["reg_beg"], t["reg_end"])
    with pytest.raises(lcd.LcdError, match="not resolved"):
        lcd.chunk_split_reads(op, t["haps"], t["phase_sets"])
    op.close()
