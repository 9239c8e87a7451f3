"""lcd_chunk_haplotag on the MI355X against the Python oracle of tests/haplotag_common.py: the whole case table as ONE chunk (records of 1 ... 129 operations with
sites on their first and last position, a deletion and an insertion across the 64-operation step, D next to I, an SNV under D and N, wrong insertions, dense sites
with 3 ... 70 pairs, three phase sets with a tie, qualities, a CG-field record, clipped footprints, duplicates), the same with min_bq 20 and min_diff 2, a sub-region,
records without bases, a table without sites and a seeded diploid chunk.  Haplotypes, phase sets, n1 / n2, the candidates' offsets, every verdict byte and the
integer statistics must be equal, not close.  A record cut short in its block is not part of any chunk: the loader refuses a file that holds one, so no chunk can
(the kernel keeps its own bound all the same; the oracle's test covers the rule)."""
import numpy as np
import pytest

import haplotag_common as hc
from bam_src_common import CONTIG

pytestmark = pytest.mark.gpu


def _codes(ref):
    return np.array(["ACGT".index(c) for c in ref], np.uint8)


def _chunk(lcd, path, reg_beg, reg_end, ref, tlen):
    return lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, reg_beg, reg_end, min_mapq=30, src=(_codes(ref), 1, tlen, 0))


def _files(tmp, name, recs, vcf, tlen):
    path = str(tmp / (name + ".bam"))
    hc.write_bam(path, recs, block=9000, tlen=tlen)
    vpath = str(tmp / (name + ".vcf"))
    open(vpath, "w").write(vcf)
    return path, vpath


def _same(got, want):
    print(got["stats"], want["stats"])
    for k in ("haps", "phase_sets", "n1", "n2", "first_site", "cand_off"):
        assert got[k] == want[k], k
    assert got["verdict"].tolist() == want["verdict"]
    assert {k: got["stats"][k] for k in hc.TAG_STAT_KEYS} == want["stats"]
    assert all(got["stats"][k] >= 0 for k in ("ms_measure", "ms_mark", "ms_reduce"))


@pytest.fixture(scope="module")
def table(lcd, tmp_path_factory):
    t = hc.build_cases()
    t["path"], t["vpath"] = _files(tmp_path_factory.mktemp("haplotag"), "cases", t["recs"], t["vcf"], hc.TLEN)
    vcf = lcd.phased_vcf_read(t["vpath"], [CONTIG])
    ch = _chunk(lcd, t["path"], t["reg_beg"], t["reg_end"], hc.ref_bases(), hc.TLEN)
    yield t, vcf, ch
    ch.close(); vcf.close()


@pytest.mark.parametrize("min_bq,min_diff", [(0, 1), (20, 2)])
def test_the_case_table_as_one_chunk(lcd, table, min_bq, min_diff):
    t, vcf, ch = table
    assert hc.table_of_lib(vcf.sites(0)) == t["table"] and vcf.stats == t["vcf_stats"]
    want = hc.haplotag(t["table"], t["bodies"], t["reg_beg"], t["reg_end"], min_bq=min_bq, min_diff=min_diff)
    assert ch.n == len(want["haps"])
    got = lcd.chunk_haplotag(ch, vcf, 0, min_bq=min_bq, min_diff=min_diff, pairs=True)
    _same(got, want)
    assert got["stats"]["n_verdict"][hc.LOWQ] == (1 if min_bq else 0) and got["stats"]["n_multi_ps"] >= 2 and got["stats"]["n_cg"] == 1
    plain = lcd.chunk_haplotag(ch, vcf, 0, min_bq=min_bq, min_diff=min_diff)      # the same call without the pair arrays
    assert "verdict" not in plain and plain["haps"] == want["haps"] and plain["phase_sets"] == want["phase_sets"]


def test_a_sub_region_and_the_dense_slot(lcd, table):
    """chunks that hold some of the records: the table in HBM is the one the first call made"""
    t, vcf, _ = table
    for name in ("dense_pairs", "three_sets_tie", "ops_129"):
        c = next(c for c in t["cases"] if c["name"] == name)
        rb = t["reg_beg"] + 100 + hc.SLOT * c["slot"]
        ch = _chunk(lcd, t["path"], rb - 10, rb + 200, hc.ref_bases(), hc.TLEN)
        try:
            want = hc.haplotag(t["table"], t["bodies"], rb - 10, rb + 200)
            assert ch.n == len(want["haps"]) == len(c["recs"])
            _same(lcd.chunk_haplotag(ch, vcf, 0, pairs=True), want)
        finally:
            ch.close()


def test_records_without_bases(lcd, table, tmp_path):
    """l_seq == 0: an SNV is OTHER, a covered indel site REF, an I operation disturbs; counted in n_no_seq"""
    t, vcf, _ = table
    at = t["reg_beg"] + 100 + hc.SLOT * next(c["slot"] for c in t["cases"] if c["name"] == "ins_wrong_bases")
    qa = t["reg_beg"] + 100 + hc.SLOT * next(c["slot"] for c in t["cases"] if c["name"] == "quality")
    recs = [hc.make_record(b"noseq", at, [(hc.EQ, 30)], no_seq=True), hc.make_record(b"noseq_i", at, [(hc.EQ, 10), (hc.I, 3), (hc.EQ, 10)], no_seq=True),
            hc.make_record(b"withseq", at, [(hc.EQ, 10), (hc.I, 3), (hc.EQ, 10)], ins={1: "ACG"}), hc.make_record(b"noseq_s", qa, [(hc.EQ, 30)], no_seq=True),
            hc.make_record(b"last", qa + 5, [(hc.EQ, 30)])]
    path, _ = _files(tmp_path, "noseq", recs, t["vcf"], hc.TLEN)
    ch = _chunk(lcd, path, at - 50, qa + 100, hc.ref_bases(), hc.TLEN)
    try:
        want = hc.haplotag(t["table"], [r["body"] for r in recs], at - 50, qa + 100)
        assert want["stats"]["n_no_seq"] == 3 and [[v for v in x["verdicts"] if v != hc.NO_PAIR] for x in want["recs"]][:4] == [[hc.REF], [hc.OTHER], [hc.ALT], [hc.OTHER]]
        _same(lcd.chunk_haplotag(ch, vcf, 0, pairs=True), want)
    finally:
        ch.close()


def test_a_table_without_sites_and_another_contig(lcd, table, tmp_path):
    t, _, ch = table
    vpath = str(tmp_path / "two.vcf")
    open(vpath, "w").write(t["vcf"].replace("##contig", "##x"))
    vcf = lcd.phased_vcf_read(vpath, ["empty", CONTIG])
    try:
        assert len(vcf.sites(0)["pos"]) == 0
        got = lcd.chunk_haplotag(ch, vcf, 0, pairs=True)
        empty = dict(t["table"], **{k: [] for k in hc.TABLE_KEYS + ("ps_value", "pool")}, max_footprint=0)
        _same(got, hc.haplotag(empty, t["bodies"], t["reg_beg"], t["reg_end"]))
        assert got["stats"]["n_tagged"] == [ch.n, 0, 0] and got["stats"]["n_pairs"] == 0
        _same(lcd.chunk_haplotag(ch, vcf, 1, pairs=True), hc.haplotag(t["table"], t["bodies"], t["reg_beg"], t["reg_end"]))
    finally:
        vcf.close()


def test_a_seeded_diploid_chunk(lcd, tmp_path):
    sim = hc.simulate(5, n_reads=300)
    path, vpath = _files(tmp_path, "sim", sim["recs"], sim["vcf"], sim["length"])
    vcf = lcd.phased_vcf_read(vpath, ["sim"])
    ch = _chunk(lcd, path, 1, sim["length"], sim["ref"], sim["length"])
    try:
        tabs, _ = hc.read_vcf(sim["vcf"].encode(), ["sim"])
        want = hc.haplotag(tabs[0], [r["body"] for r in sim["recs"]], 1, sim["length"])
        assert ch.n == 300
        got = lcd.chunk_haplotag(ch, vcf, 0, pairs=True)
        _same(got, want)
        voted = [(h, r["true_hap"]) for h, a, b, r in zip(got["haps"], got["n1"], got["n2"], sim["recs"]) if a + b]
        assert len(voted) > 250 and all(h == th for h, th in voted)
    finally:
        ch.close(); vcf.close()


def test_refusals(lcd, table):
    t, vcf, ch = table
    with pytest.raises(lcd.LcdError, match="min_diff"):
        lcd.chunk_haplotag(ch, vcf, 0, min_diff=0)
    with pytest.raises(lcd.LcdError, match="min_bq"):
        lcd.chunk_haplotag(ch, vcf, 0, min_bq=255)
    with pytest.raises(lcd.LcdError, match="contig outside"):
        lcd.chunk_haplotag(ch, vcf, 1)
    q = np.full(100, 30, np.uint8)
    host = lcd.DeviceChunk([10], [np.array([(100 << 4) | 7], np.uint32)], [q], [np.full(50, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="not made from a BAM"):
        lcd.chunk_haplotag(host, vcf, 0)
    host.close()
    op = lcd.DeviceChunk.open_from_bam(t["path"], t["path"] + ".bai", CONTIG, t["reg_beg"], t["reg_end"])
    with pytest.raises(lcd.LcdError, match="not resolved"):
        lcd.chunk_haplotag(op, vcf, 0)
    op.close()
