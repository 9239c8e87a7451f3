"""lcd_chunk_refine_records on the MI355X: one tiny BAM that holds every case of tests/refine_cases.py at once, its records rewritten in HBM from their reads' final
digars -- CIGAR, POS, bin, NM / MD / cs, then HP / PS -- byte for byte against the oracle of tests/refine_common.py, with the stats, under a skip / order
selection, and one record per call against all records in one launch."""
import struct

import numpy as np
import pytest

import bam_out_common as bo
import refine_cases as cases
import refine_common as rc
from bam_src_common import CONTIG, write_bam

pytestmark = pytest.mark.gpu
STAT_KEYS = ("n_records", "n_kept", "n_refined", "n_identical", "n_unrefined", "n_pos_moved", "n_no_digars", "n_qlen_mismatch", "n_bad_pos", "n_too_many_ops",
             "n_cg_cigar", "n_nm_replaced", "n_md_replaced", "n_cs_replaced")


@pytest.fixture(scope="module")
def setup(lcd, oracle, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("refine") / "r.bam")
    cs = cases.build()
    write_bam(path, [c["rec"] for c in cs], block=9000, tlen=cases.TLEN)
    digars_of, skipped, touched, kept = cases.resolve(cs, oracle)
    ch = lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, 1, cases.TLEN, min_mapq=cases.MIN_MAPQ, src=(cases.letters(), 1, cases.TLEN, 0))
    recs = bo.region_records([c["rec"]["body"] for c in cs], 1, cases.TLEN, cases.MIN_MAPQ)
    haps = [cs[i]["hap"] for i in kept]; ps = [cs[i]["ps"] for i in kept]
    want = rc.refined_stream(recs, digars_of, skipped, cases.WIN, cases.REF_BEG, cases.REF_END, haps, ps)
    yield dict(ch=ch, cs=cs, recs=recs, digars_of=digars_of, skipped=skipped, touched=touched, kept=kept, haps=haps, ps=ps, want=want)
    ch.close()


def _call(s, **kw):
    return s["ch"].refine_records(s["haps"], s["ps"], kw.pop("touched", s["touched"]), kw.pop("ref", cases.WIN), cases.REF_BEG, cases.REF_END, **kw)


def test_g1_every_case_byte_for_byte(setup):
    s = setup
    ch, cs, kept = s["ch"], s["cs"], s["kept"]
    assert ch.n == len(kept) == len(cs) - 1
    # the untouched reads' digars in HBM are the ones the oracle was given
    info, dg = ch.read_info(), ch.digars()
    for r, i in enumerate(kept):
        assert (info["status"][r] != 0) == s["skipped"][r], cs[i]["name"]
        if isinstance(cs[i]["digars"], str):
            if not s["skipped"][r]:
                assert dg[r].tolist() == [list(map(int, d)) for d in s["digars_of"][r]], cs[i]["name"]
    want, n_want, st_want, states = s["want"]
    got, n_got, st = _call(s)
    assert n_got == n_want == len(cs)
    o = 0
    for c, state in zip(cs, states):                                       # record by record: a mismatch names its case
        ln = struct.unpack("<i", want[o:o + 4])[0] + 4
        assert got[o:o + ln] == want[o:o + ln], (c["name"], state)
        o += ln
    assert got == want
    for k in STAT_KEYS:
        assert st[k] == st_want[k], k
    assert st["n_touched"] == len(s["touched"]) and st["bytes_digars_up"] == 24 * sum(len(d) for d in s["touched"].values()) and st["bytes_ref_up"] == len(cases.WIN)


def test_g1_selection_and_one_record_per_call(setup):
    s = setup
    n = len(s["recs"])
    want_all = s["want"][0]
    _, bodies = bo.bam_split(b"BAM\x01" + struct.pack("<ii", 0, 0) + want_all)
    skip = np.zeros(n, np.uint8); skip[[2, 5, n - 1]] = 1
    order = [i for i in range(n) if not skip[i]][::-1]
    w, nw, stw, _ = rc.refined_stream(s["recs"], s["digars_of"], s["skipped"], cases.WIN, cases.REF_BEG, cases.REF_END, s["haps"], s["ps"], skip, order)
    g, ng, st = _call(s, skip=skip, order=order)
    assert (ng, g) == (nw, w) and all(st[k] == stw[k] for k in STAT_KEYS)
    g, ng, _ = _call(s, skip=skip)                                         # table order
    assert ng == n - 3 and g == b"".join(struct.pack("<i", len(bodies[i])) + bodies[i] for i in range(n) if not skip[i])
    for i in range(n):                                                     # one record per call == its bytes in the one launch
        one = np.ones(n, np.uint8); one[i] = 0
        g, ng, _ = _call(s, skip=one)
        assert ng == 1 and g == struct.pack("<i", len(bodies[i])) + bodies[i], s["cs"][i]["name"]


def test_g1_window_spellings_and_no_touched_reads(setup):
    s = setup
    want = s["want"][0]
    let = cases.letters()[cases.REF_BEG - 1:cases.REF_END]
    assert _call(s, ref=let)[0] == want and _call(s, ref=let.lower())[0] == want
    recs = s["recs"]
    w, _, stw, _ = rc.refined_stream(recs, s["digars_of"], s["skipped"], None, 1, 0, s["haps"], s["ps"])
    g, _, st = s["ch"].refine_records(s["haps"], s["ps"], s["touched"], None)
    assert g == w and w != want and st["bytes_ref_up"] == 0
    # without touched reads every kept record follows the chunk's own digars
    own = [d.tolist() for d in s["ch"].digars()]
    w, _, stw, _ = rc.refined_stream(recs, own, s["ch"].read_info()["status"] != 0, cases.WIN, cases.REF_BEG, cases.REF_END, s["haps"], s["ps"])
    g, _, st = _call(s, touched={})
    assert g == w and all(st[k] == stw[k] for k in STAT_KEYS) and st["bytes_digars_up"] == 0


def test_g1_refusals(lcd, setup):
    s = setup
    with pytest.raises(lcd.LcdError, match="touched_reads"):
        _call(s, touched={s["ch"].n: [[10, 7, 5, 0, 0]]})
    with pytest.raises(lcd.LcdError, match="digar"):
        _call(s, touched={0: [[10, 9, 5, 0, 0]]})
    with pytest.raises(lcd.LcdError, match="order"):
        _call(s, order=[0] * len(s["recs"]))
    q = np.full(100, 30, np.uint8)
    ch = lcd.DeviceChunk([10], [np.array([(100 << 4) | 7], np.uint32)], [q], [np.full(50, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="not made from a BAM"):
        ch.refine_records([0], [0])
    ch.close()
