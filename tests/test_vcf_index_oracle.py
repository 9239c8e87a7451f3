"""The .tbi / .csi oracle checked against itself (tests/vcf_index_common.py; no library, no device): every named case reaches the condition it is named after, and
for seeded files a reader that follows the specifications -- the region's bins, htslib's lookup of the smallest offset, chunk ranges, overlap filter -- finds
through the oracle's own TBI and CSI exactly the lines a scan of the whole file finds.  That pins the loffset rule (rule 9) before any kernel runs."""
import numpy as np
import pytest

import vcf_index_common as vc


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_named_case_reaches_its_condition(name):
    gz, fmt, pred, refusal = vc.CASES[name]()
    if refusal is not None:
        with pytest.raises(vc.Refused) as e:
            vc.oracle_index(vc.scan_vcf(gz, fmt), fmt)
        assert (e.value.code, e.value.line) == refusal
        return
    scan = vc.scan_vcf(gz, fmt)
    idx = vc.parse_index(vc.oracle_index(scan, fmt))
    assert idx["hdr"]["names"] == scan["names"] and (idx["hdr"]["format"], idx["hdr"]["col_seq"], idx["hdr"]["col_beg"], idx["hdr"]["col_end"], idx["hdr"]["meta"]) == (2, 1, 2, 0, 35)
    assert pred(scan, idx), name


def test_end_over_2_29_is_a_csi_file():
    gz, _fmt, _pred, _ref = vc.CASES["refused_end_over_2_29_tbi"]()
    idx = vc.parse_index(vc.oracle_index(vc.scan_vcf(gz, vc.CSI), vc.CSI))
    assert idx["depth"] == 6


@pytest.mark.parametrize("seed", vc.SEEDS)
@pytest.mark.parametrize("lengths", [True, False])
def test_region_reader_finds_what_a_scan_finds(seed, lengths):
    gz = vc.seeded_gz(seed, 300, lengths)
    scan = vc.scan_vcf(gz, vc.CSI)
    rng = np.random.default_rng(seed)
    idxs = [vc.parse_index(vc.oracle_tbi(scan)), vc.parse_index(vc.oracle_csi(scan))]
    n_regions = n_hits = n_unset = n_past = 0
    for tid in range(len(scan["names"])):
        last = max(x["end"] for x in scan["lines"] if x["tid"] == tid)
        for beg, end in vc.regions_for(rng, scan, tid, 40):
            want = vc.lines_by_scan(scan, tid, beg, end)
            for idx in idxs:
                assert vc.lines_through_index(scan, idx, tid, beg, end) == want, (idx["fmt"], tid, beg, end)
            n_regions += 1; n_hits += bool(want); n_past += beg >= last
            lin = idxs[0]["refs"][tid]["lin"]
            w = beg >> 14
            n_unset += w < len(lin) and not any(x["tid"] == tid and x["beg"] >> 14 <= w <= (x["end"] - 1) >> 14 for x in scan["lines"])
    assert n_regions >= 150 and n_hits >= n_regions // 3 and n_unset >= 1 and n_past >= 4


def test_loffset_is_the_first_set_window_of_the_bin():
    """rule 9's two statements agree: the smallest vbeg over the overlapping lines == the value of the first set 16 kb window inside the bin's span"""
    scan = vc.scan_vcf(vc.seeded_gz(vc.SEEDS[0], 300), vc.CSI)
    idx = vc.parse_csi(vc.oracle_csi(scan))
    tbi = vc.parse_tbi(vc.oracle_tbi(scan))
    for tid, r in enumerate(idx["refs"]):
        win = {}
        for x in scan["lines"]:
            if x["tid"] == tid:
                for w in range(x["beg"] >> 14, ((x["end"] - 1) >> 14) + 1):
                    win[w] = min(win.get(w, x["vbeg"]), x["vbeg"])
        for b, lo in r["loff"].items():
            b0, b1 = vc.bin_interval(b, idx["depth"])
            assert lo == win[min(w for w in win if b0 >> 14 <= w < b1 >> 14)]
        assert set(r["bins"]) == set(tbi["refs"][tid]["bins"])          # depth 5: the same bins, the same chunks
