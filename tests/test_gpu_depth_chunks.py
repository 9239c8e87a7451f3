"""lcd_call_bam_regions_ext2's depth track (align.call_bam_regions(depth=...)) over adjacent regions of one contig on the MI355X.  The file must be the oracle's,
fed each chunk's own final haplotypes as the call returns them, with the writer's seam rule applied: a held last row joins the next chunk's first row when the
depths are equal across the seam, stays apart where they differ, and is written as it is in front of a gap; in window mode a window cut by a seam is one row."""
import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import depth_common as dc
import mods_common as mc

pytestmark = pytest.mark.gpu
NAME = "chr1"


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_chunks")
    ch = cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12)
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    fc.write_multi_fasta(fa, [(NAME, ch["ref"])])

    def span(r):
        return r["pos0"] + 1, r["pos0"] + sum(int(c) >> 4 for c in r["cigar"] if (int(c) & 15) in (0, 2, 3, 7, 8))
    # the quiet seam: nothing begins or ends at it, and every record over it reaches far into both regions, so that both chunks can phase it (a record that
    # reaches a few hundred bases into a region meets no variant there and stays unassigned in that chunk: the records that would do so are left out of the file)
    for quiet in range(4400, 5000):
        reads = [r for r in ch["reads"] if not (span(r)[0] <= quiet < span(r)[1] and (quiet - span(r)[0] < 1300 or span(r)[1] - quiet < 1300))]
        over = [r for r in reads if span(r)[0] <= quiet < span(r)[1]]
        if {r["hap"] for r in over} == {1, 2} and len(over) >= 5 and not any(span(r)[0] == quiet + 1 or span(r)[1] == quiet for r in reads):
            break
    else:
        raise AssertionError("no quiet seam")
    bodies = mc.write_multi_bam_aux(bam, [(NAME, len(ch["ref"]), reads)])
    # where every kept record's cover begins and ends (a D covers): the loud seam is chosen from these
    runs = [r for b in bodies for r in dc.cover_runs(*dc.record_ops(b)[:2], False)]
    begins, ends = {s for s, _ in runs}, {e for _, e in runs}
    assert quiet + 1 not in begins and quiet not in ends
    loud = next(s for s in range(quiet + 1400, 9000) if s + 1 in begins and s not in ends)          # a record begins right behind this one
    assert any(s <= quiet - 100 and e >= loud + 100 for s, e in runs), "no record spans both seams"
    return dict(dir=d, bam=bam, fa=fa, bodies=bodies, quiet=quiet, loud=loud, regs=[(3001, quiet), (quiet + 1, loud), (loud + 1, 10001)])


def _call(lcd, data, tag, regs, **depth):
    path = str(data["dir"] / f"{tag}.bed")
    res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], NAME, [b for b, _ in regs], [e for _, e in regs], min_mapq=30, cfg=cfg_of(lcd),
                               depth=dict(depth, path=path))
    return res, open(path).read()


def _oracle(data, regs, res, W=0, skip_dels=False):
    tabs, sums = [], dict(n_records=0, n_no_cigar=0, n_cg=0, n_no_overlap=0, n_intervals=0, bases=[0, 0, 0])
    for (rb, re_), ch in zip(regs, res["chunks"]):
        haps = [int(h) for h in ch["haps"]]
        assert len(haps) == sum(1 for _, r in bo.region_records(data["bodies"], rb, re_, 30) if r >= 0)
        rows, st = dc.depth_rows(data["bodies"], rb, re_, haps, skip_dels=skip_dels)
        tabs.append((NAME, rows))
        for k in sums:
            sums[k] = [a + b for a, b in zip(sums[k], st[k])] if k == "bases" else sums[k] + st[k]
    out = dc.sink_rows(tabs, W)
    return out, sums


def _stats_equal(res, sums, n_lines):
    st = res["depth"]
    assert {k: st[k] for k in sums} == sums and st["n_rows"] == n_lines and st["ms_mark"] > 0 and st["ms_rows"] > 0


def test_three_adjacent_regions_per_base(lcd, data):
    regs = data["regs"]
    res, text = _call(lcd, data, "base", regs)
    want, sums = _oracle(data, regs, res)
    assert text == dc.HEADER + dc.format_rows(want)
    _stats_equal(res, sums, len(want))
    assert {1, 2} <= {int(h) for c in res["chunks"] for h in c["haps"]}
    assert want[0][1] == regs[0][0] and want[-1][2] == regs[-1][1] and all(a[2] + 1 == b[1] for a, b in zip(want, want[1:]))       # the rows tile the three regions
    # the loud seam: a record begins behind it, the depths differ, the rows stay apart
    assert any(r[2] == data["loud"] for r in want) and any(r[1] == data["loud"] + 1 for r in want)
    # the quiet seam: every record that covers one side covers the other; the rows are one row when the two chunks gave those records the same haplotypes
    ids = [[id(b) for b, r in bo.region_records(data["bodies"], rb, re_, 30) if r >= 0] for rb, re_ in regs[:2]]
    hap = [dict(zip(i, (int(h) for h in c["haps"]))) for i, c in zip(ids, res["chunks"])]
    agree = all(hap[0][k] == hap[1][k] for k in hap[0] if k in hap[1])
    merged = any(r[1] <= data["quiet"] < r[2] for r in want)
    print("quiet seam: haplotypes agree", agree, "merged", merged, [(hap[0][k], hap[1][k]) for k in hap[0] if k in hap[1]])
    assert merged == agree
    assert agree, "the two chunks phased their shared records differently: the merge across the seam was not exercised"


def test_skip_dels_in_a_run(lcd, data):
    regs = data["regs"]
    res, text = _call(lcd, data, "skip", regs, skip_dels=True)
    want, sums = _oracle(data, regs, res, skip_dels=True)
    assert text == dc.HEADER + dc.format_rows(want)
    _stats_equal(res, sums, len(want))
    assert sums["n_intervals"] > sums["n_records"]                               # the reads carry deletions


@pytest.mark.parametrize("W", [900, 1])
def test_three_adjacent_regions_in_windows(lcd, data, W):
    regs = data["regs"]
    res, text = _call(lcd, data, f"win{W}", regs, window=W)
    want, sums = _oracle(data, regs, res, W=W)
    assert text == dc.HEADER_W + dc.format_rows(want)
    _stats_equal(res, sums, len(want))
    if W == 900:
        assert all((e - b + 1) % W for b, e in regs)                             # W divides no region's length
        for seam in (data["quiet"], data["loud"]):
            assert seam % W and any(r[1] <= seam < r[2] for r in want)           # a window cut by a seam is ONE row
        assert [sum(r[3][h] for r in want) for h in range(3)] == sums["bases"]
    else:
        assert len(want) == regs[-1][1] - regs[0][0] + 1


def test_a_gap_between_two_regions(lcd, data):
    regs = [(3001, 5000), (5501, 8000)]
    for W in (0, 700):
        res, text = _call(lcd, data, f"gap{W}", regs, window=W)
        want, sums = _oracle(data, regs, res, W=W)
        assert text == (dc.HEADER_W if W else dc.HEADER) + dc.format_rows(want)
        _stats_equal(res, sums, len(want))
        assert any(r[2] == 5000 for r in want) and any(r[1] == 5501 for r in want) and not any(r[1] <= 5200 <= r[2] for r in want)


def test_depth_beside_mods_and_refusals(lcd, data, tmp_path):
    regs = data["regs"][:1]
    tab = str(tmp_path / "m.tsv")
    path = str(tmp_path / "d.bed")
    res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], NAME, [regs[0][0]], [regs[0][1]], min_mapq=30, cfg=cfg_of(lcd), depth=dict(path=path), mods=dict(path=tab))
    want, _ = _oracle(data, regs, res)
    assert open(path).read() == dc.HEADER + dc.format_rows(want) and open(tab).read() == mc.HEADER and res["mods"]["n_rows"] == 0
    for bad, word in ((dict(path="-"), "goes to a file"), (dict(path=path, window=-1), "window"), (dict(path=tab), "name one file")):
        with pytest.raises(lcd.LcdError, match=word):
            lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], NAME, [regs[0][0]], [regs[0][1]], min_mapq=30, cfg=cfg_of(lcd), depth=bad, mods=dict(path=tab))
