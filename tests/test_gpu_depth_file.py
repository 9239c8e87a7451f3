"""lcd_call_files_ext2's depth track (align.call_file(depth=...), --depth FILE) on the MI355X: the synthetic two-contig BAM called in windows of chunks.  The
yardstick is per contig: lcd_call_bam_regions_ext2 with the contig's planned regions returns every chunk's final haplotypes; the oracle with each chunk's own
haplotypes and the writer's seam rule must give the contig's track, and the contigs' tracks one after the other must be the file driver's, per base and in windows,
with and without an alignment output, beside the methylation table, from two input files and through the command line.  The VCF, the BAM and the methylation table
must be the bytes of the run without the option; a run that fails leaves no track."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import depth_common as dc
import mods_common as mc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHUNK_LEN = 6000
W = 2500
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_file")
    rng = np.random.default_rng(77)
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(41, ref_len=12000, depth=12))
    order = ["chr1", "chr2"]
    reads = {k: [mc.add_calls(rng, r) for r in chs[k]["reads"]] for k in order}
    refs = {k: chs[k]["ref"] for k in order}
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    bodies = mc.write_multi_bam_aux(bam, [(k, len(refs[k]), reads[k]) for k in order])
    halves = [str(d / "a.bam"), str(d / "b.bam")]
    for h, path in enumerate(halves):
        mc.write_multi_bam_aux(path, [(k, len(refs[k]), reads[k][h::2]) for k in order])
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in order])
    return dict(dir=d, bam=bam, halves=halves, fa=fa, refs=refs, order=order, bodies=bodies)


def run(lcd, data, tag, depth=True, bam_out=True, mods=False, bams=None, **kw):
    vcf, out, trk, tab = (str(data["dir"] / f"{tag}.{x}") for x in ("vcf", "bam", "bed", "tsv"))
    kw.setdefault("chunk_len", CHUNK_LEN)
    args = dict(vcf_path=vcf, no_vcf_header=1, cfg=cfg_of(lcd), contig_mode=2, bam_out=dict(path=out, pg_line=PG) if bam_out else None, **kw)
    if depth:
        args["depth"] = dict(path=trk) if depth is True else dict(depth, path=trk)
    if mods:
        args["mods"] = dict(path=tab)
    res = lcd.call_files(bams, data["fa"], **args) if bams else lcd.call_file(data["bam"], data["fa"], **args)
    res["vcf_bytes"] = open(vcf, "rb").read()
    res["bam_bytes"] = open(out, "rb").read() if bam_out else None
    res["track"] = open(trk).read() if depth else None
    res["table"] = open(tab).read() if mods else None
    return res


@pytest.fixture(scope="module")
def base(lcd, data):
    return run(lcd, data, "base", window_chunks=3)


@pytest.fixture(scope="module")
def yard(lcd, data):
    """per contig lcd_call_bam_regions_ext2 with the contig's planned regions -> the chunks' final haplotypes; from them the oracle's tables and statistics"""
    contigs = [(k, len(data["refs"][k])) for k in data["order"]]
    plan, _ = lcd.plan_chunks(contigs, contig_mode=2, chunk_len=CHUNK_LEN)
    assert [(t, e - b + 1) for t, b, e in plan] == [(0, 6000)] * 2 + [(1, 6000)] * 2
    tabs, sums = [], dict(n_records=0, n_no_cigar=0, n_cg=0, n_no_overlap=0, n_intervals=0, bases=[0, 0, 0])
    for tid, name in enumerate(data["order"]):
        mine = [(b, e) for t, b, e in plan if t == tid]
        trk = str(data["dir"] / f"yard_{name}.bed")
        res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], name, [b for b, _ in mine], [e for _, e in mine], min_mapq=30, cfg=cfg_of(lcd), depth=dict(path=trk))
        mine_tabs = []
        for (rb, re_), ch in zip(mine, res["chunks"]):
            haps = [int(h) for h in ch["haps"]]
            assert len(haps) == sum(1 for _, r in bo.region_records(data["bodies"], rb, re_, 30, tid) if r >= 0)
            rows, st = dc.depth_rows(data["bodies"], rb, re_, haps, refid=tid)
            mine_tabs.append((name, rows))
            for k in sums:
                sums[k] = [a + b for a, b in zip(sums[k], st[k])] if k == "bases" else sums[k] + st[k]
        assert open(trk).read() == dc.HEADER + dc.format_rows(dc.sink_rows(mine_tabs))          # the per-contig driver against the oracle
        tabs += mine_tabs
    return dict(tabs=tabs, sums=sums)


def test_per_base_equals_the_oracle_with_each_chunk_s_own_haplotypes(base, yard):
    want = dc.sink_rows(yard["tabs"])
    assert base["track"] == dc.HEADER + dc.format_rows(want)
    st = base["depth"]
    assert {k: st[k] for k in yard["sums"]} == yard["sums"] and st["n_rows"] == len(want) == base["track"].count("\n") - 1
    assert st["n_records"] >= base["n_reads"] >= 60 and all(b > 0 for b in st["bases"][1:]) and st["ms_mark"] > 0
    assert {r[0] for r in want} == {"chr1", "chr2"} and any(r[3][1] > 0 and r[3][2] > 0 for r in want)
    for name in ("chr1", "chr2"):                                               # every contig is tiled from its first to its last planned position
        mine = [r for r in want if r[0] == name]
        assert mine[0][1] == 1 and mine[-1][2] == 12000 and all(a[2] + 1 == b[1] for a, b in zip(mine, mine[1:]))


def test_the_other_outputs_are_the_bytes_of_the_run_without_the_option(lcd, data, base):
    plain = run(lcd, data, "plain", depth=False, window_chunks=3)
    assert "depth" not in plain and plain["vcf_bytes"] == base["vcf_bytes"] and plain["bam_bytes"] == base["bam_bytes"]


def test_windows_without_an_alignment_output_beside_the_methylation_table(lcd, data, base, yard):
    got = run(lcd, data, "win", depth=dict(window=W), bam_out=False, mods=True, window_chunks=1)
    want = dc.sink_rows(yard["tabs"], W)
    assert got["track"] == dc.HEADER_W + dc.format_rows(want)
    assert 6000 % W and any(r[1] <= 6000 < r[2] for r in want)                   # the window cut by the chunk seam is one row
    assert got["depth"]["n_rows"] == len(want) and {k: got["depth"][k] for k in yard["sums"]} == yard["sums"]
    assert got["vcf_bytes"] == base["vcf_bytes"]
    alone = run(lcd, data, "mods_alone", depth=False, bam_out=False, mods=True, window_chunks=1)
    assert got["table"] == alone["table"] and len(alone["table"]) > 1000 and got["mods"]["n_rows"] == alone["mods"]["n_rows"] > 0


@pytest.mark.parametrize("window,overlap", [(1, 1), (4, 0)])
def test_windows_of_chunks_and_overlap_do_not_change_the_track(lcd, data, base, window, overlap):
    got = run(lcd, data, f"w{window}o{overlap}", bam_out=False, window_chunks=window, overlap=overlap)
    assert got["track"] == base["track"] and got["vcf_bytes"] == base["vcf_bytes"]


def test_two_input_files_give_the_same_track(lcd, data, base):
    got = run(lcd, data, "two", bams=data["halves"], sort_output=True)
    assert got["n_reads"] == base["n_reads"] and got["vcf_bytes"] == base["vcf_bytes"]
    rows = lambda text: [ln.split("\t") for ln in text.splitlines()[1:]]
    # the merged chunk holds the same records in another order, so a read's chunk id differs but its haplotype does not
    assert rows(got["track"]) == rows(base["track"])


def test_skip_dels_changes_the_track_and_nothing_else(lcd, data, base):
    got = run(lcd, data, "skip", depth=dict(skip_dels=True), bam_out=False)
    assert got["track"] != base["track"] and got["vcf_bytes"] == base["vcf_bytes"]
    assert got["depth"]["n_intervals"] > base["depth"]["n_intervals"] == base["depth"]["n_records"] - base["depth"]["n_no_overlap"]
    assert all(a < b for a, b in zip(got["depth"]["bases"][1:], base["depth"]["bases"][1:]))


def test_a_failed_run_leaves_no_track(lcd, data):
    trk = str(data["dir"] / "fail.bed")
    with pytest.raises(lcd.LcdError):                                             # the alignment output cannot be created: the run fails behind its refusals
        lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd),
                      bam_out=dict(path=str(data["dir"] / "no_such_dir" / "o.bam")), depth=dict(path=trk))
    assert not os.path.exists(trk)
    short = str(data["dir"] / "short.fa")
    fc.write_multi_fasta(short, [("chr1", data["refs"]["chr1"])])
    with pytest.raises(lcd.LcdError, match="no reference sequence|chr2"):            # the FASTA lacks chr2: the run fails at the load stage, after the track was created
        lcd.call_file(data["bam"], short, chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), depth=dict(path=trk))
    assert not os.path.exists(trk)
    for bad, word in ((dict(path="-"), "goes to a file"), (dict(path=""), "goes to a file"), (dict(path=trk, window=-1), "window"), (dict(path=trk, window=(1 << 30) + 1), "window")):
        with pytest.raises(lcd.LcdError, match=word):
            lcd.call_file(data["bam"], data["fa"], vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), depth=bad)
        assert not os.path.exists(trk)
    with pytest.raises(lcd.LcdError, match="name one file"):
        lcd.call_file(data["bam"], data["fa"], vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), depth=dict(path=trk), mods=dict(path=trk))
    assert not os.path.exists(trk)


def test_the_command_line(data, base):
    env = dict(os.environ, PYTHONPATH=ROOT)
    trk, vcf = str(data["dir"] / "cli.bed"), str(data["dir"] / "cli.vcf")
    r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", "call", data["fa"], data["bam"], "--all-ctg", "-H", "-o", vcf, "--chunk-len", str(CHUNK_LEN), "--depth", trk],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(trk).read() == base["track"] and open(vcf, "rb").read() == base["vcf_bytes"]
    assert f"{base['track'].count(chr(10)) - 1} depth rows" in r.stderr
