"""lcd_haplotag_files (align.haplotag_file, `cli haplotag`) on the MI355X: a simulated diploid two-contig BAM, two chunks per contig (a small chunk_len) with reads
that lie over the seam, against the phased VCF of the simulation.  Every record of the output BAM must carry exactly the HP / PS the Python oracle gives its read;
the haplotag list, the depth track and the read counts must be the oracle's; two input BAMs with --sort-merged, windows of one chunk with overlapped stages and
the SAM output give the same answers; no VCF appears and stdout stays empty."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_out_common as bo
import call_file_common as fc
import depth_common as dc
import haplotag_common as hc
import mods_common as mc
import split_common as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHUNK_LEN, LENGTH = 6000, 12000
ORDER = ["simA", "simB"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("haplotag_file")
    sims = {k: hc.simulate(21 + i, n_reads=120, length=LENGTH, chrom=k) for i, k in enumerate(ORDER)}
    reads = {k: [dict(pos0=r["pos0"], cigar=r["cig"], bseq=r["a"]["bseq"], qual=r["a"]["qual"], is_rev=bool(r["flag"] & 16)) for r in sims[k]["recs"]] for k in ORDER}
    bam, fa, vcf = str(d / "in.bam"), str(d / "ref.fa"), str(d / "phased.vcf.gz")
    bodies = mc.write_multi_bam_aux(bam, [(k, LENGTH, reads[k]) for k in ORDER])
    halves = [str(d / "a.bam"), str(d / "b.bam")]
    for h, path in enumerate(halves):
        mc.write_multi_bam_aux(path, [(k, LENGTH, reads[k][h::2]) for k in ORDER])
    refs = {k: np.array(["ACGT".index(c) for c in sims[k]["ref"]], np.uint8) for k in ORDER}
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in ORDER])
    text = sims["simA"]["vcf"] + "".join(sims["simB"]["vcf"].splitlines(True)[2:])
    open(vcf, "wb").write(gzip.compress(text.encode()))
    tables, vst = hc.read_vcf(text.encode(), ORDER)
    want = {}
    for b in bodies:
        x = bo.parse(b)
        t = hc.tag_record(tables[x["refid"]], b)
        want[x["name"]] = (t["hap"], t["ps"], t["n1"] + t["n2"])
    true_hap = {b"%s_r%d" % (k.encode(), i): r["true_hap"] for k in ORDER for i, r in enumerate(sims[k]["recs"])}
    assert any(bo.parse(b)["pos0"] < CHUNK_LEN - 100 and bo.parse(b)["end"] > CHUNK_LEN + 100 for b in bodies)       # reads over the seam: held by two chunks
    return dict(dir=d, bam=bam, halves=halves, fa=fa, vcf=vcf, bodies=bodies, tables=tables, vst=vst, want=want, true_hap=true_hap, refs=refs)


def out_bodies(path):
    return bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read())))[1]


def check_bam(data, path, n=None):
    got = out_bodies(path)
    assert len(got) == (n if n is not None else len(data["bodies"]))
    names = [bo.parse(b)["name"] for b in got]
    assert len(set(names)) == len(names)                                          # a record two chunks hold is written once
    n_tagged = 0
    for b, nm in zip(got, names):
        hap, ps, votes = data["want"][nm]
        assert sc.tags_of(b) == (hap, ps), nm
        assert not votes or hap == data["true_hap"][nm]
        n_tagged += hap != 0
    assert n_tagged > 0.9 * len(got)
    return got


@pytest.fixture(scope="module")
def base(lcd, data):
    d = data["dir"]
    out, lst, trk = str(d / "base.bam"), str(d / "base.list"), str(d / "base.bed")
    res = lcd.haplotag_file(data["bam"], data["fa"], data["vcf"], contig_mode=2, chunk_len=CHUNK_LEN, window_chunks=3, bam_out=dict(path=out), split=dict(haplotag_list=lst),
                            depth=dict(path=trk))
    return dict(res=res, out=out, lst=lst, trk=trk)


def test_every_record_carries_the_oracle_s_tags(data, base):
    got = check_bam(data, base["out"])
    res = base["res"]
    assert res["n_planned"] == 4 and res["n_vcf_lines"] == 0 and res["phased_vcf"] == data["vst"] and res["bam_out"]["n_records_out"] == len(got)
    t = res["haplotag"]
    assert t["n_records"] == res["n_reads"] > len(got) and sum(t["n_tagged"]) == t["n_records"] and t["n_pairs"] > 1000 and t["n_multi_ps"] > 0 and t["ms_mark"] > 0
    assert open(base["lst"], "rb").read() == sc.HEADER + sc.streams_of_bam(got, ORDER)[1]
    assert sorted(os.listdir(str(data["dir"]))) == sorted(["in.bam", "in.bam.bai", "a.bam", "a.bam.bai", "b.bam", "b.bam.bai", "ref.fa", "ref.fa.fai", "phased.vcf.gz",
                                                           "base.bam", "base.list", "base.bed"])


def test_the_depth_track_is_the_oracle_s_for_the_oracle_s_haplotypes(lcd, data, base):
    plan, _ = lcd.plan_chunks([(k, LENGTH) for k in ORDER], contig_mode=2, chunk_len=CHUNK_LEN)
    tabs = []
    for tid, rb, re_ in plan:
        haps = hc.haplotag(data["tables"][tid], data["bodies"], rb, re_, refid=tid)["haps"]
        tabs.append((ORDER[tid], dc.depth_rows(data["bodies"], rb, re_, haps, refid=tid)[0]))
    want = dc.sink_rows(tabs)
    assert open(base["trk"]).read() == dc.HEADER + dc.format_rows(want) and any(r[3][1] and r[3][2] for r in want)


@pytest.mark.parametrize("window,overlap", [(1, 1), (4, 0)])
def test_windows_and_overlapped_stages_do_not_change_the_output(lcd, data, base, window, overlap):
    out = str(data["dir"] / f"w{window}.bam")
    try:
        lcd.haplotag_file(data["bam"], data["fa"], data["vcf"], contig_mode=2, chunk_len=CHUNK_LEN, window_chunks=window, overlap=overlap, bam_out=dict(path=out))
        assert open(out, "rb").read() == open(base["out"], "rb").read()
    finally:
        os.path.exists(out) and os.remove(out)


def test_two_input_files_sorted_and_the_thresholds(lcd, data, base):
    out, lst = str(data["dir"] / "two.bam"), str(data["dir"] / "two.list")
    try:
        res = lcd.haplotag_files(data["halves"], data["fa"], data["vcf"], sort_output=True, contig_mode=2, chunk_len=CHUNK_LEN, bam_out=dict(path=out), split=dict(haplotag_list=lst))
        assert res["n_reads_per_file"][0] + res["n_reads_per_file"][1] == res["n_reads"] == base["res"]["n_reads"]
        # the halves name their reads by their own order: compare by position and bases instead of by name
        key = lambda b: (bo.parse(b)["refid"], bo.parse(b)["pos0"], b[32 + b[8]:bo.parse(b)["aux0"]])
        a, b = sorted((key(x), sc.tags_of(x)) for x in out_bodies(out)), sorted((key(x), sc.tags_of(x)) for x in out_bodies(base["out"]))
        assert a == b and len(a) == len(data["bodies"])
        pos = [(bo.parse(x)["refid"], bo.parse(x)["pos0"]) for x in out_bodies(out)]
        assert pos == sorted(pos)
        strict = lcd.haplotag_file(data["bam"], data["fa"], data["vcf"], contig_mode=2, chunk_len=CHUNK_LEN, snvs_only=True, min_diff=3, split=dict(haplotag_list=lst))
        assert strict["phased_vcf"]["n_indel_off"] == data["vst"]["n_ins"] + data["vst"]["n_del"] and strict["haplotag"]["n_tagged"][0] > base["res"]["haplotag"]["n_tagged"][0]
    finally:
        for p in (out, lst):
            os.path.exists(p) and os.remove(p)


def test_the_command_line_sam_output_and_an_empty_stdout(data, base):
    env = dict(os.environ, PYTHONPATH=ROOT)
    sam, lst = str(data["dir"] / "cli.sam"), str(data["dir"] / "cli.list")
    try:
        r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", "haplotag", data["fa"], data["bam"], data["vcf"], "--all-ctg", "--chunk-len", str(CHUNK_LEN), "--sam", sam,
                            "--haplotag-list", lst], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == "" and "phased sites" in r.stderr
        assert open(lst, "rb").read() == open(base["lst"], "rb").read()
        lines = [ln.split("\t") for ln in open(sam).read().splitlines() if not ln.startswith("@")]
        assert len(lines) == len(data["bodies"])
        for f in lines:
            hap, ps, _ = data["want"][f[0].encode()]
            assert ("HP:i:%d" % hap in f) == (hap != 0) and ("PS:i:%d" % ps in f) == (ps > 0), f[0]
    finally:
        for p in (sam, lst):
            os.path.exists(p) and os.remove(p)


def test_refusals_and_failures_on_the_device_path(lcd, data):
    d = data["dir"]
    before = sorted(os.listdir(str(d)))
    out = str(d / "fail.bam")
    with pytest.raises(lcd.LcdError, match="no sample NOBODY"):
        lcd.haplotag_file(data["bam"], data["fa"], data["vcf"], sample="NOBODY", contig_mode=2, bam_out=dict(path=out))
    with pytest.raises(lcd.LcdError, match="cannot open"):
        lcd.haplotag_file(data["bam"], data["fa"], str(d / "missing.vcf"), contig_mode=2, bam_out=dict(path=out))
    with pytest.raises(lcd.LcdError, match="writes no VCF"):
        lcd.haplotag_file(data["bam"], data["fa"], data["vcf"], vcf_path=str(d / "o.vcf"), bam_out=dict(path=out))
    short = str(d / "short.fa")
    fc.write_multi_fasta(short, [("simA", data["refs"]["simA"])])
    try:
        # fails at the load stage, after the outputs were created: the track is removed; the alignment writer's abort leaves its file, as in a calling run
        with pytest.raises(lcd.LcdError, match="no reference sequence|simB"):
            lcd.haplotag_file(data["bam"], short, data["vcf"], contig_mode=2, chunk_len=CHUNK_LEN, bam_out=dict(path=out), depth=dict(path=str(d / "fail.bed")))
        assert not os.path.exists(str(d / "fail.bed"))
    finally:
        for p in (short, short + ".fai", out):
            os.path.exists(p) and os.remove(p)
    assert sorted(os.listdir(str(d))) == before
