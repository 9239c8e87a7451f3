"""lcd_call_files_ext2's per-haplotype read sets (align.call_file(split=...), --split-reads / --haplotag-list) on the MI355X: the synthetic two-contig BAM of
tests/test_gpu_depth_file.py called in windows of chunks.  The yardstick is the run's own output BAM read back in Python: its records without 0x100 / 0x800,
grouped by their HP tag and formatted by the oracle in file order, must be the three FASTQ files byte for byte, and the list's columns those records' HP / PS.
The other outputs must be the bytes of the run without the option; the files do not depend on the alignment output, the windows or the overlap; two input files
give the same reads; the .gz files inflate to the plain ones and end with the BGZF EOF member; a run that fails leaves none of the four files."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import mods_common as mc
import split_common as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("split_file")
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


def read_split(prefix, gz=False):
    return [open(p, "rb").read() for p in sc.paths(prefix, gz)]


def run(lcd, data, tag, split=True, bam_out=True, extras=False, bams=None, gz=False, comment=False, **kw):
    vcf, out, pre, lst, tab, trk = (str(data["dir"] / f"{tag}.{x}") for x in ("vcf", "bam", "split", "list.tsv", "mods.tsv", "bed"))
    kw.setdefault("chunk_len", CHUNK_LEN)
    args = dict(vcf_path=vcf, no_vcf_header=1, cfg=cfg_of(lcd), contig_mode=2, bam_out=dict(path=out, pg_line=PG) if bam_out else None, **kw)
    if split:
        args["split"] = dict(prefix=pre, haplotag_list=lst, gz=gz, comment=comment)
    if extras:
        args["mods"] = dict(path=tab); args["depth"] = dict(path=trk)
    res = lcd.call_files(bams, data["fa"], **args) if bams else lcd.call_file(data["bam"], data["fa"], **args)
    res["vcf_bytes"] = open(vcf, "rb").read()
    res["bam_bytes"] = open(out, "rb").read() if bam_out else None
    res["fastq"] = read_split(pre, gz) if split else None
    res["list"] = open(lst, "rb").read() if split else None
    res["table"] = open(tab, "rb").read() if extras else None
    res["track"] = open(trk, "rb").read() if extras else None
    return res


def records_of(bam_bytes):
    stream = b"".join(m["payload"] for m in bo.bgzf_members(bam_bytes))
    return bo.bam_split(stream)[1]


@pytest.fixture(scope="module")
def base(lcd, data):
    return run(lcd, data, "base", window_chunks=3, extras=True)


def test_the_files_are_the_output_bam_s_primary_records_by_their_hp_tag(data, base):
    bodies = records_of(base["bam_bytes"])
    fq, lst, st = sc.streams_of_bam(bodies, data["order"])
    for s in range(3):
        assert base["fastq"][s] == fq[s], s
    assert base["list"] == sc.HEADER + lst
    got = base["split"]
    print({k: got[k] for k in sc.STAT_KEYS}, st)
    assert {k: got[k] for k in sc.STAT_KEYS} == st
    assert st["n_records"] == len(bodies) == base["bam_out"]["n_records_out"] + base["bam_out"]["n_filtered_out"]
    assert st["n_hap"][1] > 10 and st["n_hap"][2] > 10 and 60 <= st["n_selected"] <= base["n_reads"] and got["ms_measure"] > 0 and got["ms_emit"] > 0
    # the list's columns are those records' tags, line by line
    prim = [b for b in bodies if not bo.parse(b)["flag"] & 0x900]
    rows = [ln.split(b"\t") for ln in base["list"].splitlines()[1:]]
    assert len(rows) == len(prim)
    for row, b in zip(rows, prim):
        hp, ps = sc.tags_of(b)
        assert row == [bo.parse(b)["name"], b"H%d" % hp if hp else b"none", b"%d" % ps if ps > 0 else b"none", data["order"][bo.parse(b)["refid"]].encode()]
    # every primary record of the input appears exactly once in the whole run
    names = sorted(e.split(b"\n")[0][1:] for f in base["fastq"] for e in sc.fastq_entries(f))
    assert names == sorted(bo.parse(b)["name"] for b in data["bodies"] if not bo.parse(b)["flag"] & 0x900 and sc.parse(b)["lseq"] > 0)


def test_the_other_outputs_are_the_bytes_of_the_run_without_the_option(lcd, data, base):
    plain = run(lcd, data, "plain", split=False, window_chunks=3, extras=True)
    assert "split" not in plain and plain["vcf_bytes"] == base["vcf_bytes"] and plain["bam_bytes"] == base["bam_bytes"]
    assert plain["table"] == base["table"] and plain["track"] == base["track"] and len(plain["table"]) > 1000 and len(plain["track"]) > 1000


@pytest.mark.parametrize("window,overlap", [(1, 1), (1, 0), (3, 1)])
def test_the_same_files_without_an_alignment_output(lcd, data, base, window, overlap):
    got = run(lcd, data, f"w{window}o{overlap}", bam_out=False, window_chunks=window, overlap=overlap)
    assert got["fastq"] == base["fastq"] and got["list"] == base["list"] and got["vcf_bytes"] == base["vcf_bytes"]
    assert {k: got["split"][k] for k in sc.STAT_KEYS} == {k: base["split"][k] for k in sc.STAT_KEYS}


def test_the_comment_carries_the_tags_of_the_output_bam(lcd, data, base):
    got = run(lcd, data, "comment", comment=True, window_chunks=3)
    assert got["bam_bytes"] == base["bam_bytes"]
    fq, lst, _ = sc.streams_of_bam(records_of(got["bam_bytes"]), data["order"], comment=True)
    assert got["fastq"] == fq and got["list"] == sc.HEADER + lst
    assert got["fastq"][1].count(b"\tHP:i:1") == base["split"]["n_hap"][1] and b"\tPS:i:" in got["fastq"][2] and b"HP:i" not in got["fastq"][0]


def test_two_input_files_give_the_same_reads(lcd, data, base):
    got = run(lcd, data, "two", bams=data["halves"], sort_output=True)
    assert got["n_reads"] == base["n_reads"] and got["vcf_bytes"] == base["vcf_bytes"]
    # the input writer names a read by its index in its own file, so the halves' names are not the one file's: a read is its bases and qualities here
    read_of = lambda e: e.split(b"\n", 1)[1]
    for s in range(3):
        assert sorted(map(read_of, sc.fastq_entries(got["fastq"][s]))) == sorted(map(read_of, sc.fastq_entries(base["fastq"][s]))), s
        assert len(got["fastq"][s]) > 10000
    assert sorted(ln.split(b"\t", 1)[1] for ln in got["list"].splitlines()) == sorted(ln.split(b"\t", 1)[1] for ln in base["list"].splitlines())
    # ... and in the order of that run's own BAM
    fq, lst, _ = sc.streams_of_bam(records_of(got["bam_bytes"]), data["order"])
    assert got["fastq"] == fq and got["list"] == sc.HEADER + lst


def test_gz_files_inflate_to_the_plain_files(lcd, data, base):
    got = run(lcd, data, "gz", gz=True, bam_out=False, window_chunks=3)
    for s, p in enumerate(sc.paths(str(data["dir"] / "gz.split"), True)):
        raw = open(p, "rb").read()
        assert gzip.decompress(raw) == base["fastq"][s] and raw[-28:] == sc.EOF_MEMBER
        members = bo.bgzf_members(raw)
        assert members[-1]["isize"] == 0 and b"".join(m["payload"] for m in members) == base["fastq"][s]
    assert got["list"] == base["list"] and got["split"]["ms_deflate"] > 0


def test_a_failed_run_leaves_none_of_the_files(lcd, data):
    pre, lst = str(data["dir"] / "fail"), str(data["dir"] / "fail.tsv")
    mine = sc.paths(pre) + sc.paths(pre, True) + [lst]
    with pytest.raises(lcd.LcdError):                                             # the alignment output cannot be created: the run fails behind its refusals
        lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd),
                      bam_out=dict(path=str(data["dir"] / "no_such_dir" / "o.bam")), split=dict(prefix=pre, haplotag_list=lst))
    assert not any(os.path.exists(p) for p in mine)
    short = str(data["dir"] / "short.fa")
    fc.write_multi_fasta(short, [("chr1", data["refs"]["chr1"])])
    with pytest.raises(lcd.LcdError, match="no reference sequence|chr2"):            # the FASTA lacks chr2: the run fails at the load stage, after the files were created
        lcd.call_file(data["bam"], short, chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), split=dict(prefix=pre, gz=True, haplotag_list=lst))
    assert not any(os.path.exists(p) for p in mine)
    for bad, word in ((dict(prefix="-"), "go to files"), (dict(prefix=""), "go to files"), (dict(gz=True), "need split_prefix"), (dict(prefix=pre, haplotag_list="-"), "goes to a file"),
                      (dict(prefix=pre, haplotag_list=pre + ".h1.fastq"), "name one file"), (dict(haplotag_list=str(data["dir"] / "fail.vcf")), "name one file")):
        with pytest.raises(lcd.LcdError, match=word):
            lcd.call_file(data["bam"], data["fa"], vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), split=bad)
        assert not any(os.path.exists(p) for p in mine)


def test_the_per_contig_driver_writes_the_contig_s_reads(lcd, data, base):
    """lcd_call_bam_regions_ext2 with chr1's planned regions: the files are those of its own output BAM"""
    pre, lst, out = str(data["dir"] / "reg"), str(data["dir"] / "reg.tsv"), str(data["dir"] / "reg.bam")
    res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], "chr1", [1, 6001], [6000, 12000], min_mapq=30, cfg=cfg_of(lcd), bam_out=dict(path=out, pg_line=PG),
                               split=dict(prefix=pre, haplotag_list=lst))
    assert res["bam_out_rc"] == 0
    fq, want_lst, st = sc.streams_of_bam(records_of(open(out, "rb").read()), data["order"])
    assert read_split(pre) == fq and open(lst, "rb").read() == sc.HEADER + want_lst and {k: res["split"][k] for k in sc.STAT_KEYS} == st and st["n_selected"] > 20


def test_the_command_line(data, base):
    env = dict(os.environ, PYTHONPATH=ROOT)
    pre, lst, vcf = str(data["dir"] / "cli"), str(data["dir"] / "cli.tsv"), str(data["dir"] / "cli.vcf")
    r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", "call", data["fa"], data["bam"], "--all-ctg", "-H", "-o", vcf, "--chunk-len", str(CHUNK_LEN), "--split-reads", pre,
                        "--split-gz", "--haplotag-list", lst], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [gzip.decompress(x) for x in read_split(pre, True)] == base["fastq"] and open(lst, "rb").read() == base["list"] and open(vcf, "rb").read() == base["vcf_bytes"]
    n = base["split"]["n_hap"]
    assert f"{n[1]} + {n[2]} + {n[0]} split reads" in r.stderr
