"""MEI annotation from a TE library (-T) and supporting read names (--out-var-rnames / --out-sv-rnames) on the MI355X: one BAM of one 12 kb contig at depth 12 with the
three planted insertions of tests/vcf_fields_common.py, called in two 6 kb chunks -- two name tables, one stitch.  The expected VCF body is the oracle's formatter
(oracle/emit.c: lcdo_format_vcf_te after lcdo_annotate_te with the library, oracle/te_info.c) applied chunk by chunk to the kept records, plus the Python ALTREADS
rule with the read names the tests' own BAM reader finds for each chunk."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import emit_common as ec
import multi_bam_common as mb
import vcf_fields_common as vf
from conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK_LEN = 6000
REGIONS = [(1, 6000), (6001, 12000)]
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
TE_NAMES = [b"TE0", b"TE1", b"TE2"]
HEADER_ARGS = dict(source_version="test-1", cmdline="call ref.fa in.bam", date_yyyymmdd="20240102")


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf_fields")
    ch = vf.make_mei_chunk()
    reads = [dict(r, name=f"m64011_{7919 * i % 1000}/{i}/ccs") for i, r in enumerate(ch["reads"])]
    bam, fa, te = str(d / "in.bam"), str(d / "ref.fa"), str(d / "te.fa")
    mb.write_bam(bam, [("chr1", 12000, reads)], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    halves = [str(d / "even.bam"), str(d / "odd.bam")]
    for k, p in enumerate(halves):                                                   # the reads split by the parity of their index
        mb.write_bam(p, [("chr1", 12000, reads[k::2])], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    fc.write_multi_fasta(fa, [("chr1", ch["ref"])])
    vf.write_te_fasta(te, ch["te_seqs"], TE_NAMES)
    return dict(dir=d, ch=ch, bam=bam, halves=halves, fa=fa, te=te)


def run(lcd, data, tag, bams=None, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
    common = dict(chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), keep_records=True, **HEADER_ARGS)
    common.update(kw)
    res = lcd.call_files(bams, data["fa"], **common) if bams else lcd.call_file(data["bam"], data["fa"], **common)
    raw = open(vcf, "rb").read()
    text = gzip.decompress(raw) if kw.get("vcf_bgzf") else raw
    res["raw"], res["header"], res["body"] = raw, b"".join(l for l in text.splitlines(True) if l.startswith(b"#")), b"".join(l for l in text.splitlines(True) if not l.startswith(b"#"))
    res["bam_image"] = open(out, "rb").read()
    return res


@pytest.fixture(scope="module")
def plain(lcd, data):
    """the run without options"""
    return run(lcd, data, "plain")


@pytest.fixture(scope="module")
def full(lcd, data):
    """test 1's run: the library and the names of every record"""
    return run(lcd, data, "full", te_fasta=data["te"], rnames="all")


def per_chunk(res):
    at, out = 0, []
    for c in res["chunks"]:
        out.append(res["records"][at:at + c["n_records"]]); at += c["n_records"]
    assert at == len(res["records"]) and [(c["reg_beg"], c["reg_end"]) for c in res["chunks"]] == REGIONS
    return out


def expected(oracle, data, res, bams, mode, with_te=True):
    """-> (body text, per chunk the oracle's annotation, per chunk the read names)"""
    opt = ec.default_call_opt()
    text, anns, tabs = b"", [], []
    for recs, (rb, re_) in zip(per_chunk(res), REGIONS):
        names = vf.chunk_read_names(bams, rb, re_)
        t, ann = vf.expected_text(oracle.lib(), opt, b"chr1", recs, data["ch"]["ref"], 1, data["ch"]["te_seqs"] if with_te else None, TE_NAMES if with_te else None, mode, names)
        text += t; anns.append(ann); tabs.append(names)
    return text, anns, tabs


def test_library_and_all_read_names(lcd, oracle, data, plain, full):
    want, anns, tabs = expected(oracle, data, full, [data["bam"]], 2)
    assert full["body"] == want
    assert full["header"] == plain["header"] and b"ID=ALTREADS" in full["header"] and b"ID=MEI" in full["header"] and b"ID=REPNAME" in full["header"]
    assert [c["n_reads"] for c in full["chunks"]] == [len(t) for t in tabs] and tabs[0] != tabs[1]
    # every chunk has lines with two or more names; every line has the field
    at = 0
    lines = full["body"].decode().splitlines()
    assert len(lines) == full["n_vcf_lines"] > 10
    for recs, names in zip(per_chunk(full), tabs):
        many = 0
        for r in recs:
            if r["alt_read_names"] is None:
                pytest.fail("rnames='all' left a record without names")
            assert [n.encode() for n in r["alt_read_names"]] == [names[i] for i in r["alt_reads"][:r["AD"][1]]]
            many += len(r["alt_read_names"]) >= 2
        assert many >= 1, "vacuous: no record of this chunk has two or more supporting reads"
    assert all(l.split("\t")[8].endswith(":ALTREADS") and l.split("\t")[9].count(":") == l.split("\t")[8].count(":") for l in lines)
    # the three planted events, as the oracle annotates them
    flat_ann = [a for ann in anns for a in ann]
    for r, a in zip(full["records"], flat_ann):
        assert {k: r[k] for k in a} == a
    for x, want_name, rev in zip(data["ch"]["planted"], ("TE1", "TE2", None), (0, 1, 0)):
        r = vf.planted_record(full["records"], x)
        assert r is not None and len(r["tsd"]) >= vf.TSD_LEN and r["te_name"] == want_name and (want_name is None or r["te_is_rev"] == rev), x["kind"]
        line = [l for l in lines if l.split("\t")[1] == str(r["pos"])][0]
        if want_name:
            assert "\tMEI;" in line and f";REPNAME={'+-'[rev]}{want_name}\t" in line and (";POLYALEN=-" in line) == bool(rev)
        else:
            assert ";TSD=" in line and "MEI" not in line and "REPNAME" not in line
    assert full["te_names"] == ["TE0", "TE1", "TE2"] and full["n_mei_lines"] == 2 == full["body"].count(b"\tMEI;")
    # the alignment output does not depend on the VCF options
    assert full["bam_image"] == plain["bam_image"]


def test_sv_read_names_only(lcd, oracle, data, plain):
    got = run(lcd, data, "sv", rnames="sv")
    want, _, _ = expected(oracle, data, got, [data["bam"]], 1, with_te=False)
    assert got["body"] == want and got["header"] == plain["header"]
    a, b = got["body"].splitlines(), plain["body"].splitlines()
    assert len(a) == len(b)
    n_sv = 0
    for x, y in zip(a, b):
        if b";SVTYPE=" in y:
            assert x.split(b"\t")[8] == y.split(b"\t")[8] + b":ALTREADS" and x.split(b"\t")[9].startswith(y.split(b"\t")[9] + b":") and x.split(b"\t")[:8] == y.split(b"\t")[:8]
            n_sv += 1
        else:
            assert x == y                                                            # every other line is byte-identical to the run without options
    assert n_sv >= 3 and "te_names" not in got
    assert [r["alt_read_names"] is not None for r in got["records"]] == [bool(r["is_sv"]) for r in got["records"]]


def test_compressed_windowed_overlapped_run_gives_the_same_text(lcd, data, full):
    got = run(lcd, data, "z", te_fasta=data["te"], rnames="all", vcf_bgzf=1, window_chunks=1, overlap=1)
    assert got["header"] + got["body"] == full["header"] + full["body"] and got["n_windows"] == 2
    assert got["records"] == full["records"] and got["n_mei_lines"] == 2
    members = bo.bgzf_members(got["raw"])
    assert sum(1 for m in members if m["isize"] == 0) == 1 and len(got["raw"]) < len(full["raw"])


def test_two_input_bams_name_reads_from_the_file_major_table(lcd, oracle, data):
    got = run(lcd, data, "two", bams=data["halves"], te_fasta=data["te"], rnames="all")
    want, _, tabs = expected(oracle, data, got, data["halves"], 2)
    assert got["body"] == want and got["n_reads_per_file"][0] > 0 and got["n_reads_per_file"][1] > 0
    for recs, names in zip(per_chunk(got), tabs):
        evens = sum(1 for n in names if int(n.split(b"/")[1]) % 2 == 0)
        assert [int(n.split(b"/")[1]) % 2 for n in names] == [0] * evens + [1] * (len(names) - evens) and 0 < evens < len(names)      # file-major
        for r in recs:
            assert [n.encode() for n in r["alt_read_names"]] == [names[i] for i in r["alt_reads"][:r["AD"][1]]]
    assert any(len({int(n.split("/")[1]) % 2 for n in r["alt_read_names"]}) == 2 for r in got["records"])     # records supported by reads of both files
    assert got["n_mei_lines"] == 2


def test_region_and_chunk_entry_points_give_the_same_text(lcd, data, full):
    begs, ends = [b for b, _ in REGIONS], [e for _, e in REGIONS]
    reg = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], "chr1", begs, ends, cfg=cfg_of(lcd), te_fasta=data["te"], rnames="all")
    assert reg["vcf_body"].encode() == full["body"] and reg["records"] == full["records"] and reg["n_mei_lines"] == 2 and reg["te_names"] == ["TE0", "TE1", "TE2"]
    devs = [lcd.DeviceChunk.from_bam(data["bam"], data["bam"] + ".bai", "chr1", b, e) for b, e in REGIONS]
    items = [dict(ref=data["ch"]["ref"], ref_beg=1, reg_beg=b, reg_end=e) for b, e in REGIONS]
    got = lcd.call_chunks(devs, items, cfg_of(lcd), chrom="chr1", te_fasta=data["te"], rnames="all")
    assert got["vcf_body"].encode() == full["body"] and got["records"] == full["records"]
    none = lcd.chunks_call(devs, items, cfg_of(lcd), chrom="chr1")
    with pytest.raises(lcd.LcdError, match="name table"):                            # names wanted from chunks that have none
        lcd.chunks_call(devs, [dict(it, meta=False, ordered_read_ids=np.arange(d.n, dtype=np.int32)) for it, d in zip(items, devs)], cfg_of(lcd), chrom="chr1", rnames="sv")
    for d in devs:
        d.close()
    assert "ALTREADS" not in none["vcf_body"] and "MEI" not in none["vcf_body"] and none["vcf_body"].count("\n") == full["body"].count(b"\n")


def test_no_options_and_zeroed_options_are_byte_identical(lcd, data, plain, tmp_path):
    """lcd_call_files without options, with lcd_run_opt_t.fields NULL and with a zeroed struct (from plain C, tests/c/vcf_fields_abi.c), and the Python run"""
    exe, libdir = str(tmp_path / "vcf_fields_abi"), os.path.join(ROOT, "longcalld_amd")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "vcf_fields_abi.c"), "-L", libdir, "-llcd_hotpath",
                           "-Wl,-rpath," + libdir, "-o", exe])
    prefix = str(tmp_path / "o")
    out = subprocess.check_output([exe, data["bam"], data["fa"], prefix, data["te"]], text=True, timeout=120)
    runs = {l.split(" ", 1)[0]: re.match(r"\S+ rc (-?\d+) lines (-?\d+) mei (-?\d+)", l).groups() for l in out.splitlines()}
    assert runs["plain"] == runs["null"] == runs["zero"] == ("0", str(plain["n_vcf_lines"]), "0") and runs["te"] == ("0", str(plain["n_vcf_lines"]), "2")
    vcfs = {t: open(f"{prefix}.{t}.vcf", "rb").read() for t in ("plain", "null", "zero", "te")}
    bams = {t: open(f"{prefix}.{t}.bam", "rb").read() for t in ("plain", "null", "zero", "te")}
    assert vcfs["plain"] == vcfs["null"] == vcfs["zero"] == plain["raw"] and vcfs["te"] != vcfs["plain"] and vcfs["te"].count(b"\tMEI;") == 2
    assert bams["plain"] == bams["null"] == bams["zero"] == bams["te"] == plain["bam_image"]
    assert b"ALTREADS\t" not in plain["body"] and b"MEI;" not in plain["body"] and b";TSD=" in plain["body"]
