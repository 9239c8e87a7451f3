"""call_file / call_files with aln_format="sam" on the MI355X, on the inputs tests/test_gpu_call_file.py and tests/test_gpu_call_files.py build: the VCF is the BAM
run's byte for byte, the SAM text is the oracle formatting (tests/sam_out_common.py) of that run's out.bam, whatever window_chunks and overlap are; two inputs with
sort_output; and --sam with --refine-bam through the command line in a fresh child process."""
import os
import subprocess
import sys

import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import multi_bam_common as mb
import sam_out_common as so
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
ORDER = ["chr1", "chr2"]
NAMES = [k.encode() for k in ORDER]


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_file")
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12))
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    fc.write_multi_bam(bam, [(k, 12000, chs[k]["reads"]) for k in ORDER], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    fc.write_multi_fasta(fa, [(k, chs[k]["ref"]) for k in ORDER])
    return dict(dir=d, bam=bam, fa=fa, chs=chs)


def split_bam(path):
    return bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read())))


def want_sam(bam_path):
    """the oracle formatting of a written BAM: its header (the @PG line is already in it) and its records"""
    hdr, bodies = split_bam(bam_path)
    text, st = so.sam_text(bodies, NAMES)
    return so.sam_header(hdr, None) + text, st, bodies


def run(lcd, data, tag, fmt, inputs=None, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.{fmt}")
    common = dict(chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), no_vcf_header=1, contig_mode=2, **kw)
    if fmt == "sam":
        common["aln_format"] = "sam"
    res = lcd.call_files(inputs, data["fa"], sort_output=True, **common) if inputs else lcd.call_file(data["bam"], data["fa"], **common)
    res["vcf"], res["out"] = open(vcf, "rb").read(), out
    return res


def test_the_sam_run_is_the_bam_run_formatted(lcd, data):
    b = run(lcd, data, "plain", "bam")
    want, wst, bodies = want_sam(b["out"])
    assert len(bodies) > 60 and b"\tHP:i:" in want and b"\tPS:i:" in want and want.startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:12000\n@SQ\tSN:chr2\tLN:12000\n@RG\tID:x")
    first = None
    for tag, kw in (("w0", dict()), ("w2o0", dict(window_chunks=2, overlap=0)), ("w1o1", dict(window_chunks=1, overlap=1))):
        s = run(lcd, data, tag, "sam", **kw)
        assert s["vcf"] == b["vcf"] and s["n_vcf_lines"] == b["n_vcf_lines"] > 0, tag
        got = open(s["out"], "rb").read()
        for k, (g, w) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))):
            assert g == w, (tag, k)
        assert got == want, tag
        assert {k: v for k, v in s["sam"].items() if not k.startswith("ms_")} == wst, tag
        assert s["bam_out"]["bytes_file"] == len(got) and s["bam_out"]["ms_deflate"] == 0 and s["bam_out"]["n_records_out"] == b["bam_out"]["n_records_out"]
        assert s["bam_out"]["bytes_inflated"] == sum(4 + len(x) for x in bodies)
        first = first or s
    assert "sam" not in b
    # no output index for SAM: asked for, it is refused before a file is created; with the inputs' indexes alone the run goes through
    with pytest.raises(lcd.LcdError, match="index"):
        run(lcd, data, "idx", "sam", index=True)
    assert not os.path.exists(str(data["dir"] / "idx.sam")) and not os.path.exists(str(data["dir"] / "idx.vcf"))
    s = run(lcd, data, "idx2", "sam", index=dict(build_missing_bai=1, build_missing_fai=1))
    assert open(s["out"], "rb").read() == want and s["index"]["wrote_out_bai"] == 0 and not os.path.exists(s["out"] + ".bai")


def test_refined_records_as_sam(lcd, data):
    b = run(lcd, data, "ref", "bam", refine=True)
    s = run(lcd, data, "ref", "sam", refine=True)
    want, wst, bodies = want_sam(b["out"])
    assert open(s["out"], "rb").read() == want and s["vcf"] == b["vcf"]
    assert {k: v for k, v in s["refine"].items() if not k.startswith("ms_")} == {k: v for k, v in b["refine"].items() if not k.startswith("ms_")} and s["refine"]["n_records"] == len(bodies)


def test_two_inputs_with_sort_output(lcd, data):
    d = data["dir"]
    files = {k: mb.deal(data["chs"][k]["reads"], k, 2, borders=[6000]) for k in ORDER}
    paths = [str(d / "a.bam"), str(d / "b.bam")]
    for f, path in enumerate(paths):
        mb.write_bam(path, [(k, 12000, files[k][f]) for k in ORDER], header_text=fc.DEFAULT_HEADER, block=30000)
    b = run(lcd, data, "ab", "bam", inputs=paths)
    s = run(lcd, data, "ab", "sam", inputs=paths)
    want, wst, bodies = want_sam(b["out"])
    got = open(s["out"], "rb").read()
    assert got == want and s["vcf"] == b["vcf"] and s["n_reads_per_file"] == b["n_reads_per_file"] and len(bodies) >= 60
    pos = [(bo.parse(x)["refid"], bo.parse(x)["pos0"]) for x in bodies]
    assert pos == sorted(pos)
    assert {k: v for k, v in s["sam"].items() if not k.startswith("ms_")} == wst


def test_the_command_line_in_a_fresh_process(lcd, data):
    """--sam with --refine-bam through python -m longcalld_amd.cli, against the library's refined BAM run with the command line's (default) configuration"""
    d = data["dir"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "longcalld_amd.cli", "call", "--all-ctg", "--chunk-len", str(CHUNK_LEN), "--refine-bam", "-H"]
    lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, vcf_path=str(d / "cli_b.vcf"), bam_out=dict(path=str(d / "cli.bam"), pg_line=PG), cfg=lcd.call_cfg(0), no_vcf_header=1,
                  contig_mode=2, refine=True)
    rs = subprocess.run(base + ["--sam", str(d / "cli.sam"), "-o", str(d / "cli_s.vcf"), data["fa"], data["bam"]], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert rs.returncode == 0, rs.stderr
    assert "bytes of SAM text" in rs.stderr and "refined" in rs.stderr
    hdr, bodies = split_bam(str(d / "cli.bam"))
    got = open(str(d / "cli.sam"), "rb").read()
    lines = got.split(b"\n")
    head = [x for x in lines if x.startswith(b"@")]
    assert head[:3] == [b"@HD\tVN:1.6\tSO:coordinate", b"@SQ\tSN:chr1\tLN:12000", b"@SQ\tSN:chr2\tLN:12000"] and head[-1].startswith(b"@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:")
    assert b"--sam" in head[-1] and len(head) == 5
    assert b"\n".join(lines[len(head):]) == so.sam_text(bodies, NAMES)[0] and len(bodies) > 60
    assert open(str(d / "cli_s.vcf"), "rb").read() == open(str(d / "cli_b.vcf"), "rb").read()
    assert str(len(got)) + " bytes of SAM text" in rs.stderr
