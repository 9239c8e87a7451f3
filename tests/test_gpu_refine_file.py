"""lcd_call_files with refined alignments on the MI355X: two small contigs of plain-'M' reads called and written with refined alignments in one call.  The
record stream is that of lcd_call_bam_regions (refined) per contig (pinned to the oracle by tests/test_gpu_refine_call.py) and does not depend on window_chunks,
overlap, the VCF's -O z or --make-index; the file inflates with zlib and splits into records; its .bai equals the index oracle's for that very file, or is absent
with the stated reason; the VCF is that of the run without refine.  Two input files once."""
import gzip

import numpy as np
import pytest

import bai_common as bc
import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import multi_bam_common as mb

pytestmark = pytest.mark.gpu
CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
ORDER = ["chr1", "chr2"]


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("refine_file")
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12))
    bam, fa = str(d / "m.bam"), str(d / "ref.fa")
    fc.write_multi_bam(bam, [(k, 12000, [dict(r, cigar=fc.m_cigar(r["cigar"])) for r in chs[k]["reads"]]) for k in ORDER])
    fc.write_multi_fasta(fa, [(k, chs[k]["ref"]) for k in ORDER])
    return dict(dir=d, bam=bam, fa=fa, chs=chs)


def bodies_of(path):
    return bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read())))[1]


def run(lcd, data, tag, refine=True, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
    res = lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), no_vcf_header=1, contig_mode=2,
                        refine=refine, **kw)
    raw = open(vcf, "rb").read()
    res["text"] = (gzip.decompress(raw) if kw.get("vcf_bgzf") else raw).decode()
    res["bam"], res["bodies"] = out, bodies_of(out)
    return res


def check_index(res):
    """the .bai of the written file equals the index oracle's for that file, or the file is unsorted and the index is absent with the reason"""
    import os
    s = bc.scan_bam(open(res["bam"], "rb").read())
    try:
        want = bc.oracle_bai(len(s["refs"]), s["recs"])
    except bc.BaiRefused:
        assert res["index"]["out_bai_skipped"] == bc.ERR_ORDER and res["index"]["wrote_out_bai"] == 0 and res["index"]["out_bai_skip_reason"] and not os.path.exists(res["bam"] + ".bai")
        return "absent"
    assert res["index"]["wrote_out_bai"] == 1 and res["index"]["out_bai_skipped"] == 0 and open(res["bam"] + ".bai", "rb").read() == want
    return "written"


def test_g4_every_setting_gives_the_same_refined_stream(lcd, data):
    yard = []
    for k in ORDER:
        regs = mb.regions_of(12000, CHUNK_LEN)
        out = str(data["dir"] / f"yard_{k}.bam")
        r = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], k, [a for a, _ in regs], [b for _, b in regs], min_mapq=30, cfg=cfg_of(lcd),
                                 bam_out=dict(path=out, pg_line=PG), refine=True)
        assert r["bam_out_rc"] == 0, r["bam_out_error"]
        assert r["refine"]["n_unrefined"] == 0 and r["refine"]["n_refined"] > 20 and r["refine"]["n_log_entries"] > 0
        yard += bodies_of(out)
    plain = run(lcd, data, "plain", refine=False)
    first = None
    for tag, kw in (("w2o0", dict(window_chunks=2, overlap=0)), ("w0o0", dict(window_chunks=0, overlap=0)), ("w2o1", dict(window_chunks=2, overlap=1)),
                    ("w0o1", dict(window_chunks=0, overlap=1)), ("z", dict(vcf_bgzf=1)), ("idx", dict(index=True))):
        res = run(lcd, data, tag, **kw)
        assert res["bodies"] == yard, tag
        assert res["text"] == plain["text"] and res["n_vcf_lines"] == plain["n_vcf_lines"], tag     # the call is the run without refine
        assert res["refine"]["n_records"] == len(yard) and res["refine"]["n_unrefined"] == 0 and res["refine"]["n_refined"] > 40
        first = first or res
        assert {k: v for k, v in res["refine"].items() if not k.startswith("ms_")} == {k: v for k, v in first["refine"].items() if not k.startswith("ms_")}, tag
        if tag == "idx":
            print("output index:", check_index(res), res["index"]["out_bai_skip_reason"])
    assert [bo.parse(b)["name"] for b in plain["bodies"]] == [bo.parse(b)["name"] for b in yard] and plain["bodies"] != yard
    assert "refine" not in plain
    assert not any((w & 0xf) == 0 for b in yard for w in __import__("refine_common").core(b)["cig"])          # 'M' became '=' / 'X' in every record


def test_g4_two_input_files_once(lcd, data):
    d = data["dir"]
    files = {k: mb.deal([dict(r, cigar=fc.m_cigar(r["cigar"])) for r in data["chs"][k]["reads"]], k, 2, borders=[6000]) for k in ORDER}
    a, b = str(d / "a.bam"), str(d / "b.bam")
    for f, path in enumerate((a, b)):
        mb.write_bam(path, [(k, 12000, files[k][f]) for k in ORDER], header_text=fc.DEFAULT_HEADER, block=30000)
    outs = {}
    for refine in (False, True):
        vcf, out = str(d / f"ab{int(refine)}.vcf"), str(d / f"ab{int(refine)}.bam")
        res = lcd.call_files([a, b], data["fa"], sort_output=True, chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), no_vcf_header=1,
                             contig_mode=2, refine=refine, index=True)
        res["text"], res["bam"], res["bodies"] = open(vcf).read(), out, bodies_of(out)
        outs[refine] = res
    p, r = outs[False], outs[True]
    assert r["text"] == p["text"] and r["n_reads_per_file"] == p["n_reads_per_file"]
    assert [bo.parse(x)["name"] for x in r["bodies"]] == [bo.parse(x)["name"] for x in p["bodies"]] and len(r["bodies"]) >= 60
    tags = lambda x: [(t, ty, bytes(v)) for t, ty, v, *_ in bo.field_spans(x[bo.parse(x)["aux0"]:]) if t in (b"HP", b"PS")]
    assert [tags(x) for x in r["bodies"]] == [tags(x) for x in p["bodies"]]
    assert r["refine"]["n_records"] == len(r["bodies"]) and r["refine"]["n_unrefined"] == 0 and r["refine"]["n_refined"] > 40 and r["refine"]["n_log_entries"] > 0
    print("two files, output index:", check_index(r))
