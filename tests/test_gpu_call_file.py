"""lcd_call_files with one file on the MI355X: a whole BAM (five contigs) and a FASTA to one VCF and one phased BAM, in windows of chunks, against lcd_call_bam_regions per
contig with that contig's planned regions -- the merged code, itself pinned to the oracles (tests/test_gpu_call_chunks.py).  Records, VCF body, every chunk's flips
and n_passes, and the output BAM's record stream must not depend on window_chunks, overlap or loader_threads."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc

pytestmark = pytest.mark.gpu

CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
EOF_MEMBER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HEADER_ARGS = dict(source_version="test-1", cmdline="call ref.fa in.bam", date_yyyymmdd="20240102")


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """chr1 / chr2: the seeded 12 kb diploid contigs of kc.two_chunks; chr3: 18 kb; chr4: 12 kb without a read; chrM: 6 kb with reads"""
    d = tmp_path_factory.mktemp("call_file")
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12),
               chr3=cc.make_diploid_chunk(41, ref_len=18000, depth=12), chrM=cc.make_diploid_chunk(43, ref_len=6000, depth=12, read_len=(1000, 3000)))
    refs = dict({k: v["ref"] for k, v in chs.items()}, chr4=np.random.default_rng(4).integers(0, 4, 12000).astype(np.uint8))
    order = ["chr1", "chr2", "chr3", "chr4", "chrM"]
    reads = {k: (chs[k]["reads"] if k in chs else []) for k in order}
    bam, mbam, fa = str(d / "in.bam"), str(d / "m.bam"), str(d / "ref.fa")
    fc.write_multi_bam(bam, [(k, len(refs[k]), reads[k]) for k in order], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    fc.write_multi_bam(mbam, [(k, len(refs[k]), [dict(r, cigar=fc.m_cigar(r["cigar"])) for r in reads[k]]) for k in order])
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in order])
    return dict(dir=d, bam=bam, mbam=mbam, fa=fa, contigs=[(k, len(refs[k])) for k in order])


def yard_contig(lcd, data, chrom, begs, ends, with_bam=True):
    out = str(data["dir"] / f"yard_{chrom}_{begs[0]}.bam")
    res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], chrom, begs, ends, min_mapq=30, cfg=cfg_of(lcd),
                               bam_out=dict(path=out, pg_line=PG) if with_bam else None)
    if with_bam:
        assert res["bam_out_rc"] == 0, res["bam_out_error"]
        hdr, res["bam_bodies"] = bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(out, "rb").read())))
        res["bam_header"] = hdr
    return res


def joined(parts):
    return dict(records=[r for p in parts for r in p["records"]], vcf_body="".join(p["vcf_body"] for p in parts),
                flips=[(c["flip_hap"], c["flip_pre_PS"], c["flip_cur_PS"]) for p in parts for c in p["chunks"]], n_passes=[c["n_passes"] for p in parts for c in p["chunks"]],
                n_records=[c["n_records"] for p in parts for c in p["chunks"]], bam_bodies=[b for p in parts for b in p.get("bam_bodies", [])])


@pytest.fixture(scope="module")
def yard(lcd, data):
    """per contig lcd_call_bam_regions (with bam_out) with the contig's planned regions, concatenated over the contigs the default mode keeps"""
    plan, fb = lcd.plan_chunks(data["contigs"], chunk_len=CHUNK_LEN)
    assert fb == 0 and [(t, e - b + 1) for t, b, e in plan] == [(0, 6000)] * 2 + [(1, 6000)] * 2 + [(2, 6000)] * 3 + [(3, 6000)] * 2        # 2 + 2 + 3 + 2, chrM left out
    parts = {}
    for tid in range(4):
        mine = [(b, e) for t, b, e in plan if t == tid]
        parts[tid] = yard_contig(lcd, data, data["contigs"][tid][0], [b for b, _ in mine], [e for _, e in mine])
    y = joined([parts[t] for t in range(4)])
    y["plan"], y["parts"], y["bam_header"] = plan, parts, parts[0]["bam_header"]
    return y


def test_the_yardstick_takes_every_branch(yard):
    flips = yard["flips"]
    print("yardstick flips:", flips, "n_passes:", yard["n_passes"], "records per chunk:", yard["n_records"])
    assert any(f[0] == 1 for f in flips)                                             # a chunk whose haplotypes were swapped
    assert any(f[1] > 0 and f[0] == 0 for f in flips)                                # one joined as it is
    assert yard["n_records"][7:9] == [0, 0] and not yard["parts"][3]["records"]      # chr4 contributes no record
    assert len(yard["records"]) > 30 and yard["vcf_body"].count("\n") > 20 and len(yard["bam_bodies"]) > 100
    assert flips[0] == flips[2] == flips[4] == flips[7] == (0, -1, -1)               # the first chunk of a contig is never joined


def run(lcd, data, tag, bam=None, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
    kw.setdefault("no_vcf_header", 1)
    res = lcd.call_file(bam or data["bam"], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), keep_records=True, **kw)
    res["text"] = open(vcf).read() if not kw.get("vcf_bgzf") else None
    res["vcf"], res["bam"] = vcf, out
    image = open(out, "rb").read()
    assert image.endswith(EOF_MEMBER)
    members = bo.bgzf_members(image)
    assert sum(1 for m in members if m["isize"] == 0) == 1                           # ONE EOF member, at the end
    res["bam_header"], res["bam_bodies"] = bo.bam_split(b"".join(m["payload"] for m in members))
    return res


def same_as(got, want, n_chunks):
    assert got["n_planned"] == n_chunks == len(got["chunks"])
    assert [(c["flip_hap"], c["flip_pre_PS"], c["flip_cur_PS"]) for c in got["chunks"]] == want["flips"]
    assert [c["n_passes"] for c in got["chunks"]] == want["n_passes"] and [c["n_records"] for c in got["chunks"]] == want["n_records"]
    assert got["records"] == want["records"] and got["n_records"] == len(want["records"])
    assert got["text"] == want["vcf_body"] and got["n_vcf_lines"] == want["vcf_body"].count("\n")
    assert got["bam_bodies"] == want["bam_bodies"]                                   # the phased BAM's record stream, HP / PS tags included
    assert got["bam_out"]["n_records_out"] + got["bam_out"]["n_filtered_out"] == len(want["bam_bodies"])


@pytest.mark.parametrize("window,overlap,threads", [(1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 0, 0), (2, 1, 1), (2, 1, 3)])
def test_every_schedule_equals_the_yardstick(lcd, data, yard, window, overlap, threads):
    got = run(lcd, data, f"w{window}o{overlap}t{threads}", window_chunks=window, overlap=overlap, loader_threads=threads)
    same_as(got, yard, 9)
    assert [(c["tid"], c["reg_beg"], c["reg_end"]) for c in got["chunks"]] == yard["plan"]
    assert got["n_empty"] == 2 and got["n_loaded"] == 7 and got["plan_fallback"] == 0
    assert got["n_region_loads"] == 9                                                # every region read and inflated once
    assert got["n_windows"] == -(-9 // (window or 32))
    assert got["n_reads"] == sum(c["n_reads"] for c in got["chunks"]) > 0 and got["chunks"][7]["n_reads"] == got["chunks"][8]["n_reads"] == 0
    assert got["bam_header"] == yard["bam_header"]
    assert got["ms_wall"] > 0 and got["peak_device_bytes"] > 0


def test_all_contigs_and_a_region_string(lcd, data, yard):
    got = run(lcd, data, "all", window_chunks=4, overlap=0, contig_mode=2)
    m = yard_contig(lcd, data, "chrM", [1], [6000])
    assert m["records"] and "chrM\t" in m["vcf_body"]
    want = joined([yard["parts"][t] for t in range(4)] + [m])
    same_as(got, want, 10)
    assert got["text"].splitlines()[-1].startswith("chrM\t") and got["chunks"][9]["tid"] == 4     # chrM's records come after chr4's (none)
    got = run(lcd, data, "region", window_chunks=1, overlap=0, regions=["chr3:4000-15000"])
    assert [(c["tid"], c["reg_beg"], c["reg_end"]) for c in got["chunks"]] == [(2, 4000, 9999), (2, 10000, 15000)]       # chunks from 4000
    same_as(got, joined([yard_contig(lcd, data, "chr3", [4000, 10000], [9999, 15000])]), 2)


def test_plain_m_cigars_are_loaded_once_and_give_the_same_result(lcd, data, yard):
    got = run(lcd, data, "mcig", bam=data["mbam"], window_chunks=2, overlap=0)
    assert got["n_region_loads"] == got["n_planned"] == 9                            # lcd_call_bam_regions reads such a region twice
    for k in ("records", "vcf_body"):
        assert (got["records"] if k == "records" else got["text"]) == yard[k]
    assert [(c["flip_hap"], c["flip_pre_PS"], c["flip_cur_PS"]) for c in got["chunks"]] == yard["flips"] and [c["n_passes"] for c in got["chunks"]] == yard["n_passes"]


def header_text(lcd, contigs, sample):
    lib = lcd.load_library()
    names = (C.c_char_p * len(contigs))(*[n.encode() for n, _ in contigs]); lens = (C.c_int64 * len(contigs))(*[l for _, l in contigs])
    out = C.c_void_p()
    lib.lcd_vcf_header.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_char_p, C.POINTER(C.c_void_p)]
    assert lib.lcd_vcf_header(HEADER_ARGS["source_version"].encode(), HEADER_ARGS["cmdline"].encode(), HEADER_ARGS["date_yyyymmdd"].encode(), len(contigs), names, lens,
                              sample.encode(), C.byref(out)) > 0
    text = C.string_at(out).decode()
    C.CDLL(None).free(out)
    return text


def test_the_vcf_file_plain_and_compressed(lcd, data, yard):
    want = header_text(lcd, data["contigs"], "sample7") + yard["vcf_body"]           # every contig of the BAM header, chrM included; SM of the @RG line
    got = run(lcd, data, "plain", window_chunks=4, overlap=0, no_vcf_header=0, **HEADER_ARGS)
    assert got["text"] == want and "##contig=<ID=chrM,length=6000>" in want and want.splitlines()[-1 - yard["vcf_body"].count("\n")].endswith("\tsample7")
    got = run(lcd, data, "z", window_chunks=4, overlap=1, no_vcf_header=0, vcf_bgzf=1, sample_name="given", **HEADER_ARGS)
    image = open(got["vcf"], "rb").read()
    assert gzip.decompress(image).decode() == header_text(lcd, data["contigs"], "given") + yard["vcf_body"]
    assert image.endswith(EOF_MEMBER) and sum(1 for m in bo.bgzf_members(image) if m["isize"] == 0) == 1
    nosm = run(lcd, data, "nosm", bam=data["mbam"], window_chunks=0, overlap=0, no_vcf_header=0, regions=["chr4"], **HEADER_ARGS)
    assert nosm["text"] == header_text(lcd, data["contigs"], data["mbam"])           # no @RG: the BAM path; chr4 has no record


def test_the_first_error_stops_the_pipeline_and_leaves_no_eof_member(lcd, data):
    """a FASTA index without chr3: the loader fails on the third window while the first two are being called and written"""
    fa = str(data["dir"] / "short.fa")
    os.symlink(data["fa"], fa)
    open(fa + ".fai", "w").write("".join(l for l in open(data["fa"] + ".fai") if not l.startswith("chr3\t")))
    for overlap in (1, 0):
        vcf, out = str(data["dir"] / f"err{overlap}.vcf.gz"), str(data["dir"] / f"err{overlap}.bam")
        with pytest.raises(lcd.LcdError, match="chr3"):
            lcd.call_file(data["bam"], fa, chunk_len=CHUNK_LEN, window_chunks=2, overlap=overlap, loader_threads=2, vcf_path=vcf, vcf_bgzf=1, bam_out=dict(path=out), cfg=cfg_of(lcd))
        for path in (vcf, out):
            image = open(path, "rb").read()
            assert not image.endswith(EOF_MEMBER) and all(m["isize"] > 0 for m in bo.bgzf_members(image))
