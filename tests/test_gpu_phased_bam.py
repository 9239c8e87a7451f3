"""lcd_call_bam_regions with bam_out on the MI355X: two adjacent regions with reads across the cut, called and written as a phased BAM in one call.  The VCF side must be
what lcd_call_bam_regions gives; the file must inflate with zlib block by block to the input's header plus the @PG line and the oracle's record stream
(tests/bam_out_common.py) for the call's final haplotypes and phase sets, every shared read written once, by the first region."""
import ctypes as C

import pytest

import bam_out_common as bo
import call_chunks_common as kc
import clean_vars_common as cc
from test_gpu_clean_vars import write_chunk_bam

pytestmark = pytest.mark.gpu
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:test"


def _inputs(tmp_path, seed):
    whole = cc.make_diploid_chunk(seed, ref_len=12000, depth=12)
    chs = kc.split_chunk(whole, [6000])
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    write_chunk_bam(whole, bam)
    kc.write_fasta(fa, "chr11", whole)
    return whole, chs, bam, fa


def _names(path, reg_beg, reg_end):
    from longcalld_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.lcd_bam_load_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(_lib.LcdBamReads)]
    L.lcd_bam_reads_free.argtypes = [C.POINTER(_lib.LcdBamReads)]
    L.lcd_io_last_error.restype = C.c_char_p
    r = _lib.LcdBamReads()
    n = L.lcd_bam_load_region(path.encode(), b"chr11", reg_beg, reg_end, 30, 2, C.byref(r))
    assert n >= 0, L.lcd_io_last_error()
    names = [C.string_at(C.addressof(r.name_pool.contents) + r.name_off[i]) for i in range(n)]
    L.lcd_bam_reads_free(C.byref(r))
    return names


@pytest.mark.parametrize("seed", [kc.SEED_FLIP, kc.SEED_JOIN])
def test_two_regions_called_and_written_in_one_call(lcd, tmp_path, seed):
    whole, chs, bam, fa = _inputs(tmp_path, seed)
    begs, ends = [ch["reg_beg"] for ch in chs], [ch["reg_end"] for ch in chs]
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    plain = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", begs, ends, min_mapq=30, cfg=cfg)
    out = str(tmp_path / "out.bam")
    got = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", begs, ends, min_mapq=30, cfg=cfg, bam_out=dict(path=out, pg_line=PG, block_payload=0))
    assert got["bam_out_rc"] == 0, got["bam_out_error"]
    # the VCF side is untouched
    assert got["records"] == plain["records"] and got["vcf_body"] == plain["vcf_body"] and len(got["records"]) > 15
    for g, p in zip(got["chunks"], plain["chunks"]):
        assert g["haps"].tolist() == p["haps"].tolist() and g["phase_sets"].tolist() == p["phase_sets"].tolist()
    # the file, block by block through zlib
    hdr_in, bodies = bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(bam, "rb").read())))
    members = bo.bgzf_members(open(out, "rb").read())
    assert members[-1]["isize"] == 0 and all(m["isize"] > 0 for m in members[:-1])
    stream = b"".join(m["payload"] for m in members)
    want = bo.header_with_pg(hdr_in, PG.encode())
    assert stream.startswith(want) and members[0]["payload"] == want      # the header has its own block
    n_out = n_shared = n_tagged = 0
    for c, ch in enumerate(chs):
        recs = bo.region_records(bodies, ch["reg_beg"], ch["reg_end"], 30)
        assert len([1 for _, r in recs if r >= 0]) == len(got["chunks"][c]["haps"])
        sk, sf = bo.skip_counts(recs, chs[c - 1]["reg_beg"], chs[c - 1]["reg_end"]) if c else (0, 0)
        s, n = bo.tagged_stream(recs, got["chunks"][c]["haps"], got["chunks"][c]["phase_sets"], sk, sf)
        want += s; n_out += n; n_shared += sk
        n_tagged += int((got["chunks"][c]["haps"] != 0).sum())
    assert n_shared > 0 and n_tagged > 10 and n_out == len(bodies)       # reads cross the cut; each is written once
    assert stream == want
    assert got["bam_out"]["n_records_out"] == n_out and got["bam_out"]["n_filtered_out"] == 0
    assert got["bam_out"]["bytes_inflated"] == len(stream) and got["bam_out"]["bytes_file"] == sum(m["bsize"] for m in members)
    assert b"HPi" in stream and b"PSi" in stream
    # and back through the host loader: the same reads in the same order
    names = _names(out, whole["reg_beg"], whole["reg_end"])
    assert names == _names(bam, whole["reg_beg"], whole["reg_end"]) and len(names) == len(bodies)


def test_an_unwritable_output_leaves_the_vcf_side_valid(lcd, tmp_path):
    whole, chs, bam, fa = _inputs(tmp_path, kc.SEED_JOIN)
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    got = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", [chs[0]["reg_beg"]], [chs[0]["reg_end"]], min_mapq=30, cfg=cfg,
                               bam_out=dict(path=str(tmp_path / "no_such_dir" / "out.bam")))
    assert got["bam_out_rc"] < 0 and "cannot open" in got["bam_out_error"]
    plain = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", [chs[0]["reg_beg"]], [chs[0]["reg_end"]], min_mapq=30, cfg=cfg)
    assert got["records"] == plain["records"] and got["vcf_body"] == plain["vcf_body"] and len(got["records"]) > 5   # (freed normally by the wrapper)
