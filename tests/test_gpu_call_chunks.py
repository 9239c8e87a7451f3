"""lcd_chunks_call and lcd_call_bam_regions on the MI355X: chunks (or regions of an indexed BAM + a FASTA) to stitched genotype records and VCF body lines in one
call, against the composition of the existing oracles (tests/call_chunks_common.py::oracle_call) byte for byte, and against the same chain stepped through the
library's single exports."""
import ctypes as C

import numpy as np
import pytest

import call_chunks_common as kc
import clean_vars_common as cc
from test_gpu_clean_vars import device_chunk, write_chunk_bam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prod():
    from longcalld_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def need_ref(oracle):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")


def item_of(ch):
    return dict(ref=ch["ref"], ref_beg=ch["ref_beg"], reg_beg=ch["reg_beg"], reg_end=ch["reg_end"], is_ont=ch.get("is_ont", 0),
                ordered_read_ids=np.arange(len(ch["reads"]), dtype=np.int32), is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8))


@pytest.mark.parametrize("seed", [kc.SEED_FLIP, kc.SEED_JOIN])
def test_two_chunks_stitched_equal_the_oracle_and_the_stepped_chain(lcd, oracle, prod, seed):
    need_ref(oracle)
    chs = kc.two_chunks(seed)
    devs = [device_chunk(lcd, ch) for ch in chs]
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    before = lcd.copy_counters()
    got = lcd.chunks_call(devs, [item_of(ch) for ch in chs], cfg)
    assert lcd.copy_counters() == before                                          # no digar and no base crossed PCIe
    want = kc.oracle_call(lcd, oracle, chs, max_len=kc.TWO_CHUNK_MAX_LEN)
    kc.same_call(got, want)
    assert got["chunks"][1]["flip_hap"] == (1 if seed == kc.SEED_FLIP else 0) and got["chunks"][1]["flip_pre_PS"] > 0
    step = kc.stepped_call(lcd, oracle, prod, chs, devs, lcd.pass_opt(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    kc.same_call(got, step, state_keys=("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps", "var_phase_set", "hap_to_cons_alle", "hap_to_alle_profile"))
    for g in got["chunks"]:                                                       # what lcd_read_tags takes
        assert g["haps"].tolist() == g["state"]["haps"].tolist() and len(g["phase_sets"]) == len(g["haps"])
    single = [lcd.chunks_call([d], [item_of(ch)], cfg) for d, ch in zip(devs, chs)]   # one chunk alone: the same table, no stitch
    for s, g in zip(single, got["chunks"]):
        cc.same_clean_vars(s["chunks"][0]["cv"], g["cv"])
        assert s["chunks"][0]["flip_hap"] == 0 and s["chunks"][0]["flip_pre_PS"] == -1
    for d in devs:
        d.close()


def test_somatic_and_refine_settings_are_refused(lcd):
    ch = kc.two_chunks(kc.SEED_JOIN)[0]
    dev = device_chunk(lcd, ch)
    for cfg in (lcd.call_cfg(0, clean=dict(out_somatic=1)), lcd.call_cfg(0, opt=dict(collect_ref_read_aln_str=1))):
        with pytest.raises(lcd.LcdError, match="-2"):
            lcd.chunks_call([dev], [item_of(ch)], cfg)
    assert lcd.chunks_call([], [])["records"] == []
    dev.close()


def test_hg002_chunk_from_bam_and_fasta_equals_the_oracle_composition(lcd, oracle, tmp_path):
    """the real HG002 chunk, moved to the start of a small contig so that the test FASTA stays small, through lcd_call_bam_regions: read order from the NM-less
    records (position, end descending, name), reference window fetched with the reference's padding"""
    need_ref(oracle)
    ch = kc.shift_chunk(cc.events_chunk(), 50001)
    bam, fa = str(tmp_path / "hg002.bam"), str(tmp_path / "ref.fa")
    write_chunk_bam(ch, bam)
    kc.write_fasta(fa, "chr11", ch)
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=3000))
    got = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", [ch["reg_beg"]], [ch["reg_end"]], min_mapq=0, cfg=cfg)
    order = kc.python_order([r["pos0"] for r in ch["reads"]], [kc.read_end(r) for r in ch["reads"]], [0] * len(ch["reads"]), [f"r{i}" for i in range(len(ch["reads"]))])
    assert got["chunks"][0]["ordered_read_ids"].tolist() == order.tolist()
    # the library fetched [ref_beg - 50 000, ref_end + 50 000] cut to the contig: N around the window; the oracle side gets the same bases
    lo = max(50000, ch["reg_beg"] - 1) - 50000 + 1
    hi = min(ch["whole_ref_len"] - 50000 - 1, ch["reg_end"] - 1) + 50000 + 1
    wide = np.full(hi - lo + 1, 4, np.uint8)
    wide[ch["ref_beg"] - lo:ch["ref_beg"] - lo + len(ch["ref"])] = ch["ref"]
    want = kc.oracle_call(lcd, oracle, [dict(ch, ref=wide, ref_beg=lo)], max_len=3000, orders=[order])
    kc.same_call(got, want)
    assert got["chunks"][0]["n_passes"] == want["chunks"][0]["n_passes"] == 2 and len(got["records"]) > 300 and got["vcf_body"].count("\n") > 200
    # cand_var_t.alt_ref_base reaches the text: noisy-region gap records whose anchor base is not the reference base at their position (src/collect_var.c:1544)
    odd = kc.anchor_differs(got["records"])
    assert odd and all(got["chunks"][0]["cv"]["alt_ref_base"][r["cand_i"]] != 4 for r in odd)
    lines = {int(l.split("\t")[1]): l.split("\t") for l in got["vcf_body"].splitlines()}
    assert any(r["pos"] in lines and lines[r["pos"]][3][0] != lines[r["pos"]][4][0] for r in odd)


def m_cigar(cig):
    """an EQX CIGAR as minimap2 writes it without --eqx: '=' and 'X' runs joined into 'M'"""
    out = []
    for c in cig:
        op, ln = int(c) & 0xf, int(c) >> 4
        op = 0 if op in (7, 8) else op
        if out and out[-1][0] == op:
            out[-1][1] += ln
        else:
            out.append([op, ln])
    return np.array([(ln << 4) | op for op, ln in out], np.uint32)


def test_two_regions_of_an_m_cigar_bam_equal_the_oracle_composition(lcd, oracle, tmp_path):
    """plain-M records without cs / MD tags: the first pass leaves them without a digar source, the wrapper makes the chunks again with the fetched window as the
    reference to compare with, and the result is that of the same reads with EQX CIGARs; the two regions are stitched"""
    need_ref(oracle)
    whole = cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12)
    chs = kc.split_chunk(whole, [6000])
    bam, fa = str(tmp_path / "m.bam"), str(tmp_path / "ref.fa")
    write_chunk_bam(dict(whole, reads=[dict(r, cigar=m_cigar(r["cigar"])) for r in whole["reads"]]), bam)
    kc.write_fasta(fa, "chr11", whole)
    name = {id(r): f"r{i}" for i, r in enumerate(whole["reads"])}
    orders = [kc.python_order([r["pos0"] for r in ch["reads"]], [kc.read_end(r) for r in ch["reads"]], [0] * len(ch["reads"]), [name[id(r)] for r in ch["reads"]]) for ch in chs]
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    got = lcd.call_bam_regions(bam, bam + ".bai", fa, "chr11", [ch["reg_beg"] for ch in chs], [ch["reg_end"] for ch in chs], min_mapq=30, cfg=cfg)
    for g, o in zip(got["chunks"], orders):
        assert g["ordered_read_ids"].tolist() == o.tolist() and not g["is_skipped"].any()
    want = kc.oracle_call(lcd, oracle, chs, max_len=kc.TWO_CHUNK_MAX_LEN, orders=orders)
    kc.same_call(got, want)
    assert got["chunks"][1]["flip_pre_PS"] > 0 and len(got["records"]) > 15


def test_planted_insertion_whose_anchor_is_a_snp_reaches_the_vcf_line(lcd, oracle):
    """cand_var_t.alt_ref_base through the table to the text: the insertion's ALT begins with the SNP's base, not with the reference base (src/collect_var.c:1544)"""
    need_ref(oracle)
    ch, pos = kc.planted_anchor_chunk()
    dev = device_chunk(lcd, ch)
    got = lcd.chunks_call([dev], [item_of(ch)])
    kc.same_call(got, kc.oracle_call(lcd, oracle, [ch]))
    odd = kc.anchor_differs(got["records"])
    assert [r["pos"] for r in odd] == [pos] and got["chunks"][0]["cv"]["alt_ref_base"][odd[0]["cand_i"]] == odd[0]["alt"][0][0] != odd[0]["ref"][0]
    line = [l.split("\t") for l in got["vcf_body"].splitlines() if l.split("\t")[1] == str(pos) and len(l.split("\t")[4]) == 6]
    assert len(line) == 1 and line[0][3][0] != line[0][4][0]
    dev.close()

