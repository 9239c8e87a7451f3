"""lcd_chunk_clean_vars on the MI355X: the first round of collect_var_main (candidate sites, pile-up, classification + extra noisy regions, read x variant
profile) on a device-resident chunk, field for field against the C oracle (tests/c/clean_vars_oracle.c) on the oracle's digars of the same records."""
import struct

import numpy as np
import pytest

import clean_vars_common as cc
from test_clean_vars_oracle import edge_chunk
from test_io import _bgzf, _write_bai

pytestmark = pytest.mark.gpu


def device_chunk(lcd, ch):
    r = ch["reads"]
    return lcd.DeviceChunk([x["pos0"] for x in r], [x["cigar"] for x in r], [x["qual"] for x in r], [x["bseq"] for x in r], ch["reg_beg"], ch["reg_end"],
                           ch["whole_ref_len"], is_ont=ch.get("is_ont", 0))


def chunk_args(lcd, ch, digs):
    """the caller's side of the call: pre_process_noisy_regs (device) on sdust's low-complexity intervals (device), reads in position order"""
    low = lcd.sdust(ch["ref"])
    ci = cc.chunk_inputs(ch, digs)
    pre = lcd.pre_process_noisy_regs(ci["chunk_noisy"], low, ci["read_beg"], ci["read_end"], ci["read_ivs"])
    return dict(ordered_read_ids=np.arange(len(ch["reads"]), dtype=np.int32), ref=ch["ref"], ref_beg=ch["ref_beg"], ref_end=ch["ref_beg"] + len(ch["ref"]) - 1,
                reg_beg=ch["reg_beg"], reg_end=ch["reg_end"], pre_regs=pre, low_comp=low, is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8))


def oracle_of(ch, digs, a, opt):
    return cc.run_oracle(ch, digs, opt, pre_regs=a["pre_regs"], low_comp=a["low_comp"], ordered=a["ordered_read_ids"])


@pytest.mark.parametrize("seed", [3, 17, 29])
def test_hifi_chunks_equal_the_oracle_and_no_digar_crosses_pcie(lcd, oracle, seed):
    ch = cc.make_diploid_chunk(seed)
    digs = cc.read_digars(ch, oracle)
    a = chunk_args(lcd, ch, digs)
    opt = lcd.clean_opt(0)
    dev = device_chunk(lcd, ch)
    before = lcd.copy_counters()
    got = dev.clean_vars(**a, opt=opt)
    assert lcd.copy_counters()[0] == before[0]                 # no digar bytes device -> host
    assert got["qual_upload_bytes"] == sum(len(x["qual"]) for x in ch["reads"])
    want = oracle_of(ch, digs, a, opt)
    assert want["n_vars"] > 30 and len(want["alleles"]) > 0
    cc.same_clean_vars(got, want)
    again = dev.clean_vars(**a, opt=opt)                       # the qualities went up once
    assert again["qual_upload_bytes"] == 0
    cc.same_clean_vars(again, want)
    dev.close()


def test_ont_strand_bias_chunk_equals_the_oracle(lcd, oracle):
    ch = cc.make_diploid_chunk(41, is_ont=1, depth=40, err=0.004, n_bias=12)
    digs = cc.read_digars(ch, oracle, is_ont=1)
    a = chunk_args(lcd, ch, digs)
    dev = device_chunk(lcd, ch)
    ont, hifi = lcd.clean_opt(1), lcd.clean_opt(0)
    got = dev.clean_vars(**a, opt=ont)
    cc.same_clean_vars(got, oracle_of(ch, digs, a, ont))
    plain = dev.clean_vars(**a, opt=hifi)
    cc.same_clean_vars(plain, oracle_of(ch, digs, a, hifi))
    assert got["n_vars"] < plain["n_vars"]                     # the strand-biased sites leave the candidate list
    dev.close()


def test_edge_case_chunk_equals_the_oracle(lcd, oracle):
    ch, pre, low = edge_chunk()
    digs = cc.read_digars(ch, oracle)
    for opt in (lcd.clean_opt(0), lcd.clean_opt(1)):
        want = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low)
        dev = device_chunk(lcd, ch)
        got = dev.clean_vars(np.arange(len(ch["reads"])), ch["ref"], ch["ref_beg"], ch["ref_beg"] + len(ch["ref"]) - 1, ch["reg_beg"], ch["reg_end"], pre, low,
                             is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8), opt=opt)
        cc.same_clean_vars(got, want)
        dev.close()


def test_batch_of_8_equals_8_single_calls(lcd, oracle):
    chs = [cc.make_diploid_chunk(100 + i, ref_len=15000) for i in range(8)]
    digs = [cc.read_digars(ch, oracle) for ch in chs]
    args = [chunk_args(lcd, ch, d) for ch, d in zip(chs, digs)]
    devs = [device_chunk(lcd, ch) for ch in chs]
    opt = lcd.clean_opt(0)
    single = [d.clean_vars(**a, opt=opt) for d, a in zip(devs, args)]
    batch = lcd.chunk_clean_vars_batch(devs, args, opt)
    for s, b, ch, dg, a in zip(single, batch, chs, digs, args):
        cc.same_clean_vars(b, s)
        cc.same_clean_vars(b, oracle_of(ch, dg, a, opt))
    for d in devs:
        d.close()


def write_chunk_bam(ch, path, chrom="chr11"):
    """the chunk's records as a coordinate-sorted BAM + .bai (the writers of tests/test_io.py)"""
    refs = [(chrom, ch["whole_ref_len"])]
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n"
    d = b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", len(refs))
    for nm, ln in refs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    recs = []
    for i, r in enumerate(ch["reads"]):
        name = f"r{i}".encode() + b"\0"
        cig = np.asarray(r["cigar"], "<u4"); qlen = len(r["qual"])
        flag = 16 if r["is_rev"] else 0
        body = struct.pack("<iiBBHHHiiii", 0, r["pos0"], len(name), 60, 4680, len(cig), flag, qlen, -1, -1, 0) + name + cig.tobytes() + \
            np.asarray(r["bseq"], np.uint8).tobytes() + np.asarray(r["qual"], np.uint8).tobytes()
        u0 = len(d)
        d += struct.pack("<i", len(body)) + body
        rl = sum(int(c) >> 4 for c in cig if (int(c) & 0xf) in (0, 2, 3, 7, 8))
        recs.append(dict(tid=0, pos=r["pos0"], end=r["pos0"] + max(rl, 1), u0=u0, u1=len(d)))
    block = 30000; coffs = []
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    coffs.append(coffs[-1] + 1)
    for x in recs:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", len(refs), recs)


def test_chunk_from_bam_gives_the_same_result(lcd, oracle, tmp_path):
    ch = cc.make_diploid_chunk(57)
    digs = cc.read_digars(ch, oracle)
    a = chunk_args(lcd, ch, digs)
    opt = lcd.clean_opt(0)
    path = str(tmp_path / "c.bam")
    write_chunk_bam(ch, path)
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", ch["reg_beg"], ch["reg_end"], min_mapq=0)
    assert dev.n == len(ch["reads"])
    a["is_rev"] = (np.asarray(dev.meta["flag"]) & 0x10 != 0).astype(np.uint8)
    got = dev.clean_vars(**a, opt=opt)
    assert got["qual_upload_bytes"] == 0                       # the qualities already lie in HBM
    host = device_chunk(lcd, ch)
    cc.same_clean_vars(got, host.clean_vars(**a, opt=opt))
    cc.same_clean_vars(got, oracle_of(ch, digs, a, opt))
    dev.close(); host.close()


def real_args(lcd, ch, digs):
    """chunk_args for a chunk whose reference slice starts at ref_beg != 1: sdust's 0-based intervals shifted as chunk->low_comp_cr is filled
    (src/bam_utils.c:1579)"""
    o = ch["ref_beg"]
    low = lcd.sdust(ch["ref"])
    low_cr = np.stack([o + low[:, 0] - 1, o + low[:, 1] - 1], 1).astype(np.int64)
    ci = cc.chunk_inputs(ch, digs)
    pre = lcd.pre_process_noisy_regs(ci["chunk_noisy"], low_cr, ci["read_beg"], ci["read_end"], ci["read_ivs"])
    return dict(ordered_read_ids=np.arange(len(ch["reads"]), dtype=np.int32), ref=ch["ref"], ref_beg=o, ref_end=o + len(ch["ref"]) - 1, reg_beg=ch["reg_beg"],
                reg_end=ch["reg_end"], pre_regs=pre, low_comp=low_cr, is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8))


def test_real_hg002_chunk_host_array_and_bam_equal_the_oracle(lcd, oracle, tmp_path):
    """the HG002 HiFi chunk of tests/golden/testdata_events.npz through lcd_chunk_create and through lcd_chunk_create_from_bam on the same records written as a
    BAM: both equal each other and the oracle, field for field"""
    ch = cc.events_chunk()
    digs = cc.read_digars(ch, oracle)
    a = real_args(lcd, ch, digs)
    opt = lcd.clean_opt(0)
    want = oracle_of(ch, digs, a, opt)
    assert want["n_vars"] > 100 and len(want["regs"]) > 10 and len(want["alleles"]) > 1000
    host = device_chunk(lcd, ch)
    before = lcd.copy_counters()
    got = host.clean_vars(**a, opt=opt)
    assert lcd.copy_counters()[0] == before[0]
    cc.same_clean_vars(got, want)
    path = str(tmp_path / "hg002.bam")
    write_chunk_bam(ch, path)
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", ch["reg_beg"], ch["reg_end"], min_mapq=0)
    assert dev.n == len(ch["reads"])
    a["is_rev"] = (np.asarray(dev.meta["flag"]) & 0x10 != 0).astype(np.uint8)
    cc.same_clean_vars(dev.clean_vars(**a, opt=opt), want)
    host.close(); dev.close()
