"""lcd_chunk_tag_records on the MI355X: the HP:i / PS:i rewrite of a chunk's records where the inflate left them in HBM, byte for byte against the oracle of
tests/bam_out_common.py, on one synthetic BAM whose records straddle BGZF blocks and carry every named condition of the rule."""
import struct

import numpy as np
import pytest

import bam_out_common as bo
from bam_src_common import CONTIG, record, write_bam

pytestmark = pytest.mark.gpu
BIG = 3000000000
MIN_MAPQ = 30


def _read(i, pos0, qlen, flag=0):
    # names of different lengths: the records and their auxiliary blocks start at every byte offset modulo 4
    return dict(name=(b"rd%d" % i) + b"x" * (i % 5), pos0=pos0, flag=flag, qlen=qlen, bseq=np.full((qlen + 1) // 2, 0x11, np.uint8), qual=np.full(qlen, 30, np.uint8))


def cases():
    """[(condition, raw auxiliary bytes, qlen, flag, mapq, hap, ps)] in file order; hap / ps are used for the kept ones"""
    rg = b"RGZgrp1\0"
    c = [
        ("no_aux", b"", 120, 0, 60, 0, 0),
        ("no_aux_append", b"", 121, 0, 60, 1, 4000),
        ("long_25kb_record", rg + b"NMi\x03\0\0\0", 16001, 0, 60, 2, 4000),         # beside a short record, at odd offsets
        ("short_40_byte_aux", rg + b"XAAqXBBC\x03\0\0\0HPiNMC\x01" + b"XZZhello\0", 33, 0, 60, 1, 4000),   # (the bytes HPi inside a B array)
        ("HP_C_equal", rg + b"HPC\x01", 140, 0, 60, 1, 0),
        ("HP_i_equal", b"HPi\x02\0\0\0" + rg, 141, 0, 60, 2, 0),
        ("PS_i_equal", b"PSi\xa0\x0f\0\0", 142, 0, 60, 0, 4000),
        ("PS_I_equal", b"PSI\x00\x5e\xd0\xb2", 143, 16, 60, 1, BIG),
        ("HP_C_different", b"HPC\x01NMC\x05", 144, 0, 60, 2, 4000),
        ("HP_Z", b"HPZ1\0" + rg, 145, 0, 60, 1, 0),
        ("HP_f", b"HPf\0\0\x80\x3f", 146, 0, 60, 1, 0),
        ("PS_s_negative", b"PSs\xff\xff", 147, 0, 60, 0, 5),
        ("both_replaced", b"PSi\x01\0\0\0XAAqHPi\x01\0\0\0", 148, 0, 60, 2, 7),
        ("HP_kept_PS_replaced", b"HPC\x02PSC\x09" + rg, 149, 0, 60, 2, 300),
        ("hap_0_deletes_HP", b"XAAqHPC\x01", 150, 0, 60, 0, 0),
        ("ps_0_deletes_PS", b"PSi\x07\0\0\0", 151, 0, 60, 0, 0),
        ("ps_minus_1_deletes_PS", b"PSi\x07\0\0\0XAAq", 152, 0, 60, 1, -1),
        ("two_HP_first_replaced", b"HPC\x01HPC\x02", 153, 0, 60, 2, 0),
        ("two_HP_first_deleted", b"HPC\x01" + rg + b"HPC\x02", 154, 0, 60, 0, 0),
        ("HPi_in_Z", b"XZZHPi\x01\0", 155, 0, 60, 0, 0),
        ("B_past_the_record", b"XBBi\xe8\x03\0\0\x01\0\0\0HPC\x01", 156, 0, 60, 1, 0),
        ("Z_without_NUL", b"XZZabcHPC\x01", 157, 0, 60, 0, 4000),
        ("ps_above_2^32", b"PSi\x05\0\0\0", 158, 0, 60, 1, (1 << 32) + 5),
        ("cs_in_front", b"csZ" + b":100*ag" * 300 + b"\0" + b"PSi\x01\0\0\0HPC\x02", 159, 0, 60, 1, 9),
    ]
    for k, (fl, mq) in enumerate(((4, 60), (256, 60), (2048, 60), (0, 3))):
        c.append((f"filtered_{fl}_{mq}_tags", b"HPC\x01XAAqPSi\x07\0\0\0PSC\x01", 60 + k, fl, mq, 2, 9))
        c.append((f"filtered_{fl}_{mq}_plain", b"XAAq", 70 + k, fl, mq, 2, 9))
    for k in range(8):
        c.append((f"tail_{k}", (b"HPC\x01" if k & 1 else b"") + (b"PSi\x07\0\0\0" if k & 2 else b""), 200 + 7 * k, 0, 60, k % 3, 4000 if k & 4 else 0))
    return c


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tags") / "t.bam")
    cs = cases()
    recs = []
    for i, (_, aux, qlen, flag, mapq, _, _) in enumerate(cs):
        a = _read(i, 500 + 230 * i, qlen, flag)
        recs.append(record(a, [(qlen << 4) | 7], [(None, None, aux)], mapq=mapq))
    write_bam(path, recs, block=9000)
    return path, cs, [r["body"] for r in recs]


def expected(cs, bodies, reg_beg, reg_end, sk=0, sf=0, trace=None):
    recs = bo.region_records(bodies, reg_beg, reg_end, MIN_MAPQ)
    kept = [i for i, b in enumerate(bodies) if any(b is rb and r >= 0 for rb, r in recs)]
    haps = [cs[i][5] for i in kept]; ps = [cs[i][6] for i in kept]
    return bo.tagged_stream(recs, haps, ps, sk, sf, trace), haps, ps


def test_every_named_condition_byte_for_byte(lcd, bam):
    path, cs, bodies = bam
    assert len(cs) == 40
    ch = lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, 1, 29000, min_mapq=MIN_MAPQ)
    trace = []
    (want, n_want), haps, ps = expected(cs, bodies, 1, 29000, trace=trace)
    assert ch.n == len(haps) == 32 and n_want == 40
    for m in ("HP:kept_in_place:C", "HP:kept_in_place:i", "PS:kept_in_place:i", "PS:kept_in_place:I", "HP:replaced:C", "HP:replaced:Z", "HP:replaced:f", "PS:replaced:s",
              "PS:replaced:C", "HP:unwanted_deleted:C", "PS:unwanted_deleted:i", "HP:appended_absent", "PS:appended_absent", "HP:filtered_deleted", "PS:filtered_deleted",
              "HP:filtered_absent", "HP:unwanted_absent"):
        assert m in trace, m
    got, n_got = ch.tag_records(haps, ps)
    assert n_got == n_want and len(got) == len(want)
    o = 0
    for i, (name, *_rest) in enumerate(cs):                              # record by record: a mismatch names its condition
        ln = struct.unpack("<i", want[o:o + 4])[0] + 4
        assert got[o:o + ln] == want[o:o + ln], name
        o += ln
    assert got == want
    # skip counts: of 0 and of more than 0, kept and filtered separately
    for sk, sf in ((3, 0), (0, 2), (5, 3), (32, 8), (40, 40)):
        (w, nw), _, _ = expected(cs, bodies, 1, 29000, sk, sf)
        g, ng = ch.tag_records(haps, ps, sk, sf)
        assert (ng, g) == (nw, w), (sk, sf)
    ch.close()


def test_a_region_in_the_middle_of_the_file(lcd, bam):
    """the iterator's overlap rule: records that end in front of the region are not in the table, the walk stops at the region's end"""
    path, cs, bodies = bam
    ch = lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, 3001, 6000, min_mapq=MIN_MAPQ)
    (want, n_want), haps, ps = expected(cs, bodies, 3001, 6000)
    assert 0 < n_want < 40 and ch.n == len(haps)
    got, n_got = ch.tag_records(haps, ps)
    assert (n_got, got) == (n_want, want)
    ch.close()


def test_a_chunk_from_host_arrays_is_refused(lcd):
    q = np.full(100, 30, np.uint8)
    ch = lcd.DeviceChunk([10], [np.array([(100 << 4) | 7], np.uint32)], [q], [np.full(50, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="not made from a BAM"):
        ch.tag_records([0], [0])
    ch.close()
