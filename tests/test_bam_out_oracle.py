"""The oracle of the phased alignment output (tests/bam_out_common.py) against a case table written by hand: each row is a record's auxiliary block, whether the
loader kept the record, a hap and a ps, and the expected auxiliary bytes spelled out; the named conditions the GPU test relies on are asserted from the oracle's
own trace.  Then the region rules: which records a region's iterator yields and the skip counts at a cut."""
import struct

import numpy as np

import bam_out_common as bo
from bam_src_common import record

HP = lambda v: b"HPi" + struct.pack("<I", v)
PS = lambda v: b"PSi" + struct.pack("<I", v)
BIG = 3000000000            # 0xb2d05e00

#   name, auxiliary block, kept, hap, ps, expected auxiliary block, trace entries that must appear
CASES = [
    ("no_aux_nothing_wanted",     b"",                                   1, 0, 0,    b"",                                  ["HP:unwanted_absent", "PS:unwanted_absent"]),
    ("no_aux_both_appended",      b"",                                   1, 2, 1000, b"HPi\x02\0\0\0PSi\xe8\x03\0\0",       ["HP:appended_absent", "PS:appended_absent"]),
    ("HP_C_equal_stays_C",        b"HPC\x01",                            1, 1, 0,    b"HPC\x01",                           ["HP:kept_in_place:C"]),
    ("HP_i_equal",                b"HPi\x02\0\0\0",                      1, 2, 0,    b"HPi\x02\0\0\0",                     ["HP:kept_in_place:i"]),
    ("PS_i_equal",                b"PSi\xe8\x03\0\0",                    1, 0, 1000, b"PSi\xe8\x03\0\0",                   ["PS:kept_in_place:i"]),
    ("PS_I_equal_above_2^31",     b"PSI\x00\x5e\xd0\xb2",                1, 0, BIG,  b"PSI\x00\x5e\xd0\xb2",               ["PS:kept_in_place:I"]),
    ("PS_i_is_negative_for_big",  b"PSi\x00\x5e\xd0\xb2",                1, 0, BIG,  b"PSi\x00\x5e\xd0\xb2",               ["PS:replaced:i"]),   # deleted, appended: the same bytes
    ("HP_C_different",            b"HPC\x01NMC\x05",                     1, 2, 0,    b"NMC\x05HPi\x02\0\0\0",               ["HP:replaced:C"]),
    ("HP_Z_is_0",                 b"HPZ1\0",                             1, 1, 0,    b"HPi\x01\0\0\0",                     ["HP:replaced:Z"]),
    ("HP_f_is_0",                 b"HPf\0\0\x80\x3f",                    1, 1, 0,    b"HPi\x01\0\0\0",                     ["HP:replaced:f"]),
    ("PS_s_negative",             b"PSs\xff\xff",                        1, 0, 5,    b"PSi\x05\0\0\0",                     ["PS:replaced:s"]),
    ("both_replaced_HP_then_PS",  b"PSi\x01\0\0\0XAAqHPi\x01\0\0\0",     1, 2, 7,    b"XAAqHPi\x02\0\0\0PSi\x07\0\0\0",     ["HP:replaced:i", "PS:replaced:i"]),
    ("HP_kept_PS_replaced",       b"HPC\x02PSC\x09RGZa\0",               1, 2, 300,  b"HPC\x02RGZa\0PSi\x2c\x01\0\0",       ["HP:kept_in_place:C", "PS:replaced:C"]),
    ("hap_0_deletes_HP",          b"XAAqHPC\x01",                        1, 0, 0,    b"XAAq",                              ["HP:unwanted_deleted:C"]),
    ("ps_0_deletes_PS",           b"PSi\x07\0\0\0",                      1, 0, 0,    b"",                                  ["PS:unwanted_deleted:i"]),
    ("ps_minus_1_deletes_PS",     b"PSi\x07\0\0\0XAAq",                  1, 1, -1,   b"XAAqHPi\x01\0\0\0",                 ["PS:unwanted_deleted:i"]),
    ("two_HP_first_replaced",     b"HPC\x01HPC\x02",                     1, 2, 0,    b"HPC\x02HPi\x02\0\0\0",               ["HP:replaced:C"]),
    ("two_HP_first_equal",        b"HPC\x01HPC\x02",                     1, 1, 0,    b"HPC\x01HPC\x02",                    ["HP:kept_in_place:C"]),
    ("two_HP_first_deleted",      b"HPC\x01HPC\x02",                     1, 0, 0,    b"HPC\x02",                           ["HP:unwanted_deleted:C"]),
    ("HPi_inside_a_B_array",      b"XBBC\x03\0\0\0HPi",                  1, 1, 0,    b"XBBC\x03\0\0\0HPiHPi\x01\0\0\0",     ["HP:appended_absent"]),
    ("HPi_inside_a_Z_value",      b"XZZHPi\x01\0",                       1, 0, 0,    b"XZZHPi\x01\0",                      ["HP:unwanted_absent"]),
    ("B_array_past_the_record",   b"XBBi\xe8\x03\0\0\x01\0\0\0HPC\x01",  1, 1, 0,    b"XBBi\xe8\x03\0\0\x01\0\0\0HPC\x01HPi\x01\0\0\0", ["HP:appended_absent"]),
    ("Z_without_NUL",             b"XZZabcHPC\x01",                      1, 0, 0,    b"XZZabcHPC\x01",                     ["HP:unwanted_absent"]),
    ("ps_above_2^32_low_bits",    b"",                                   1, 0, (1 << 32) + 5, b"PSi\x05\0\0\0",            ["PS:appended_absent"]),
    ("filtered_with_tags",        b"HPC\x01XAAqPSi\x07\0\0\0PSC\x01",    0, 2, 9,    b"XAAqPSC\x01",                       ["HP:filtered_deleted", "PS:filtered_deleted"]),
    ("filtered_without_tags",     b"XAAq",                               0, 1, 1,    b"XAAq",                              ["HP:filtered_absent", "PS:filtered_absent"]),
]

NAMED = ["HP:kept_in_place:C", "HP:kept_in_place:i", "PS:kept_in_place:i", "PS:kept_in_place:I", "HP:replaced:C", "HP:replaced:Z", "HP:replaced:f", "PS:replaced:s",
         "HP:unwanted_deleted:C", "PS:unwanted_deleted:i", "HP:appended_absent", "PS:appended_absent", "HP:filtered_deleted", "PS:filtered_deleted", "HP:filtered_absent"]


def small_read(name=b"q", pos0=100, qlen=4, flag=0):
    return dict(name=name, pos0=pos0, flag=flag, qlen=qlen, bseq=np.full((qlen + 1) // 2, 0x11, np.uint8), qual=np.full(qlen, 30, np.uint8))


def body_of(aux, **kw):
    a = small_read(**{k: v for k, v in kw.items() if k != "mapq"})
    return record(a, [(a["qlen"] << 4) | 7], [(None, None, aux)], mapq=kw.get("mapq", 60))["body"]


def test_case_table_byte_for_byte_and_every_named_condition_reached():
    seen = set()
    for name, aux, kept, hap, ps, want, marks in CASES:
        trace = []
        assert bo.tag_aux(aux, kept, hap, ps, trace) == want, name
        for m in marks:
            assert m in trace, (name, m, trace)
        seen.update(trace)
        body = body_of(aux)
        got = bo.tag_record(body, kept, hap, ps)
        assert got == body[:len(body) - len(aux)] + want, name               # everything in front of the auxiliary block is untouched
    assert not [m for m in NAMED if m not in seen]


def test_aux2i_and_the_fixed_fields():
    assert [bo.aux2i(t, v) for t, v in (("c", b"\xfd"), ("C", b"\xfd"), ("s", b"\xff\xff"), ("S", b"\xff\xff"), ("i", b"\0\x5e\xd0\xb2"), ("I", b"\0\x5e\xd0\xb2"),
                                         ("f", b"\0\0\x80\x3f"), ("Z", b"12"), ("A", b"1"))] == [-3, 253, -1, 65535, BIG - (1 << 32), BIG, 0, 0, 0]
    x = bo.parse(body_of(b"NMC\x01", name=b"abc", pos0=777, qlen=5, flag=16, mapq=7))
    assert (x["pos0"], x["end"], x["flag"], x["mapq"], x["name"]) == (777, 782, 16, 7, b"abc")
    assert bo.parse(body_of(b"", pos0=50, qlen=9, flag=4))["end"] == 51              # the unmapped flag: one base, whatever the CIGAR says


def test_region_records_and_skip_counts_at_a_cut():
    """two regions [1, 1000] and [1001, 2000]: reads that cross the cut are yielded by both iterators; the second region skips exactly those"""
    spec = [(b"a", 10, 50, 0, 60), (b"b", 900, 150, 0, 60), (b"lowq", 950, 100, 0, 3), (b"c", 990, 10, 0, 60), (b"sec", 995, 20, 256, 60), (b"unm", 1000, 30, 4, 0),
            (b"d", 1000, 1, 0, 60), (b"e", 1001, 40, 0, 60), (b"sup", 1500, 10, 2048, 60), (b"f", 1999, 10, 0, 60), (b"g", 2000, 10, 0, 60)]
    bodies = [body_of(b"", name=n, pos0=p, qlen=q, flag=f, mapq=m) for n, p, q, f, m in spec]
    names = lambda recs: [(bo.parse(b)["name"], r) for b, r in recs]
    r1 = bo.region_records(bodies, 1, 1000, 30)
    # `d` starts at 0-based 1000 = 1-based 1001: outside region 1 (pos0 >= reg_end ends the walk); `c` ends at 1000
    assert names(r1) == [(b"a", 0), (b"b", 1), (b"lowq", -1), (b"c", 2), (b"sec", -1)]
    r2 = bo.region_records(bodies, 1001, 2000, 30)
    # `c` (ends at 1-based 1000) does not reach region 2; `unm` spans one base: 1-based 1001
    assert names(r2) == [(b"b", 0), (b"lowq", -1), (b"sec", -1), (b"unm", -1), (b"d", 1), (b"e", 2), (b"sup", -1), (b"f", 3)]
    assert bo.skip_counts(r2, 1, 1000) == (1, 2)                                    # b; lowq and sec
    haps, ps = [1, 2, 0, 1], [500, 500, 0, 1900]
    full, n_full = bo.tagged_stream(r2, haps, ps)
    cut, n_cut = bo.tagged_stream(r2, haps, ps, 1, 2)
    assert (n_full, n_cut) == (8, 5) and full.endswith(cut)
    first = bo.tag_record(r2[0][0], True, 1, 500)
    assert full.startswith(struct.pack("<i", len(first)) + first) and first.endswith(b"HPi\x01\0\0\0PSi\xf4\x01\0\0")
    hdr, split = bo.bam_split(b"BAM\x01" + struct.pack("<i", 3) + b"@x\n" + struct.pack("<i", 0) + cut)
    assert [bo.parse(b)["name"] for b in split] == [b"unm", b"d", b"e", b"sup", b"f"]
    assert bo.header_with_pg(hdr, b"@PG\tID:x") == b"BAM\x01" + struct.pack("<i", 12) + b"@x\n@PG\tID:x\n" + struct.pack("<i", 0)
