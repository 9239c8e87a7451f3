"""The SAM oracle of tests/sam_out_common.py checked against something other than itself (no GPU): the SAM specification's own example lines typed in as
literals, every named condition of the case table proved reached from the oracle's trace, line -> record -> line as the identity, the header rule, and %g."""
import struct

import pytest

import sam_out_common as so

# SAM specification, section 1.1 (the example alignment), tabs for the blanks: the lines of version 1.4 and, where later versions changed r001 / r003, those too
SPEC_LINES = [
    b"r001\t163\tref\t7\t30\t8M2I4M1D3M\t=\t37\t39\tTTAGATAAAGGATACTG\t*\n",
    b"r002\t0\tref\t9\t30\t3S6M1P1I4M\t*\t0\t0\tAAAAGATAAGGATA\t*\n",
    b"r003\t0\tref\t9\t30\t5H6M\t*\t0\t0\tAGCTAA\t*\tNM:i:1\n",
    b"r004\t0\tref\t16\t30\t6M14N5M\t*\t0\t0\tATAGCTTCAGC\t*\n",
    b"r003\t16\tref\t29\t30\t6H5M\t*\t0\t0\tTAGGC\t*\tNM:i:0\n",
    b"r001\t83\tref\t37\t30\t9M\t=\t7\t-39\tCAGCGCCAT\t*\n",
    b"r001\t99\tref\t7\t30\t8M2I4M1D3M\t=\t37\t39\tTTAGATAAAGGATACTG\t*\n",
    b"r003\t0\tref\t9\t30\t5S6M\t*\t0\t0\tGCCTAAGCTAA\t*\tSA:Z:ref,29,-,6H5M,17,0;\n",
    b"r003\t2064\tref\t29\t17\t6H5M\t*\t0\t0\tTAGGC\t*\tSA:Z:ref,9,+,5S6M,30,1;\n",
    b"r001\t147\tref\t37\t30\t9M\t=\t7\t-39\tCAGCGCCAT\t*\n",
]


def _by_hand(name, flag, pos1, mapq, cig, nrefid, pnext1, tlen, seq, fields=()):
    """a record built field by field, independent of parse_line"""
    ops = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6}
    return so.mk(name, pos0=pos1 - 1, flag=flag, qlen=len(seq), cig=[(n << 4) | ops[o] for n, o in cig], fields=list(fields), mapq=mapq, refid=0, nrefid=nrefid, npos=pnext1 - 1,
                 tlen=tlen, nibbles=[so.BASES16.index(b) for b in seq], qual=[0xff] * len(seq))


def test_the_specification_s_example_lines():
    recs = [
        _by_hand(b"r001", 163, 7, 30, [(8, "M"), (2, "I"), (4, "M"), (1, "D"), (3, "M")], 0, 37, 39, "TTAGATAAAGGATACTG"),
        _by_hand(b"r002", 0, 9, 30, [(3, "S"), (6, "M"), (1, "P"), (1, "I"), (4, "M")], -1, 0, 0, "AAAAGATAAGGATA"),
        _by_hand(b"r003", 0, 9, 30, [(5, "H"), (6, "M")], -1, 0, 0, "AGCTAA", [("NM", "C", 1)]),
        _by_hand(b"r004", 0, 16, 30, [(6, "M"), (14, "N"), (5, "M")], -1, 0, 0, "ATAGCTTCAGC"),
        _by_hand(b"r003", 16, 29, 30, [(6, "H"), (5, "M")], -1, 0, 0, "TAGGC", [("NM", "i", 0)]),
        _by_hand(b"r001", 83, 37, 30, [(9, "M")], 0, 7, -39, "CAGCGCCAT"),
        _by_hand(b"r001", 99, 7, 30, [(8, "M"), (2, "I"), (4, "M"), (1, "D"), (3, "M")], 0, 37, 39, "TTAGATAAAGGATACTG"),
        _by_hand(b"r003", 0, 9, 30, [(5, "S"), (6, "M")], -1, 0, 0, "GCCTAAGCTAA", [("SA", "Z", b"ref,29,-,6H5M,17,0;")]),
        _by_hand(b"r003", 2064, 29, 17, [(6, "H"), (5, "M")], -1, 0, 0, "TAGGC", [("SA", "Z", b"ref,9,+,5S6M,30,1;")]),
        _by_hand(b"r001", 147, 37, 30, [(9, "M")], 0, 7, -39, "CAGCGCCAT"),
    ]
    for body, want in zip(recs, SPEC_LINES):
        assert so.sam_line(body, [b"ref"])[0] == want
        assert so.sam_line(so.parse_line(want, [b"ref"]), [b"ref"])[0] == want


def test_auxiliary_types_as_the_specification_writes_them():
    """section 1.5's TYPE column: A printable character, i integer, f float, Z string, H hex string, B array -- typed in, not derived"""
    body = so.mk(b"x", qlen=2, cig=[(2 << 4) | 0], nibbles=[1, 8], qual=[0, 60],
                 fields=[("XA", "A", b"!"), ("Xc", "c", -1), ("XI", "I", 4000000000), ("Xf", "f", 0.5), ("XZ", "Z", b"a b:c"), ("XH", "H", b"1AE301"), ("XB", "B", ("s", [-3, 4])),
                         ("XF", "B", ("f", [1.5, -2.0, 1e10])), ("XE", "B", ("C", []))])
    assert so.sam_line(body, so.NAMES)[0] == (b"x\t0\tchr1\t101\t60\t2M\t*\t0\t0\tAT\t!]\tXA:A:!\tXc:i:-1\tXI:i:4000000000\tXf:f:0.5\tXZ:Z:a b:c\tXH:H:1AE301\tXB:B:s,-3,4\t"
                                              b"XF:B:f,1.5,-2,1e+10\tXE:B:C\n")


def test_percent_g_boundaries():
    """literals from printf("%g") of glibc, typed in"""
    f = lambda x: so.fmt_g(struct.unpack("<I", struct.pack("<f", x))[0])
    assert [f(x) for x in (0.0, -0.0, 1.0, 100000.0, 999999.0, 1000000.0, 0.0001, 0.00001, 0.1, 123456.7, 1234567.0, 0.25, -2.5e-7)] == \
        ["0", "-0", "1", "100000", "999999", "1e+06", "0.0001", "1e-05", "0.1", "123457", "1.23457e+06", "0.25", "-2.5e-07"]
    assert [so.fmt_g(b) for b in (0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x00000001, 0x7f7fffff, 0x497423f8)] == \
        ["inf", "-inf", "nan", "-nan", "nan", "1.4013e-45", "3.40282e+38", "1e+06"]          # 999999.5 is a tie: the even neighbour is 1000000


CONDITIONS = ["qname:empty", "qname:name", "qname:star_does_not_fit", "rname:star_negative", "rname:star_past_table", "rname:name", "rnext:star_negative", "rnext:star_past_table",
              "rnext:equal", "rnext:name", "tlen:negative", "cigar:star", "cigar:op_above_9", "cg:cigar_from_field", "cg:no_field", "cg:field_not_B_I", "layout:bad", "seq:star_empty",
              "qual:star_ff_first", "qual:ff_later_only", "aux:walk_stopped", "aux:A", "aux:c", "aux:C", "aux:s", "aux:S", "aux:i", "aux:I", "aux:f", "aux:Z", "aux:H", "aux:B"] + \
             ["aux:B:%s:%d" % (s, n) for s in "cCsSiIf" for n in (0, 1, 63, 64, 65)]


def test_every_named_condition_is_reached():
    cs = so.cases()
    assert len({name for name, _ in cs}) == len(cs)
    trace = []
    text, st = so.sam_text([b for _, b in cs], so.NAMES, trace)
    for m in CONDITIONS:
        assert m in trace, m
    by = {name: so.sam_line(b, so.NAMES) for name, b in cs}
    # the cases say what their names promise
    assert by["l_seq_0"][0].split(b"\t")[9:11] == [b"*", b"*\n"] and by["l_seq_1"][0].split(b"\t")[9] == b"A"
    for n in (63, 64, 65, 127, 128, 129):
        assert len(by["l_seq_%d" % n][0].split(b"\t")[9]) == n == len(by["l_seq_%d" % n][0].rstrip(b"\n").split(b"\t")[10])
    assert by["all_16_nibbles"][0].split(b"\t")[9] == b"=ACMGRSVTWYHKDBN"
    assert by["odd_len_last_low_nibble_set"][0].split(b"\t")[9] == b"ACGTACG"
    assert by["cigar_digit_steps"][0].split(b"\t")[5] == b"9M10I99D100N999S1000H9999P10000=99999X100000M999999I1000000D9999999N10000000S99999999H100000000P268435455=0X1M"
    assert by["op_above_9"][0].split(b"\t")[5] == b"3?5?1B"
    assert by["CG_cigar"][0].split(b"\t")[5] == b"5S30M2D100000=" and b"CG:B" not in by["CG_cigar"][0] and by["CG_cigar"][0].endswith(b"\tNM:i:1\tXZ:Z:after\n")
    assert by["CG_cigar_empty_array"][0].split(b"\t")[5] == b"*"
    for k in ("CG_miss_three_words", "CG_miss_first_len", "CG_miss_first_op", "CG_miss_second_op", "CG_miss_type_Z", "CG_miss_subtype_i"):
        assert b"\tCG:" in by[k][0] and by[k][1]["cg_cigar"] == 0, k
    assert by["CG_behind_a_stopped_walk"][0].split(b"\t")[5] == b"8S200N" and by["CG_behind_a_stopped_walk"][1]["walk_stopped"] == 1
    assert by["Z_without_NUL"][0].endswith(b"\tXA:A:k\n") and by["B_past_the_record"][0].endswith(b"\tNM:i:3\n") and by["unknown_type"][0].endswith(b"\tOK:Z:yes\n")
    assert by["two_bytes_left"][0].endswith(b"\tOK:i:1\n") and by["two_bytes_left"][1]["walk_stopped"] == 1
    assert by["scalars_min_max"][0].endswith(b"\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295\tYc:i:127\tYC:i:0\tYs:i:32767\tYS:i:0\tYi:i:2147483647"
                                             b"\tYI:i:0\tZi:i:-1\tZs:i:-10\tZc:i:-9\n")
    assert by["refid_minus_1"][0] == b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\t!(/6=DKR\n"
    assert by["tlen_negative"][0].split(b"\t")[3:9] == [b"2147483647", b"60", b"8M", b"=", b"6", b"-2147483648"]
    assert by["rnext_different"][0].split(b"\t")[6:9] == [b"c", b"1", b"-1"] and by["rnext_equal"][0].split(b"\t")[2] == b"chrUn_KI270742v1"
    assert by["refid_past_table"][0].split(b"\t")[2] == b"*" and by["refid_past_table"][0].split(b"\t")[6] == b"*"
    assert by["empty_name"][0].startswith(b"*\t0\t") and len(by["name_254"][0].split(b"\t")[0]) == 254 and by["name_without_NUL"][0].startswith(b"abcdefgZ\t")
    assert by["layout_cut_in_the_qualities"][0] == b"lay\t0\tchr1\t101\t60\t*\t*\t0\t0\t*\t*\n" == by["layout_cut_in_the_cigar"][0] == by["layout_negative_l_seq"][0] == by["layout_l_seq_2^31"][0]
    assert by["layout_cut_in_the_name"][0] == b"*\t0\tchr1\t101\t60\t*\t*\t0\t0\t*\t*\n" == by["layout_fixed_fields_only"][0]
    assert by["scalar_floats"][0].rstrip(b"\n").split(b"\t")[11:18] == [b"f0:f:0", b"f1:f:-0", b"f2:f:inf", b"f3:f:-inf", b"f4:f:nan", b"f5:f:-nan", b"f6:f:1.4013e-45"]
    assert by["B_f"][0].split(b"\t")[11:13] == [b"F0:B:f", b"F1:B:f,0"]
    assert st == dict(n_records=len(cs), bytes_records=sum(4 + len(b) for _, b in cs), bytes_text=len(text), n_float_values=len(so.FLOAT_BITS) + 1 + 63 + 64 + 65, n_cg_cigar=2,
                      n_walk_stopped=5, n_bad_layout=6)


def test_line_to_record_to_line_is_the_identity():
    n = 0
    for name, body in so.cases() + [("big", so.big_record())]:
        line, info = so.sam_line(body, so.NAMES)
        if info["n_float"]:
            continue
        assert so.sam_line(so.parse_line(line, so.NAMES), so.NAMES)[0] == line, name
        n += 1
    assert n == len(so.cases()) + 1 - 2                                   # all but B_f and scalar_floats


def test_the_big_record():
    body = so.big_record()
    line, info = so.sam_line(body, so.NAMES)
    c = line.rstrip(b"\n").split(b"\t")
    assert len(c[9]) == len(c[10]) == 70001 and c[5].count(b"M") + c[5].count(b"I") + c[5].count(b"D") + c[5].count(b"N") + c[5].count(b"S") + c[5].count(b"H") + c[5].count(b"P") + \
        c[5].count(b"=") + c[5].count(b"X") == 40000
    assert c[12].startswith(b"fi:B:C,") and c[12].count(b",") == 70001 and c[13] == b"np:i:17" and info == dict(cg_cigar=0, walk_stopped=0, bad_layout=0, n_float=0)


def _block(text, refs):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for nm, ln in refs:
        out += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    return out


REFS = [(b"chr1", 1000), (b"chrM", 16569)]
SQ = b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrM\tLN:16569\n"


@pytest.mark.parametrize("text, pg, want", [
    (b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrM\tLN:16569\n", None, b"@HD\tVN:1.6\n" + SQ),
    (b"@HD\tVN:1.6\n" + SQ, b"@PG\tID:x", b"@HD\tVN:1.6\n" + SQ + b"@PG\tID:x\n"),
    (b"@HD\tVN:1.6\n" + SQ + b"\0\0\0", b"@PG\tID:x", b"@HD\tVN:1.6\n" + SQ + b"@PG\tID:x\n"),                 # NUL padding: the line goes in front of it, the padding goes
    (b"@HD\tVN:1.6\tSO:coordinate\n", None, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),                                # no @SQ: behind @HD
    (b"@HD\tVN:1.6\tSO:coordinate", b"@PG\tID:x", b"@HD\tVN:1.6\tSO:coordinate\n" + SQ + b"@PG\tID:x\n"),          # no newline at the end of the stored text
    (b"@RG\tID:a\tSM:s\n", None, SQ + b"@RG\tID:a\tSM:s\n"),                                                        # no @HD: at the front
    (b"@CO\t@SQ\tSN:not_a_line\n", None, SQ + b"@CO\t@SQ\tSN:not_a_line\n"),                                       # @SQ inside a line is no @SQ line
    (b"@HDX\tfoo\n", None, SQ + b"@HDX\tfoo\n"),
    (b"", None, SQ),
    (b"", b"@PG\tID:x", SQ + b"@PG\tID:x\n"),
    (b"\0\0", None, SQ),
    (b"@HD\tVN:1.6", None, b"@HD\tVN:1.6\n" + SQ),
])
def test_the_header_rule(text, pg, want):
    assert so.sam_header(_block(text, REFS), pg) == want


def test_a_header_without_contigs_gets_no_sq_lines():
    assert so.sam_header(_block(b"@HD\tVN:1.6\n", []), None) == b"@HD\tVN:1.6\n" and so.sam_header(_block(b"", []), None) == b""
