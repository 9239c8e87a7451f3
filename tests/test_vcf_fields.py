"""VCF content without a device: the TE library read from a FASTA file (lcd_te_lib_from_fasta) against the kseq-equivalent Python reader and the oracle's k-mer
check; the formatter with supporting read names (lcd_format_vcf_fields) against the oracle's formatter plus the Python ALTREADS rule of tests/vcf_fields_common.py;
the planted mobile-element insertions, proven from the oracles' output alone; the command line; the new symbols and struct layouts; the file-level entry point
called from plain C with a NULL and with a zeroed options struct."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import call_chunks_common as kc
import call_file_common as fc
import emit_common as ec
import vcf_fields_common as vf
from conftest import ROOT

NEW = ["lcd_te_lib_from_fasta", "lcd_te_lib_from_fasta_free", "lcd_format_vcf_fields", "lcd_alt_read_names", "lcd_vcf_fields_out_free", "lcd_chunks_call_fields",
       "lcd_call_bam_regions", "lcd_call_files"]


# ---------------- the TE file reader ----------------
def _seqs(seed=5):
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) for n in (300, 64, 517)]


def _fasta(seqs, width=60, eol=b"\n", lower=False, headers=None, last_eol=True):
    out = b""
    for i, s in enumerate(seqs):
        s = s.lower() if lower else s
        out += b">" + (headers[i] if headers else b"te%d" % i) + eol
        out += b"".join(s[k:k + width] + eol for k in range(0, len(s), width))
    return out if last_eol else out[:len(out) - len(eol)]


S = _seqs()
FILES = {
    "multi_line": _fasta(S),
    "one_line_each": _fasta(S, width=10000),
    "lower_case": _fasta(S, lower=True),
    "mixed_case": _fasta([S[0][:100].lower() + S[0][100:], S[1]]),
    "description": _fasta(S, headers=[b"AluY family=SINE len=300", b"L1HS\tLINE", b"SVA_F  x  y"]),
    "crlf": _fasta(S, eol=b"\r\n", headers=[b"a desc", b"b", b"c\tx"]),
    "no_final_newline": _fasta(S, last_eol=False),
    "empty_file": b"",
    "no_record": b"just text\nwithout a header\n",
    "empty_sequence": b">first\n" + S[0] + b"\n>hollow\n>third\n" + S[1] + b"\n>last_hollow\n",
    "empty_sequence_crlf": b">first\r\n" + S[0] + b"\r\n>hollow\r\n\r\n>third\r\n" + S[1] + b"\r\n",
    "blank_lines": b"\n\n>a\n\n" + S[0][:150] + b"\n\n" + S[0][150:] + b"\n\n>b\n" + S[1] + b"\n\n",
    "junk_in_front": b"# comment\nACGT\n>a\n" + S[0] + b"\n",
    "with_n_and_iupac": b">a\n" + S[0][:120] + b"NNNNNRYK" + S[0][120:] + b"\n",
    "fastq": b"@q1 d\n" + S[1] + b"\n+\n" + b"I" * len(S[1]) + b"\n@q2\n" + S[0] + b"\n+q2\n" + b"#" * len(S[0]) + b"\n",
    "fastq_truncated": b">ok\n" + S[1] + b"\n@bad\n" + S[0] + b"\n+\n" + b"I" * 10 + b"\n",
    "at_sign_starts_a_record": b">a\n" + S[1] + b"\n@b c\n" + S[0] + b"\n",
    "empty_name": b">\n" + S[1] + b"\n> spaced\n" + S[0] + b"\n",
}


def _probes(seqs, rng):
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    out = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 90)])]
    for s in seqs:
        s = s.upper()
        for a in range(0, max(1, len(s) - 60), 45):
            out += [s[a:a + 75], s[a:a + 75].translate(comp)[::-1]]
    return out


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
@pytest.mark.parametrize("case", sorted(FILES))
def test_te_file_reader_equals_the_python_reader(lcd, oracle, tmp_path, case, gz):
    path = str(tmp_path / ("te.fa.gz" if gz else "te.fa"))
    open(path, "wb").write(gzip.compress(FILES[case]) if gz else FILES[case])
    want = vf.read_te_file(path)
    assert want == vf.kseq_records(FILES[case])
    with lcd.te_lib_from_fasta(path) as got:
        assert [n.encode() for n in got.names] == [n for n, _ in want] and got.seq_lens == [len(s) for _, s in want] and got.n == len(want)
        orc = oracle.lib()
        lib = vf.oracle_te_lib(orc, [s for _, s in want])
        rng = np.random.default_rng(1)
        hits = 0
        for p in _probes([s for _, s in want], rng):
            a = got.check(np.frombuffer(p, np.uint8))
            b = vf.oracle_check_te(orc, lib, np.frombuffer(p, np.uint8))
            assert a[0] == b[0] and (a[0] < 0 or a[1] == b[1]), (case, p)
            hits += a[0] >= 0
        orc.lcdo_te_lib_destroy(lib)
    if case in ("multi_line", "lower_case", "description", "crlf"):
        assert [s.upper() for _, s in want] == S and hits >= 20          # the cases the issue names carry the three sequences whole
    if case == "description":
        assert [n for n, _ in want] == [b"AluY", b"L1HS", b"SVA_F"]
    if case == "crlf":
        assert [n for n, _ in want] == [b"a", b"b", b"c"]
    if case in ("empty_file", "no_record"):
        assert want == [] and hits == 0
    if case == "empty_sequence":
        assert [(n, len(s)) for n, s in want] == [(b"first", 300), (b"hollow", 0), (b"third", 64), (b"last_hollow", 0)]
    if case == "empty_sequence_crlf":                                     # kseq keeps the lone '\r' of a sequence of one byte (its rule needs more than one)
        assert [(n, s if len(s) < 2 else len(s)) for n, s in want] == [(b"first", 300), (b"hollow", b"\r"), (b"third", 64)]
    if case == "fastq":
        assert [(n, len(s)) for n, s in want] == [(b"q1", 64), (b"q2", 300)]
    if case == "fastq_truncated":
        assert [n for n, _ in want] == [b"ok"]


def test_an_empty_sequence_keeps_its_index_and_never_matches(lcd, tmp_path):
    path = str(tmp_path / "te.fa")
    open(path, "wb").write(b">hollow\n>real\n" + S[0] + b"\n")
    with lcd.te_lib_from_fasta(path) as lib:
        assert lib.names == ["hollow", "real"] and lib.seq_lens == [0, 300]
        assert lib.check(np.frombuffer(S[0][20:140], np.uint8)) == (1, 0)
        assert lib.check(np.frombuffer(S[2][:120], np.uint8))[0] == -1


def test_a_missing_te_file_is_an_error_with_its_path(lcd, tmp_path):
    path = str(tmp_path / "absent" / "te.fa")
    with pytest.raises(lcd.LcdError, match=re.escape(path)) as e:
        lcd.te_lib_from_fasta(path)
    assert "-30" in str(e.value)
    lib = lcd.load_library()
    assert lib.lcd_te_lib_from_fasta(None, 0, None, None, None, None) == -4
    h, names, n = C.c_void_p(), C.POINTER(C.c_char_p)(), C.c_int()
    good = str(tmp_path / "t.fa"); open(good, "wb").write(FILES["multi_line"])
    assert lib.lcd_te_lib_from_fasta(good.encode(), 16, C.byref(h), C.byref(names), None, C.byref(n)) == -4 and not h
    assert lib.lcd_te_lib_from_fasta(good.encode(), 0, C.byref(h), C.byref(names), None, C.byref(n)) == 0 and n.value == 3     # seq_lens may be NULL; 0 = 15
    lib.lcd_te_lib_from_fasta_free(h, names, None, n.value)


# ---------------- the formatter with read names ----------------
def rec(pos, ref, alts, GT, PS, DP, AD, alt_reads, type_=8, is_sv=0, is_clean=1, QUAL=60, GQ=50):
    return dict(pos=pos, PS=PS, type=type_, ref_len=len(ref), n_alt=len(alts), alt_len=[len(a) for a in alts], ref=bytes(ref), alt=[bytes(a) for a in alts], GT=list(GT), DP=DP,
                AD=list(AD), QUAL=QUAL, GQ=GQ, is_sv=is_sv, is_clean=is_clean, alt_reads=list(alt_reads), cand_i=0)


def prod_format(lcd, opt, recs, te_names, mode, names, n_reads=None, chrom=b"chr7"):
    """lcd_format_vcf_fields -> (return code, text or None, MEI lines)"""
    lib = lcd.load_library()
    keep = []
    arr = vf.var1_array(recs, keep)
    off = np.zeros(len(names) + 1, np.uint64); pool = bytearray()
    for i, x in enumerate(names):
        off[i] = len(pool); pool += x + b"\0"
    tn = (C.c_char_p * max(1, len(te_names)))(*te_names) if te_names is not None else None
    text, mei = C.c_void_p(), C.c_int(-1)
    fn = lib.lcd_format_vcf_fields
    rc = fn(C.cast(C.pointer(opt), fn.argtypes[0]), chrom, C.cast(arr, fn.argtypes[2]), len(recs), tn, mode, len(names) if n_reads is None else n_reads,
            off.ctypes.data_as(C.POINTER(C.c_uint64)), bytes(pool) + b"\0", C.byref(text), C.byref(mei))
    out = C.string_at(text) if text else None
    if text:
        ec._libc.free(text)
    return rc, out, mei.value


def oracle_format(orc, opt, recs, te_names, mode, names, chrom=b"chr7"):
    keep = []
    arr = vf.var1_array(recs, keep)
    return b"".join(vf.add_altreads(l, r, mode, names) for l, r in zip(vf.oracle_lines(orc, opt, chrom, arr, len(recs), te_names), recs) if l is not None)


NAMES = [b"r", b"m64012_190920_173625/1/ccs", b"n" * 250, b"x/1", b"q"] + [b"read_%03d" % i for i in range(5, 40)]
HAND = dict(
    het_snp_ps=rec(100, [0], [[2]], (0, 1), 100, 12, (6, 6, 0), [3, 0, 7, 9, 1, 2]),
    hom_sv=rec(2000, [1], [[1] + [0, 1, 2, 3] * 10], (1, 1), 1900, 9, (0, 9, 0), [8, 7, 6, 5, 4, 3, 2, 1, 0], type_=1, is_sv=1, is_clean=0),
    unphased=rec(2500, [3], [[0]], (1, 0), 0, 8, (4, 4, 0), [10, 12, 14, 16]),
    het_del_sv_ps=rec(3000, [2] + [1] * 40, [[2]], (1, 0), 100, 10, (5, 5, 0), [2, 39, 0, 20, 11], type_=2, is_sv=1, is_clean=0),
    two_alt=rec(4000, [0, 1], [[0], [0, 1, 1]], (1, 2), 100, 14, (1, 6, 7), [5, 6, 7, 8, 9, 10], type_=1),
    one_long_name=rec(5000, [1], [[3]], (0, 1), 4900, 6, (3, 3, 0), [2, 0, 2]),
)


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle.lib()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_formatter_equals_the_python_oracle_on_hand_built_records(lcd, orc, mode):
    opt = ec.default_call_opt()
    recs = list(HAND.values())
    rc, got, _ = prod_format(lcd, opt, recs, None, mode, NAMES)
    want = oracle_format(orc, opt, recs, None, mode, NAMES)
    assert rc == len(recs) and got == want
    lines = got.decode().splitlines()
    plain = oracle_format(orc, opt, recs, None, 0, NAMES).decode().splitlines()
    for key, line, base in zip(HAND, lines, plain):
        r = HAND[key]
        fmt, sample = line.split("\t")[8:10]
        if mode == 2 or (mode == 1 and r["is_sv"]):
            b = base.split("\t")
            assert line.split("\t")[:8] == b[:8] and fmt == b[8] + ":ALTREADS" and sample.startswith(b[9] + ":"), key
        else:
            assert line == base and "ALTREADS" not in line, key             # mode 1 on a non-SV record: no field at all
    if mode == 2:
        col = {k: l.split("\t") for k, l in zip(HAND, lines)}
        assert col["het_snp_ps"][8] == "GT:DP:AD:VAF:GQ:PS:ALTREADS" and col["het_snp_ps"][9] == "0|1:12:6,6:0.500:50:100:x/1,r,read_007,read_009,m64012_190920_173625/1/ccs," + "n" * 250
        assert col["hom_sv"][8] == "GT:DP:AD:VAF:GQ:ALTREADS" and col["hom_sv"][9].endswith(":50:read_008,read_007,read_006,read_005,q,x/1," + "n" * 250 + ",m64012_190920_173625/1/ccs,r")
        assert col["unphased"][8] == "GT:DP:AD:VAF:GQ:ALTREADS" and col["unphased"][9].startswith("0/1:")
        assert col["two_alt"][9].endswith(":100:read_005,read_006,read_007,read_008,read_009,read_010") and ":1,6,7:" in col["two_alt"][9]    # allele 1's reads only
        assert col["one_long_name"][9].endswith(":" + "n" * 250 + ",r," + "n" * 250)
    assert prod_format(lcd, opt, recs, None, 0, [], n_reads=0)[1] == plain_text(lcd, opt, recs)      # mode 0 needs no names and is lcd_format_vcf_te


def plain_text(lcd, opt, recs, te_names=None, chrom=b"chr7"):
    lib = lcd.load_library()
    keep = []
    arr = vf.var1_array(recs, keep)
    tn = (C.c_char_p * max(1, len(te_names)))(*te_names) if te_names is not None else None
    t = C.c_void_p()
    lib.lcd_format_vcf_te.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    assert lib.lcd_format_vcf_te(C.byref(opt), chrom, arr, len(recs), tn, C.byref(t)) >= 0
    out = C.string_at(t); ec._libc.free(t)
    return out


def test_a_record_without_alt_reads_gets_a_dot(lcd, orc):
    opt = ec.default_call_opt(); opt.min_alt_dp = 0                       # (-d 0: write_var_to_vcf's AD[1] filter lets the record through)
    recs = [rec(700, [1], [[2]], (0, 1), 700, 9, (9, 0, 0), []), rec(900, [1], [[2] * 41], (1, 1), 0, 9, (9, 0, 0), [], type_=1, is_sv=1, is_clean=0)]
    for mode in (1, 2):
        rc, got, _ = prod_format(lcd, opt, recs, None, mode, NAMES)
        assert rc == 2 and got == oracle_format(orc, opt, recs, None, mode, NAMES)
        a, b = got.decode().splitlines()
        assert b.endswith(":ALTREADS\t1/1:9:9,0:0.000:50:.") and a.endswith(":700:." if mode == 2 else ":700")
    opt.min_alt_dp = 2
    assert prod_format(lcd, opt, recs, None, 2, NAMES)[:2] == (0, b"")


def test_mei_keys_and_read_names_together(lcd, orc):
    opt = ec.default_call_opt()
    r = dict(HAND["hom_sv"])
    keep = []
    recs = [HAND["het_snp_ps"], r]
    arr = vf.var1_array(recs, keep)
    tsd = np.array([0, 1, 2, 3, 3], np.uint8); keep.append(tsd)
    arr[1].tsd_len, arr[1].polya_len, arr[1].te_seq_i, arr[1].te_is_rev, arr[1].tsd_pos1 = 5, -14, 2, 1, 2001
    arr[1].tsd_seq = tsd.ctypes.data_as(ec.u8p)
    te_names = [b"AluY", b"L1HS", b"SVA_F"]
    want = b"".join(vf.add_altreads(l, x, 1, NAMES) for l, x in zip(vf.oracle_lines(orc, opt, b"chr7", arr, 2, te_names), recs))
    lib = lcd.load_library()
    off = np.zeros(len(NAMES) + 1, np.uint64); pool = bytearray()
    for i, x in enumerate(NAMES):
        off[i] = len(pool); pool += x + b"\0"
    tn = (C.c_char_p * 3)(*te_names)
    text, mei = C.c_void_p(), C.c_int(-1)
    fn = lib.lcd_format_vcf_fields
    rc = fn(C.cast(C.pointer(opt), fn.argtypes[0]), b"chr7", C.cast(arr, fn.argtypes[2]), 2, tn, 1, len(NAMES), off.ctypes.data_as(C.POINTER(C.c_uint64)), bytes(pool), C.byref(text),
            C.byref(mei))
    got = C.string_at(text); ec._libc.free(text)
    assert rc == 2 and got == want and mei.value == 1
    assert b"\tMEI;END=2000;SVTYPE=INS;SVLEN=40;TSD=ACGTT;TSDLEN=5;POLYALEN=-14;TSDPOS1=2001;REPNAME=-SVA_F\tGT:DP:AD:VAF:GQ:ALTREADS\t" in got


def test_a_line_of_more_than_64_kb(lcd, orc):
    """the reference grows its line buffer for the names (src/vcf_utils.c:236-242); here nothing is fixed in size"""
    names = [(b"movie%05d/" % i) + b"z" * 190 + b"/ccs" for i in range(400)]
    opt = ec.default_call_opt()
    recs = [rec(10, [0], [[1]], (1, 1), 0, 400, (0, 400, 0), list(range(399, -1, -1))), HAND["unphased"]]
    rc, got, _ = prod_format(lcd, opt, recs, None, 2, names)
    assert rc == 2 and got == oracle_format(orc, opt, recs, None, 2, names)
    first = got.split(b"\n")[0]
    assert len(first) > 65536 and first.endswith(names[1] + b"," + names[0]) and first.count(b",") == 399 + 1


@pytest.mark.parametrize("bad", ["past_the_end", "negative", "more_than_stored", "in_a_later_record"])
def test_an_index_outside_the_chunks_reads_is_an_error(lcd, bad):
    opt = ec.default_call_opt()
    recs = [dict(HAND["het_snp_ps"]), dict(HAND["unphased"])]
    n_reads = len(NAMES)
    if bad == "past_the_end":
        recs[0]["alt_reads"] = [3, 0, n_reads, 9, 1, 2]
    elif bad == "negative":
        recs[0]["alt_reads"] = [3, 0, -1, 9, 1, 2]
    elif bad == "more_than_stored":
        recs[0]["alt_reads"] = [3, 0]                                     # AD[1] = 6 with two stored indices
    else:
        recs[1]["alt_reads"] = [10, 12, 14, 1 << 30]
    rc, text, _ = prod_format(lcd, opt, recs, None, 2, NAMES)
    assert rc == -4 and text is None
    assert "outside" in lcd.load_library().lcd_last_error().decode()
    assert prod_format(lcd, opt, recs, None, 0, NAMES)[0] == 2            # without names the indices are not read
    if bad == "in_a_later_record":
        assert prod_format(lcd, opt, recs, None, 1, NAMES)[0] == 2        # ... nor for a record the mode leaves out
    assert prod_format(lcd, opt, recs, None, 3, NAMES)[0] == -4 and prod_format(lcd, opt, recs, None, -1, NAMES)[0] == -4


# ---------------- the planted insertions, from the oracles alone ----------------
TE_NAMES = [b"TE0", b"TE1", b"TE2"]


@pytest.fixture(scope="module")
def planted(lcd, oracle):
    """the seeded contig cut into the two 6 kb chunks of the GPU tests, through the oracles end to end; then lcdo_annotate_te with the library and the formatter"""
    ch = vf.make_mei_chunk()
    chs = kc.split_chunk(ch, [6000])
    w = kc.oracle_call(lcd, oracle, chs, max_len=kc.TWO_CHUNK_MAX_LEN)
    opt = ec.default_call_opt()
    out, at = [], 0
    for c, f in zip(chs, w["chunks"]):
        recs = w["records"][at:at + f["n_records"]]; at += f["n_records"]
        names = [b"chr1_r%d" % i for i in range(len(c["reads"]))]
        text, ann = vf.expected_text(oracle.lib(), opt, b"chr1", recs, ch["ref"], 1, ch["te_seqs"], TE_NAMES, 2, names)
        none_text, none_ann = vf.expected_text(oracle.lib(), opt, b"chr1", recs, ch["ref"], 1, None, None, 0, names)
        out.append(dict(recs=recs, text=text, ann=ann, none_text=none_text, none_ann=none_ann))
    return ch, out


def _line_of(text, pos):
    hit = [l for l in text.decode().splitlines() if l.split("\t")[1] == str(pos)]
    assert len(hit) == 1
    return hit[0]


def test_the_planted_insertions_reach_their_conditions(planted):
    ch, out = planted
    for x, chunk in zip(ch["planted"], (0, 1, 1)):
        o = out[chunk]
        r = vf.planted_record(o["recs"], x)
        assert r is not None and not r["is_clean"] and r["GT"][0] != r["GT"][1], x["kind"]       # a het SV from a noisy region
        a = o["ann"][o["recs"].index(r)]
        line = _line_of(o["text"], r["pos"])
        assert len(a["tsd"]) >= vf.TSD_LEN and a["tsd"][:vf.TSD_LEN] == bytes(ch["ref"][x["p"]:x["p"] + vf.TSD_LEN]) and a["tsd_pos1"] == r["pos"] + 1 and ";TSD=" in line
        if x["kind"] == "forward":
            assert (a["te_seq_i"], a["te_is_rev"]) == (1, 0) and a["polya_len"] >= 10 and "\tMEI;" in line and ";REPNAME=+TE1\t" in line
        elif x["kind"] == "reverse":
            assert (a["te_seq_i"], a["te_is_rev"]) == (2, 1) and a["polya_len"] <= -10 and "\tMEI;" in line and ";REPNAME=-TE2\t" in line and ";POLYALEN=-" in line
        else:
            assert a["te_seq_i"] == -1 and a["polya_len"] >= 10 and "MEI" not in line and "REPNAME" not in line
        # without a library the duplication is still reported, the element is not
        assert o["none_ann"][o["recs"].index(r)]["te_seq_i"] == -1 and ";TSD=" in _line_of(o["none_text"], r["pos"]) and "MEI" not in _line_of(o["none_text"], r["pos"])
    for o in out:                                                                               # both chunks give lines with two or more names
        assert any(l.split("\t")[9].split(":")[-1].count(",") >= 1 for l in o["text"].decode().splitlines())
        assert sum(1 for r in o["recs"] if r["is_sv"]) >= 1 and sum(1 for r in o["recs"] if not r["is_sv"]) >= 3


def test_the_generator_plants_what_the_issue_describes():
    ch = vf.make_mei_chunk()
    tes = ch["te_seqs"]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    assert len(tes) == 3 and all(280 <= len(t) <= 320 for t in tes)
    for x in ch["planted"]:
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[np.array(x["seq"], np.uint8)])
        assert len(s) == 232 and x["seq"][:12] == ch["ref"][x["p"]:x["p"] + 12].tolist() and ch["ref"][x["p"] - 1] != x["seq"][-1]
        if x["kind"] == "forward":
            assert s[12:212] in tes[1] and s[212:] == b"A" * 20
        elif x["kind"] == "reverse":
            assert s[12:32] == b"T" * 20 and s[32:].translate(comp)[::-1] in tes[2]
        else:
            assert s[212:] == b"A" * 20 and all(s[12:212] not in t for t in tes)
    carriers = [r for r in ch["reads"] if r["hap"] == 1]
    assert 10 <= len(carriers) < len(ch["reads"])


# ---------------- the command line ----------------
def test_cli_accepts_the_three_options_and_hands_them_to_the_job(lcd, monkeypatch, capsys):
    from longcalld_amd import cli
    seen = []
    stats = dict(plan_fallback=0, n_planned=2, n_windows=1, n_reads=7, n_vcf_lines=5, ms_wall=12.0)

    def fake_file(bam, fa, **kw):
        seen.append(("file", bam, fa, kw))
        return dict(stats, **({"n_mei_lines": 3, "te_names": ["a"]} if kw.get("te_fasta") else {}))

    def fake_files(bams, fa, **kw):
        seen.append(("files", list(bams), fa, kw))
        return dict(stats, n_reads_per_file=[3, 4])
    monkeypatch.setattr(lcd, "call_file", fake_file)
    monkeypatch.setattr(lcd, "call_files", fake_files)
    for argv, te, rn in ((["--te-lib", "te.fa"], "te.fa", None), (["--te-lib", "x.fa.gz", "--sv-rnames"], "x.fa.gz", "sv"), (["--te-lib=y.fa"], "y.fa", None),
                         (["--var-rnames"], None, "all"), (["--sv-rnames", "--var-rnames"], None, "all"), (["--var-rnames", "--sv-rnames", "--te-lib=z.fa"], "z.fa", "all"),
                         ([], None, None)):
        seen.clear()
        assert cli.main(["call"] + argv + ["ref.fa", "in.bam"]) == 0
        kind, bam, fa, kw = seen[0]
        assert (kind, bam, fa) == ("file", "in.bam", "ref.fa") and kw["te_fasta"] == te and kw["rnames"] == rn
        err = capsys.readouterr().err
        assert ("3 MEI records" in err) == (te is not None) and "5 VCF lines" in err
    seen.clear()
    assert cli.main(["call", "--te-lib", "te.fa", "--sv-rnames", "--add-bam", "b.bam", "ref.fa", "in.bam"]) == 0
    assert seen[0][0] == "files" and seen[0][1] == ["in.bam", "b.bam"] and seen[0][3]["te_fasta"] == "te.fa" and seen[0][3]["rnames"] == "sv"


def _cli(*args):
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def test_cli_refusals_that_stay():
    r = _cli("call", "--out-som-var-rnames", "ref.fa", "in.bam")
    assert r.returncode == 2 and r.stdout == "" and len(r.stderr.strip().splitlines()) == 1 and "somatic" in r.stderr and "not supported" in r.stderr
    for args in (["--te-lib"], ["ref.fa", "in.bam", "--te-lib"]):
        r = _cli("call", *args)
        assert r.returncode == 2 and "needs a value" in r.stderr, args
    assert _cli("call", "-T").returncode == 2
    # the reference's own spellings keep their refusal (tests/test_call_file_abi.py pins it) and name the spelling that works, as -X / -L do
    for args, new in ((["-T", "te.fa"], "--te-lib FILE"), (["--trans-elem=te.fa"], "--te-lib FILE"), (["--out-var-rnames"], "--var-rnames"), (["--out-sv-rnames"], "--sv-rnames")):
        r = _cli("call", *args, "ref.fa", "in.bam")
        assert r.returncode == 2 and r.stdout == "" and len(r.stderr.strip().splitlines()) == 1 and "not supported" in r.stderr and new in r.stderr, args
    r = _cli("call", "--help")
    assert r.returncode == 0 and "--te-lib FILE" in r.stdout and "--var-rnames" in r.stdout and "--sv-rnames" in r.stdout
    assert "--out-som-var-rnames" in r.stdout.split("Not supported")[1] and "-T (use --te-lib)" in r.stdout.split("Not supported")[1]


def test_python_keywords_are_checked(lcd):
    with pytest.raises(ValueError, match="rnames"):
        lcd.call_file("in.bam", "ref.fa", rnames="som")
    for f in (lcd.chunks_call, lcd.call_chunks, lcd.call_bam_regions, lcd.call_file, lcd.call_files, lcd.te_lib_from_fasta):
        assert callable(f)
    import inspect
    for f in (lcd.chunks_call, lcd.call_bam_regions, lcd.call_file):
        assert {"te_fasta", "rnames"} <= set(inspect.signature(f).parameters)


# ---------------- ABI ----------------
def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def _abi_exe(tmp_path):
    exe = str(tmp_path / "vcf_fields_abi")
    libdir = os.path.join(ROOT, "longcalld_amd")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "vcf_fields_abi.c"), "-L", libdir, "-llcd_hotpath",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    from longcalld_amd import _lib
    want = dict(l.split() for l in subprocess.check_output([_abi_exe(tmp_path)], text=True).splitlines())
    for name, cls in {"lcd_vcf_fields_t": _lib.LcdVcfFields, "lcd_vcf_fields_out_t": _lib.LcdVcfFieldsOut, "lcd_run_opt_t": _lib.LcdRunOpt, "lcd_run_out_t": _lib.LcdRunOut,
                      "lcd_writer_opt_t": _lib.LcdWriterOpt}.items():
        assert C.sizeof(cls) == int(want[name]), name
        fields = [k.split(".")[1] for k in want if k.startswith(name + ".")]
        assert fields == [f[0] for f in cls._fields_], name
        for f in fields:
            assert getattr(cls, f).offset == int(want[f"{name}.{f}"]), (name, f)
    assert (_lib.LCD_RNAMES_NONE, _lib.LCD_RNAMES_SV, _lib.LCD_RNAMES_ALL) == tuple(int(want[k]) for k in ("LCD_RNAMES_NONE", "LCD_RNAMES_SV", "LCD_RNAMES_ALL"))


def _abi_runs(out):
    return {l.split(" ", 1)[0]: re.match(r"\S+ rc (-?\d+) lines (-?\d+) mei (-?\d+) err ?(.*)", l).groups() for l in out.splitlines()}


def test_file_entry_point_from_c_with_null_and_zeroed_options(tmp_path):
    """no device here: the runs end at the first input check that fails -- the same one, with the same message, whether the options struct is absent, NULL or zeroed;
    an unreadable TE file is reported with its path before any output file exists"""
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    fc.write_multi_bam(bam, [("chr1", 100, [])])
    fc.write_multi_fasta(fa, [("chr1", np.zeros(100, np.uint8))])
    os.remove(fa + ".fai")
    exe = _abi_exe(tmp_path)
    te = str(tmp_path / "no_such_te.fa")
    runs = _abi_runs(subprocess.check_output([exe, bam, fa, str(tmp_path / "o"), te], text=True))
    assert runs["plain"][0] == runs["null"][0] == runs["zero"][0] == "-30" and runs["plain"][3] == runs["null"][3] == runs["zero"][3] and fa + ".fai" in runs["plain"][3]
    assert runs["te"][0] == "-30" and te in runs["te"][3]
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]                 # no output file was created by any of them


def test_driver_argument_errors(lcd, tmp_path):
    from longcalld_amd import _lib
    lib = lcd.load_library()
    cfg = lcd.call_cfg()
    recs, n, text = C.POINTER(_lib.LcdVar1)(), C.c_int(0), C.c_void_p()
    fo = _lib.LcdVcfFieldsOut()
    for f in (_lib.LcdVcfFields(None, 0, 3), _lib.LcdVcfFields(None, 0, -1), _lib.LcdVcfFields(None, 16, 0), _lib.LcdVcfFields(str(tmp_path / "none.fa").encode(), 0, 0)):
        rc = lib.lcd_chunks_call_fields(0, None, C.byref(cfg), b"chr1", C.byref(f), C.byref(recs), C.byref(n), C.byref(text), C.byref(fo))
        assert rc == (-30 if f.te_fasta_path else -4) and not text and fo.n_te_seqs == 0
    assert "none.fa" in lib.lcd_last_error().decode()
    lib.lcd_vcf_fields_out_free(C.byref(fo)); lib.lcd_vcf_fields_out_free(None)
    vf = _lib.LcdVcfFields(); fo2 = _lib.LcdVcfFieldsOut(); fo2.n_te_seqs = 7
    ro, out = _lib.LcdRunOpt(fields=C.pointer(vf)), _lib.LcdRunOut(fields_out=C.pointer(fo2))
    inp = _lib.LcdInputs()
    assert lib.lcd_call_files(C.byref(inp), None, None, C.byref(ro), None, C.byref(out)) == -4 and fo2.n_te_seqs == 0
    fo2.n_te_seqs = 7
    assert lib.lcd_call_files(None, None, None, C.byref(ro), None, C.byref(out)) == -4 and fo2.n_te_seqs == 0
