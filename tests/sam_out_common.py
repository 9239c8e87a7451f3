"""Pure-Python oracle of the SAM text output (lcd_records_to_sam, lcd_tagged_to_sam, lcd_write_phased): one BAM record body -> its SAM line, the header text,
glibc's %g of a float32, a parser from a line back to a record, and the case table the GPU test runs.  Written from the rules of include/lcd_hotpath.h
(lcd_tagged_to_sam) on bam_src_common.aux_walk (the field walk and its stop rule).  sam_line leaves a named entry in `trace` for every decision, so that
tests/test_sam_out_oracle.py can prove from the oracle's own output that each condition of the case table was reached."""
import struct

import numpy as np

import bam_out_common as bo
from bam_src_common import aux_field, record

OPS = "MIDNSHP=XB"
BASES16 = "=ACMGRSVTWYHKDBN"
INT_FMT = dict(c="<b", C="<B", s="<h", S="<H", i="<i", I="<I")


def fmt_g(bits):
    """glibc's printf("%g", (double)x) of the float32 with these bits: Python's %g is correctly rounded on the exact value; the sign of a NaN is glibc's"""
    bits &= 0xffffffff
    sign = "-" if bits >> 31 else ""
    if (bits >> 23) & 0xff == 0xff:
        return sign + ("nan" if bits & 0x7fffff else "inf")
    return "%g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def _cigar_text(words):
    return "".join("%d%s" % (w >> 4, OPS[w & 15] if (w & 15) < 10 else "?") for w in words)


def sam_line(body, names, trace=None):
    """a record body (without its block_size word) + the contigs' names -> (the line as bytes with its newline, info); info: cg_cigar, walk_stopped, bad_layout
    (0 / 1 each) and n_float"""
    tr = trace if trace is not None else []
    refid, pos, lname, mapq, _bin, nc, flag, lseq, nrefid, npos, tlen = struct.unpack("<iiBBHHHiiii", body[:32])
    n = len(body)
    a_cig = 32 + lname; a_seq = a_cig + 4 * nc; a_qual = a_seq + (lseq + 1) // 2; a_aux = a_qual + lseq
    layout_ok = lseq >= 0 and a_aux <= n
    name_ok = 32 + lname <= n
    info = dict(cg_cigar=0, walk_stopped=0, bad_layout=0 if layout_ok else 1, n_float=0)
    nm = [x if isinstance(x, bytes) else x.encode() for x in names]

    def ref_name(r, what):
        if r < 0:
            tr.append(what + ":star_negative"); return b"*"
        if r >= len(nm):
            tr.append(what + ":star_past_table"); return b"*"
        tr.append(what + ":name")
        return nm[r] if nm[r] else b"*"

    if not name_ok:
        tr.append("qname:star_does_not_fit"); qname = b"*"
    else:
        qname = body[32:32 + lname].split(b"\0")[0]
        tr.append("qname:empty" if not qname else "qname:name")
        qname = qname or b"*"
    cols = [qname, b"%d" % flag, ref_name(refid, "rname"), b"%d" % (pos + 1), b"%d" % mapq]
    fields, cg = [], None
    if layout_ok:
        aux = body[a_aux:]
        fields = bo.field_spans(aux)
        if (fields[-1][4] if fields else 0) != len(aux):
            info["walk_stopped"] = 1; tr.append("aux:walk_stopped")
        words = struct.unpack("<%dI" % nc, body[a_cig:a_seq])
        if nc == 2 and words[0] == (((lseq << 4) & 0xffffffff) | 4) and (words[1] & 15) == 3:
            first = next((f for f in fields if f[0] == b"CG"), None)
            if first is None:
                tr.append("cg:no_field")
            elif first[1] != "B" or first[2][:1] != b"I":
                tr.append("cg:field_not_B_I")
            else:
                cg = first; info["cg_cigar"] = 1; tr.append("cg:cigar_from_field")
                words = struct.unpack("<%dI" % ((len(cg[2]) - 5) // 4), cg[2][5:])
        if not words:
            tr.append("cigar:star")
        elif any((w & 15) > 9 for w in words):
            tr.append("cigar:op_above_9")
        cols.append(_cigar_text(words).encode() if words else b"*")
    else:
        tr.append("layout:bad"); cols.append(b"*")
    if nrefid < 0 or nrefid >= len(nm):
        tr.append("rnext:star_negative" if nrefid < 0 else "rnext:star_past_table"); cols.append(b"*")
    elif nrefid == refid:
        tr.append("rnext:equal"); cols.append(b"=")
    else:
        cols.append(ref_name(nrefid, "rnext"))
    cols += [b"%d" % (npos + 1), b"%d" % tlen]
    if tlen < 0:
        tr.append("tlen:negative")
    if not layout_ok or lseq == 0:
        cols += [b"*", b"*"]
        if layout_ok:
            tr.append("seq:star_empty")
    else:
        sq = body[a_seq:a_qual]
        cols.append("".join(BASES16[(sq[q >> 1] >> (0 if q & 1 else 4)) & 15] for q in range(lseq)).encode())
        ql = body[a_qual:a_aux]
        if ql[0] == 0xff:
            tr.append("qual:star_ff_first"); cols.append(b"*")
        else:
            if 0xff in ql:
                tr.append("qual:ff_later_only")
            cols.append(bytes((b + 33) & 0xff for b in ql))
    for f in fields:
        tag, ty, val = f[0], f[1], f[2]
        if f is cg:
            continue
        tr.append("aux:" + ty)
        if ty == "A":
            txt = b"A:" + val
        elif ty in INT_FMT:
            txt = b"i:%d" % struct.unpack(INT_FMT[ty], val)[0]
        elif ty == "f":
            txt = b"f:" + fmt_g(struct.unpack("<I", val)[0]).encode(); info["n_float"] += 1
        elif ty in "ZH":
            txt = ty.encode() + b":" + val
        else:
            sub, cnt = chr(val[0]), struct.unpack("<I", val[1:5])[0]
            tr.append("aux:B:%s:%d" % (sub, cnt))
            if sub == "f":
                vals = [fmt_g(x) for x in struct.unpack("<%dI" % cnt, val[5:])]; info["n_float"] += cnt
            else:
                vals = ["%d" % x for x in struct.unpack("<%d%s" % (cnt, INT_FMT[sub][1]), val[5:])]
            txt = b"B:" + sub.encode() + b"".join(b"," + v.encode() for v in vals)
        cols.append(tag + b":" + txt)
    return b"\t".join(cols) + b"\n", info


def sam_text(bodies, names, trace=None):
    """bodies -> (the lines back to back, the statistics lcd_sam_stats_t must show)"""
    out, st = [], dict(n_records=0, bytes_records=0, bytes_text=0, n_float_values=0, n_cg_cigar=0, n_walk_stopped=0, n_bad_layout=0)
    for b in bodies:
        line, info = sam_line(b, names, trace)
        out.append(line)
        st["n_records"] += 1; st["bytes_records"] += 4 + len(b); st["bytes_text"] += len(line); st["n_float_values"] += info["n_float"]
        st["n_cg_cigar"] += info["cg_cigar"]; st["n_walk_stopped"] += info["walk_stopped"]; st["n_bad_layout"] += info["bad_layout"]
    return b"".join(out), st


def stream(bodies):
    return b"".join(struct.pack("<i", len(b)) + b for b in bodies)


def header_parts(hdr):
    """a BAM header block -> (text bytes as stored, [(name, length)])"""
    l_text = struct.unpack("<i", hdr[4:8])[0]
    o = 8 + l_text
    n_ref = struct.unpack("<i", hdr[o:o + 4])[0]; o += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack("<i", hdr[o:o + 4])[0]
        refs.append((hdr[o + 4:o + 4 + ln].split(b"\0")[0], struct.unpack("<i", hdr[o + 4 + ln:o + 8 + ln])[0])); o += 8 + ln
    return hdr[8:8 + l_text], refs


def sam_header(header_block, pg_line):
    """the SAM header of lcd_bam_writer_open (LCD_ALN_SAM): the text without trailing NULs, pg_line (bytes or None) appended as the BAM writer appends it, a newline at the end;
    no line starting with @SQ<tab> and a table with contigs: @SQ lines in table order behind a leading @HD line, or at the front"""
    text, refs = header_parts(header_block)
    text = text.rstrip(b"\0")
    if pg_line:
        text += (b"" if not text or text.endswith(b"\n") else b"\n") + pg_line + b"\n"
    if text and not text.endswith(b"\n"):
        text += b"\n"
    if not any(ln.startswith(b"@SQ\t") for ln in text.split(b"\n")) and refs:
        sq = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in refs)
        first = text.split(b"\n")[0]
        at = len(first) + 1 if first == b"@HD" or first.startswith(b"@HD\t") else 0
        text = text[:at] + sq + text[at:]
    return text


# ---------------- a line back to a record ----------------
def parse_line(line, names):
    """a SAM line without float fields -> a record body whose line it is (integers get the smallest type that holds them; bin 0)"""
    nm = [x if isinstance(x, bytes) else x.encode() for x in names]
    c = line.rstrip(b"\n").split(b"\t")
    qname = b"" if c[0] == b"*" else c[0]
    refid = -1 if c[2] == b"*" else nm.index(c[2])
    nrefid = -1 if c[6] == b"*" else refid if c[6] == b"=" else nm.index(c[6])
    words, num = [], b""
    if c[5] != b"*":
        for ch in c[5]:
            if chr(ch).isdigit():
                num += bytes([ch])
            else:
                words.append((int(num) << 4) | (OPS.index(chr(ch)) if chr(ch) in OPS else 15)); num = b""
    seq = b"" if c[9] == b"*" else c[9]
    nib = [BASES16.index(chr(x)) for x in seq] + [0]
    packed = bytes((nib[2 * k] << 4) | nib[2 * k + 1] for k in range((len(seq) + 1) // 2))
    qual = b"\xff" * len(seq) if c[10] == b"*" else bytes((x - 33) & 0xff for x in c[10])
    aux = b""
    for f in c[11:]:
        tag, ty, val = f[:2], chr(f[3]), f[5:]
        if ty == "i":
            v = int(val)
            t = next(t for t, (lo, hi) in (("C", (0, 255)), ("c", (-128, 127)), ("S", (0, 65535)), ("s", (-32768, 32767)), ("I", (0, 2 ** 32 - 1)), ("i", (-2 ** 31, 2 ** 31 - 1)))
                     if lo <= v <= hi)
            aux += aux_field(tag, t, v)
        elif ty == "A":
            aux += aux_field(tag, "A", val)
        elif ty in "ZH":
            aux += aux_field(tag, ty, val)
        else:
            assert ty == "B" and chr(val[0]) != "f"
            aux += aux_field(tag, "B", (chr(val[0]), [int(x) for x in val[2:].split(b",")] if len(val) > 1 else []))
    name = qname + b"\0"
    return struct.pack("<iiBBHHHiiii", refid, int(c[3]) - 1, len(name), int(c[4]), 0, len(words), int(c[1]), len(seq), nrefid, int(c[7]) - 1, int(c[8])) + name + \
        struct.pack("<%dI" % len(words), *words) + packed + qual + aux


# ---------------- the case table ----------------
NAMES = [b"chr1", b"chrUn_KI270742v1", b"c"]
# float32 bit patterns on the boundaries of %g (tests/c/sam_float_check.cpp walks all of them and their neighbours on the CPU)
FLOAT_BITS = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff,
              0x3f800000, 0x49742400, 0x497423f0, 0x497423f8, 0x38d1b717, 0x38d1b716, 0x3e800000, 0x461c4000, 0x47c34f80, 0x4b189680, 0x3dcccccd, 0x411ffffb,
              0x411ffffa, 0x501502f9, 0x2edbe6ff, 0xc2f6e979]


def mk(name=b"r", pos0=100, flag=0, qlen=8, cig=None, fields=(), mapq=60, refid=0, nrefid=-1, npos=-1, tlen=0, nibbles=None, qual=None):
    """bam_src_common.record with the core fields it fixes patched afterwards"""
    nib = list(nibbles) if nibbles is not None else [(1, 2, 4, 8)[k & 3] for k in range(qlen)]
    assert len(nib) == qlen
    nib2 = nib + [0]
    a = dict(name=name, pos0=pos0, flag=flag, qlen=qlen, bseq=np.array([(nib2[2 * k] << 4) | nib2[2 * k + 1] for k in range((qlen + 1) // 2)], np.uint8),
             qual=np.asarray(qual if qual is not None else [(7 * k) % 60 for k in range(qlen)], np.uint8))
    body = bytearray(record(a, cig if cig is not None else [(qlen << 4) | 0], list(fields), mapq=mapq)["body"])
    struct.pack_into("<i", body, 0, refid); struct.pack_into("<iii", body, 20, nrefid, npos, tlen)
    if name == b"":                                     # record() always ends the name with a NUL: an empty name is that NUL alone
        assert body[8] == 1
    return bytes(body)


def raw(x):
    return (None, None, x)


def cases():
    """[(condition, body)]: the smallest shapes at which the formatter can go wrong"""
    c = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        c.append(("l_seq_%d" % n, mk(b"q%d" % n, qlen=n, cig=[(n << 4) | 0] if n else [], pos0=n)))
    c.append(("odd_len_last_low_nibble_set", bytes(_low_nibble(mk(b"odd", qlen=7)))))
    c.append(("all_16_nibbles", mk(b"nib", qlen=16, nibbles=range(16))))
    c.append(("qual_ff_first", mk(b"qf", qlen=5, qual=[0xff, 1, 2, 3, 4])))
    c.append(("qual_ff_later_only", mk(b"ql", qlen=5, qual=[1, 0xff, 2, 93, 0xff])))
    c.append(("n_cigar_1", mk(b"c1", cig=[(8 << 4) | 7])))
    c.append(("n_cigar_64", mk(b"c64", qlen=64, cig=[(1 << 4) | (k % 9) for k in range(64)])))
    c.append(("n_cigar_65", mk(b"c65", qlen=65, cig=[((k * 37 % 1000 + 1) << 4) | (k % 10) for k in range(65)])))
    c.append(("op_above_9", mk(b"op", cig=[(3 << 4) | 10, (5 << 4) | 15, (1 << 4) | 9])))
    steps = [v for p in range(1, 9) for v in (10 ** p - 1, 10 ** p)] + [(1 << 28) - 1, 0, 1]
    c.append(("cigar_digit_steps", mk(b"dg", cig=[(v << 4) | (k % 9) for k, v in enumerate(steps)])))
    c.append(("refid_minus_1", mk(b"u", refid=-1, pos0=-1, flag=4, mapq=0, cig=[])))
    c.append(("rnext_equal", mk(b"eq", refid=1, nrefid=1, npos=12345, tlen=777)))
    c.append(("rnext_different", mk(b"df", refid=0, nrefid=2, npos=0, tlen=-1)))
    c.append(("refid_past_table", mk(b"pt", refid=3, nrefid=3)))
    c.append(("rnext_past_table", mk(b"np", refid=2, nrefid=70000)))
    c.append(("tlen_negative", mk(b"tn", refid=0, nrefid=0, npos=5, tlen=-2147483648, pos0=2147483646)))
    c.append(("empty_name", mk(b"")))
    c.append(("name_254", mk(bytes(33 + k % 90 for k in range(254)))))
    sc = [("Xc", "c", -128), ("XC", "C", 255), ("Xs", "s", -32768), ("XS", "S", 65535), ("Xi", "i", -2147483648), ("XI", "I", 4294967295), ("Yc", "c", 127), ("YC", "C", 0),
          ("Ys", "s", 32767), ("YS", "S", 0), ("Yi", "i", 2147483647), ("YI", "I", 0), ("Zi", "i", -1), ("Zs", "s", -10), ("Zc", "c", -9)]
    c.append(("scalars_min_max", mk(b"sc", fields=sc)))
    c.append(("type_A", mk(b"ta", fields=[("XA", "A", b"q"), ("XB", "A", b"~")])))
    c.append(("Z_H_empty_and_long", mk(b"zh", fields=[("ZE", "Z", b""), ("HE", "H", b""), ("ZL", "Z", bytes(33 + k % 94 for k in range(1234))), ("HL", "H", b"1AE3" * 77),
                                                      ("Z1", "Z", b"x")])))
    for sub, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", -2 ** 31, 2 ** 31 - 1), ("I", 0, 2 ** 32 - 1)):
        pat = (lo, hi, 0, lo // 3 if lo else hi // 3, 9, 10, 99, 100)       # both ends, and each side of the digit-count steps every subtype holds
        c.append(("B_%s" % sub, mk(b"b" + sub.encode(), fields=[("B%d" % k, "B", (sub, [pat[(j + k) % 8] for j in range(n)])) for k, n in enumerate((0, 1, 63, 64, 65))])))
    counts = (0, 1, 63, 64, 65)
    c.append(("B_f", _float_bits(mk(b"bf", fields=[("F%d" % k, "B", ("f", [0.0] * n)) for k, n in enumerate(counts)]), [(FLOAT_BITS * 3)[:n] for n in counts])))
    c.append(("scalar_floats", _float_bits(mk(b"sf", fields=[("f%d" % (k % 10), "f", 0.0) for k in range(len(FLOAT_BITS))]), [[b] for b in FLOAT_BITS], scalar=True)))
    c.append(("Z_without_NUL", mk(b"zn", fields=[("XA", "A", b"k"), raw(b"XZZabcHPC\x01")])))
    c.append(("B_past_the_record", mk(b"bp", fields=[("NM", "C", 3), raw(b"XBBi\xe8\x03\0\0\x01\0\0\0HPC\x01")])))
    c.append(("unknown_type", mk(b"ut", fields=[("OK", "Z", b"yes"), raw(b"XQq\x01\x02"), ("NO", "Z", b"never")])))
    c.append(("two_bytes_left", mk(b"tb", fields=[("OK", "C", 1), raw(b"XY")])))
    cgw = [(5 << 4) | 4, (30 << 4) | 0, (2 << 4) | 2, (100000 << 4) | 7]
    cgf = ("CG", "B", ("I", cgw))
    c.append(("CG_cigar", mk(b"cg", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[("NM", "C", 1), cgf, ("XZ", "Z", b"after")])))
    c.append(("CG_cigar_empty_array", mk(b"cg0", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[("CG", "B", ("I", []))])))
    c.append(("CG_miss_three_words", mk(b"cm3", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3, (1 << 4) | 0], fields=[cgf])))
    c.append(("CG_miss_first_len", mk(b"cml", qlen=8, cig=[(7 << 4) | 4, (200 << 4) | 3], fields=[cgf])))
    c.append(("CG_miss_first_op", mk(b"cmo", qlen=8, cig=[(8 << 4) | 5, (200 << 4) | 3], fields=[cgf])))
    c.append(("CG_miss_second_op", mk(b"cms", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 2], fields=[cgf])))
    c.append(("CG_miss_no_field", mk(b"cmn", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[("XG", "B", ("I", cgw))])))
    c.append(("CG_miss_type_Z", mk(b"cmz", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[("CG", "Z", b"5S30M"), cgf])))
    c.append(("CG_miss_subtype_i", mk(b"cmi", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[("CG", "B", ("i", cgw)), cgf])))
    c.append(("CG_behind_a_stopped_walk", mk(b"cmw", qlen=8, cig=[(8 << 4) | 4, (200 << 4) | 3], fields=[raw(b"XZZabc"), cgf])))
    ok = mk(b"lay", qlen=40, cig=[(40 << 4) | 0], fields=[("NM", "C", 1)])
    c.append(("layout_cut_in_the_qualities", ok[:32 + 4 + 4 + 20 + 11]))
    c.append(("layout_cut_in_the_cigar", ok[:32 + 4 + 2]))
    c.append(("layout_cut_in_the_name", ok[:32 + 2]))
    c.append(("layout_fixed_fields_only", ok[:32]))
    neg = bytearray(ok); struct.pack_into("<i", neg, 16, -5)
    c.append(("layout_negative_l_seq", bytes(neg)))
    huge = bytearray(ok); struct.pack_into("<i", huge, 16, 2 ** 31 - 1)
    c.append(("layout_l_seq_2^31", bytes(huge)))
    c.append(("name_without_NUL", _no_nul(mk(b"abcdefg"))))
    return c


def _low_nibble(body):
    b = bytearray(body)
    lname, nc, lseq = b[8], struct.unpack_from("<H", b, 12)[0], struct.unpack_from("<i", b, 16)[0]
    assert lseq & 1
    b[32 + lname + 4 * nc + lseq // 2] |= 0x0b          # the unused low nibble of the last byte
    return b


def _no_nul(body):
    b = bytearray(body)
    b[32 + b[8] - 1] = ord("Z")
    return bytes(b)


def _float_bits(body, bits_per_field, scalar=False):
    """overwrite the values of a record's f / B:f fields with exact bit patterns (struct.pack would quieten a signalling NaN)"""
    b = bytearray(body)
    lname, nc, lseq = b[8], struct.unpack_from("<H", b, 12)[0], struct.unpack_from("<i", b, 16)[0]
    o = 32 + lname + 4 * nc + (lseq + 1) // 2 + lseq
    for bits in bits_per_field:
        if scalar:
            assert chr(b[o + 2]) == "f"
            struct.pack_into("<I", b, o + 3, bits[0]); o += 7
        else:
            assert b[o + 2:o + 4] == b"Bf" and struct.unpack_from("<I", b, o + 4)[0] == len(bits)
            struct.pack_into("<%dI" % len(bits), b, o + 8, *bits); o += 8 + 4 * len(bits)
    assert o == len(b)
    return bytes(b)


def big_record():
    """l_seq 70 001, 40 000 CIGAR words, a B:C array of 70 001 elements (a kinetics array is as long as the read)"""
    n = 70001
    rng = np.random.default_rng(11)
    return mk(b"big/70001/ccs", qlen=n, nibbles=rng.integers(0, 16, n).tolist(), qual=rng.integers(0, 94, n).tolist(),
              cig=[(int(v) << 4) | int(o) for v, o in zip(rng.integers(1, 3000, 40000), rng.integers(0, 9, 40000))],
              fields=[("RG", "Z", b"grp"), ("fi", "B", ("C", rng.integers(0, 256, n).tolist())), ("np", "i", 17)])
