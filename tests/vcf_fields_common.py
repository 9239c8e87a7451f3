"""The Python side of the VCF-fields tests (MEI annotation from a TE library, supporting read names): a reader of FASTA / FASTQ files equivalent to kseq_read
(src/kseq.h:175-215, what make_te_kmer_idx reads its -T file with, src/kmer.c:120-148), the ALTREADS formatter written from write_var_to_vcf
(src/vcf_utils.c:205-253), drivers of the oracles' annotation and formatter (oracle/emit.c: lcdo_annotate_te, lcdo_format_vcf_te; oracle/te_info.c) on record dicts,
and a seeded generator that plants mobile-element insertions into a clean_vars_common.make_diploid_chunk-style contig.  Expected values come from here and from the
oracles, never from the library under test."""
import ctypes as C
import gzip

import numpy as np

import bam_out_common as bo
import clean_vars_common as cc
import emit_common as ec

RNAMES = {None: 0, "sv": 1, "all": 2}
_SPACE = b" \t\n\v\f\r"


# ---------------- kseq_read ----------------
def kseq_records(data):
    """bytes of an (inflated) FASTA / FASTQ file -> [(name, sequence)] as kseq_read yields them.
      * the scan for a record stops at '>' or '@'; the name ends at the first isspace() byte; unless that byte is the newline, the rest of the line is the comment;
      * sequence lines run up to a line that STARTS with '>', '@' or '+'; an empty line is skipped; after every line read, ONE trailing '\\r' is dropped while the
        sequence holds more than one byte (ks_getuntil2, :140, on the string it appends to) -- nothing is dropped when the file had already ended;
      * '+': the rest of that line is skipped, quality lines are read until they hold as many bytes as the sequence; a missing or shorter quality string ends the
        records (kseq_read returns -2, and the caller's `while (kseq_read(ks) >= 0)` stops)."""
    n, pos, last, out = len(data), 0, 0, []

    def rest_of_line(s):
        nonlocal pos
        if pos >= n:
            return False
        e = data.find(b"\n", pos)
        e = n if e < 0 else e
        s += data[pos:e]
        pos = min(e + 1, n)
        if len(s) > 1 and s[-1:] == b"\r":
            del s[-1]
        return True

    while True:
        if last == 0:
            while pos < n and data[pos] not in b">@":
                pos += 1
            if pos >= n:
                return out
            last = data[pos]; pos += 1
        if pos >= n:
            return out
        e = pos
        while e < n and data[e] not in _SPACE:
            e += 1
        name, c = data[pos:e], (data[e] if e < n else 0)
        pos = min(e + 1, n)
        if c != 10:
            rest_of_line(bytearray())
        seq, c = bytearray(), -1
        while pos < n:
            c = data[pos]; pos += 1
            if c in b">+@":
                break
            if c != 10:
                seq.append(c)
                rest_of_line(seq)
            c = -1
        if c in (62, 64):
            last = c
        if c == 43:
            e = data.find(b"\n", pos)
            if e < 0:
                return out
            pos = e + 1
            qual = bytearray()
            while rest_of_line(qual) and len(qual) < len(seq):
                pass
            last = 0
            if len(qual) != len(seq):
                return out
        out.append((bytes(name), bytes(seq)))


def read_te_file(path):
    """gzopen / gzread: a gzip file is inflated, anything else is read as it is"""
    raw = open(path, "rb").read()
    return kseq_records(gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw)


def write_te_fasta(path, seqs, names=None, width=60):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">" + (names[i] if names else b"TE%d" % i) + b" family=%d\n" % i)
            for k in range(0, len(s), width):
                f.write(bytes(s[k:k + width]) + b"\n")


# ---------------- ALTREADS, src/vcf_utils.c:205-253 ----------------
def altreads_value(rec, names):
    """the names of alt_read_i[0 .. AD[1]) joined by ',' (:245-249); "." when AD[1] == 0 (:251)"""
    n = rec["AD"][1]
    return b"." if n <= 0 else b",".join(names[r] for r in rec["alt_reads"][:n])


def qualifies(rec, mode):
    """:208 / :234, germline: output_var_rnames || (is_sv && output_sv_rnames)"""
    return mode == 2 or (mode == 1 and bool(rec["is_sv"]))


def add_altreads(line, rec, mode, names):
    """one body line without read names (bytes, with its newline) -> the line write_var_to_vcf writes with them: ':ALTREADS' behind the FORMAT keys -- that is behind
    the optional ':PS' (:206-210) -- and ':' + the value behind the sample's last field (:243-253)"""
    if not qualifies(rec, mode):
        return line
    assert line.endswith(b"\n")
    col = line[:-1].split(b"\t")
    assert len(col) == 10
    col[8] += b":ALTREADS"
    col[9] += b":" + altreads_value(rec, names)
    return b"\t".join(col) + b"\n"


# ---------------- the oracles on record dicts ----------------
def var1_array(recs, keep):
    """record dicts (align._var1_dict / emit_common.make_variants) -> an array of Var1 with the annotation members as lcd_make_variants leaves them"""
    arr = (ec.Var1 * max(1, len(recs)))()
    for v, r in zip(arr, recs):
        v.pos, v.PS, v.type, v.ref_len, v.n_alt_allele = r["pos"], r["PS"], r["type"], r["ref_len"], r["n_alt"]
        bufs = [np.frombuffer(bytes(r["ref"]) + b"\0", np.uint8).copy()] + [np.frombuffer(bytes(a) + b"\0", np.uint8).copy() for a in r["alt"]]
        ar = np.array(list(r["alt_reads"]) + [0], np.int32)
        keep += bufs + [ar]
        v.ref_bases = bufs[0].ctypes.data_as(ec.u8p)
        for a in range(r["n_alt"]):
            v.alt_len[a] = len(r["alt"][a]); v.alt_bases[a] = bufs[1 + a].ctypes.data_as(ec.u8p)
        v.GT[0], v.GT[1] = r["GT"]
        v.DP, v.QUAL, v.GQ, v.is_sv, v.is_clean = r["DP"], r["QUAL"], r["GQ"], r["is_sv"], r["is_clean"]
        for k in range(3):
            v.AD[k] = r["AD"][k]
        v.n_alt_reads = len(r["alt_reads"]); v.alt_read_i = ar.ctypes.data_as(ec.i32p)
        v.cand_i = r.get("cand_i", 0)
        v.tsd_len, v.polya_len, v.te_seq_i, v.te_is_rev, v.tsd_pos1, v.tsd_pos2 = 0, 0, -1, 0, -1, -1
    return arr


def oracle_te_lib(orc, seqs, k=15):
    orc.lcdo_te_lib_create.restype = C.c_void_p
    orc.lcdo_te_lib_create.argtypes = [C.c_int, C.POINTER(C.c_char_p), ec.i32p, C.c_int]
    orc.lcdo_te_lib_destroy.argtypes = [C.c_void_p]
    arr = (C.c_char_p * max(len(seqs), 1))(*[bytes(s) for s in seqs]); lens = (C.c_int * max(len(seqs), 1))(*[len(s) for s in seqs])
    return orc.lcdo_te_lib_create(len(seqs), arr, lens, k)


def oracle_check_te(orc, lib, codes):
    """lcdo_check_te_seq -> (te_seq_i or -1, is_rev)"""
    orc.lcdo_check_te_seq.argtypes = [C.c_void_p, ec.u8p, C.c_int, ec.i32p]
    a = np.ascontiguousarray(codes, np.uint8)
    a = a if a.size else np.zeros(1, np.uint8)
    rev = C.c_int(0)
    return int(orc.lcdo_check_te_seq(lib, a.ctypes.data_as(ec.u8p), len(codes), C.byref(rev))), int(rev.value)


def oracle_annotate(orc, opt, te_lib, ref_codes, ref_beg, arr, n):
    """lcdo_annotate_te (collect_te_info_from_cons per SV-size gap record) on the array; -> the annotation members per record"""
    ref = np.ascontiguousarray(ref_codes, np.uint8).tobytes()
    orc.lcdo_annotate_te.restype = C.c_int
    orc.lcdo_annotate_te.argtypes = [C.POINTER(ec.CallOpt), C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(ec.Var1), C.c_int]
    orc.lcdo_annotate_te(C.byref(opt), 2, 100, 10, 0.8, te_lib, ref, ref_beg, ref_beg + len(ref) - 1, arr, n)
    return [dict(tsd=bytes(arr[i].tsd_seq[j] for j in range(arr[i].tsd_len)), polya_len=arr[i].polya_len, te_seq_i=arr[i].te_seq_i, te_is_rev=arr[i].te_is_rev,
                 tsd_pos1=arr[i].tsd_pos1, tsd_pos2=arr[i].tsd_pos2) for i in range(n)]


def oracle_lines(orc, opt, chrom, arr, n, te_names):
    """lcdo_format_vcf_te record by record -> per record its body line (bytes) or None when write_var_to_vcf's filters drop it"""
    orc.lcdo_format_vcf_te.restype = C.c_int
    names = (C.c_char_p * max(len(te_names), 1))(*te_names) if te_names is not None else None
    out = []
    for i in range(n):
        t = C.c_void_p()
        nl = orc.lcdo_format_vcf_te(C.byref(opt), C.c_char_p(chrom), C.byref(arr[i]), 1, names, C.byref(t))
        text = C.string_at(t)
        ec._libc.free(t)
        assert nl == text.count(b"\n") and nl in (0, 1)
        out.append(text if nl else None)
    return out


def expected_text(orc, opt, chrom, recs, ref_codes, ref_beg, te_seqs, te_names, mode, names):
    """one chunk: its record dicts, its reference window, the library, the names mode and the chunk's read names -> (the body text, the oracle's annotation per record)"""
    keep = []
    arr = var1_array(recs, keep)
    lib = oracle_te_lib(orc, te_seqs) if te_seqs is not None else None
    ann = oracle_annotate(orc, opt, lib, ref_codes, ref_beg, arr, len(recs))
    lines = oracle_lines(orc, opt, chrom, arr, len(recs), te_names)
    for i in range(len(recs)):
        if arr[i].tsd_seq:
            ec._libc.free(C.cast(arr[i].tsd_seq, C.c_void_p))
    if lib:
        orc.lcdo_te_lib_destroy(lib)
    return b"".join(add_altreads(l, r, mode, names) for l, r in zip(lines, recs) if l is not None), ann


# ---------------- read names of a chunk, from the BAM ----------------
def bam_bodies(path):
    return bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read())))[1]


def chunk_read_names(bam_paths, reg_beg, reg_end, min_mapq=30, refid=0):
    """the names of a chunk's reads in the chunk's read order: per file, in input order, the region iterator's kept records in file order (file-major)"""
    names = []
    for p in bam_paths:
        names += [bo.parse(body)["name"] for body, r in bo.region_records(bam_bodies(p), reg_beg, reg_end, min_mapq, refid) if r >= 0]
    return names


# ---------------- planted mobile-element insertions ----------------
TSD_LEN, CUT_LEN, TAIL_LEN = 12, 200, 20
PLANT_AT = (2500, 8000, 9800)                  # 0-based insertion points: one in the first 6 kb chunk, two in the second


def te_library(seed=2024):
    """three seeded random sequences of 280 to 320 bases (letters)"""
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(280, 321)))]) for _ in range(3)]


def _codes(letters):
    return [b"ACGT".index(c) for c in letters]


def make_mei_chunk(seed=7, ref_len=12000, depth=12, read_len=(2000, 6000), err=0.001, lowq=0.003):
    """a seeded diploid contig in the style of clean_vars_common.make_diploid_chunk (SNPs and small indels on one or both haplotypes, both strands, random errors,
    low-quality bases) with three het insertions on haplotype 0, each in front of 0-based position p:
      forward   ref[p : p + 12] (the target-site duplication: the bases that FOLLOW the insertion point), 200 bases cut from library sequence 1, 20 A;
      reverse   ref[p : p + 12], 20 T, the reverse complement of a 200-base cut of library sequence 2;
      orphan    ref[p : p + 12], 200 random bases, 20 A: a duplication and a poly-A tail, no TE.
    The base in front of each insertion point is set to differ from the insertion's last base, so that the event cannot be moved to the left; no other event lies
    within 400 bases of a planted one.  -> make_diploid_chunk's dict plus te_seqs and planted = [dict(p, kind, te_i, seq)]"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, ref_len).astype(np.uint8)
    tes = te_library()
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    planted = []
    for p, kind in zip(PLANT_AT, ("forward", "reverse", "orphan")):
        tsd = [int(x) for x in ref[p:p + TSD_LEN]]
        if kind == "forward":
            a = int(rng.integers(0, len(tes[1]) - CUT_LEN + 1)); seq = tsd + _codes(tes[1][a:a + CUT_LEN]) + [0] * TAIL_LEN; te_i = 1
        elif kind == "reverse":
            a = int(rng.integers(0, len(tes[2]) - CUT_LEN + 1)); seq = tsd + [3] * TAIL_LEN + _codes(tes[2][a:a + CUT_LEN].translate(comp)[::-1]); te_i = 2
        else:
            seq = tsd + rng.integers(0, 4, CUT_LEN).tolist() + [0] * TAIL_LEN; te_i = -1
        if ref[p - 1] == seq[-1]:
            ref[p - 1] = (seq[-1] + 1) % 4
        planted.append(dict(p=p, kind=kind, te_i=te_i, seq=seq))
    haps = [dict(), dict()]
    free = [q for q in range(300, ref_len - 300) if all(abs(q - x["p"]) > 400 for x in planted)]
    for q in np.sort(rng.choice(free, ref_len // 400, replace=False)):
        q = int(q)
        k = rng.random()
        ev = ("X", int((ref[q] + rng.integers(1, 4)) % 4)) if k < 0.7 else ("I", rng.integers(0, 4, int(rng.integers(1, 4))).tolist()) if k < 0.85 else ("D", int(rng.integers(1, 4)))
        z = rng.random()
        for h in ((0,) if z < 0.4 else (1,) if z < 0.8 else (0, 1)):
            haps[h][q] = ev
    for x in planted:
        haps[0][x["p"]] = ("I", x["seq"])
    reads = []
    for s in np.sort(rng.integers(0, ref_len - read_len[0], int(depth * ref_len / np.mean(read_len)))):
        h = int(rng.integers(0, 2))
        r = cc.read_from_hap(ref, int(s), int(rng.integers(*read_len)), haps[h], rng=rng, err=err, lowq=lowq)
        r["is_rev"], r["hap"] = int(rng.integers(0, 2)), h + 1
        reads.append(r)
    reads = [reads[i] for i in np.argsort([r["pos0"] for r in reads], kind="stable")]
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=ref_len, whole_ref_len=ref_len, is_ont=0, te_seqs=tes, planted=planted)


def planted_record(recs, x):
    """the record of a planted insertion: an INS whose anchor is the base in front of the insertion point (1-based position p) and whose length is the planted one"""
    hit = [r for r in recs if r["type"] == 1 and abs(r["pos"] - x["p"]) <= 2 and r["is_sv"] and abs(r["alt_len"][0] - 1 - len(x["seq"])) <= 2]
    return hit[0] if hit else None
