"""Inputs and pure-Python oracles for chunks made from ANY BAM (lcd_chunk_create_from_bam_src): which of the reference's four digar sources a record gets
(collect_digars_from_bam, src/collect_var.c:1072-1079; has_equal_X_in_bam_cigar, src/bam_utils.c:51-66; bam_aux_get's field walk) and the SA-tag palindrome rule
(is_ont_palindrome_clip + check_ont_palindrome, src/bam_utils.c:642-698).
  * one seeded reference of 30 kb and 60 reads of 2-6 kb on it, each from ONE alignment given in all four shapes (EQX CIGAR, cs, MD, plain 'M' + bases): two
    haplotypes that share planted X / I / D sites, per-read errors, noisy stretches, clips;
  * a BAM writer on tests/test_io.py's _bgzf / _write_bai that takes a CIGAR and a list of auxiliary fields per record (every field type, broken fields too);
  * the selection rule and the SA rule restated in Python, the SA rule with the branch it took; the named SA cases with their expected flags (worked out by hand
    below, not taken from the oracle).
Used by tests/test_bam_sources_oracle.py (CPU) and tests/test_gpu_bam_sources.py."""
import functools
import struct

import numpy as np

from digar_inputs import BASES, pack4, quals
from test_io import _bgzf, _write_bai

CONTIG, TLEN = "chrS", 30000
SRC_EQX, SRC_CS, SRC_MD, SRC_REF = 0, 1, 2, 3
END_CLIP_REG = 30


# ---------------- one alignment in the four shapes ----------------
def build_on_ref(rng, ref, pos0, ops):
    """ops: [(op, len, payload | None)] EQX operations on the shared reference `ref` (codes 0-3) from 0-based pos0; payload = the X / I bases (codes), else random
    (an X base always differs from the reference).  -> dict(pos0, eqx, mcig, cs, md, bseq, qlen, rlen)"""
    read, cs, md = [], [], []
    md_cnt = 0
    rp = pos0
    for o, l, pay in ops:
        if o == 7:
            read.append(ref[rp:rp + l]); cs.append(b":%d" % l); md_cnt += l; rp += l
        elif o == 8:
            for k in range(l):
                r = int(ref[rp + k]); q = int(pay[k]) if pay is not None else (r + int(rng.integers(1, 4))) & 3
                assert q != r
                read.append(np.array([q], np.uint8)); cs.append(b"*" + bytes([BASES[r] | 32, BASES[q] | 32]))
                md.append(b"%d" % md_cnt + bytes([BASES[r]])); md_cnt = 0
            rp += l
        elif o == 1:
            ins = np.asarray(pay, np.uint8) if pay is not None else rng.integers(0, 4, l).astype(np.uint8)
            read.append(ins); cs.append(b"+" + bytes(BASES[b] | 32 for b in ins))
        elif o == 2:
            cs.append(b"-" + bytes(BASES[b] | 32 for b in ref[rp:rp + l])); md.append(b"%d^" % md_cnt + bytes(BASES[b] for b in ref[rp:rp + l])); md_cnt = 0; rp += l
        elif o == 4:
            read.append(rng.integers(0, 4, l).astype(np.uint8))
    md.append(b"%d" % md_cnt)
    read = np.concatenate(read) if read else np.zeros(0, np.uint8)
    eqx = np.array([(l << 4) | o for o, l, _ in ops], np.uint32)
    m = []
    for o, l, _ in ops:
        o2 = 0 if o in (7, 8) else o
        if m and o2 == 0 and (m[-1] & 0xf) == 0:
            m[-1] += l << 4
        else:
            m.append((l << 4) | o2)
    return dict(pos0=int(pos0), eqx=eqx, mcig=np.array(m, np.uint32), cs=b"".join(cs), md=b"".join(md), bseq=pack4(read), qlen=len(read), rlen=rp - pos0)


def _read_ops(rng, ref, pos0, rlen, hap, sites, noisy, clips):
    """events of one read: the planted sites of its haplotype inside [pos0 + 20, pos0 + rlen - 20), per-read errors in between (noisy 1: dense inside one
    250-base stretch; noisy 2: dense everywhere, a read the per-read ratios skip); events are kept at least 3 '=' bases apart, so the four shapes describe the same alignment without adjacent operations to merge"""
    ev = {p: e for p, e in sites.items() if pos0 + 20 <= p < pos0 + rlen - 20 and e[3] == hap}
    nz = int(rng.integers(pos0 + 100, pos0 + rlen - 400)) if noisy else -1
    p = pos0 + 10
    while p < pos0 + rlen - 30:
        p += int(rng.geometric(1 / 10 if noisy == 2 or nz <= p < nz + 250 else 1 / 700))
        if p < pos0 + rlen - 30 and p not in ev:
            k = int(rng.integers(0, 3))
            ev[p] = (8, 1, None, hap) if k == 0 else (1, int(rng.integers(1, 40 if rng.random() < 0.1 else 4)), None, hap) if k == 1 else (2, int(rng.integers(1, 40 if rng.random() < 0.1 else 4)), None, hap)
    ops = []
    if clips[0]:
        ops.append((clips[0][0], clips[0][1], None))
    at = pos0
    for p in sorted(ev):
        o, l, pay, _ = ev[p]
        if p - at < 3 or p + (l if o in (8, 2) else 0) > pos0 + rlen - 10:
            continue
        ops.append((7, p - at, None)); ops.append((o, l, pay)); at = p + (l if o in (8, 2) else 0)
    ops.append((7, pos0 + rlen - at, None))
    if clips[1]:
        ops.append((clips[1][0], clips[1][1], None))
    return ops


@functools.lru_cache(maxsize=None)
def seeded(seed=7, n=60):
    """-> (ref codes (30 kb), [alignment dicts in position order]); alignment i additionally carries qual, flag, and the SA value of the seeded file (or None)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, TLEN).astype(np.uint8)
    sites = {}
    for p in range(600, TLEN - 600, 170):
        p += int(rng.integers(0, 40)); k = int(rng.integers(0, 3)); hap = int(rng.integers(0, 2))
        if k == 0:
            sites[p] = (8, 1, np.array([(int(ref[p]) + int(rng.integers(1, 4))) & 3], np.uint8), hap)
        elif k == 1:
            ln = int(rng.integers(1, 9))
            sites[p] = (1, ln, rng.integers(0, 4, ln).astype(np.uint8), hap)
        else:
            sites[p] = (2, int(rng.integers(1, 9)), None, hap)
    pos = np.sort(rng.integers(300, TLEN - 6500, n))
    al = []
    for i in range(n):
        rlen = int(rng.integers(2000, 6000))
        pal = i % 7 == 3
        clip = lambda: (4 if rng.random() < 0.8 or pal else 5, int(rng.integers(50, 120)) if pal or rng.random() < 0.4 else int(rng.integers(1, 30)))
        clips = (clip() if pal or rng.random() < 0.4 else None, clip() if pal or rng.random() < 0.4 else None)
        a = build_on_ref(rng, ref, int(pos[i]), _read_ops(rng, ref, int(pos[i]), rlen, i & 1, sites, noisy=2 if i % 10 == 0 else 1 if i % 5 == 0 else 0, clips=clips))
        a["qual"] = quals(rng, a["qlen"]); a["flag"] = 16 if i % 3 == 1 else 0; a["name"] = f"r/{i}".encode()
        # SA tags of the seeded file: every 7th read is a palindrome (its supplementary alignment covers the primary), another 7th has one elsewhere
        a["sa"] = b"%s,%d,%s,%dM%dS,60,3;" % (CONTIG.encode(), a["pos0"] + 1, b"+" if a["flag"] else b"-", a["rlen"], 80) if pal else \
            b"chrOther,%d,+,%dM,20,9;" % (a["pos0"] + 20000, a["rlen"]) if i % 7 == 5 else None
        al.append(a)
    return ref, al


def ref_letters(ref):
    return bytes(BASES[b] for b in ref)


# ---------------- BAM records with any auxiliary block ----------------
def aux_field(tag, ty, val):
    """one auxiliary field; ty in A c C s S i I f Z H B (B: val = (subtype, values)); ty None: val is raw bytes (a broken field)"""
    if ty is None:
        return bytes(val)
    t = tag.encode() if isinstance(tag, str) else tag
    if ty == "A":
        return t + b"A" + bytes(val[:1])
    if ty in "cCsSiIf":
        return t + ty.encode() + struct.pack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I", f="f")[ty], val)
    if ty in "ZH":
        return t + ty.encode() + bytes(val) + b"\0"
    sub, vals = val
    return t + b"B" + sub.encode() + struct.pack("<i", len(vals)) + b"".join(struct.pack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I", f="f")[sub], v) for v in vals)


def decoys(rng):
    """fields of every type whose names are none of cs / MD / SA / CG; Z values that look like the tags that matter"""
    d = [("XA", "A", b"q"), ("Xc", "c", -3), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000), ("NM", "I", 7), ("Xf", "f", 0.25),
         ("XZ", "Z", b"cs:Z::10*at;SA,MD"), ("XH", "H", b"1AE301"), ("Xb", "B", ("c", [-1, 2])), ("XB", "B", ("C", [1, 2, 3])), ("Xt", "B", ("s", [-5])),
         ("XT", "B", ("S", [5, 6])), ("Xj", "B", ("i", list(range(int(rng.integers(0, 9)))))), ("XJ", "B", ("I", [1 << 31])), ("Xg", "B", ("f", [1.5, -2.0])), ("ZZ", "Z", b"")]
    return [d[k] for k in rng.permutation(len(d))]


def record(a, cig, fields, mapq=60):
    """a BAM record body for alignment `a` with the CIGAR words `cig` and the auxiliary fields [(tag, type, value)] in order"""
    name = a["name"] + b"\0"
    cig = np.asarray(cig, "<u4")
    aux = b"".join(aux_field(*f) for f in fields)
    body = struct.pack("<iiBBHHHiiii", 0, a["pos0"], len(name), mapq, 4680, len(cig), a["flag"], a["qlen"], -1, -1, 0) + name + cig.tobytes() + \
        np.asarray(a["bseq"], np.uint8).tobytes()[:(a["qlen"] + 1) // 2] + np.asarray(a["qual"], np.uint8).tobytes() + aux
    rl = sum(int(c >> 4) for c in cig if int(c & 0xf) in (0, 2, 3, 7, 8))
    return dict(body=body, pos0=a["pos0"], end=a["pos0"] + max(rl, 1), cig=cig, aux=aux, a=a, flag=a["flag"])


def write_bam(path, recs, block=9000, tlen=TLEN):
    """records (position order) -> a sorted single-contig BAM + .bai; tlen: the contig's length in the header"""
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n"
    d = bytearray(b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", 1) + struct.pack("<i", len(CONTIG) + 1) + CONTIG.encode() + b"\0" + struct.pack("<i", tlen))
    idx = []
    for x in recs:
        u0 = len(d); d += struct.pack("<i", len(x["body"])) + x["body"]
        idx.append(dict(tid=0, pos=x["pos0"], end=x["end"], u0=u0, u1=len(d)))
    coffs = []
    d = bytes(d)
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    for x in idx:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", 1, idx)


def records_as(kind, rng=None, sa=True):
    """the seeded alignments as records of one kind: 'eqx' (EQX CIGAR), 'cs' / 'md' ('M' CIGAR + that tag), 'ref' ('M' CIGAR alone), or 'mixed' (read i: kind i % 4).
    Decoy fields of every type go in front of, and between, the tags that matter; EQX reads carry cs + MD decoys now and then; SA tags as seeded() planted them"""
    rng = rng or np.random.default_rng(3)
    _, al = seeded()
    out = []
    for i, a in enumerate(al):
        k = ("eqx", "cs", "md", "ref")[i % 4] if kind == "mixed" else kind
        dz = decoys(rng)
        cut = sorted(int(x) for x in rng.integers(0, len(dz) + 1, 3))
        f = dz[:cut[0]]
        if k == "cs":
            f += [("cs", "Z", a["cs"])] + dz[cut[0]:cut[1]] + ([("MD", "Z", a["md"])] if i % 8 < 4 else [])
        elif k == "md":
            f += [("MD", "Z", a["md"])] + dz[cut[0]:cut[1]]
        elif k == "eqx" and i % 8 == 0:
            f += [("MD", "Z", a["md"])] + dz[cut[0]:cut[1]] + [("cs", "Z", a["cs"])]
        else:
            f += dz[cut[0]:cut[1]]
        if sa and a["sa"] is not None:
            f += [("SA", "Z", a["sa"])]
        f += dz[cut[1]:cut[2]]
        out.append(record(a, a["eqx"] if k == "eqx" else a["mcig"], f))
    return out


# ---------------- the rules, restated ----------------
def aux_walk(aux):
    """bam_aux_get's walk: the complete fields in order as (tag, type, value bytes); a field that runs past the block ends the walk silently"""
    out, p, n = [], 0, len(aux)
    size = dict(A=1, c=1, C=1, s=2, S=2, i=4, I=4, f=4)
    while p + 3 <= n:
        tag, ty = aux[p:p + 2], chr(aux[p + 2]); p += 3
        if ty in size:
            sz = size[ty]
        elif ty in "ZH":
            e = aux.find(b"\0", p)
            if e < 0:
                break
            sz = e - p + 1
        elif ty == "B":
            if p + 5 > n or chr(aux[p]) not in size or chr(aux[p]) == "A":
                break
            sz = 5 + struct.unpack("<I", aux[p + 1:p + 5])[0] * size[chr(aux[p])]
        else:
            break
        if n - p < sz:
            break
        out.append((tag, ty, aux[p:p + sz - 1] if ty in "ZH" else aux[p:p + sz])); p += sz
    return out


def first_field(fields, name):
    for tag, ty, val in fields:
        if tag == name:
            return ty, val
    return None


def select_source(cig, aux):
    """-> (LCD_SRC_*, deciding field (type, value) | None): the first of '=' / 'X' / 'M' decides EQX or not; else the first cs, else the first MD, else REF"""
    for c in cig:
        op = int(c) & 0xf
        if op in (7, 8):
            return SRC_EQX, None
        if op == 0:
            break
    f = aux_walk(aux)
    cs, md = first_field(f, b"cs"), first_field(f, b"MD")
    return (SRC_CS, cs) if cs else (SRC_MD, md) if md else (SRC_REF, None)


def _decimal(s):
    t = s[1:] if s[:1] in (b"-", b"+") else s
    if not t or not t.isdigit():
        return None
    v = min(int(t), 2 ** 31 - 1)
    return -v if s[:1] == b"-" else v


def sa_rule(sa, pos0, end_pos, flag, is_ont):
    """-> (flags: bit 0 left clip / bit 1 right clip is palindromic, trace): `sa` = (type, value) of the first SA field or None.  trace = 'not_ont' | 'no_tag' |
    'not_Z' | one item per piece: 'empty' (between two ';'), 'skipped', or (branch, overlap) with branch in contain / left_partial / left_none / right_partial / inside /
    right_none -- the walk stops at the first palindromic entry"""
    if not is_ont:
        return 0, "not_ont"
    if sa is None:
        return 0, "no_tag"
    if sa[0] != "Z":
        return 0, "not_Z"
    A, B = pos0 + 1, end_pos
    plen = B - A + 1
    trace, pal = [], False
    pieces = bytes(sa[1]).split(b";")
    for k, piece in enumerate(pieces):
        if not piece:
            if k + 1 < len(pieces):          # (what follows the last ';' is not a piece)
                trace.append("empty")
            continue
        f = piece.split(b",")
        pos = _decimal(f[1]) if len(f) >= 4 else None
        if len(f) < 4 or not f[0] or pos is None or len(f[2]) != 1 or not f[3]:
            trace.append("skipped"); continue
        sa_end, k, cg = pos, 0, f[3]
        while k < len(cg):
            ln = 0
            while k < len(cg) and cg[k:k + 1].isdigit():
                ln = min(ln * 10 + int(cg[k:k + 1]), 2 ** 31 - 1); k += 1
            if k >= len(cg):
                break
            if cg[k:k + 1] in (b"M", b"D", b"=", b"X"):
                sa_end += ln
            k += 1
        sa_len, ov = sa_end - pos + 1, 0
        if pos <= A:
            if sa_end >= B:
                br, ov = "contain", plen
            elif sa_end >= A:
                br, ov = "left_partial", sa_end - A + 1
            else:
                br = "left_none"
        elif pos <= B:
            if sa_end >= B:
                br, ov = "right_partial", B - pos + 1
            else:
                br, ov = "inside", sa_len
        else:
            br = "right_none"
        trace.append((br, ov))
        if float(ov) >= float(plen) * 0.9:
            pal = True
            break
    return (0 if not pal else 1 if flag & 16 else 2), trace


def record_rule(rec, is_ont):
    """a record() -> (source, deciding field, palindrome flags)"""
    src, fld = select_source(rec["cig"], rec["aux"])
    return src, fld, sa_rule(first_field(aux_walk(rec["aux"]), b"SA"), rec["pos0"], rec["end"], rec["flag"], is_ont)[0]


def expected(orc, rec, ref_seq, ref_beg, ref_end, reg_beg, reg_end, is_ont, pal=None):
    """what the chunk must hold for this record: its source's oracle with the SA rule's flags (pal: override them) -> (source, flags, oracle dict | dict(rc=-2))"""
    src, fld, fl = record_rule(rec, is_ont)
    if pal is not None:
        fl = pal
    a = rec["a"]
    args = (reg_beg, reg_end, TLEN, orc.digar_opt(is_ont), fl & 1, (fl >> 1) & 1)
    if src == SRC_EQX:
        e = orc.collect_digar_from_eqx_cigar(a["pos0"], rec["cig"], a["qual"], *args)
    elif src in (SRC_CS, SRC_MD):
        if fld[0] != "Z":
            e = dict(rc=-2)
        else:
            e = (orc.collect_digar_from_cs_tag if src == SRC_CS else orc.collect_digar_from_MD_tag)(a["pos0"], rec["cig"], bytes(fld[1]), a["qual"], *args)
    elif ref_seq is None:
        e = dict(rc=-2)
    else:
        e = orc.collect_digar_from_ref_seq(a["pos0"], rec["cig"], a["bseq"], a["qual"], ref_seq, ref_beg, ref_end, *args)
    return src, fl, e


# ---------------- the named SA cases ----------------
# A primary of `rlen` reference bases at 0-based P is [A, B] = [P + 1, P + rlen]; an entry `pos,<L counted bases>` ends at sa_end = pos + L (the reference adds the
# lengths to pos itself), so sa_len = L + 1.  `flag` below is worked out by hand from check_ont_palindrome's four assignments and overlap >= 0.9 * rlen; a
# palindromic forward read gets the RIGHT-clip flag (2), a reverse one (flag 16) the LEFT-clip flag (1).  {A} and {B} in `sa` are replaced per record.
#   name, rlen, BAM flag, is_ont, SA field (type, value) | None, expected flags, expected trace
SA_CASES = [
    ("containment",             1000, 0,  1, ("Z", "chrS,{A-10},-,1100M,60,0;"),                 2, [("contain", 1000)]),
    ("left_partial",            1000, 0,  1, ("Z", "chrS,{A-50},-,1000M,60,0;"),                 2, [("left_partial", 951)]),        # sa_end = A + 950
    ("left_partial_too_short",  1000, 0,  1, ("Z", "chrS,{A-500},-,1000M,60,0;"),                0, [("left_partial", 501)]),
    ("left_of_the_primary",     1000, 0,  1, ("Z", "chrS,{A-2000},-,100M,60,0;"),                0, [("left_none", 0)]),
    ("right_partial",           1000, 0,  1, ("Z", "chrS,{A+50},-,1000M,60,0;"),                 2, [("right_partial", 950)]),       # B - pos + 1
    ("inside",                  1000, 0,  1, ("Z", "chrS,{A+10},-,950M,60,0;"),                  2, [("inside", 951)]),              # sa_len
    ("right_of_the_primary",    1000, 0,  1, ("Z", "chrS,{B+1},-,1000M,60,0;"),                  0, [("right_none", 0)]),
    ("exactly_0.9_len_1000",    1000, 0,  1, ("Z", "chrS,{A+10},-,899M,60,0;"),                  2, [("inside", 900)]),              # 900 >= 1000 * 0.9 == 900.0
    ("one_short_len_1000",      1000, 0,  1, ("Z", "chrS,{A+10},-,898M,60,0;"),                  0, [("inside", 899)]),
    ("exactly_0.9_len_10",      10,   0,  1, ("Z", "chrS,{A+1},-,8M,60,0;"),                     2, [("right_partial", 9)]),         # sa_end = A + 9 = B; 9 >= 10 * 0.9 == 9.0
    ("one_short_len_10",        10,   0,  1, ("Z", "chrS,{A+2},-,8M,60,0;"),                     0, [("right_partial", 8)]),
    ("second_entry",            1000, 0,  1, ("Z", "chrS,{B+5000},+,100M,60,0;chrS,{A},-,1000M,60,0;"), 2, [("right_none", 0), ("contain", 1000)]),
    ("another_rname",           1000, 0,  1, ("Z", "chrOther,{A},-,1000M,60,1;"),                2, [("contain", 1000)]),
    ("plus_strand_entry",       1000, 0,  1, ("Z", "chrS,{A},+,1000M,60,1;"),                    2, [("contain", 1000)]),
    ("reverse_primary",         1000, 16, 1, ("Z", "chrS,{A},+,1000M,60,1;"),                    1, [("contain", 1000)]),
    ("ops_S_N_I_H_in_the_cigar", 1000, 16, 1, ("Z", "chrS,{A},-,100S500M300N200I400M50H,60,1;"), 1, [("left_partial", 901)]),        # 900 counted: N / I / S / H are not
    ("N_is_not_counted",        1000, 0,  1, ("Z", "chrS,{A},-,400M5000N400M,60,1;"),            0, [("left_partial", 801)]),        # (counting N would contain the primary)
    ("D_eq_X_are_counted",      1000, 0,  1, ("Z", "chrS,{A},-,300=1X300D1X300=,60,1;"),         2, [("left_partial", 903)]),
    ("letter_without_digits",   1000, 0,  1, ("Z", "chrS,{A},-,M500M=400M,60,1;"),               2, [("left_partial", 901)]),
    ("missing_cigar",           1000, 0,  1, ("Z", "chrS,{A},-;"),                               0, ["skipped"]),
    ("missing_strand_and_cigar", 1000, 0, 1, ("Z", "chrS,{A}"),                                  0, ["skipped"]),
    ("empty_rname",             1000, 0,  1, ("Z", ",{A},-,1000M,60,0"),                         0, ["skipped"]),
    ("pos_not_a_number_then_a_good_entry", 1000, 0, 1, ("Z", "chrS,abc,-,1000M;chrS,{A},-,1000M,60,0"), 2, ["skipped", ("contain", 1000)]),
    ("empty_pieces",            1000, 0,  1, ("Z", ";;chrS,{A},-,1000M,60,0;;"),                 2, ["empty", "empty", ("contain", 1000)]),
    ("SA_of_type_A",            1000, 0,  1, ("A", "x"),                                         0, "not_Z"),
    ("no_SA",                   1000, 0,  1, None,                                               0, "no_tag"),
    ("is_ont_0",                1000, 0,  0, ("Z", "chrS,{A-10},-,1100M,60,0;"),                 0, "not_ont"),
    ("forward_primary",         1000, 0,  1, ("Z", "chrS,{A-10},+,1100M,60,0;"),                 2, [("contain", 1000)]),
]


def sa_case_records():
    """the named cases as records on the shared reference, position order: 40S <rlen>= 40S (clips longer than end_clip_reg: a palindrome flag changes the digars),
    one planted mismatch in the long ones; case k is given as source class k % 4 -> [(case, record)]"""
    import re
    ref, _ = seeded()
    rng = np.random.default_rng(11)
    out = []
    for k, case in enumerate(SA_CASES):
        name, rlen, flag, is_ont, sa, want, trace = case
        P = 400 + 900 * k
        ops = [(4, 40, None)] + ([(7, 400, None), (8, 1, None), (7, rlen - 401, None)] if rlen > 500 else [(7, rlen, None)]) + [(4, 40, None)]
        a = build_on_ref(rng, ref, P, ops)
        a["qual"] = np.full(a["qlen"], 40, np.uint8); a["flag"] = flag; a["name"] = f"sa/{k}".encode()
        env = dict(A=P + 1, B=P + rlen)
        dz = decoys(rng)
        kind = k % 4
        f = dz[:5] + ([("cs", "Z", a["cs"])] if kind == 1 else [("MD", "Z", a["md"])] if kind == 2 else []) + dz[5:9]
        if sa is not None:
            val = re.sub(r"\{([^}]*)\}", lambda m: str(eval(m.group(1), {}, env)), sa[1]).encode()
            f.append(("SA", sa[0], val))
        f += dz[9:12]
        out.append((case, record(a, a["eqx"] if kind == 0 else a["mcig"], f)))
    assert 400 + 900 * len(SA_CASES) + 1100 < TLEN
    return out
