"""The per-haplotype CpG methylation table (lcd_chunk_mod_pileup, mods_kernel.hip) restated in Python from its rules, the records it is tested on, and a table of
named cases.  There is no reference implementation: this oracle is the specification's yardstick, and tests/test_mods_oracle.py checks it against tables worked
out by hand.

Conventions the rules leave open, fixed here and in include/lcd_hotpath.h alike:
  * positions p are 1-based, as the chunk's region [reg_beg, reg_end] and its reference window [ref_beg, ref_end] are; a row's text columns are start = p - 1 and
    end = p (combined rows: end = p + 1, the CpG's two bases);
  * a kept record is judged in this order: no MM -> n_no_mm; hard_clip; mn_mismatch; syntax (anywhere in the MM text); no wanted group -> n_no_group; overrun and
    ml_short (both on the wanted group; ml_short counts the bytes of the groups up to and including it);
  * an occurrence is judged in this order: unlisted under '?' -> nothing at all; not in an M / = / X op (or behind the CIGAR's last base) -> n_unaligned; p outside
    the region -> n_outside; no CpG site of the record's strand at p -> n_off_context; else one of the site's nine counters;
  * combine_strands: a row's key is the position of the CpG's C -- p for a '+' site, p - 1 for a '-' site -- and a chunk adds up what IT counted under each key.
    A CpG that straddles a region's end (C at reg_end, G at reg_end + 1) therefore gives one row in each of the two chunks, both with the key reg_end; whoever
    joins the rows of several chunks (merge_rows here, the same rule for any reader of several tables) adds rows of equal key.  Without combine_strands no key
    can repeat: regions are disjoint.
"""
import struct

import numpy as np

import bam_out_common as bo
from bam_src_common import aux_field, aux_walk, record, write_bam  # noqa: F401

NIB = "=ACMGRSVTWYHKDBN"
CODE_OF = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
STAT_KEYS = ("n_records", "n_no_mm", "n_no_group", "n_hard_clip", "n_mn_mismatch", "n_syntax", "n_overrun", "n_ml_short", "n_unaligned", "n_outside", "n_off_context",
             "n_counted")
HEADER = "#chrom\tstart\tend\tcode\tstrand\tn_all\tmod_all\tn_h1\tmod_h1\tn_h2\tmod_h2\tn_filtered\n"
MOD, CANON, FILT = 0, 1, 2


# ---------------- records ----------------
def pack_seq(s):
    n = [NIB.index(c) for c in s] + [0]
    return np.array([(n[i] << 4) | n[i + 1] for i in range(0, len(s), 2)], np.uint8)


def cigar_words(text):
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | "MIDNSHP=X".index(ch)); num = ""
    return out


def parse_body(body):
    refid, pos0, lname, mapq, _bin, ncig, flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    o = 32 + lname
    cig = struct.unpack("<%dI" % ncig, body[o:o + 4 * ncig]); o += 4 * ncig
    sq = body[o:o + (lseq + 1) // 2]; o += (lseq + 1) // 2 + lseq
    seq = [(sq[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(lseq)]
    return dict(pos0=pos0, mapq=mapq, flag=flag, lseq=lseq, cigar=[(w & 15, w >> 4) for w in cig], seq=seq, aux=body[o:])


def find_tags(aux):
    """-> (MM text | None, ML bytes | None, MN | None) by the rules 'Tags of a record'"""
    f = aux_walk(aux)
    mm = next((v for t, ty, v in f if t == b"MM" and ty == "Z"), None)
    if mm is None:
        mm = next((v for t, ty, v in f if t == b"Mm" and ty == "Z"), None)
    ml = next((v[5:] for t, ty, v in f if t == b"ML" and ty == "B" and v[:1] == b"C"), None)
    if ml is None:
        ml = next((v[5:] for t, ty, v in f if t == b"Ml" and ty == "B" and v[:1] == b"C"), None)
    mn = None
    for t, ty, v in f:
        if t == b"MN" and ty in "cCsSiI":
            mn = struct.unpack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I")[ty], v)[0]
            break
    return mm, ml, mn


def parse_mm(text):
    """-> [dict(base, strand, codes, chebi, flag, deltas)] or None for a syntax error"""
    groups, p, n = [], 0, len(text)
    t = text.decode("latin-1")
    while p < n:
        if t[p] not in "ACGTUN" or p + 1 >= n or t[p + 1] not in "+-":
            return None
        base, strand = t[p], t[p + 1]
        p += 2; q = p
        if p < n and "a" <= t[p] <= "z":
            while p < n and "a" <= t[p] <= "z":
                p += 1
            codes, chebi = list(t[q:p]), False
        elif p < n and "0" <= t[p] <= "9":
            while p < n and "0" <= t[p] <= "9":
                p += 1
            codes, chebi = [t[q:p]], True
        else:
            return None
        flag = ""
        if p < n and t[p] in ".?":
            flag = t[p]; p += 1
        deltas = []
        while p < n and t[p] == ",":
            p += 1; q = p
            while p < n and "0" <= t[p] <= "9":
                p += 1
            if p == q or p - q > 10:
                return None
            deltas.append(int(t[q:p]))
        if p >= n or t[p] != ";":
            return None
        p += 1
        groups.append(dict(base=base, strand=strand, codes=codes, chebi=chebi, flag=flag, deltas=deltas))
    return groups


def classify(v, s, T):
    return MOD if v >= T else CANON if 255 - min(s, 255) >= T else FILT


def record_calls(x, code="m", T=204):
    """one kept record -> (verdict, [(stored index, class, listed)], trace); verdict: 'ok' or the statistic the record falls into"""
    tr = {}
    mm, ml, mn = find_tags(x["aux"])
    tr["mm"], tr["ml"], tr["mn"] = mm, ml, mn
    if mm is None:
        return "n_no_mm", [], tr
    reasons = []
    if any(op == 5 for op, _ in x["cigar"]):
        reasons.append("n_hard_clip")
    if mn is not None and mn != x["lseq"]:
        reasons.append("n_mn_mismatch")
    groups = parse_mm(mm)
    if groups is None:
        reasons.append("n_syntax")
    want, ml_off = None, 0
    for g in groups or []:
        if g["base"] == "C" and g["strand"] == "+" and not g["chebi"] and code in g["codes"]:
            want = g
            break
        ml_off += len(g["codes"]) * len(g["deltas"])
    tr["ml_off"], tr["group"] = ml_off, want
    rev = bool(x["flag"] & 16)
    stored = 4 if rev else 2
    occ = [i for i, b in enumerate(x["seq"]) if b == stored]
    if rev:
        occ.reverse()
    called = []
    if want is not None:
        o = -1
        for d in want["deltas"]:
            o += d + 1
            called.append(o)
        if called and called[-1] >= len(occ):
            reasons.append("n_overrun")
        if len(ml or b"") < ml_off + len(want["codes"]) * len(want["deltas"]):
            reasons.append("n_ml_short")
    tr["reasons"], tr["called"], tr["n_occ"] = reasons, called, len(occ)
    if reasons:
        return reasons[0], [], tr
    if want is None:
        return "n_no_group", [], tr
    nc, ci = len(want["codes"]), want["codes"].index(code)
    cls = {}
    for k, o in enumerate(called):
        row = ml[ml_off + k * nc: ml_off + (k + 1) * nc]
        cls[o] = classify(row[ci], sum(row), T)
    calls = []
    for o, i in enumerate(occ):
        if o in cls:
            calls.append((i, cls[o], True))
        elif want["flag"] != "?":
            calls.append((i, CANON, False))
    return "ok", calls, tr


def ref_pos_of(x, i):
    """the 1-based reference position of stored base i, or None when it is not in an M / = / X op"""
    q, r = 0, x["pos0"] + 1
    for op, ln in x["cigar"]:
        cq, cr = op in (0, 1, 4, 7, 8), op in (0, 2, 3, 7, 8)
        if cq and q <= i < q + ln:
            return r + (i - q) if op in (0, 7, 8) else None
        q += ln if cq else 0
        r += ln if cr else 0
    return None


def pileup(bodies, ref, ref_beg, reg_beg, reg_end, haps, min_mapq=30, code="m", T=204, combine=False, trace=None, refid=0):
    """the table of one chunk: bodies = every record body of the file in order, ref = codes 0-4 with ref[0] at position ref_beg, haps per kept read of the chunk
    -> (rows [(key position, strand, nine counters hap-major: mod, canon, filtered)], stats dict)"""
    recs = bo.region_records(bodies, reg_beg, reg_end, min_mapq, refid)
    st = {k: 0 for k in STAT_KEYS}
    tab = {}
    at = lambda p: int(ref[p - ref_beg]) if ref_beg <= p < ref_beg + len(ref) else 4
    for body, r in recs:
        if r < 0:
            continue
        x = parse_body(body)
        st["n_records"] += 1
        verdict, calls, tr = record_calls(x, code, T)
        ev = []
        if verdict != "ok":
            st[verdict] += 1
        rev = bool(x["flag"] & 16)
        for i, c, listed in calls:
            p = ref_pos_of(x, i)
            if p is None:
                st["n_unaligned"] += 1; ev.append((i, "unaligned")); continue
            if not reg_beg <= p <= reg_end:
                st["n_outside"] += 1; ev.append((i, "outside")); continue
            site = (at(p) == 2 and at(p - 1) == 1) if rev else (at(p) == 1 and at(p + 1) == 2)
            if not site:
                st["n_off_context"] += 1; ev.append((i, "off_context")); continue
            st["n_counted"] += 1; ev.append((i, "counted", p, c, listed))
            tab.setdefault((p, "-" if rev else "+"), [0] * 9)[3 * int(haps[r]) + c] += 1
        if trace is not None:
            trace.append(dict(body=body, read=r, verdict=verdict, events=ev, **tr))
    rows = [(p, s, tuple(v)) for (p, s), v in sorted(tab.items())]
    return (combine_rows(rows) if combine else rows), st


def combine_rows(rows):
    out = {}
    for p, s, v in rows:
        k = p if s == "+" else p - 1
        out[k] = tuple(a + b for a, b in zip(out.get(k, (0,) * 9), v))
    return [(k, ".", v) for k, v in sorted(out.items())]


def merge_rows(tables):
    """the rows of several chunks in plan order as one table: rows of equal key and strand that meet at a boundary are added (combine_strands only)"""
    out = []
    for rows in tables:
        for p, s, v in rows:
            if out and out[-1][0] == p and out[-1][1] == s:
                out[-1] = (p, s, tuple(a + b for a, b in zip(out[-1][2], v)))
            else:
                out.append((p, s, tuple(v)))
    return out


def format_rows(rows, chrom, code="m"):
    """the data lines of the table (HEADER is written once per file)"""
    out = []
    for p, s, v in rows:
        n = [v[3 * h] + v[3 * h + 1] for h in range(3)]
        out.append("\t".join(str(a) for a in (chrom, p - 1, p + 1 if s == "." else p, code, s, sum(n), v[0] + v[3] + v[6], n[1], v[3], n[2], v[6], v[2] + v[5] + v[8])) + "\n")
    return "".join(out)


# ---------------- the case table ----------------
def mm_fields(mm=None, ml=None, mn=None, low=False):
    f = []
    if mm is not None:
        f.append(("Mm" if low else "MM", "Z", mm))
    if ml is not None:
        f.append(("Ml" if low else "ML", "B", ("C", list(ml))))
    if mn is not None:
        f.append(("MN", "i", mn))
    return f


def filler(n, cpg=(), c=()):
    """n bases of A / T with CG planted at every index of cpg and a lone C at every index of c"""
    s = [("A", "T", "T", "A", "T")[i % 5] for i in range(n)]
    for i in cpg:
        s[i], s[i + 1] = "C", "G"
    for i in c:
        s[i] = "C"
    return "".join(s)


def straddle_mm(n_calls, head=b"C+m", bounds=(64, 128)):
    """head + n_calls deltas of value 0, zero-padded to 10 digits wherever that makes a number straddle byte b of the text or byte b of the delta list, b in bounds"""
    t = bytearray(head)
    for _ in range(n_calls):
        o = len(t) + 1                                         # where the number starts
        w = 10 if any(o < b and len(head) + b <= o + 9 for b in bounds) else 1
        t += b"," + b"0" * w
    return bytes(t + b";")


def number_spans(mm):
    """[(first, last)] byte index of every number of the text's delta lists"""
    out, i = [], 0
    while i < len(mm):
        if mm[i:i + 1] == b"," and i + 1 < len(mm):
            j = i + 1
            while j < len(mm) and mm[j:j + 1].isdigit():
                j += 1
            out.append((i + 1, j - 1)); i = j
        else:
            i += 1
    return out


SLOT, FIRST_SLOT = 300, 990
REG_BEG = 1001


def _c(name, ref, seq=None, cigar=None, flag=0, mapq=60, fields=None, hap=1, off=0, rows=(), stats=None, pred=None, alt=None):
    seq = ref if seq is None else seq
    return dict(name=name, ref=ref, seq=seq, cigar=cigar or "%dM" % len(seq), flag=flag, mapq=mapq, fields=fields if fields is not None else [], hap=hap, off=off,
                rows=list(rows), stats=stats or {}, pred=pred, alt=alt or {})


def _verdict(v):
    return lambda t: t["verdict"] == v


def _reasons(*r):
    return lambda t: tuple(t["reasons"]) == r


def case_table():
    """[case]: one record each, `ref` written at the case's slot (slot k starts at 0-based FIRST_SLOT + SLOT * k), the record at slot + off.
    rows: what the record adds under the default options as (0-based offset of the position in the slot, strand, class); stats: what it adds to the statistics
    beside n_records; alt: {(code, T): rows} where other options change the rows; pred(trace entry) proves the condition is reached."""
    T = []
    cg3 = filler(40, cpg=(5, 15, 25))
    # -- the region's first position is the G of a CpG: a '-' site whose C lies outside
    e0 = "TTATTATTACGATTATTATT"
    T.append(_c("minus_site_at_reg_beg", e0, flag=16, fields=mm_fields(b"C+m,0;", [255]), hap=1, rows=[(10, "-", MOD)],
                pred=lambda t: t["events"] == [(10, "counted", REG_BEG, MOD, True)]))
    T.append(_c("plus_site_in_front_of_reg_beg", e0, fields=mm_fields(b"C+m,0;", [255]), hap=2, stats=dict(n_outside=1), pred=lambda t: t["events"] == [(9, "outside")]))
    T[-1]["same_slot"] = True
    # -- l_seq at the wave's width
    for n, cpg in ((63, (0, 30, 61)), (64, (0, 31, 62)), (65, (0, 63)), (129, (62, 63 + 1, 126 + 1))):
        s = filler(n, cpg=cpg)
        vals = [255, 0, 128][:len(cpg)]
        T.append(_c("lseq_%d" % n, s, fields=mm_fields(b"C+m" + b",0" * len(cpg) + b";", vals), hap=1 + n % 2, rows=[(p, "+", k) for k, p in enumerate(cpg)],
                    pred=lambda t, n=n: len(t["called"]) == t["n_occ"] and t["verdict"] == "ok"))
    s = filler(65, cpg=(0, 62))
    T.append(_c("lseq_65_reverse", s, flag=16, fields=mm_fields(b"C+m,0,0;", [255, 128]), hap=2, rows=[(63, "-", MOD), (1, "-", FILT)], pred=_verdict("ok")))
    # -- numbers across byte 64 and byte 128 of the text (and of the delta list)
    s = "CG" * 64 + "A"
    mm = straddle_mm(64)
    T.append(_c("numbers_straddle_64_128", s, fields=mm_fields(mm, [(255, 0, 128)[i % 3] for i in range(64)]), hap=2, rows=[(2 * i, "+", i % 3) for i in range(64)],
                pred=lambda t: all(any(a < b <= z for a, z in number_spans(t["mm"])) for b in (64, 67, 128, 131)) and len(t["called"]) == 64))
    # -- deltas
    T.append(_c("ten_digit_delta", cg3, fields=mm_fields(b"C+m,0,9999999999;", [255, 255]), stats=dict(n_overrun=1), pred=_reasons("n_overrun")))
    T.append(_c("delta_2_pow_32", cg3, fields=mm_fields(b"C+m,4294967296;", [255]), stats=dict(n_overrun=1), pred=_reasons("n_overrun")))
    T.append(_c("delta_0_run", cg3, fields=mm_fields(b"C+m,0,0,0;", [255, 255, 0]), hap=0, rows=[(5, "+", MOD), (15, "+", MOD), (25, "+", CANON)], pred=_verdict("ok")))
    T.append(_c("leading_zeros", cg3, fields=mm_fields(b"C+m,0000000001,000;", [255, 128]), hap=1, rows=[(5, "+", CANON), (15, "+", MOD), (25, "+", FILT)], pred=_verdict("ok")))
    # -- flags
    T.append(_c("flag_dot", cg3, fields=mm_fields(b"C+m.,1;", [255]), hap=1, rows=[(5, "+", CANON), (15, "+", MOD), (25, "+", CANON)], pred=lambda t: t["group"]["flag"] == "."))
    T.append(_c("flag_question", cg3, fields=mm_fields(b"C+m?,1;", [255]), hap=1, rows=[(15, "+", MOD)], pred=lambda t: t["group"]["flag"] == "?" and len(t["events"]) == 1))
    T.append(_c("flag_none", cg3, fields=mm_fields(b"C+m,1;", [128]), hap=2, rows=[(5, "+", CANON), (15, "+", FILT), (25, "+", CANON)], pred=lambda t: t["group"]["flag"] == ""))
    T.append(_c("empty_wanted_group", cg3, fields=mm_fields(b"C+m;", None), hap=2, rows=[(5, "+", CANON), (15, "+", CANON), (25, "+", CANON)], pred=lambda t: t["ml"] is None and t["verdict"] == "ok"))
    T.append(_c("empty_wanted_group_question", cg3, fields=mm_fields(b"C+m?;", []), hap=2, pred=lambda t: t["verdict"] == "ok" and not t["events"]))
    # -- code lists
    T.append(_c("mh_interleaved", cg3, fields=mm_fields(b"C+mh?,0,0;", [30, 220, 10, 20]), hap=1, rows=[(5, "+", FILT), (15, "+", CANON)],
                alt={("h", 204): [(5, "+", MOD), (15, "+", CANON)]}, pred=lambda t: len(t["group"]["codes"]) == 2))
    T.append(_c("h_then_m", cg3, fields=mm_fields(b"C+h,0,1;C+m,1;", [0, 0, 255]), hap=1, rows=[(5, "+", CANON), (15, "+", MOD), (25, "+", CANON)],
                alt={("h", 204): [(5, "+", CANON), (15, "+", CANON), (25, "+", CANON)]}, pred=lambda t: t["ml_off"] == 2))
    T.append(_c("m_then_h", cg3, fields=mm_fields(b"C+m,1;C+h,0,1;", [255, 0, 128]), hap=1, rows=[(5, "+", CANON), (15, "+", MOD), (25, "+", CANON)],
                alt={("h", 204): [(5, "+", CANON), (15, "+", CANON), (25, "+", FILT)]}, pred=lambda t: t["ml_off"] == 0))
    T.append(_c("other_groups_in_front", cg3, fields=mm_fields(b"G-m,0;C+76792,0,0;N+n?,0;C-m.,0;C+m,0;", [9, 9, 9, 9, 9, 255]), hap=2,
                rows=[(5, "+", MOD), (15, "+", CANON), (25, "+", CANON)], alt={("h", 204): []}, pred=lambda t: t["ml_off"] == 5))
    T.append(_c("second_matching_group_ignored", cg3, fields=mm_fields(b"C+m,0;C+m,1;", [255, 255]), hap=2, rows=[(5, "+", MOD), (15, "+", CANON), (25, "+", CANON)],
                alt={("h", 204): []}, pred=_verdict("ok")))
    # -- spellings
    T.append(_c("Mm_Ml", cg3, fields=mm_fields(b"C+m?,2;", [255], low=True), hap=1, rows=[(25, "+", MOD)], pred=lambda t: t["mm"] == b"C+m?,2;"))
    T.append(_c("MM_over_Mm", cg3, fields=[("Mm", "Z", b"C+m?,0;"), ("Ml", "B", ("C", [0])), ("MM", "i", 7), ("ML", "B", ("c", [1])), ("MM", "Z", b"C+m?,1;"), ("MM", "Z", b"C+m?,2;"),
                                         ("ML", "B", ("C", [255]))], hap=1, rows=[(15, "+", MOD)], pred=lambda t: t["mm"] == b"C+m?,1;" and bytes(t["ml"]) == b"\xff"))
    T.append(_c("field_past_the_record_hides_MM", cg3, fields=[(None, None, b"XBBi\xe8\x03\0\0\x01\0\0\0")] + mm_fields(b"C+m,0;", [255]), stats=dict(n_no_mm=1), pred=_verdict("n_no_mm")))
    # -- strands and the CIGAR
    T.append(_c("reverse_three_sites", cg3, flag=16, fields=mm_fields(b"C+m,0,1;", [255, 128]), hap=2, rows=[(26, "-", MOD), (16, "-", CANON), (6, "-", FILT)], pred=_verdict("ok")))
    r = "TTCAT" + filler(20, cpg=(8,)) + "ATCTT"
    T.append(_c("soft_clips", r[5:25], seq=r, cigar="5S20M5S", fields=mm_fields(b"C+m,0,0,0;", [255, 255, 255]), hap=1, rows=[(8, "+", MOD)], stats=dict(n_unaligned=2),
                pred=lambda t: [e[1] for e in t["events"]] == ["unaligned", "counted", "unaligned"]))
    T.append(_c("soft_clip_question_unlisted", r[5:25], seq=r, cigar="5S20M5S", fields=mm_fields(b"C+m?,1;", [0]), hap=1, rows=[(8, "+", CANON)], pred=lambda t: len(t["events"]) == 1))
    T.append(_c("call_in_insertion", "ATTATTATACGTTATTAT", seq="ATTATTATCGACGTTATTAT", cigar="8M2I10M", fields=mm_fields(b"C+m,0,0;", [255, 0]), hap=1, rows=[(9, "+", CANON)],
                stats=dict(n_unaligned=1), pred=lambda t: t["events"][0] == (8, "unaligned")))
    T.append(_c("deletion_takes_the_G", "ATTATTATCGTTATTAT", seq="ATTATTATCTTATTAT", cigar="9M1D7M", fields=mm_fields(b"C+m,0;", [255]), hap=2, rows=[(8, "+", MOD)], pred=_verdict("ok")))
    T.append(_c("C_over_non_CpG", "ATTATTATCATTATTAT", fields=mm_fields(b"C+m,0;", [255]), stats=dict(n_off_context=1), pred=lambda t: t["events"] == [(8, "off_context")]))
    T.append(_c("forward_C_over_minus_site", "ATTATTATCGTTATTAT", seq="ATTATTATCCTTATTAT", fields=mm_fields(b"C+m,0,0;", [255, 255]), hap=1, rows=[(8, "+", MOD)],
                stats=dict(n_off_context=1), pred=lambda t: t["events"][1] == (9, "off_context")))
    T.append(_c("ambiguity_codes_match_nothing", "ATSATMATCGTT=TTAT".replace("S", "C").replace("M", "C").replace("=", "C"), seq="ATSATMATCGTT=TTAT", fields=mm_fields(b"C+m,0;", [255]), hap=1,
                rows=[(8, "+", MOD)], pred=lambda t: t["n_occ"] == 1))
    T.append(_c("N_cigar_skip", "ATCGT" + "TTTTT" + "ACGAT", seq="ATCGTACGAT", cigar="5M5N5M", fields=mm_fields(b"C+m,0,0;", [255, 128]), hap=1, rows=[(2, "+", MOD), (11, "+", FILT)], pred=_verdict("ok")))
    both = "ATTATTATCGTTATTAT"
    T.append(_c("both_strands_forward", both, fields=mm_fields(b"C+m,0;", [255]), hap=1, rows=[(8, "+", MOD)], pred=_verdict("ok")))
    T.append(_c("both_strands_reverse", both, flag=16, fields=mm_fields(b"C+m,0;", [0]), hap=2, rows=[(9, "-", CANON)], pred=_verdict("ok")))
    T[-1]["same_slot"] = True
    # -- thresholds
    six = filler(70, cpg=(5, 15, 25, 35, 45, 55))
    T.append(_c("threshold_values", six, fields=mm_fields(b"C+m,0,0,0,0,0,0;", [128, 127, 255, 254, 0, 1]), hap=1,
                rows=[(5, "+", FILT), (15, "+", FILT), (25, "+", MOD), (35, "+", MOD), (45, "+", CANON), (55, "+", CANON)],
                alt={("m", 128): [(5, "+", MOD), (15, "+", CANON), (25, "+", MOD), (35, "+", MOD), (45, "+", CANON), (55, "+", CANON)],
                     ("m", 255): [(5, "+", FILT), (15, "+", FILT), (25, "+", MOD), (35, "+", FILT), (45, "+", CANON), (55, "+", FILT)]}, pred=_verdict("ok")))
    T.append(_c("v_equals_T", six, fields=mm_fields(b"C+m?,0,0,0,0;", [204, 203, 51, 52]), hap=2, rows=[(5, "+", MOD), (15, "+", FILT), (25, "+", CANON), (35, "+", FILT)],
                alt={("m", 128): [(5, "+", MOD), (15, "+", MOD), (25, "+", CANON), (35, "+", CANON)], ("m", 255): [(5, "+", FILT), (15, "+", FILT), (25, "+", FILT), (35, "+", FILT)]},
                pred=_verdict("ok")))
    T.append(_c("sum_saturates", cg3, fields=mm_fields(b"C+mh?,0;", [200, 200]), hap=1, rows=[(5, "+", FILT)], alt={("h", 204): [(5, "+", FILT)], ("m", 128): [(5, "+", MOD)]},
                pred=lambda t: sum(t["ml"]) > 255))
    # -- bad records
    bad = lambda name, why, **kw: T.append(_c(name, cg3, stats={why[0]: 1}, pred=_reasons(*why), **kw))
    bad("hard_clip", ("n_hard_clip",), cigar="2H40M", fields=mm_fields(b"C+m,0;", [255]))
    bad("mn_mismatch", ("n_mn_mismatch",), fields=mm_fields(b"C+m,0;", [255], mn=41))
    T.append(_c("mn_equal", cg3, fields=mm_fields(b"C+m?,0;", [255], mn=40), hap=1, rows=[(5, "+", MOD)], pred=lambda t: t["mn"] == 40))
    for k, txt in enumerate((b"C+m,;", b"C+m,,1;", b"C+m,0", b"X+m;", b"C*m;", b"C+M;", b"C+m,12345678901;", b"C+;", b"C+m.?;", b"C+m5;", b"C+m,0;C", b"C+m,0;;", b"C+m,0;C+h, 1;", b"C+m,1a;",
                             b"c+m;", b"C+m;" + b"A+a" + b",0" * 40 + b",x;")):
        bad("syntax_%d" % k, ("n_syntax",), fields=mm_fields(txt, [255] * 4))
    bad("overrun", ("n_overrun",), fields=mm_fields(b"C+m,3;", [255]))
    bad("overrun_reverse", ("n_overrun",), flag=16, fields=mm_fields(b"C+m,1,1;", [255, 255]))
    bad("ml_short", ("n_ml_short",), fields=mm_fields(b"C+m,0,0;", [255]))
    bad("ml_missing", ("n_ml_short",), fields=mm_fields(b"C+m,0;", None))
    bad("ml_short_by_earlier_groups", ("n_ml_short",), fields=mm_fields(b"C+h,0,0;C+m;", [1]))
    bad("ml_signed_is_not_ML", ("n_ml_short",), fields=[("MM", "Z", b"C+m,0;"), ("ML", "B", ("c", [1]))])
    bad("hard_clip_before_mn", ("n_hard_clip", "n_mn_mismatch"), cigar="40M3H", fields=mm_fields(b"C+m,0;", [255], mn=7))
    bad("mn_before_syntax", ("n_mn_mismatch", "n_syntax"), fields=mm_fields(b"C+m,", [255], mn=39))
    bad("syntax_before_overrun", ("n_syntax",), fields=mm_fields(b"C+m,9;C+h,z;", [255]))   # (its first group alone is an overrun: a bad text is never walked)
    bad("overrun_before_ml_short", ("n_overrun", "n_ml_short"), fields=mm_fields(b"C+m,0,7;", [255]))
    T.append(_c("no_mm", cg3, fields=[("RG", "Z", b"grp")], stats=dict(n_no_mm=1), pred=_verdict("n_no_mm")))
    T.append(_c("no_mm_hard_clip", cg3, cigar="1H40M", stats=dict(n_no_mm=1), pred=_verdict("n_no_mm")))
    T.append(_c("empty_mm", cg3, fields=mm_fields(b"", []), stats=dict(n_no_group=1), pred=_verdict("n_no_group")))
    T.append(_c("no_wanted_group", cg3, fields=mm_fields(b"A+a,0;C-m,0;C+h,0;", [1, 2, 128]), stats=dict(n_no_group=1), alt={("h", 204): [(5, "+", FILT), (15, "+", CANON), (25, "+", CANON)]},
                pred=_verdict("n_no_group")))
    T.append(_c("filtered_flag", cg3, flag=0x100, fields=mm_fields(b"C+m,0;", [255]), pred=None))
    T.append(_c("filtered_mapq", cg3, mapq=3, fields=mm_fields(b"C+m,0;", [255]), pred=None))
    # -- the region's last position is the C of a CpG
    T.append(_c("plus_site_at_reg_end", e0, fields=mm_fields(b"C+m,0;", [255]), hap=1, rows=[(9, "+", MOD)], pred=lambda t: t["events"][0][1] == "counted"))
    T.append(_c("minus_site_behind_reg_end", e0, flag=16, fields=mm_fields(b"C+m,0;", [255]), hap=2, stats=dict(n_outside=1), pred=lambda t: t["events"] == [(10, "outside")]))
    T[-1]["same_slot"] = True
    return T


OPTION_SETS = (("m", 204, False), ("h", 204, False), ("m", 128, False), ("m", 255, False), ("m", 204, True))


def build_cases():
    """-> dict(cases, bodies, recs (for write_bam), ref codes (ref[0] = position 1), reg_beg, reg_end, haps per kept read, tlen)"""
    cases = case_table()
    slot = -1
    for c in cases:
        if not c.get("same_slot"):
            slot += 1
        c["slot0"] = FIRST_SLOT + SLOT * slot
    tlen = cases[-1]["slot0"] + 1000
    rng = np.random.default_rng(5)
    ref = np.where(rng.integers(0, 2, tlen) == 0, 0, 3).astype(np.uint8)           # A / T only: every C and G of the reference is planted by a case
    recs, haps = [], []
    for i, c in enumerate(cases):
        s0 = c["slot0"]
        ref[s0:s0 + len(c["ref"])] = [CODE_OF[b] for b in c["ref"]]
        a = dict(name=b"case%02d" % i, pos0=s0 + c["off"], flag=c["flag"], qlen=len(c["seq"]), bseq=pack_seq(c["seq"]), qual=np.full(len(c["seq"]), 30, np.uint8))
        recs.append(record(a, cigar_words(c["cigar"]), c["fields"], mapq=c["mapq"]))
        if not (c["flag"] & 0x904) and c["mapq"] >= 30:
            haps.append(c["hap"])
    reg_end = cases[-1]["slot0"] + 10                                              # 1-based position of the last slot's C
    assert cases[0]["slot0"] + 11 == REG_BEG
    return dict(cases=cases, bodies=[r["body"] for r in recs], recs=recs, ref=ref, reg_beg=REG_BEG, reg_end=reg_end, haps=haps, tlen=tlen)


def expected_by_hand(cases):
    """the table and the statistics the cases' hand-written rows add up to under the default options"""
    tab, st = {}, {k: 0 for k in STAT_KEYS}
    for c in cases:
        if (c["flag"] & 0x904) or c["mapq"] < 30:
            continue
        st["n_records"] += 1
        for k, v in c["stats"].items():
            st[k] += v
        for off, s, cl in c["rows"]:
            tab.setdefault((c["slot0"] + off + 1, s), [0] * 9)[3 * c["hap"] + cl] += 1
            st["n_counted"] += 1
    return [(p, s, tuple(v)) for (p, s), v in sorted(tab.items())], st


def expected_alt(cases, code, T):
    """under other options: the hand-written rows of the cases that name them -> (rows, [(first, last) position of those cases' slots])"""
    tab, spans = {}, []
    for c in cases:
        if (code, T) not in c["alt"]:
            continue
        spans.append((c["slot0"] + 1, c["slot0"] + SLOT))
        for off, s, cl in c["alt"][(code, T)]:
            tab.setdefault((c["slot0"] + off + 1, s), [0] * 9)[3 * c["hap"] + cl] += 1
    return [(p, s, tuple(v)) for (p, s), v in sorted(tab.items())], spans


# ---------------- a seeded chunk ----------------
def seeded(seed=11, n_reads=200, span=6000, first=2000):
    """reads of 0.3 - 3 kb over a window with planted CpGs, both strands, three haps, mixed flags and every kind of record -> dict as build_cases gives"""
    rng = np.random.default_rng(seed)
    tlen = first + span + 4000
    ref = rng.choice(np.array([0, 3], np.uint8), tlen, p=[0.5, 0.5])
    for p in rng.choice(np.arange(100, tlen - 100, 7), 500, replace=False):
        ref[p], ref[p + 1] = 1, 2
    for p in rng.choice(np.arange(100, tlen - 100), 300, replace=False):
        if ref[p - 1] != 1 and ref[p + 1] != 2:
            ref[p] = rng.choice([1, 2])
    starts = np.sort(rng.integers(first - 1500, first + span, n_reads))
    recs, haps = [], []
    for i, p0 in enumerate(starts):
        p0 = int(p0); ln = int(rng.integers(300, 3001)); ln = min(ln, tlen - p0 - 10)
        seq, cig, r = [], [], p0
        if rng.random() < 0.3:
            k = int(rng.integers(1, 40)); seq += list(rng.integers(0, 4, k)); cig.append((k << 4) | 4)
        while r < p0 + ln:
            m = int(min(rng.integers(1, 200), p0 + ln - r))
            blk = ref[r:r + m].copy()
            mut = rng.random(m) < 0.02
            blk[mut] = rng.integers(0, 4, int(mut.sum()))
            seq += list(blk); cig.append((m << 4) | int(rng.choice([0, 7, 8], p=[0.8, 0.15, 0.05]))); r += m
            x = rng.random()
            if x < 0.3:
                k = int(rng.integers(1, 6)); seq += list(rng.integers(0, 4, k)); cig.append((k << 4) | 1)
            elif x < 0.6 and r + 8 < p0 + ln:
                k = int(rng.integers(1, 6)); cig.append((k << 4) | 2); r += k
        if rng.random() < 0.3:
            k = int(rng.integers(1, 40)); seq += list(rng.integers(0, 4, k)); cig.append((k << 4) | 4)
        s = "".join("ACGT"[b] for b in seq)
        rev = bool(rng.random() < 0.5)
        flag = (16 if rev else 0) | (0x100 if rng.random() < 0.04 else 0)
        n_occ = s.count("G" if rev else "C")
        kind = rng.random()
        fields = [("RG", "Z", b"g1"), ("NM", "i", 3)]
        if kind < 0.06 or n_occ == 0:
            pass
        else:
            nc = 2 if rng.random() < 0.4 else 1
            gaps, left = [], n_occ
            while left > 0:
                d = int(rng.choice([0, 0, 0, 1, 2, 11, 150]))
                if d + 1 > left:
                    break
                gaps.append(d); left -= d + 1
            fl = (b"", b".", b"?")[int(rng.integers(0, 3))]
            txt = (b"C+mh" if nc == 2 else b"C+m") + fl + b"".join(b",%d" % d for d in gaps) + b";"
            ml = []
            for _ in gaps:
                v = int(rng.choice([0, 3, 60, 128, 203, 204, 250, 255]))
                ml += [v, int(rng.integers(0, 256 - v))] if nc == 2 else [v]
            pre, n_pre = b"", 0
            if rng.random() < 0.3:
                pre, n_pre = b"A+a,0;", 1
            if kind < 0.10:
                txt = txt[:-1] + b",99999;"; ml += [1] * nc
            elif kind < 0.13:
                ml = ml[:-1]
            elif kind < 0.16:
                txt = txt[:-1]
            fields += [("MM", "Z", pre + txt), ("ML", "B", ("C", [7] * n_pre + ml))]
            if rng.random() < 0.3:
                fields.append(("MN", "i", len(s) + (1 if kind > 0.97 else 0)))
        a = dict(name=b"sd%03d" % i, pos0=p0, flag=flag, qlen=len(s), bseq=pack_seq(s), qual=np.full(len(s), 30, np.uint8))
        recs.append(record(a, cig, fields, mapq=60 if rng.random() > 0.04 else 5))
    return dict(bodies=[r["body"] for r in recs], recs=recs, ref=ref, tlen=tlen, first=first, span=span, rng=rng)


def haps_for(bodies, reg_beg, reg_end, seed, min_mapq=30):
    """a hap 0 / 1 / 2 per kept read of the region, fixed by the read's position in the file and the seed"""
    recs = bo.region_records(bodies, reg_beg, reg_end, min_mapq)
    idx = {id(b): i for i, b in enumerate(bodies)}
    return [int((idx[id(b)] * 7 + seed) % 3) for b, r in recs if r >= 0]


# ---------------- whole files ----------------
def add_calls(rng, read):
    """MM / ML for a read of call_file_common's kind (pos0, cigar, bseq, qual, is_rev): most occurrences of the base called, a few skipped -> the read with its aux bytes"""
    n = len(read["qual"])
    sq = np.asarray(read["bseq"], np.uint8)
    nib = [(int(sq[i >> 1]) >> (0 if i & 1 else 4)) & 15 for i in range(n)]
    n_occ = sum(1 for b in nib if b == (4 if read["is_rev"] else 2))
    gaps, left = [], n_occ
    while left > 0:
        d = int(rng.choice([0, 0, 0, 0, 1, 3]))
        if d + 1 > left:
            break
        gaps.append(d); left -= d + 1
    ml = [int(x) for x in rng.choice([0, 10, 128, 230, 255], len(gaps))]
    fl = (b"", b".", b"?")[int(rng.integers(0, 3))]
    return dict(read, aux=aux_field("MM", "Z", b"C+m" + fl + b"".join(b",%d" % d for d in gaps) + b";") + aux_field("ML", "B", ("C", ml)) + aux_field("MN", "i", n))


def write_multi_bam_aux(path, contigs, header_text=b"@HD\tVN:1.6\tSO:coordinate\n", block=30000):
    """call_file_common.write_multi_bam for reads that carry auxiliary bytes (read["aux"]) -> the record bodies in file order"""
    from test_io import _bgzf, _write_bai
    d = b"BAM\x01" + struct.pack("<i", len(header_text)) + header_text + struct.pack("<i", len(contigs))
    for nm, ln, _ in contigs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    recs, bodies = [], []
    for tid, (nm, _ln, reads) in enumerate(contigs):
        for i, r in enumerate(reads):
            name = f"{nm}_r{i}".encode() + b"\0"
            cig = np.asarray(r["cigar"], "<u4"); qlen = len(r["qual"])
            body = struct.pack("<iiBBHHHiiii", tid, r["pos0"], len(name), 60, 4680, len(cig), 16 if r["is_rev"] else 0, qlen, -1, -1, 0) + name + cig.tobytes() + \
                np.asarray(r["bseq"], np.uint8).tobytes() + np.asarray(r["qual"], np.uint8).tobytes() + r.get("aux", b"")
            u0 = len(d)
            d += struct.pack("<i", len(body)) + body
            rl = sum(int(c) >> 4 for c in cig if (int(c) & 0xf) in (0, 2, 3, 7, 8))
            recs.append(dict(tid=tid, pos=r["pos0"], end=r["pos0"] + max(rl, 1), u0=u0, u1=len(d))); bodies.append(body)
    coffs = []
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    coffs.append(coffs[-1] + 1)
    for x in recs:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", len(contigs), recs)
    return bodies


def parse_table(text):
    """the table's text -> [(chrom, start, end, code, strand, n_all, mod_all, n_h1, mod_h1, n_h2, mod_h2, n_filtered)]"""
    lines = text.split("\n")
    assert lines[0] + "\n" == HEADER and lines[-1] == ""
    return [tuple(c if k in (0, 3, 4) else int(c) for k, c in enumerate(ln.split("\t"))) for ln in lines[1:-1]]
