"""Haplotagging against a phased VCF (lcd_phased_vcf_read, lcd_chunk_haplotag; haplotag_kernel.hip) restated in Python from its rules (include/lcd_hotpath.h).  There
is no reference implementation: the rules are the project's.
  * read_vcf: the reader's line rules, the normalisation, the phase sets and the per-contig tables; dump(): the text both this reader and the stand-alone C program
    (tests/c/haplotag_vcf_sanitize.cpp) print;
  * haplotag(): candidates, pairs, verdicts and votes.  The verdict is written PER POSITION from the expanded operation list (every reference position knows what
    lies on it, every boundary which insertions), not per operation as the kernel does it;
  * a table of named cases on one contig, each with the predicate that proves it reaches the condition it is named for;
  * a diploid simulator: het SNV / INS / DEL sites planted on two haplotypes of a random reference, reads with exact CIGARs from either haplotype.
Conventions: positions are 1-based; kinds 0 SNV, 1 INS, 2 DEL; verdicts NONE REF ALT OTHER LOWQ = 0 .. 4, 255 = a candidate that is no pair."""
import gzip
import io
import struct

import numpy as np

import bam_out_common as bo
import depth_common as dc
from bam_src_common import CONTIG, record, write_bam  # noqa: F401
from depth_common import D, EQ, H, I, M, N, P, S, X  # noqa: F401

NONE, REF, ALT, OTHER, LOWQ, NO_PAIR = 0, 1, 2, 3, 4, 255
SNV, INS, DEL = 0, 1, 2
NT16 = "=ACMGRSVTWYHKDBN"
VCF_STAT_KEYS = ("n_lines", "n_sites", "n_unknown_contig", "n_filtered", "n_unphased", "n_hom", "n_other_gt", "n_both_alt", "n_symbolic", "n_complex", "n_long_indel",
                 "n_indel_off", "n_snv", "n_ins", "n_del", "n_phase_sets")
TAG_STAT_KEYS = ("n_records", "n_pairs", "n_verdict", "n_tagged", "n_multi_ps", "n_cg", "n_bad_record", "n_no_seq")


class VcfError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


# ---------------- the reader ----------------
def _number(s):
    """all digits, 1 ... 18 of them -> int | None"""
    return int(s) if 1 <= len(s) <= 18 and all(48 <= c <= 57 for c in s) else None


def _plain(s):
    u = s.upper()
    return u if u and all(c in b"ACGTN" for c in u) else None


def vcf_bytes(path):
    """the file's text; gzip / BGZF by the magic bytes.  A member cut short is VcfError(-30)"""
    raw = open(path, "rb").read()
    if raw[:2] != b"\x1f\x8b":
        return raw
    try:
        return gzip.GzipFile(fileobj=io.BytesIO(raw)).read()
    except (EOFError, OSError, gzip.BadGzipFile) as e:
        raise VcfError(-30, "read error: %s" % e)


def read_vcf(text, names, sample=None, max_indel=50, snvs_only=False):
    """-> (tables: one dict of lists per contig of `names`, stats)"""
    st = dict.fromkeys(VCF_STAT_KEYS, 0)
    if max_indel < 1:
        raise VcfError(-4, "max_indel")
    names = [n.encode() if isinstance(n, str) else n for n in names]
    sites = [[] for _ in names]
    n_head, col_s = 0, -1
    for ln, line in enumerate(text.split(b"\n"), 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        if line[:1] == b"#":
            if line == b"#CHROM" or line.startswith(b"#CHROM\t"):
                head = line.split(b"\t")
                n_head = len(head)
                if n_head < 10:
                    raise VcfError(-4, "line %d: no sample column" % ln)
                col_s = 9
                if sample is not None:
                    want = sample.encode() if isinstance(sample, str) else sample
                    if want not in head[9:]:
                        raise VcfError(-4, "no sample")
                    col_s = 9 + head[9:].index(want)
            continue
        if col_s < 0:
            raise VcfError(-4, "line %d: a data line in front of the #CHROM line" % ln)
        col = line.split(b"\t")
        if len(col) < n_head:
            raise VcfError(-4, "line %d has %d columns" % (ln, len(col)))
        pos = _number(col[1])
        if pos is None or pos < 1:
            raise VcfError(-4, "line %d: POS" % ln)
        st["n_lines"] += 1

        def out(key):
            st[key] += 1

        if col[0] not in names:
            out("n_unknown_contig"); continue
        tid = names.index(col[0])
        if col[6] not in (b"PASS", b"."):
            out("n_filtered"); continue
        fmt, smp = col[8].split(b":"), col[col_s].split(b":")
        if fmt[0] != b"GT":
            out("n_other_gt"); continue
        if b"/" in smp[0]:
            out("n_unphased"); continue
        gt = smp[0].split(b"|")
        ab = [_number(g) for g in gt]
        if len(gt) != 2 or None in ab:
            out("n_other_gt"); continue
        a, b = ab
        if a == b:
            out("n_hom"); continue
        alts = col[4].split(b",")
        if max(a, b) > len(alts):
            out("n_other_gt"); continue
        if (a == 0) == (b == 0):
            out("n_both_alt"); continue
        r, al = _plain(col[3]), _plain(alts[(a or b) - 1])
        if r is None or al is None:
            out("n_symbolic"); continue
        while len(r) > 1 and len(al) > 1 and r[-1] == al[-1]:
            r, al = r[:-1], al[:-1]
        while len(r) > 1 and len(al) > 1 and r[0] == al[0]:
            r, al, pos = r[1:], al[1:], pos + 1
        s = dict(pos=pos, hap=1 if a else 2, len=1, ref_code=0, alt_code=0, ins=b"", ps=0)
        if len(r) == 1 and len(al) == 1 and r != al:
            s.update(kind=SNV, ref_code=NT16.index(chr(r[0])), alt_code=NT16.index(chr(al[0])))
        elif len(r) == 1 and len(al) > 1 and r[0] == al[0]:
            s.update(kind=INS, ins=al[1:], len=len(al) - 1)
        elif len(al) == 1 and len(r) > 1 and r[0] == al[0]:
            s.update(kind=DEL, len=len(r) - 1)
        else:
            out("n_complex"); continue
        if s["kind"] != SNV:
            if s["len"] > max_indel:
                out("n_long_indel"); continue
            if snvs_only:
                out("n_indel_off"); continue
        if b"PS" in fmt[1:] and 1 + fmt[1:].index(b"PS") < len(smp):
            v = _number(smp[1 + fmt[1:].index(b"PS")])
            if v is not None and v > 0:
                s["ps"] = v
        st["n_sites"] += 1
        st[("n_snv", "n_ins", "n_del")[s["kind"]]] += 1
        sites[tid].append(s)
    if col_s < 0:
        raise VcfError(-4, "no #CHROM line")
    tables = []
    for lst in sites:
        lst = sorted(lst, key=lambda s: s["pos"])                               # (stable)
        wide = next((s["pos"] for s in lst if not s["ps"]), 0)
        t = dict(pos=[], kind=[], hap_of_alt=[], len=[], ref_code=[], alt_code=[], ins_off=[], ps_idx=[], ps_value=[], pool=[], max_footprint=0)
        for s in lst:
            ps = s["ps"] or wide
            if ps not in t["ps_value"]:
                t["ps_value"].append(ps)
            t["pos"].append(s["pos"]); t["kind"].append(s["kind"]); t["hap_of_alt"].append(s["hap"]); t["len"].append(s["len"])
            t["ref_code"].append(s["ref_code"]); t["alt_code"].append(s["alt_code"]); t["ps_idx"].append(t["ps_value"].index(ps))
            t["ins_off"].append(len(t["pool"]) if s["kind"] == INS else 0)
            t["pool"] += [NT16.index(chr(c)) for c in s["ins"]]
            t["max_footprint"] = max(t["max_footprint"], (1, 2, s["len"] + 1)[s["kind"]])
        st["n_phase_sets"] += len(t["ps_value"])
        tables.append(t)
    return tables, st


TABLE_KEYS = ("pos", "kind", "hap_of_alt", "len", "ref_code", "alt_code", "ins_off", "ps_idx")


def dump(tables, st):
    """the text of the tables and the statistics: what tests/c/haplotag_vcf_sanitize.cpp prints"""
    out = ["stats " + " ".join(str(st[k]) for k in VCF_STAT_KEYS)]
    for c, t in enumerate(tables):
        out.append("contig %d sites %d sets %d pool %d max_footprint %d" % (c, len(t["pos"]), len(t["ps_value"]), len(t["pool"]), t["max_footprint"]))
        out += [" ".join(str(int(t[k][i])) for k in TABLE_KEYS) for i in range(len(t["pos"]))]
        out.append("ps" + "".join(" %d" % int(v) for v in t["ps_value"]))
        out.append("pool " + "".join(NT16[int(c)] for c in t["pool"]))
    return "\n".join(out) + "\n"


def table_of_lib(a):
    """PhasedVcf.sites() -> the same dict of lists"""
    t = {k: [int(v) for v in a[k]] for k in TABLE_KEYS + ("ps_value", "pool")}
    t["max_footprint"] = int(a["max_footprint"])
    return t


# ---------------- verdicts and votes ----------------
def footprint(t, s):
    p, k = t["pos"][s], t["kind"][s]
    return p, (p, p + 1, p + t["len"][s])[k]


def expand(pos1, ops):
    """the operation list per position: on[p] = ('M', base index) | (D or N, op index); ins[r] = [(length, first base index)] of the I operations at the boundary
    r - 1 | r; span[k] = (first position, length) of D / N operation k; -> on, ins, span, end"""
    on, ins, span = {}, {}, {}
    p, q = pos1, 0
    for k, (op, ln) in enumerate(ops):
        if ln == 0:
            continue
        if op in (M, EQ, X):
            for e in range(ln):
                on[p + e] = ("M", q + e)
            p += ln; q += ln
        elif op in (D, N):
            for e in range(ln):
                on[p + e] = (op, k)
            span[k] = (p, ln); p += ln
        elif op == I:
            ins.setdefault(p, []).append((ln, q)); q += ln
        elif op == S:
            q += ln
    return on, ins, span, p - 1


def record_fields(body):
    """-> dict(pos1, ops | None (broken layout), cg, lseq, code(q), qual(q))"""
    refid, pos0, lname, _mapq, _bin, ncig, _flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    pos1, ops, cg = dc.record_ops(body)
    o = 32 + lname + 4 * ncig
    return dict(pos1=pos1, ops=ops, cg=cg, lseq=lseq, code=lambda q: (body[o + (q >> 1)] >> (0 if q & 1 else 4)) & 15, qual=lambda q: body[o + (lseq + 1) // 2 + q])


def pair_verdict(t, s, rec, x, min_bq):
    """the verdict of site s for a record (record_fields) with the expansion x of its operations"""
    on, ins, span, end = x
    beg = rec["pos1"]
    pos, kind, ln = t["pos"][s], t["kind"][s], t["len"][s]
    fb, fe = footprint(t, s)
    if fe < beg or fb > end:
        return NO_PAIR
    if fb < beg or fe > end:
        return NONE
    disturbed = alt = False
    for p in range(fb, fe + 1):
        what = on[p]
        if what[0] != "M":
            own = kind == DEL and what[0] == D and span[what[1]] == (pos + 1, ln)
            alt, disturbed = alt or own, disturbed or not own
    for r in range(fb + 1, fe + 1):
        for iln, q in ins.get(r, ()):
            own = kind == INS and r == pos + 1 and iln == ln and q + iln <= rec["lseq"] and \
                [rec["code"](q + e) for e in range(iln)] == t["pool"][t["ins_off"][s]:t["ins_off"][s] + ln]
            alt, disturbed = alt or own, disturbed or not own
    if disturbed:
        return OTHER
    if alt:
        return ALT
    if kind != SNV:
        return REF
    q = on[pos][1]
    if q >= rec["lseq"]:
        return OTHER
    if rec["qual"](q) < min_bq:
        return LOWQ
    c = rec["code"](q)
    return ALT if c == t["alt_code"][s] else REF if c == t["ref_code"][s] else OTHER


def tag_record(t, body, min_bq=0, min_diff=1):
    """-> dict(hap, ps, n1, n2, first (first candidate), verdicts (per candidate), n_sets, bad, cg, no_seq)"""
    rec = record_fields(body)
    out = dict(hap=0, ps=0, n1=0, n2=0, first=0, verdicts=[], n_sets=0, bad=rec["ops"] is None, cg=bool(rec["cg"]), no_seq=False)
    if out["bad"]:
        return out
    out["no_seq"] = rec["lseq"] == 0
    x = expand(rec["pos1"], rec["ops"])
    beg, end = rec["pos1"], x[3]
    if end < beg:
        return out
    cand = [s for s in range(len(t["pos"])) if beg - (t["max_footprint"] - 1) <= t["pos"][s] <= end]
    out["first"] = cand[0] if cand else int(np.searchsorted(np.asarray(t["pos"], np.int64), beg - (t["max_footprint"] - 1))) if t["pos"] else 0
    out["verdicts"] = [pair_verdict(t, s, rec, x, min_bq) for s in cand]
    votes = {}                                                                  # ps_idx -> [n1, n2, first voting candidate]
    for k, (s, v) in enumerate(zip(cand, out["verdicts"])):
        if v in (REF, ALT):
            h = t["hap_of_alt"][s] if v == ALT else 3 - t["hap_of_alt"][s]
            e = votes.setdefault(t["ps_idx"][s], [0, 0, k])
            e[h - 1] += 1
    out["n_sets"] = len(votes)
    if votes:
        ps = min(votes, key=lambda k: (-(votes[k][0] + votes[k][1]), votes[k][2]))
        out["n1"], out["n2"] = votes[ps][:2]
        out["hap"] = 1 if out["n1"] - out["n2"] >= min_diff else 2 if out["n2"] - out["n1"] >= min_diff else 0
        out["ps"] = t["ps_value"][ps] if out["hap"] else 0
    return out


def haplotag(t, bodies, reg_beg, reg_end, min_bq=0, min_diff=1, min_mapq=30, refid=0):
    """the chunk of region [reg_beg, reg_end] -> dict(haps, phase_sets, n1, n2 per kept read; first_site, cand_off, verdict per kept record; stats; recs: the
    per-record dicts)"""
    assert min_diff >= 1
    st = dict(n_records=0, n_pairs=0, n_verdict=[0] * 5, n_tagged=[0] * 3, n_multi_ps=0, n_cg=0, n_bad_record=0, n_no_seq=0)
    out = dict(haps=[], phase_sets=[], n1=[], n2=[], first_site=[], cand_off=[0], verdict=[], stats=st, recs=[])
    for body, r in bo.region_records(bodies, reg_beg, reg_end, min_mapq, refid):
        if r < 0:
            continue
        x = tag_record(t, body, min_bq, min_diff)
        out["recs"].append(x)
        for k, key in (("hap", "haps"), ("ps", "phase_sets"), ("n1", "n1"), ("n2", "n2"), ("first", "first_site")):
            out[key].append(x[k])
        out["verdict"] += x["verdicts"]; out["cand_off"].append(len(out["verdict"]))
        st["n_records"] += 1; st["n_cg"] += x["cg"]; st["n_bad_record"] += x["bad"]; st["n_no_seq"] += x["no_seq"]; st["n_tagged"][x["hap"]] += 1
        st["n_multi_ps"] += x["n_sets"] > 1
        for v in x["verdicts"]:
            if v != NO_PAIR:
                st["n_pairs"] += 1; st["n_verdict"][v] += 1
    return out


# ---------------- records and VCF lines on one contig ----------------
TLEN = 60000
_REF = None


def ref_bases():
    """the contig: A C G T at random, fixed"""
    global _REF
    if _REF is None:
        _REF = "".join("ACGT"[c] for c in np.random.default_rng(77).integers(0, 4, TLEN))
    return _REF


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) & 3]


def make_record(name, pos1, ops, edits=None, ins=None, qual=30, quals=None, flag=0, mapq=60, no_seq=False, fields=(), ref=None, cg=False):
    """a record at 1-based pos1 with the operations [(code, length)]: under M / = / X the contig's bases, `edits` {reference position: base} replace them; an I
    operation takes its bases from ins[its index] (else C ...); quals {reference position: byte} over the default `qual`"""
    ref = ref or ref_bases()
    seq, q_of, p = [], {}, pos1
    for k, (op, ln) in enumerate(ops):
        if op in (M, EQ, X):
            for e in range(ln):
                q_of[p + e] = len(seq); seq.append((edits or {}).get(p + e, ref[p + e - 1]))
        elif op == I:
            seq += list((ins or {}).get(k, "C" * ln))
        elif op == S:
            seq += ["G"] * ln
        if op in dc.CONSUMES_REF:
            p += ln
    qv = np.full(len(seq), qual, np.uint8)
    for rp, v in (quals or {}).items():
        qv[q_of[rp]] = v
    s = "" if no_seq else "".join(seq)
    a = dict(name=name, pos0=pos1 - 1, flag=flag, qlen=len(s), bseq=dc.pack_seq(s) if s else np.zeros(0, np.uint8), qual=qv[:len(s)])
    if cg:
        rl = sum(ln for op, ln in ops if op in dc.CONSUMES_REF)
        r = record(a, dc.words([(S, len(s)), (N, rl)]), [("NM", "i", 0), ("CG", "B", ("I", dc.words(ops)))] + list(fields), mapq=mapq)
    else:
        r = record(a, dc.words(ops), list(fields), mapq=mapq)
    r["end"] = min(r["end"], TLEN)
    return r


def vcf_line(chrom, pos, ref, alt, gt, ps=None, flt="PASS", extra_fmt=True):
    fmt, smp = ("GT:DP", gt + ":9") if extra_fmt else ("GT", gt)
    if ps is not None:
        fmt, smp = fmt + ":PS", smp + ":%s" % ps
    return "%s\t%d\t.\t%s\t%s\t50\t%s\t.\t%s\t%s\n" % (chrom, pos, ref, alt, flt, fmt, smp)


VCF_HEAD = "##fileformat=VCFv4.2\n##contig=<ID=%s,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n" % (CONTIG, TLEN)


def snv(pos, gt="1|0", ps=None, k=1):
    b = ref_bases()[pos - 1]
    return vcf_line(CONTIG, pos, b, other(b, k), gt, ps)


def ins_site(pos, bases, gt="1|0", ps=None):
    b = ref_bases()[pos - 1]
    return vcf_line(CONTIG, pos, b, b + bases, gt, ps)


def del_site(pos, ln, gt="1|0", ps=None):
    return vcf_line(CONTIG, pos, ref_bases()[pos - 1:pos + ln], ref_bases()[pos - 1], gt, ps)


def alt_base(pos, k=1):
    return other(ref_bases()[pos - 1], k)


def not_ins(bases):
    """an insertion of the same length with another first base"""
    return other(bases[0]) + bases[1:]


def step_ops(n):
    """n operations, M 1 and I 1 in turn, ending in an M; an even n begins with a clip"""
    body = [(M, 1) if k % 2 == 0 else (I, 1) for k in range(n if n % 2 else n - 1)]
    return body if n % 2 else [(S, 2)] + body


SLOT, REG_BEG = 400, 2001


def case_table():
    """-> ([dict(name, recs, lines (VCF), pred(per-record oracle dicts in the case's order, table) -> bool)], reg_beg, reg_end).  Slot k starts at REG_BEG + 100 + SLOT k;
    a case's sites lie inside its slot, its phase set is its own unless the case is about phase sets"""
    T, slot = [], [0]

    def at(off=0):
        return REG_BEG + 100 + SLOT * slot[0] + off

    def add(name, recs, lines, pred):
        T.append(dict(name=name, recs=recs if isinstance(recs, list) else [recs], lines=lines, pred=pred, slot=slot[0]))
        slot[0] += 1

    def ps():
        return at()

    pairs = lambda x: [v for v in x["verdicts"] if v != NO_PAIR]
    for n in (1, 63, 64, 65, 128, 129):
        ops = [(M, 30)] if n == 1 else step_ops(n)
        a, b = at(), at() + sum(ln for op, ln in ops if op == M) - 1
        add("ops_%d" % n, make_record(b"ops%d" % n, a, ops, edits={a: alt_base(a)}), [snv(a, "1|0", ps()), snv(b, "1|0", ps())],
            lambda r, t, n=n: len(record_fields(r[0]["body"])["ops"]) == n and pairs(r[0]) == [ALT, REF] and (r[0]["hap"], r[0]["n1"], r[0]["n2"]) == (0, 1, 1))
    # a deletion whose anchor is the last operation of the first 64 and whose D is the first of the next; the same with another length
    add("del_across_steps", [make_record(b"delx", at(), [(M, 1)] * 64 + [(D, 3), (M, 5)]), make_record(b"delx4", at(), [(M, 1)] * 64 + [(D, 4), (M, 5)])],
        [del_site(at(63), 3, "0|1", ps())], lambda r, t: pairs(r[0]) == [ALT] and r[0]["hap"] == 2 and pairs(r[1]) == [OTHER] and r[1]["hap"] == 0)
    add("ins_lane_0", [make_record(b"insx", at(), [(M, 1)] * 64 + [(I, 2), (M, 5)], ins={64: "GT"}), make_record(b"insref", at(), [(M, 1)] * 64 + [(M, 5)])],
        [ins_site(at(63), "GT", "1|0", ps())], lambda r, t: pairs(r[0]) == [ALT] and r[0]["hap"] == 1 and pairs(r[1]) == [REF] and r[1]["hap"] == 2)
    add("del_next_to_ins", [make_record(b"i_d", at(), [(M, 20), (I, 1), (D, 2), (M, 20)]), make_record(b"d_i", at(), [(M, 20), (D, 2), (I, 1), (M, 20)])],
        [del_site(at(19), 2, "1|0", ps())], lambda r, t: pairs(r[0]) == [OTHER] and pairs(r[1]) == [ALT])
    add("snv_under_d_and_n", [make_record(b"under_d", at(), [(M, 10), (D, 5), (M, 10)]), make_record(b"under_n", at(), [(M, 10), (N, 5), (M, 10)])],
        [snv(at(12), "1|0", ps())], lambda r, t: pairs(r[0]) == [OTHER] and pairs(r[1]) == [OTHER] and r[0]["hap"] == r[1]["hap"] == 0)
    add("ins_wrong_bases", [make_record(b"wrongb", at(), [(M, 10), (I, 3), (M, 10)], ins={1: not_ins("ACG")}), make_record(b"wrongl", at(), [(M, 10), (I, 2), (M, 10)], ins={1: "AC"}),
                            make_record(b"rightb", at(), [(M, 10), (I, 3), (M, 10)], ins={1: "ACG"})],
        [ins_site(at(9), "ACG", "0|1", ps())], lambda r, t: [pairs(x) for x in r] == [[OTHER], [OTHER], [ALT]] and r[2]["hap"] == 2)
    add("no_site", make_record(b"nosite", at(), [(M, 50)]), [], lambda r, t: pairs(r[0]) == [] and r[0]["hap"] == 0)
    dense = [at(2 * k) for k in range(70)]
    counts = (3, 4, 5, 7, 8, 9, 63, 64, 65, 70)
    add("dense_pairs", [make_record(b"dense%d" % m, at(), [(M, 2 * m - 1)], edits={p: alt_base(p) for p in dense[:m:2]}) for m in counts],
        [snv(p, "1|0" if k % 3 else "0|1", ps()) for k, p in enumerate(dense)], lambda r, t: [len(pairs(x)) for x in r] == list(counts) and any(x["hap"] for x in r))
    # three sets in one read: A and B with two votes each (A first in the table), C with one; the second read gives B a third
    A, B, C = at(), at() + 1, at() + 2
    sets = [snv(at(10), "1|0", A), snv(at(20), "0|1", B), snv(at(30), "1|0", A), snv(at(40), "0|1", B), snv(at(50), "1|0", C), snv(at(60), "0|1", B)]
    alts = {at(o): alt_base(at(o)) for o in (10, 20, 30, 40, 50, 60)}
    add("three_sets_tie", [make_record(b"tie", at(), [(M, 55)], edits=alts), make_record(b"notie", at(), [(M, 65)], edits=alts)], sets,
        lambda r, t, A=A, B=B: (r[0]["n_sets"], r[0]["ps"], r[0]["hap"], r[0]["n1"], r[0]["n2"]) == (3, A, 1, 2, 0) and (r[1]["ps"], r[1]["hap"], r[1]["n2"]) == (B, 2, 3))
    add("min_diff", make_record(b"diff1", at(), [(M, 50)], edits={at(10): alt_base(at(10)), at(20): alt_base(at(20))}), [snv(at(10), "1|0", ps()), snv(at(20), "1|0", ps()), snv(at(30), "1|0", ps())],
        lambda r, t: (r[0]["n1"], r[0]["n2"]) == (2, 1))                        # (hap 1 with min_diff 1, none with 2)
    add("quality", [make_record(b"qff", at(), [(M, 50)], qual=0xff, edits={at(10): alt_base(at(10))}), make_record(b"qlow", at(), [(M, 50)], quals={at(10): 5}, edits={at(10): alt_base(at(10))}),
                    make_record(b"third", at(), [(M, 50)], edits={at(10): alt_base(at(10), 2)})],
        [snv(at(10), "1|0", ps())], lambda r, t: pairs(r[0]) == [ALT] and pairs(r[2]) == [OTHER])       # (qlow: LOWQ with min_bq above 5, ALT without)
    add("cg_field", make_record(b"cgrec", at(), step_ops(129), edits={at(): alt_base(at())}, cg=True), [snv(at(), "0|1", ps())], lambda r, t: r[0]["cg"] and pairs(r[0]) == [ALT] and r[0]["hap"] == 2)
    add("outside_the_span", [make_record(b"cutdel", at(), [(M, 21)]), make_record(b"cutins", at(), [(M, 11)]), make_record(b"leftcut", at(25), [(M, 30)])],
        [ins_site(at(10), "TT", "1|0", ps()), del_site(at(20), 6, "1|0", ps()), snv(at(22), "1|0", ps())],
        lambda r, t: pairs(r[0]) == [REF, NONE] and pairs(r[1]) == [NONE] and pairs(r[2]) == [NONE] and NO_PAIR in r[2]["verdicts"])
    add("clips_pads_zero_lengths", make_record(b"clips", at(), [(H, 3), (S, 4), (M, 10), (P, 2), (I, 0), (D, 0), (M, 10), (9, 3), (M, 5), (S, 2)], edits={at(22): alt_base(at(22))}),
        [snv(at(22), "1|0", ps()), del_site(at(9), 2, "0|1", ps())], lambda r, t: pairs(r[0]) == [REF, ALT] and r[0]["n1"] == 2)
    add("duplicate_sites", make_record(b"dup", at(), [(M, 30)], edits={at(10): alt_base(at(10))}), [snv(at(10), "1|0", ps()), snv(at(10), "1|0", ps()), snv(at(10), "0|1", ps(), k=2)],
        lambda r, t: pairs(r[0]) == [ALT, ALT, OTHER] and r[0]["n1"] == 2)
    add("filtered_records", [make_record(b"lowmq", at(), [(M, 30)], mapq=5), make_record(b"suppl", at(), [(M, 30)], flag=0x800), make_record(b"kept", at(), [(M, 30)])],
        [snv(at(10), "1|0", ps())], lambda r, t: len(r) == 1 and r[0]["hap"] == 2)
    reg_end = REG_BEG + 100 + SLOT * slot[0] + 99
    return T, REG_BEG, reg_end


def build_cases():
    """-> dict(cases, recs (position order), bodies, vcf (text), table, reg_beg, reg_end)"""
    cases, reg_beg, reg_end = case_table()
    recs = sorted((r for c in cases for r in c["recs"]), key=lambda r: r["pos0"])
    vcf = VCF_HEAD + "".join(ln for c in cases for ln in c["lines"])
    tables, st = read_vcf(vcf.encode(), [CONTIG])
    return dict(cases=cases, recs=recs, bodies=[r["body"] for r in recs], vcf=vcf, table=tables[0], vcf_stats=st, reg_beg=reg_beg, reg_end=reg_end)


def case_results(t, out):
    """the oracle's per-record dicts of haplotag(), each with its record's body, by record name"""
    by = {}
    kept = [r for r in t["recs"] if not (r["flag"] & bo.FILTER_FLAGS) and bo.parse(r["body"])["mapq"] >= 30]
    assert len(kept) == len(out["recs"])
    for r, x in zip(kept, out["recs"]):
        by[bo.parse(r["body"])["name"]] = dict(x, body=r["body"])
    return by


# ---------------- the simulator ----------------
def simulate(seed, n_reads=200, length=12000, read_len=(600, 3000), n_sets=2, noise=0.01, chrom="sim"):
    """two haplotypes of a random reference with het sites about every 90 bases, reads with exact M / I / D CIGARs from either one and substitution noise away from the
    sites -> dict(ref, vcf, recs (position order, each with `true_hap`), sites)"""
    rng = np.random.default_rng(seed)
    ref = "".join("ACGT"[c] for c in rng.integers(0, 4, length))
    sites, p = {}, 120
    while p < length - 200:
        kind = int(rng.choice([SNV, SNV, INS, DEL])); hap = int(rng.integers(1, 3)); ln = 1 if kind == SNV else int(rng.integers(1, 8))
        sites[p] = dict(pos=p, kind=kind, hap=hap, len=ln, alt=other(ref[p - 1], int(rng.integers(1, 4))), ins="".join("ACGT"[c] for c in rng.integers(0, 4, ln)))
        p += ln + int(rng.integers(40, 140))
    near = set()
    for s in sites.values():
        near.update(range(s["pos"] - 2, s["pos"] + s["len"] + 3))
    lines, bound = [], [length * (k + 1) // n_sets for k in range(n_sets)]
    for s in sites.values():
        ps = 1000 + next(k for k, b in enumerate(bound) if s["pos"] <= b)
        gt = "1|0" if s["hap"] == 1 else "0|1"
        b = ref[s["pos"] - 1]
        lines.append(vcf_line(chrom, s["pos"], b, s["alt"], gt, ps) if s["kind"] == SNV else vcf_line(chrom, s["pos"], b, b + s["ins"], gt, ps) if s["kind"] == INS
                     else vcf_line(chrom, s["pos"], ref[s["pos"] - 1:s["pos"] + s["len"]], b, gt, ps))
    recs = []
    for i in range(n_reads):
        hap = 1 + i % 2
        beg = int(rng.integers(1, length - read_len[1] - 10)); end = beg + int(rng.integers(*read_len))
        while beg in near:
            beg += 1
        while end in near:
            end += 1
        ops, edits, ins, run, p = [], {}, {}, 0, beg
        while p <= end:
            s = sites.get(p)
            run += 1
            if rng.random() < noise and p not in near:
                edits[p] = other(ref[p - 1], int(rng.integers(1, 4)))
            if s and s["hap"] == hap:
                if s["kind"] == SNV:
                    edits[p] = s["alt"]
                elif s["kind"] == INS:
                    ops += [(M, run), (I, s["len"])]; ins[len(ops) - 1] = s["ins"]; run = 0
                else:
                    ops += [(M, run), (D, s["len"])]; run = 0; p += s["len"]
            p += 1
        ops.append((M, run))
        r = make_record(b"sim%04d" % i, beg, ops, edits=edits, ins=ins, ref=ref, flag=16 if i % 3 == 0 else 0)
        r["true_hap"] = hap
        recs.append(r)
    recs.sort(key=lambda r: r["pos0"])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
    return dict(ref=ref, vcf=head + "".join(lines), recs=recs, sites=sites, length=length)


# ---------------- crafted VCF inputs ----------------
HEAD2 = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"


def line2(chrom, pos, ref, alt, s1, s2="0/0", flt="PASS", fmt="GT:PS"):
    return "%s\t%s\t.\t%s\t%s\t9\t%s\t.\t%s\t%s\t%s\n" % (chrom, pos, ref, alt, flt, fmt, s1, s2)


# every line holds for SEVERAL rules; the one counted is the first in the rules' order: (line, the counter it must raise)
FIRST_REASON = [
    (line2("chrZ", 10, "A", "<DEL>", "1/1", flt="q10"), "n_unknown_contig"),
    (line2("c1", 10, "A", "<DEL>", "1/1", flt="q10"), "n_filtered"),
    (line2("c1", 10, "A", "<DEL>", "1/1", fmt="DP:GT"), "n_other_gt"),
    (line2("c1", 10, "A", "<DEL>", "1/1"), "n_unphased"),
    (line2("c1", 10, "A", "<DEL>", "./."), "n_unphased"),
    (line2("c1", 10, "A", "<DEL>", "1|1"), "n_hom"),
    (line2("c1", 10, "A", "<DEL>", "5|5"), "n_hom"),
    (line2("c1", 10, "A", "<DEL>", ".|1"), "n_other_gt"),
    (line2("c1", 10, "A", "<DEL>", "1"), "n_other_gt"),
    (line2("c1", 10, "A", "<DEL>", "0|1|1"), "n_other_gt"),
    (line2("c1", 10, "A", "<DEL>", "0|2"), "n_other_gt"),
    (line2("c1", 10, "A", "<DEL>,*", "1|2"), "n_both_alt"),
    (line2("c1", 10, "A", "<DEL>", "0|1"), "n_symbolic"),
    (line2("c1", 10, "A", "*", "0|1"), "n_symbolic"),
    (line2("c1", 10, "A", "A[c1:30[", "1|0"), "n_symbolic"),
    (line2("c1", 10, "A", ".", "1|0"), "n_symbolic"),
    (line2("c1", 10, "AC" + "G" * 60, "GT", "1|0"), "n_complex"),
    (line2("c1", 10, "ACG", "TCA", "1|0"), "n_complex"),                         # an MNP
    (line2("c1", 10, "A", "A", "1|0"), "n_complex"),
    (line2("c1", 10, "A" + "C" * 51, "A", "1|0"), "n_long_indel"),
    (line2("c1", 10, "A", "A" + "C" * 51, "1|0"), "n_long_indel"),
    (line2("c1", 10, "A", "A" + "C" * 50, "1|0"), "n_ins"),
    (line2("c1", 10, "a", "t", "1|0"), "n_snv"),
    (line2("c1", 10, "AT", "A", "0|1", flt="."), "n_del"),
]

# normalisation: (REF, ALT list, GT) at POS 100 -> (pos, kind, len, hap_of_alt, inserted bases)
NORMALISE = [
    (("CAA", "C,CA", "0|2"), (100, DEL, 1, 2, "")),                             # CAA -> CA: the suffix A goes (CA -> C); C is as short as it gets
    (("CAA", "C,CA", "1|0"), (100, DEL, 2, 1, "")),
    (("GATTC", "GATTTC", "0|1"), (101, INS, 1, 2, "T")),                         # suffix then prefix: TTC goes (GA -> GAT), then G: A -> AT at 101
    (("ACGT", "ATGT", "1|0"), (101, SNV, 1, 1, "")),                             # an MNP-shaped SNV: suffix GT, prefix A
    (("TC", "TCAGC", "1|0"), (100, INS, 3, 1, "CAG")),                           # suffix C: T -> TCAG
]


def crafted_files():
    """[(name, file bytes, dict(names, sample, max_indel, snvs_only))]: inputs for both readers; some end in an error"""
    two = dict(names=["c1", "c2"], sample=None, max_indel=50, snvs_only=0)
    good = HEAD2 + "".join(l for l, _ in FIRST_REASON)
    mix = HEAD2 + line2("c2", 500, "A", "G", "0|1:7") + line2("c1", 300, "A", "G", "1|0:.") + line2("c2", 100, "AT", "A", "1|0:7") + line2("c1", 100, "C", "CTT", "0|1:9") + \
        line2("c1", 200, "A", "T", "1|0") + line2("c2", 300, "G", "C", "1|0:0", fmt="GT:DP:PS") + line2("c1", 100, "C", "G", "0|1:9") + line2("c2", 50, "T", "A", "1|0", fmt="GT")
    big = HEAD2 + line2("c1", 7, "A", "A" + "ACGT" * 2500, "1|0:3") + line2("c1", 9, "T" + "GGCA" * 2500, "T", "0|1:3") + line2("c1", 11, "ACGT" * 2500, "ACGT" * 2499 + "ACGA", "0|1:3")
    out = [("first_reason", good.encode(), two), ("interleaved_unsorted_missing_ps", mix.encode(), two), ("second_sample", mix.replace("\t0/0\n", "\t1|0:44\n").encode(), dict(two, sample="S2")),
           ("snvs_only", mix.encode(), dict(two, snvs_only=1)), ("alleles_10kb", big.encode(), dict(two, max_indel=20000)), ("alleles_10kb_default", big.encode(), two),
           ("no_trailing_newline", mix.encode().rstrip(b"\n"), two), ("crlf", mix.replace("\n", "\r\n").encode(), two), ("empty_file", b"", two), ("header_only", HEAD2.encode(), two),
           ("gzip", gzip.compress(mix.encode()), two), ("gzip_two_members", gzip.compress(HEAD2.encode()) + gzip.compress(mix[len(HEAD2):].encode()), two),
           ("gzip_cut_short", gzip.compress(mix.encode() * 40)[:-30], two),
           ("truncated_line", (mix + "c1\t400\t.\tA").encode(), two), ("short_line_in_the_middle", (HEAD2 + "c1\t5\t.\tA\tG\t9\tPASS\t.\tGT\t0|1\n" + mix[len(HEAD2):]).encode(), two),
           ("empty_fields", (HEAD2 + "c1\t5\t\t\t\t\t\t\t\t\t\n" + "c1\t6\t.\tA\tG\t9\t.\t.\tGT\t\t\n" + "c1\t7\t.\tA\t,\t9\t.\t.\tGT:PS\t0|1:\t\n" + "\t8\t.\tA\tG\t9\t.\t.\tGT:PS\t0|1:\t\n").encode(), two),
           ("bad_pos", (HEAD2 + "c1\tx\t.\tA\tG\t9\t.\t.\tGT\t0|1\t0|1\n").encode(), two), ("pos_zero", (HEAD2 + "c1\t0\t.\tA\tG\t9\t.\t.\tGT\t0|1\t0|1\n").encode(), two),
           ("no_sample_column", (HEAD2.replace("\tFORMAT\tS1\tS2", "") + "c1\t5\t.\tA\tG\t9\t.\t.\n").encode(), two), ("unknown_sample", mix.encode(), dict(two, sample="S3")),
           ("data_before_header", ("c1\t5\t.\tA\tG\t9\t.\t.\tGT\t0|1\t0|1\n" + HEAD2).encode(), two), ("no_contigs", mix.encode(), dict(two, names=[]))]
    return out
