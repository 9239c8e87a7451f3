"""The per-haplotype depth track (lcd_chunk_depth, depth_kernel.hip) restated in Python from its rules (include/lcd_hotpath.h), twice and independently: depth_rows
walks a record's operations once and keeps a difference array, depth_rows_naive loops over every covered position of every operation and counts.  Beside them the
window rule (lcd_depth_windows), the seam rule of the driver's writer (DepthSink), the text (lcd_depth_format), the records the tests are made of and a table of
named cases.  There is no reference implementation: the rules are the project's.

Conventions: positions are 1-based; a row is (beg, end, (depth of haplotype 0, 1, 2)); a window row carries three sums instead.  A record's operations are its own
CIGAR, or those of its first CG field when that is B,I / B,i with at least n_cigar and fewer than 2^29 entries and the record's first operation is `<l_seq>S`."""
import struct

import numpy as np

import bam_out_common as bo
from bam_src_common import CONTIG, aux_walk, record, write_bam  # noqa: F401
from mods_common import cigar_words, pack_seq  # noqa: F401

STAT_KEYS = ("n_records", "n_no_cigar", "n_cg", "n_no_overlap", "n_intervals", "bases", "n_rows")
HEADER = "#chrom\tstart\tend\tdepth_all\tdepth_h1\tdepth_h2\tdepth_unassigned\n"
HEADER_W = "#chrom\tstart\tend\tbases_all\tbases_h1\tbases_h2\tbases_unassigned\n"
OPS = "MIDNSHP=XB"
M, I, D, N, S, H, P, EQ, X, B = range(10)
CONSUMES_REF = (M, D, N, EQ, X)


def words(ops):
    """[(code, length)] -> CIGAR words"""
    return [(ln << 4) | op for op, ln in ops]


def text_ops(text):
    return [(w & 15, w >> 4) for w in cigar_words(text)]


# ---------------- the operations of a record ----------------
def record_ops(body):
    """-> (pos1, [(code, length)] | None when the fields run past the record, read through the CG field?)"""
    refid, pos0, lname, _mapq, _bin, ncig, _flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    o = 32 + lname
    if lseq < 0 or len(body) < o + 4 * ncig + (lseq + 1) // 2 + lseq:
        return pos0 + 1, None, False
    cig = struct.unpack("<%dI" % ncig, body[o:o + 4 * ncig])
    own = [(w & 15, w >> 4) for w in cig]
    if ncig >= 1 and refid >= 0 and pos0 >= 0 and own[0] == (S, lseq):
        for tag, ty, val in aux_walk(body[o + 4 * ncig + (lseq + 1) // 2 + lseq:]):
            if tag == b"CG":                                                    # the first CG field decides
                if ty == "B" and chr(val[0]) in "Ii":
                    cnt = struct.unpack("<I", val[1:5])[0]
                    if ncig <= cnt < 1 << 29:
                        return pos0 + 1, [(w & 15, w >> 4) for w in struct.unpack("<%dI" % cnt, val[5:5 + 4 * cnt])], True
                break
    return pos0 + 1, own, False


def covers(op, skip_dels):
    return op in (M, EQ, X) or (op == D and not skip_dels)


def cover_runs(pos1, ops, skip_dels):
    """the record's covered positions as maximal runs [(first, last)], unclipped: cover goes on over whatever consumes no reference"""
    runs, p, open_at = [], pos1, None
    for op, ln in ops:
        if ln == 0 or op not in CONSUMES_REF:
            continue
        if covers(op, skip_dels):
            if open_at is None:
                open_at = p
        elif open_at is not None:
            runs.append((open_at, p - 1)); open_at = None
        p += ln
    if open_at is not None:
        runs.append((open_at, p - 1))
    return runs


def _kept(bodies, reg_beg, reg_end, haps, min_mapq, refid):
    out = []
    for body, r in bo.region_records(bodies, reg_beg, reg_end, min_mapq, refid):
        if r >= 0:
            assert haps[r] in (0, 1, 2)
            out.append((body, haps[r]))
    return out


def _rows_of_depth(depth, reg_beg):
    """three per-position arrays -> the maximal runs of equal triples"""
    n = len(depth[0])
    rows, k0 = [], 0
    for k in range(1, n + 1):
        if k == n or any(depth[h][k] != depth[h][k0] for h in range(3)):
            rows.append((reg_beg + k0, reg_beg + k - 1, tuple(int(depth[h][k0]) for h in range(3)))); k0 = k
    return rows


def depth_rows(bodies, reg_beg, reg_end, haps, skip_dels=False, min_mapq=30, trace=None, refid=0):
    """the difference-array oracle -> (rows, statistics); trace gets one entry per kept record: body, ops, cg, runs (unclipped), clipped"""
    n = reg_end - reg_beg + 1
    diff = np.zeros((3, n + 1), np.int64)
    st = dict(n_records=0, n_no_cigar=0, n_cg=0, n_no_overlap=0, n_intervals=0, bases=[0, 0, 0], n_rows=0)
    for body, hap in _kept(bodies, reg_beg, reg_end, haps, min_mapq, refid):
        st["n_records"] += 1
        pos1, ops, cg = record_ops(body)
        entry = dict(body=body, ops=ops, cg=cg, runs=[], clipped=[], hap=hap)
        if trace is not None:
            trace.append(entry)
        if not ops:
            st["n_no_cigar"] += 1
            continue
        st["n_cg"] += cg
        entry["runs"] = cover_runs(pos1, ops, skip_dels)
        for s, e in entry["runs"]:
            if e < reg_beg or s > reg_end:
                continue
            a, b = max(s, reg_beg), min(e, reg_end)
            entry["clipped"].append((a, b))
            diff[hap][a - reg_beg] += 1; diff[hap][b + 1 - reg_beg] -= 1
            st["bases"][hap] += b - a + 1
        st["n_intervals"] += len(entry["clipped"])
        st["n_no_overlap"] += not entry["clipped"]
    rows = _rows_of_depth(np.cumsum(diff, axis=1)[:, :n], reg_beg)
    st["n_rows"] = len(rows)
    return rows, st


def depth_rows_naive(bodies, reg_beg, reg_end, haps, skip_dels=False, min_mapq=30, refid=0):
    """the same rules, position by position: every operation marks its positions of the region in the record's own flag array"""
    n = reg_end - reg_beg + 1
    depth = [[0] * n for _ in range(3)]
    st = dict(n_records=0, n_no_cigar=0, n_cg=0, n_no_overlap=0, n_intervals=0, bases=[0, 0, 0], n_rows=0)
    for body, hap in _kept(bodies, reg_beg, reg_end, haps, min_mapq, refid):
        st["n_records"] += 1
        pos1, ops, cg = record_ops(body)
        if ops is None or len(ops) == 0:
            st["n_no_cigar"] += 1
            continue
        st["n_cg"] += 1 if cg else 0
        mine, p = [False] * n, pos1
        for op, ln in ops:
            if op not in (M, D, N, EQ, X):
                continue
            if op != N and not (op == D and skip_dels):
                for q in range(max(p, reg_beg), min(p + ln - 1, reg_end) + 1):
                    mine[q - reg_beg] = True
            p += ln
        n_iv = 0
        for k in range(n):
            if mine[k]:
                depth[hap][k] += 1; st["bases"][hap] += 1
                n_iv += k == 0 or not mine[k - 1]
        st["n_intervals"] += n_iv
        st["n_no_overlap"] += n_iv == 0
    rows = []
    for k in range(n):
        t = (depth[0][k], depth[1][k], depth[2][k])
        if rows and rows[-1][2] == t:
            rows[-1] = (rows[-1][0], reg_beg + k, t)
        else:
            rows.append((reg_beg + k, reg_beg + k, t))
    st["n_rows"] = len(rows)
    return rows, st


# ---------------- windows, the writer's seam rule, the text ----------------
def windows(rows, W):
    """window k is [k W + 1, (k + 1) W]: one row per window that meets the rows' span: (beg, end, three sums of depth x positions), integers only"""
    assert W >= 1
    out = []
    for beg, end, d in rows:
        p = beg
        while p <= end:
            k = (p - 1) // W
            q = min(end, (k + 1) * W)
            if out and (out[-1][0] - 1) // W == k:
                b0, _, s = out[-1]
                out[-1] = (b0, q, tuple(s[h] + d[h] * (q - p + 1) for h in range(3)))
            else:
                out.append((p, q, tuple(d[h] * (q - p + 1) for h in range(3))))
            p = q + 1
    return out


def sink_rows(tables, W=0):
    """the writer of a run over the chunks' tables [(chrom, rows)] in plan order -> [(chrom, beg, end, values)]: a chunk's last row is held back; per base it joins
    the next chunk's first row when the contig is equal, held.end + 1 == next.beg and the depths are equal; window rows (W > 0) are added when the contig and the
    window index are equal and held.end + 1 == next.beg; otherwise the held row is written as it is"""
    out, held = [], None
    for chrom, rows in tables:
        rows = windows(rows, W) if W else list(rows)
        assert rows
        if held is not None:
            hc, hb, he, hv = held
            b, e, v = rows[0]
            if hc == chrom and he + 1 == b and ((hb - 1) // W == (b - 1) // W if W else hv == v):
                rows[0] = (hb, e, tuple(hv[h] + v[h] for h in range(3)) if W else v)
            else:
                out.append(held)
        out += [(chrom, b, e, v) for b, e, v in rows[:-1]]
        held = (chrom,) + tuple(rows[-1])
    if held is not None:
        out.append(held)
    return out


def format_rows(rows, chrom=None):
    """rows (beg, end, values) with chrom, or (chrom, beg, end, values) -> `chrom start end all h1 h2 unassigned` lines"""
    out = []
    for r in rows:
        c, b, e, v = r if chrom is None else (chrom,) + tuple(r)
        out.append(f"{c}\t{b - 1}\t{e}\t{v[0] + v[1] + v[2]}\t{v[1]}\t{v[2]}\t{v[0]}\n")
    return "".join(out)


def check_tiling(rows, reg_beg, reg_end, st):
    """the rows tile the region, adjacent rows differ, and the sum of length x depth is `bases`"""
    assert rows and rows[0][0] == reg_beg and rows[-1][1] == reg_end
    for a, b in zip(rows, rows[1:]):
        assert a[1] + 1 == b[0] and a[2] != b[2]
    assert all(b <= e for b, e, _ in rows)
    assert [sum((e - b + 1) * d[h] for b, e, d in rows) for h in range(3)] == list(st["bases"])
    assert st["n_rows"] == len(rows)


# ---------------- records ----------------
TLEN = 60000
_REF = None


def ref_codes():
    """the contig: A / T at random, fixed"""
    global _REF
    if _REF is None:
        _REF = np.where(np.random.default_rng(7).integers(0, 2, TLEN) == 0, 0, 3).astype(np.uint8)
    return _REF


def make_record(name, pos1, ops, hap=1, flag=0, mapq=60, fields=(), rng=None):
    """a record at 1-based pos1 with the operations [(code, length)]: the bases under M / = / X are the contig's where it has them, the others A"""
    ref = ref_codes()
    seq, p = [], pos1 - 1
    for op, ln in ops:
        if op in (M, EQ, X):
            seq += ["ACGT"[ref[q]] if 0 <= q < TLEN else "A" for q in range(p, p + ln)] if ln < 100000 else ["A"] * ln
        elif op in (I, S):
            seq += ["A"] * ln
        if op in CONSUMES_REF:
            p += ln
    s = "".join(seq)
    a = dict(name=name, pos0=pos1 - 1, flag=flag, qlen=len(s), bseq=pack_seq(s) if s else np.zeros(0, np.uint8), qual=np.full(len(s), 30, np.uint8))
    r = record(a, words(ops), list(fields), mapq=mapq)
    r["end"] = min(r["end"], TLEN)                                              # (the index's end only: the loader measures the record itself)
    r["hap"] = hap
    return r


def cg_record(name, pos1, real_ops, hap=1, n_in_field=None, sub="I"):
    """a record whose 16-bit field holds the placeholder `<l_seq>S<n>N` and whose operations lie in a CG:B field (n_in_field: cut the field short)"""
    lseq = sum(ln for op, ln in real_ops if op in (M, I, S, EQ, X))
    rl = sum(ln for op, ln in real_ops if op in CONSUMES_REF)
    ref = ref_codes()
    s = "".join("ACGT"[ref[(pos1 - 1 + k) % TLEN]] for k in range(lseq))
    a = dict(name=name, pos0=pos1 - 1, flag=0, qlen=lseq, bseq=pack_seq(s), qual=np.full(lseq, 30, np.uint8))
    w = words(real_ops)[:n_in_field]
    r = record(a, words([(S, lseq), (N, rl)]), [("NM", "i", 0), ("CG", "B", (sub, w))])
    r["end"] = min(r["end"], TLEN); r["hap"] = hap
    return r


def pattern_ops(n):
    """n operations of mixed kinds that begin and end with an M: every seventh a D, every eleventh an N, every fifth an I"""
    out = []
    for i in range(n):
        out.append((M, 2) if i in (0, n - 1) else (D, 2) if i % 7 == 3 else (N, 3) if i % 11 == 5 else (I, 1) if i % 5 == 1 else (EQ, 1) if i % 2 else (M, 2))
    return out


def seam_ops(op, at, ln=3):
    """`at` one-base Ms (words 0 .. at - 1), the operation in word `at`, one more M"""
    return [(M, 1)] * at + [(op, ln), (M, 4)]


SLOT, REG_BEG = 300, 2001


def case_table():
    """[dict(name, recs [record], pred(trace entries of the case's records, skip_dels) -> bool)]; slot k starts at REG_BEG + 100 + SLOT * k"""
    T, slot = [], [0]

    def at(off=0):
        return REG_BEG + 100 + SLOT * slot[0] + off

    def add(name, recs, pred, same_slot=False):
        T.append(dict(name=name, recs=recs if isinstance(recs, list) else [recs], pred=pred))
        if not same_slot:
            slot[0] += 1

    one = lambda t, sd: len(t[0]["clipped"]) == 1
    add("no_ops", make_record(b"no_ops", at(), []), lambda t, sd: t[0]["ops"] == [] and not t[0]["clipped"])
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        add("ops_%d" % n, make_record(b"ops_%d" % n, at(), pattern_ops(n), hap=n % 3), lambda t, sd, n=n: len(t[0]["ops"]) == n and (n < 6 or len(t[0]["clipped"]) > 1))
    for w in (63, 64):
        add("ins_word_%d" % w, make_record(b"ins_%d" % w, at(), seam_ops(I, w)), lambda t, sd, w=w: t[0]["ops"][w][0] == I and t[0]["ops"][w - 1][0] == M and one(t, sd))
        add("del_word_%d" % w, make_record(b"del_%d" % w, at(), seam_ops(D, w), hap=2), lambda t, sd, w=w: t[0]["ops"][w][0] == D and len(t[0]["clipped"]) == (2 if sd else 1))
        add("skip_word_%d" % w, make_record(b"skip_%d" % w, at(), seam_ops(N, w), hap=0), lambda t, sd, w=w: t[0]["ops"][w][0] == N and len(t[0]["clipped"]) == 2)
    add("hifi_like_200", make_record(b"hifi200", at(), [(EQ, 1) if i % 2 == 0 else (I, 1) if i % 4 == 1 else (X, 1) if i % 8 == 3 else (D, 1) for i in range(199)] + [(EQ, 2)]),
        lambda t, sd: len(t[0]["ops"]) == 200 and (sd or one(t, sd)))
    add("eq_x_runs", make_record(b"eqx", at(), text_ops("5=1X5=2X3=")), lambda t, sd: {o for o, _ in t[0]["ops"]} == {EQ, X} and one(t, sd))
    add("clips", make_record(b"clips", at(), text_ops("3H5S20M4S2H")), lambda t, sd: t[0]["ops"][0][0] == H and t[0]["ops"][-1][0] == H and t[0]["runs"] == [(t[0]["runs"][0][0], t[0]["runs"][0][0] + 19)])
    add("zero_length_ops", make_record(b"zeros", at(), [(M, 5)] + [(c, 0) for c in range(10)] + [(M, 5)]), lambda t, sd: sum(ln == 0 for _, ln in t[0]["ops"]) == 10 and one(t, sd)
        and t[0]["clipped"][0][1] - t[0]["clipped"][0][0] == 9)
    add("unknown_code_9", make_record(b"code9", at(), [(M, 5), (B, 3), (M, 5)]), lambda t, sd: t[0]["ops"][1] == (B, 3) and one(t, sd) and t[0]["clipped"][0][1] - t[0]["clipped"][0][0] == 9)
    add("cg_field_70000", cg_record(b"cg70000", at(), [(EQ, 1), (I, 1)] * 34999 + [(EQ, 1), (D, 1)]), lambda t, sd: t[0]["cg"] and len(t[0]["ops"]) == 70000)
    add("cg_field_too_short", cg_record(b"cgshort", at(), [(M, 10), (I, 2), (M, 10)], n_in_field=1), lambda t, sd: not t[0]["cg"] and t[0]["ops"][1][0] == N and not t[0]["clipped"])
    add("cg_field_signed", cg_record(b"cgsigned", at(), [(M, 10), (D, 2), (M, 10)], sub="i", hap=2), lambda t, sd: t[0]["cg"] and len(t[0]["ops"]) == 3)
    add("far_skip_past_2_31", make_record(b"farskip", at(), [(M, 10)] + [(N, 268435455)] * 9 + [(M, 10)]),
        lambda t, sd: t[0]["runs"][1][0] > 1 << 31 and t[0]["clipped"] == [(t[0]["runs"][0][0], t[0]["runs"][0][0] + 9)])
    add("identical_300", [make_record(b"same%03d" % i, at(20), [(M, 100)], hap=1) for i in range(300)], lambda t, sd: len(t) == 300 and len({tuple(x["clipped"]) for x in t}) == 1)
    add("staggered_130", [make_record(b"stag%03d" % i, at(i), [(M, 150)], hap=i % 3) for i in range(130)], lambda t, sd: [x["clipped"][0][0] for x in t] == list(range(t[0]["clipped"][0][0], t[0]["clipped"][0][0] + 130)))
    add("haps_mixed", [make_record(b"hap%d" % i, at(10 * i), [(M, 100)], hap=i % 3) for i in range(6)], lambda t, sd: {x["hap"] for x in t} == {0, 1, 2})
    n_slots = slot[0]
    reg_end = REG_BEG + 100 + SLOT * n_slots + 99
    span = reg_end - REG_BEG + 1
    edge = [
        ("spans_the_region", make_record(b"spans", REG_BEG - 50, [(M, span + 100)], hap=2), lambda t, sd: t[0]["clipped"] == [(REG_BEG, reg_end)] and t[0]["runs"][0][0] < REG_BEG and t[0]["runs"][0][1] > reg_end),
        ("only_a_deletion_inside", make_record(b"delonly", REG_BEG - 10, [(M, 5), (D, span + 20), (M, 5)], hap=1), lambda t, sd: (not t[0]["clipped"]) if sd else t[0]["clipped"] == [(REG_BEG, reg_end)]),
        ("only_a_skip_inside", make_record(b"skiponly", REG_BEG - 9, [(M, 5), (N, span + 20), (M, 5)], hap=1), lambda t, sd: not t[0]["clipped"] and len(t[0]["runs"]) == 2),
        ("ends_at_reg_beg", make_record(b"endbeg", REG_BEG - 29, [(M, 30)], hap=0), lambda t, sd: t[0]["clipped"] == [(REG_BEG, REG_BEG)]),
        ("ends_at_reg_end", make_record(b"endend", reg_end - 39, [(M, 40)], hap=0), lambda t, sd: t[0]["clipped"] == [(reg_end - 39, reg_end)]),
        ("begins_at_reg_end", make_record(b"begend", reg_end, [(M, 40)], hap=2), lambda t, sd: t[0]["clipped"] == [(reg_end, reg_end)]),
    ]
    for name, r, pred in edge:
        T.append(dict(name=name, recs=[r], pred=pred))
    return T, REG_BEG, reg_end


def build_cases():
    """-> dict(cases, recs (position order, for write_bam), bodies, haps per kept read, reg_beg, reg_end, ref, tlen)"""
    cases, reg_beg, reg_end = case_table()
    recs = sorted((r for c in cases for r in c["recs"]), key=lambda r: r["pos0"])           # (stable: equal positions keep their order)
    return dict(cases=cases, recs=recs, bodies=[r["body"] for r in recs], haps=haps_of(recs, reg_beg, reg_end), reg_beg=reg_beg, reg_end=reg_end, ref=ref_codes(), tlen=TLEN)


def haps_of(recs, reg_beg, reg_end, min_mapq=30):
    """the records' own haps for the kept reads of a region"""
    by_body = {id(r["body"]): r["hap"] for r in recs}
    return [by_body[id(b)] for b, k in bo.region_records([r["body"] for r in recs], reg_beg, reg_end, min_mapq) if k >= 0]


def tile_records(base, T):
    """records whose cover begins on chosen positions around the tile bounds of a region that starts at `base` (tile size T): offsets 0, 1, 62 ... 65, T - 2 ... T + 1,
    2T - 1, 2T, and ends on others; one long record lies over all of them"""
    offs = [0, 1, 62, 63, 64, 65, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T]
    recs = [make_record(b"long", base - 20, [(M, 2 * T + 100)], hap=0)]
    recs += [make_record(b"tile%02d" % i, base + o, [(M, 7 + i)], hap=1 + i % 2) for i, o in enumerate(offs)]
    return sorted(recs, key=lambda r: r["pos0"])


OP_CHOICES = (M, M, M, EQ, X, I, D, N, S, H, P, B)


def seeded_chunk(seed, n_rec=None, reg_len=None):
    """a small chunk of random records (every code, zero lengths, up to 140 operations) around a region -> (recs, reg_beg, reg_end)"""
    rng = np.random.default_rng(seed)
    reg_len = reg_len or int(rng.integers(1, 400))
    n_rec = int(rng.integers(0, 13)) if n_rec is None else n_rec
    reg_beg = 5000
    recs = []
    for i in range(n_rec):
        n_ops = int(rng.choice([0, 1, 2, 5, 20, 64, 70, 140]))
        ops = [(int(rng.choice(OP_CHOICES)), int(rng.choice([0, 1, 1, 2, 3, 9, 40]))) for _ in range(n_ops)]
        recs.append(make_record(b"r%03d" % i, int(rng.integers(reg_beg - 200, reg_beg + reg_len + 20)), ops, hap=int(rng.integers(0, 3)),
                                mapq=int(rng.choice([60, 60, 60, 5])), flag=int(rng.choice([0, 0, 16, 0x100]))))
    recs.sort(key=lambda r: r["pos0"])
    return recs, reg_beg, reg_beg + reg_len - 1
