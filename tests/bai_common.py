"""The .bai oracle: an independent pure-Python index writer and reader (struct + zlib) written from the rules of include/lcd_hotpath.h ("indexes"), a BAM
generator with explicit BGZF member borders, and the table of named cases.  Every case carries a predicate that proves from the ORACLE's own output that the
case is reached (tests/vars_cases.py does the same for the variant kernels).

    build_bam(refs, recs, cuts, ...)   -> bytes of a BAM whose members end exactly at the given offsets of the inflated stream
    scan_bam(bam)                      -> header, member table, record table (interval, flag, virtual offsets) by plain gzip decoding
    oracle_bai(n_ref, recs)            -> the index bytes (rules 1-9), or BaiRefused(code, record number)
    parse_bai / query                  -> the reader of specification 5.3: candidate bins, linear-index cut, merged chunks
"""
import struct
import zlib

import numpy as np

ERR_ORDER, ERR_CSI = -50, -51
PAYLOADS = (1, 700, 4000, 65280)


class BaiRefused(Exception):
    def __init__(self, code, recno):
        super().__init__(f"code {code} at record {recno}")
        self.code, self.recno = code, recno


# ---------------------------------------------------------------- writer of BAM files ----------------------------------------------------------------
def member(payload):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


def header_bytes(refs, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    d = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for nm, ln in refs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    return d


def record(tid, pos, ops, flag=0, mapq=60, name="r", aux=b"", cg=False):
    """one BAM record (with its block_size word).  ops: [(op, len)]; bases and qualities are zeros.  cg: the operations go into a CG:B,I tag behind the
    placeholder CIGAR <l_seq>S<ref_len>N, as a writer does for more than 65 535 operations"""
    qlen = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
    rl = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
    cig = np.array([(ln << 4) | op for op, ln in ops], "<u4")
    if cg:
        aux = aux + b"CGBI" + struct.pack("<i", len(cig)) + cig.tobytes()
        cig = np.array([(qlen << 4) | 4, (rl << 4) | 3], "<u4")
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(cig), flag, qlen, -1, -1, 0) + nm + cig.tobytes() + bytes((qlen + 1) // 2) + bytes(qlen) + aux
    return struct.pack("<i", len(body)) + body


def build_bam(refs, recs, cuts=(), payloads=None, rng=None, eof=True):
    """header in members of its own, then the records.  Member borders of the record part: `cuts` are offsets RELATIVE TO THE FIRST RECORD at which a member ends
    (a value given twice leaves an empty member there); between them the stream is cut by `payloads` (cycled; default 65280), or by sizes drawn from PAYLOADS
    with rng.  -> bytes"""
    hdr = header_bytes(refs)
    body = b"".join(recs)
    out = b"".join(member(hdr[o:o + 65280]) for o in range(0, len(hdr), 65280))
    borders = sorted(c for c in cuts if 0 <= c <= len(body))
    at, k, bi = 0, 0, 0
    while at < len(body) or bi < len(borders):
        size = int(rng.choice(PAYLOADS)) if rng is not None else (payloads[k % len(payloads)] if payloads else 65280)
        k += 1
        end = min(len(body), at + size)
        if bi < len(borders) and borders[bi] <= end:
            end = borders[bi]; bi += 1
        out += member(body[at:end])
        at = end
    return out + (member(b"") if eof else b"")


# ---------------------------------------------------------------- independent reader of BAM files ----------------------------------------------------------------
def members_of(bam):
    """[(compressed offset, inflated offset, payload length)] + the inflated stream"""
    tab, parts, o, u = [], [], 0, 0
    while o < len(bam):
        assert bam[o:o + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", bam, o + 16)[0] + 1
        payload = zlib.decompress(bam[o + 18:o + bsize - 8], -15)
        assert len(payload) == struct.unpack_from("<I", bam, o + bsize - 4)[0]
        tab.append((o, u, len(payload))); parts.append(payload)
        o += bsize; u += len(payload)
    return tab, b"".join(parts)


def voff(tab, fsize, p):
    """rule 5: the member whose payload holds byte p - 1; at that payload's very end the immediately following member's start (the file size if none follows)"""
    if p <= tab[0][1]:
        return tab[0][0] << 16
    for k, (c, u, n) in enumerate(tab):
        if u + n >= p:                                   # (never an empty member: u < p here)
            if p < u + n:
                return (c << 16) | (p - u)
            return (tab[k + 1][0] if k + 1 < len(tab) else fsize) << 16
    raise AssertionError("offset behind the stream")


def ref_len_of(d, o, bs):
    """reference length of the record at d[o:o + bs] (behind its block_size word): its CIGAR, or the CG tag's behind the placeholder"""
    tid, pos, lname, _mq, _bin, nc, flag, lseq = struct.unpack_from("<iiBBHHHi", d, o)
    c0 = o + 32 + lname
    cig = list(struct.unpack_from(f"<{nc}I", d, c0))
    if nc >= 1 and tid >= 0 and pos >= 0 and (cig[0] & 15) == 4 and (cig[0] >> 4) == lseq:
        a, end = c0 + 4 * nc + (lseq + 1) // 2 + lseq, o + bs
        while a + 3 <= end:
            tag, ty = d[a:a + 2], chr(d[a + 2]); a += 3
            if ty in "AcC":
                sz = 1
            elif ty in "sS":
                sz = 2
            elif ty in "iIf":
                sz = 4
            elif ty in "ZH":
                sz = d.index(b"\0", a) - a + 1
            elif ty == "B":
                sub, cnt = chr(d[a]), struct.unpack_from("<I", d, a + 1)[0]
                es = 1 if sub in "cC" else 2 if sub in "sS" else 4
                if tag == b"CG":
                    if sub in "Ii" and cnt >= nc:
                        cig = list(struct.unpack_from(f"<{cnt}I", d, a + 5))
                    break
                sz = 5 + cnt * es
            else:
                break
            if tag == b"CG":
                break
            a += sz
    return sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))


def scan_bam(bam):
    """-> dict(refs, tab, stream, recs): recs = [dict(tid, pos, end, flag, mapq, name, u0, u1, vbeg, vend)] in file order"""
    tab, d = members_of(bam)
    assert d[:4] == b"BAM\x01"
    o = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref = struct.unpack_from("<i", d, o)[0]; o += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", d, o)[0]
        refs.append((d[o + 4:o + 4 + ln - 1].decode(), struct.unpack_from("<i", d, o + 4 + ln)[0])); o += 8 + ln
    recs = []
    while o + 4 <= len(d):
        bs = struct.unpack_from("<i", d, o)[0]
        tid, pos, lname, mq, _bin, _nc, flag, _lseq = struct.unpack_from("<iiBBHHHi", d, o + 4)
        rl = ref_len_of(d, o + 4, bs)
        end = pos + (1 if (flag & 4) or rl <= 0 else rl)
        u0, u1 = o, o + 4 + bs
        recs.append(dict(tid=tid, pos=pos, end=end, flag=flag, mapq=mq, name=d[o + 36:o + 36 + lname - 1].decode(), u0=u0, u1=u1,
                         vbeg=voff(tab, len(bam), u0), vend=voff(tab, len(bam), u1)))
        o = u1
    return dict(refs=refs, tab=tab, stream=d, recs=recs, fsize=len(bam))


# ---------------------------------------------------------------- the index: writer ----------------------------------------------------------------
def reg2bin(beg, end):                                   # SAM specification 5.3
    end -= 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return base + (beg >> sh)
    return 0


def oracle_bai(n_ref, recs):
    """rules 2-9 on a record table (dicts with tid, pos, end, flag, vbeg, vend) -> bytes; BaiRefused(code, record number) by rule 3"""
    per = [dict(bins={}, lin={}, n_map=0, n_unmap=0, first=None, last=None) for _ in range(n_ref)]
    n_no_coor, prev, seen_no_coor, run = 0, None, False, None
    for i, x in enumerate(recs):
        if x["tid"] < 0 or x["pos"] < 0:
            n_no_coor += 1; seen_no_coor = True; run = None
            continue
        if seen_no_coor:
            raise BaiRefused(ERR_ORDER, i)
        if prev is not None and (x["tid"], x["pos"]) < prev:
            raise BaiRefused(ERR_ORDER, i)
        if x["end"] > 1 << 29:
            raise BaiRefused(ERR_CSI, i)
        prev = (x["tid"], x["pos"])
        b = reg2bin(x["pos"], x["end"])
        c = per[x["tid"]]
        if run == (x["tid"], b):
            c["bins"][b][-1][1] = x["vend"]                                       # the run goes on
        else:
            ch = c["bins"].setdefault(b, [])
            if ch and ch[-1][1] >> 16 >= x["vbeg"] >> 16:                          # rule 6: merged into the chunk before it in its bin
                ch[-1][1] = x["vend"]
            else:
                ch.append([x["vbeg"], x["vend"]])
            run = (x["tid"], b)
        c["n_unmap" if x["flag"] & 4 else "n_map"] += 1
        c["first"] = x["vbeg"] if c["first"] is None else c["first"]
        c["last"] = x["vend"]
        for w in range(x["pos"] >> 14, ((x["end"] - 1) >> 14) + 1):
            c["lin"][w] = min(c["lin"].get(w, x["vbeg"]), x["vbeg"])
    out = b"BAI\x01" + struct.pack("<i", n_ref)
    for c in per:
        if c["first"] is None:
            out += struct.pack("<ii", 0, 0)
            continue
        out += struct.pack("<i", len(c["bins"]) + 1)
        for b in sorted(c["bins"]):
            out += struct.pack("<Ii", b, len(c["bins"][b])) + b"".join(struct.pack("<QQ", s, e) for s, e in c["bins"][b])
        out += struct.pack("<IiQQQQ", 37450, 2, c["first"], c["last"], c["n_map"], c["n_unmap"])
        n_intv = max(c["lin"]) + 1
        offs, p = [], 0
        for w in range(n_intv):
            p = c["lin"].get(w, p); offs.append(p)
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in offs)
    return out + struct.pack("<Q", n_no_coor)


# ---------------------------------------------------------------- the index: reader ----------------------------------------------------------------
def parse_bai(b):
    assert b[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", b, 4)[0]
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, o)[0]; o += 4
        bins, meta = {}, None
        for _k in range(n_bin):
            bn, nch = struct.unpack_from("<Ii", b, o); o += 8
            ch = [struct.unpack_from("<QQ", b, o + 16 * k) for k in range(nch)]; o += 16 * nch
            if bn == 37450:
                meta = dict(off_beg=ch[0][0], off_end=ch[0][1], n_mapped=ch[1][0], n_unmapped=ch[1][1])
            else:
                bins[bn] = ch
        n_intv = struct.unpack_from("<i", b, o)[0]; o += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", b, o)); o += 8 * n_intv
        refs.append(dict(bins=bins, lin=lin, meta=meta, n_bin=n_bin))
    n_no_coor = struct.unpack_from("<Q", b, o)[0] if o + 8 <= len(b) else None
    assert o + (8 if n_no_coor is not None else 0) == len(b)
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for sh, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(base + (beg >> sh), base + (end >> sh) + 1))
    return out


def query(idx, tid, beg, end):
    """the merged chunks that can hold records overlapping [beg, end) (0-based half-open): candidate bins, cut at the linear index's offset of beg's window"""
    r = idx["refs"][tid]
    if not r["bins"] or end <= beg:
        return []
    lin = r["lin"]
    min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    ch = sorted(c for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > min_off)
    merged = []
    for s, e in ch:
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return merged


def records_through_index(scan, idx, tid, beg, end):
    """the records (indices into scan['recs']) a reader finds for [beg, end): it seeks to each chunk's begin, reads records until the chunk's end, keeps overlaps"""
    by_v = {}
    for i, x in enumerate(scan["recs"]):
        by_v.setdefault(x["vbeg"], i)
    vs = sorted(by_v)
    got = []
    for s, e in query(idx, tid, beg, end):
        k = int(np.searchsorted(np.array(vs, np.uint64), np.uint64(s)))     # a chunk begins at a record's begin
        assert k < len(vs) and vs[k] == s, "a chunk does not begin at a record"
        i = by_v[s]
        while i < len(scan["recs"]) and scan["recs"][i]["vbeg"] < e:
            x = scan["recs"][i]
            if x["tid"] == tid and x["pos"] < end and x["end"] > beg:
                got.append(i)
            i += 1
    return got


def records_by_scan(scan, tid, beg, end):
    return [i for i, x in enumerate(scan["recs"]) if x["tid"] == tid and x["pos"] >= 0 and x["pos"] < end and x["end"] > beg]


def regions_for(rng, refs, tid, n_random):
    """whole contig, single bases, windows aligned to 2^14 and to 2^14 +- 1, random ones: (beg, end) 0-based half-open"""
    ln = refs[tid][1]
    out = [(0, ln)]
    for _ in range(n_random // 4):
        p = int(rng.integers(0, ln)); out.append((p, p + 1))
    for _ in range(n_random // 4):
        w = int(rng.integers(0, (ln >> 14) + 1)) << 14
        d0, d1 = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
        b = max(0, w + d0); out.append((b, max(b + 1, min(ln, w + (int(rng.integers(1, 4)) << 14) + d1))))
    for _ in range(n_random // 2):
        b = int(rng.integers(0, ln)); out.append((b, min(ln, b + int(rng.integers(1, 60000)))))
    return out


# ---------------------------------------------------------------- seeded files ----------------------------------------------------------------
SEED_REFS = [("chrA", 400000), ("chrE", 90000), ("chrB", 3000000), ("chrC", 120000)]


def seeded_records(rng, n=300, n_no_coor=5):
    """n records over chrA / chrB / chrC (chrE stays empty) in coordinate order + n_no_coor records without coordinate; HiFi-like intervals from 200 b to 40 kb,
    a few placed-unmapped ones, secondary / supplementary flags, dense stretches (several records per bin run) and bin changes"""
    tids = np.sort(rng.choice([0, 2, 3], n, p=[0.3, 0.5, 0.2]))
    recs = []
    for t in (0, 2, 3):
        k = int((tids == t).sum())
        ln = SEED_REFS[t][1]
        pos = np.sort(rng.integers(0, ln - 45000, k))
        for p in pos:
            span = int(rng.choice([200, 3000, 15000, 25000, 40000])) + int(rng.integers(0, 500))
            flag = int(rng.choice([0, 16, 256, 2048, 4], p=[0.45, 0.35, 0.05, 0.05, 0.1]))
            ops = [(4, int(rng.integers(1, 30))), (7, 40), (3, span - 80), (8, 1), (7, 39)] if rng.random() < 0.5 else [(7, 50), (2, span - 100), (7, 50)]
            aux = b"NMi" + struct.pack("<i", 3) if rng.random() < 0.5 else b"csZ" + b":40*ag" * int(rng.integers(1, 200)) + b"\0"
            recs.append(record(t, int(p), ops, flag=flag, mapq=int(rng.choice([60, 30, 5])), name=f"q{len(recs)}", aux=aux))
    for k in range(n_no_coor):
        recs.append(record(-1, -1, [], flag=4, mapq=0, name=f"u{k}", aux=b"X" * 0))
    return recs


def seeded_bam(seed, n=300, n_no_coor=5):
    rng = np.random.default_rng(seed)
    recs = seeded_records(rng, n, n_no_coor)
    return build_bam(SEED_REFS, recs, rng=rng)


SEEDS = list(range(101, 121))      # 20 seeded record tables (checked with the oracle alone: at least half of every file's regions are non-empty)


# ---------------------------------------------------------------- named cases ----------------------------------------------------------------
REFS = [("c0", 1 << 30), ("c1", 200000), ("c2", 100000000)]
M = lambda n: [(7, n)]                                    # noqa: E731


def _lens(recs):
    return np.cumsum([0] + [len(r) for r in recs])


def _case_member_end():
    recs = [record(1, 100 * i, M(50), name=f"a{i}") for i in range(6)]
    o = _lens(recs)
    bam = build_bam(REFS, recs, cuts=[int(o[2]), int(o[4])])
    def pred(s, idx):
        # records 1 and 3 end exactly at a member's end: their vend is a member start with offset 0, and equals the next record's vbeg
        r = s["recs"]
        starts = {c for c, _u, _n in s["tab"]}
        return all(r[i]["vend"] & 0xffff == 0 and (r[i]["vend"] >> 16) in starts and r[i]["vend"] == r[i + 1]["vbeg"] for i in (1, 3)) and r[5]["vend"] >> 16 == s["tab"][-1][0]
    return bam, pred, None


def _case_straddle():
    recs = [record(1, 10, M(50), name="s0"), record(1, 20, M(3000), name="s1"), record(1, 30, M(50), name="s2"), record(1, 40, M(9000), name="s3"), record(1, 50, M(50), name="s4")]
    bam = build_bam(REFS, recs, payloads=[3000])
    def pred(s, idx):
        def n_members(x):
            return sum(1 for _c, u, n in s["tab"] if n and u < x["u1"] and u + n > x["u0"])
        return n_members(s["recs"][1]) == 2 and n_members(s["recs"][3]) > 2
    return bam, pred, None


def _case_empty_member():
    recs = [record(1, 100 * i, M(50), name=f"e{i}") for i in range(4)]
    o = _lens(recs)
    bam = build_bam(REFS, recs, cuts=[int(o[2]), int(o[2])])
    def pred(s, idx):
        k = [i for i, (_c, _u, n) in enumerate(s["tab"][:-1]) if n == 0]
        r = s["recs"]
        # the empty member is the one that follows record 1's payload: vend(1) = vbeg(2) = its start
        return len(k) == 1 and r[1]["vend"] == s["tab"][k[0]][0] << 16 == r[2]["vbeg"]
    return bam, pred, None


def _case_runs(apart):
    # bin 4681 (window 0), then bin 4682, then bin 4681 again is impossible in a sorted file; a parent bin comes back instead: 585 (a record crossing 2^14), then
    # 4682 (inside window 1), then 585 again (crossing 2^15)
    recs = [record(1, 16000, M(1000), name="p0"), record(1, 16500, M(100), name="k0"), record(1, 16600, M(100), name="k1"), record(1, 32000, M(1000), name="p1")]
    o = _lens(recs)
    bam = build_bam(REFS, recs, cuts=[int(o[1]), int(o[3])] if apart else [])
    def pred(s, idx):
        ch = idx["refs"][1]["bins"].get(585, [])
        return len(ch) == (2 if apart else 1) and len(idx["refs"][1]["bins"][4682]) == 1
    return bam, pred, None


def _case_bins():
    recs = [record(0, (1 << 14) - 10, M(20), name="b14"), record(0, (1 << 17) - 10, M(20), name="b17"), record(0, (1 << 26) - 10, M(20), name="b26"), record(0, (1 << 26) + 5, M(20), name="leaf")]
    bam = build_bam(REFS, recs)
    def pred(s, idx):
        b = idx["refs"][0]["bins"]
        return 0 in b and 585 in b and 73 in b and 4681 + (1 << 12) in b          # crossing 2^14 -> level 17 bin 585; crossing 2^17 -> level 20 bin 73; crossing 2^26 -> bin 0
    return bam, pred, None


def _case_windows():
    recs = [record(2, 5 << 14, [(7, 10), (3, (6 << 14)), (7, 10)], name="long"), record(2, (13 << 14) + 5, M(20), name="after")]
    bam = build_bam(REFS, recs)
    def pred(s, idx):
        lin = idx["refs"][2]["lin"]
        v0, v1 = s["recs"][0]["vbeg"], s["recs"][1]["vbeg"]
        # windows 5..11 set by the long read (7 >= 5), window 12 unset (takes window 11's value), window 13 the second record; windows 0..4 unset -> 0
        return len(lin) == 14 and lin[:5] == [0] * 5 and lin[5:12] == [v0] * 7 and lin[12] == v0 and lin[13] == v1 and v1 != v0
    return bam, pred, None


def _case_unmapped_placed():
    recs = [record(1, 500, M(50), name="m"), record(1, 500, M(50), flag=4 | 1 | 64, name="u"), record(1, 600, M(50), name="m2")]
    bam = build_bam(REFS, recs)
    def pred(s, idx):
        m = idx["refs"][1]["meta"]
        return m["n_mapped"] == 2 and m["n_unmapped"] == 1 and s["recs"][1]["end"] == 501
    return bam, pred, None


def _case_cg():
    recs = [record(2, 1000, [(7, 100), (3, 70000), (7, 100)], cg=True, name="cg"), record(2, 60000, M(10), name="in")]
    bam = build_bam(REFS, recs)
    def pred(s, idx):
        return s["recs"][0]["end"] == 1000 + 70200 and len(idx["refs"][2]["lin"]) == ((1000 + 70200 - 1) >> 14) + 1 and 585 in idx["refs"][2]["bins"]
    return bam, pred, None


def _case_empty_contig():
    recs = [record(0, 5, M(10), name="x"), record(2, 7, M(10), name="y")]
    bam = build_bam(REFS, recs)
    def pred(s, idx):
        r = idx["refs"]
        return r[0]["n_bin"] == 2 and r[1]["n_bin"] == 0 and r[1]["lin"] == [] and r[2]["n_bin"] == 2
    return bam, pred, None


def _case_no_coor_end():
    recs = [record(1, 5, M(10), name="x")] + [record(-1, -1, [], flag=4, name=f"n{i}") for i in range(3)] + [record(1, -1, [], flag=4, name="n3")]
    bam = build_bam(REFS, recs)
    return bam, (lambda s, idx: idx["n_no_coor"] == 4 and idx["refs"][1]["meta"]["n_mapped"] == 1), None


def _case_no_records():
    return build_bam(REFS, []), (lambda s, idx: idx["n_no_coor"] == 0 and all(r["n_bin"] == 0 for r in idx["refs"]) and len(s["recs"]) == 0), None


def _case_unsorted():
    recs = [record(1, 500, M(10), name="a"), record(1, 700, M(10), name="b"), record(1, 699, M(10), name="c")]
    return build_bam(REFS, recs), None, (ERR_ORDER, 2)


def _case_after_no_coor():
    recs = [record(1, 500, M(10), name="a"), record(-1, -1, [], flag=4, name="n"), record(1, 600, M(10), name="b")]
    return build_bam(REFS, recs), None, (ERR_ORDER, 2)


def _case_csi():
    recs = [record(0, 100, M(10), name="a"), record(0, (1 << 29) - 5, M(10), name="far")]
    return build_bam(REFS, recs), None, (ERR_CSI, 1)


CASES = {
    "record_ends_at_member_end": _case_member_end, "record_straddles_members": _case_straddle, "empty_member_in_the_middle": _case_empty_member,
    "bin_runs_same_member_merged": lambda: _case_runs(False), "bin_runs_members_apart": lambda: _case_runs(True), "bin0_and_level_crossings": _case_bins,
    "long_read_then_unset_window_and_unset_window0": _case_windows, "unmapped_but_placed": _case_unmapped_placed, "cg_tag_read": _case_cg,
    "empty_contig_between": _case_empty_contig, "no_coordinate_at_end": _case_no_coor_end, "no_records": _case_no_records,
    "refused_out_of_order": _case_unsorted, "refused_indexed_after_no_coordinate": _case_after_no_coor, "refused_end_over_2_29": _case_csi,
}


def table_arrays(recs):
    """the record table as the arrays lcd_bai_from_records takes"""
    return (np.array([x["tid"] for x in recs], np.int32), np.array([x["pos"] for x in recs], np.int64), np.array([x["end"] for x in recs], np.int64),
            np.array([x["flag"] for x in recs], np.int32), np.array([x["vbeg"] for x in recs], np.uint64), np.array([x["vend"] for x in recs], np.uint64))
