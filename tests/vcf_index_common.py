"""The .tbi / .csi oracle: an independent pure-Python index writer and reader (struct + zlib + re) written from the rules of include/lcd_hotpath.h ("VCF indexes")
and from the tabix / CSI specifications, a .vcf.gz generator with explicit BGZF member borders, and the table of named cases.  Every case carries a predicate that
proves from the ORACLE's own output that the case is reached (tests/bai_common.py does the same for the .bai).  Nothing here touches the library.

    build_gz(text, cuts, payloads, rng) -> bytes of a BGZF file whose members end exactly at the given offsets of the text
    scan_vcf(gz, fmt)                   -> member table, data lines (contig, interval, virtual offsets), the header's longest contig length; Refused(code, line)
    oracle_tbi / oracle_csi(scan)       -> the UNCOMPRESSED index bytes; Refused(code, None) when the format cannot hold the file
    parse_tbi / parse_csi, query, lines_through_index -> the reader of the specifications (htslib's lookup of the smallest offset included)
"""
import re
import struct
import zlib

import numpy as np

ERR_ORDER, ERR_CSI, ERR_LINE = -55, -56, -57
TBI, CSI = "tbi", "csi"
MAX_DEPTH = 8
PAYLOADS = (1, 300, 2000, 7000)


class Refused(Exception):
    def __init__(self, code, line):
        super().__init__(f"code {code} at data line {line}")
        self.code, self.line = code, line


# ---------------------------------------------------------------- BGZF ----------------------------------------------------------------
def member(payload):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


def build_gz(text, cuts=(), payloads=None, rng=None, eof=True):
    """members of `text`: `cuts` are offsets at which a member ends (a value given twice leaves an empty member there); between them the text is cut by
    `payloads` (cycled; default 65280) or by sizes drawn from PAYLOADS with rng"""
    out, at, k, bi = b"", 0, 0, 0
    borders = sorted(c for c in cuts if 0 <= c <= len(text))
    while at < len(text) or bi < len(borders):
        size = int(rng.choice(PAYLOADS)) if rng is not None else (payloads[k % len(payloads)] if payloads else 65280)
        k += 1
        end = min(len(text), at + size)
        if bi < len(borders) and borders[bi] <= end:
            end = borders[bi]; bi += 1
        out += member(text[at:end])
        at = end
    return out + (member(b"") if eof else b"")


def members_of(gz):
    """[(compressed offset, inflated offset, payload length)] + the inflated stream"""
    tab, parts, o, u = [], [], 0, 0
    while o < len(gz):
        assert gz[o:o + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", gz, o + 16)[0] + 1
        payload = zlib.decompress(gz[o + 18:o + bsize - 8], -15)
        assert len(payload) == struct.unpack_from("<I", gz, o + bsize - 4)[0]
        tab.append((o, u, len(payload))); parts.append(payload)
        o += bsize; u += len(payload)
    return tab, b"".join(parts)


def inflate(gz):
    return members_of(gz)[1]


def ends_with_eof_member(gz):
    return gz[-28:] == member(b"")


def voff(tab, fsize, p):
    """rule 5: the member whose payload holds byte p - 1; at that payload's very end the immediately following member's start (the file size if none follows)"""
    if not tab:
        return fsize << 16
    if p <= tab[0][1]:
        return tab[0][0] << 16
    for k, (c, u, n) in enumerate(tab):
        if u + n >= p:
            if p < u + n:
                return (c << 16) | (p - u)
            return (tab[k + 1][0] if k + 1 < len(tab) else fsize) << 16
    raise AssertionError("offset behind the stream")


# ---------------------------------------------------------------- the line scanner ----------------------------------------------------------------
def interval_of(cols):
    """rule 3 -> (beg, end) of a data line's columns"""
    pos = int(cols[1])
    beg = max(pos - 1, 0)
    end = beg + max(1, len(cols[3]))
    info = cols[7]
    v = None
    if info.startswith(b"END="):
        v = info[4:]
    else:
        k = info.find(b";END=")
        if k >= 0:
            v = info[k + 5:]
    if v is not None:
        m = re.match(rb"[0-9]+", v)
        if m and int(m.group()) > beg:
            end = int(m.group())
    return beg, end


def scan_vcf(gz, fmt=TBI):
    """-> dict(tab, stream, fsize, lines, names, n_meta, max_clen); lines = [dict(tid, chrom, beg, end, u0, u1, vbeg, vend)] in file order.  Refused(code, data line)
    for the first refused line (rules 2-4 and the cap of rule 6)"""
    tab, d = members_of(gz)
    fsize = len(gz)
    cap = 1 << 29 if fmt == TBI else 1 << (14 + 3 * MAX_DEPTH)
    lines, names, tids, n_meta, max_clen = [], [], {}, 0, 0
    o, prev = 0, None
    while o < len(d):
        e = d.find(b"\n", o)
        u1 = len(d) if e < 0 else e + 1
        ln = d[o:(len(d) if e < 0 else e)]
        if ln[:1] == b"#":
            n_meta += 1
            if ln.startswith(b"##contig=<"):
                m = re.search(rb"[<,]length=", ln[9:])
                if m:
                    dg = re.match(rb"[0-9]+", ln[9 + m.end():])
                    if dg:
                        max_clen = max(max_clen, int(dg.group()))
        else:
            no = len(lines)
            cols = ln.split(b"\t")
            if len(cols) < 8 or not cols[0] or not re.fullmatch(rb"[0-9]+", cols[1]):
                raise Refused(ERR_LINE, no)
            beg, end = interval_of(cols)
            if end > cap:
                raise Refused(ERR_CSI, no)
            if prev is not None and prev[0] == cols[0]:
                if beg < prev[1]:
                    raise Refused(ERR_ORDER, no)
            else:
                if cols[0] in tids:
                    raise Refused(ERR_ORDER, no)
                tids[cols[0]] = len(names); names.append(cols[0])
            prev = (cols[0], beg)
            lines.append(dict(tid=tids[cols[0]], chrom=cols[0], beg=beg, end=end, u0=o, u1=u1, vbeg=voff(tab, fsize, o), vend=voff(tab, fsize, u1)))
        o = u1
    return dict(tab=tab, stream=d, fsize=fsize, lines=lines, names=names, n_meta=n_meta, max_clen=max_clen)


# ---------------------------------------------------------------- the index: writer ----------------------------------------------------------------
def reg2bin(beg, end, depth):
    """hts_reg2bin of the CSI specification with min_shift 14"""
    end -= 1
    s, t = 14, ((1 << (3 * depth)) - 1) // 7
    for lv in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (lv - 1))
    return 0


def bin_interval(b, depth):
    """[lo, hi) of bin b"""
    for lv in range(depth + 1):
        first = ((1 << (3 * lv)) - 1) // 7
        if b < first + (1 << (3 * lv)):
            sh = 14 + 3 * (depth - lv)
            return (b - first) << sh, (b - first + 1) << sh
    raise AssertionError("bin outside the depth")


def depth_of(scan):
    want = scan["max_clen"] if scan["max_clen"] > 0 else max([x["end"] for x in scan["lines"]], default=0)
    d = 5
    while (1 << (14 + 3 * d)) < want:
        d += 1
    return d


def _contigs(scan, depth):
    per = [dict(bins={}, lin={}, n=0, first=None, last=None, rows=[]) for _ in scan["names"]]
    run = None
    for x in scan["lines"]:
        b = reg2bin(x["beg"], x["end"], depth)
        c = per[x["tid"]]
        if run == (x["tid"], b):
            c["bins"][b][-1][1] = x["vend"]
        else:
            ch = c["bins"].setdefault(b, [])
            if ch and ch[-1][1] >> 16 >= x["vbeg"] >> 16:
                ch[-1][1] = x["vend"]
            else:
                ch.append([x["vbeg"], x["vend"]])
            run = (x["tid"], b)
        c["n"] += 1
        c["first"] = x["vbeg"] if c["first"] is None else c["first"]
        c["last"] = x["vend"]
        c["rows"].append((x["beg"], x["end"], x["vbeg"]))
        for w in range(x["beg"] >> 14, ((x["end"] - 1) >> 14) + 1):
            c["lin"][w] = min(c["lin"].get(w, x["vbeg"]), x["vbeg"])
    return per


def _aux(names):
    nm = b"".join(n + b"\0" for n in names)
    return struct.pack("<iiiiii", 2, 1, 2, 0, ord("#"), 0) + struct.pack("<i", len(nm)) + nm


def oracle_tbi(scan):
    if any(x["end"] > 1 << 29 for x in scan["lines"]):
        raise Refused(ERR_CSI, None)
    out = b"TBI\x01" + struct.pack("<i", len(scan["names"])) + _aux(scan["names"])
    for c in _contigs(scan, 5):
        out += struct.pack("<i", len(c["bins"]) + 1)
        for b in sorted(c["bins"]):
            out += struct.pack("<Ii", b, len(c["bins"][b])) + b"".join(struct.pack("<QQ", s, e) for s, e in c["bins"][b])
        out += struct.pack("<IiQQQQ", 37450, 2, c["first"], c["last"], c["n"], 0)
        n_intv = max(c["lin"]) + 1
        offs, p = [], 0
        for w in range(n_intv):
            p = c["lin"].get(w, p); offs.append(p)
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in offs)
    return out + struct.pack("<Q", 0)


def oracle_csi(scan):
    depth = depth_of(scan)
    if depth > MAX_DEPTH or any(x["end"] > 1 << (14 + 3 * depth) for x in scan["lines"]):
        raise Refused(ERR_CSI, None)
    aux = _aux(scan["names"])
    out = b"CSI\x01" + struct.pack("<iii", 14, depth, len(aux)) + aux + struct.pack("<i", len(scan["names"]))
    for c in _contigs(scan, depth):
        rows = np.array(c["rows"], dtype=np.int64).reshape(-1, 3)
        out += struct.pack("<i", len(c["bins"]) + 1)
        for b in sorted(c["bins"]):
            lo, hi = bin_interval(b, depth)
            over = rows[(rows[:, 0] < hi) & (rows[:, 1] > lo)]            # rule 9 as its definition says: every line of the contig that overlaps the bin's interval
            out += struct.pack("<IQi", b, int(over[:, 2].min()), len(c["bins"][b])) + b"".join(struct.pack("<QQ", s, e) for s, e in c["bins"][b])
        out += struct.pack("<IQiQQQQ", ((1 << (3 * depth + 3)) - 1) // 7 + 1, 0, 2, c["first"], c["last"], c["n"], 0)
    return out + struct.pack("<Q", 0)


def oracle_index(scan, fmt):
    return oracle_tbi(scan) if fmt == TBI else oracle_csi(scan)


# ---------------------------------------------------------------- the index: reader ----------------------------------------------------------------
def _parse_aux(b, o):
    fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<iiiiiii", b, o)
    names = b[o + 28:o + 28 + l_nm].split(b"\0")[:-1] if l_nm else []
    return dict(format=fmt, col_seq=cs, col_beg=cb, col_end=ce, meta=meta, skip=skip, names=names), o + 28 + l_nm


def parse_tbi(b):
    assert b[:4] == b"TBI\x01"
    n_ref = struct.unpack_from("<i", b, 4)[0]
    hdr, o = _parse_aux(b, 8)
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, o)[0]; o += 4
        bins, meta = {}, None
        for _k in range(n_bin):
            bn, nch = struct.unpack_from("<Ii", b, o); o += 8
            ch = [struct.unpack_from("<QQ", b, o + 16 * k) for k in range(nch)]; o += 16 * nch
            if bn == 37450:
                meta = dict(off_beg=ch[0][0], off_end=ch[0][1], n=ch[1][0])
            else:
                bins[bn] = ch
        n_intv = struct.unpack_from("<i", b, o)[0]; o += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", b, o)); o += 8 * n_intv
        refs.append(dict(bins=bins, lin=lin, meta=meta, n_bin=n_bin))
    assert o + 8 == len(b) and struct.unpack_from("<Q", b, o)[0] == 0
    return dict(fmt=TBI, depth=5, hdr=hdr, refs=refs)


def parse_csi(b):
    assert b[:4] == b"CSI\x01"
    min_shift, depth, l_aux = struct.unpack_from("<iii", b, 4)
    assert min_shift == 14
    hdr, o = _parse_aux(b, 16)
    assert o == 16 + l_aux
    n_ref = struct.unpack_from("<i", b, o)[0]; o += 4
    pseudo = ((1 << (3 * depth + 3)) - 1) // 7 + 1
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, o)[0]; o += 4
        bins, loff, meta = {}, {}, None
        for _k in range(n_bin):
            bn, lo, nch = struct.unpack_from("<IQi", b, o); o += 16
            ch = [struct.unpack_from("<QQ", b, o + 16 * k) for k in range(nch)]; o += 16 * nch
            if bn == pseudo:
                meta = dict(off_beg=ch[0][0], off_end=ch[0][1], n=ch[1][0])
            else:
                bins[bn] = ch; loff[bn] = lo
        refs.append(dict(bins=bins, loff=loff, meta=meta, n_bin=n_bin))
    assert o + 8 == len(b) and struct.unpack_from("<Q", b, o)[0] == 0
    return dict(fmt=CSI, depth=depth, hdr=hdr, refs=refs)


def parse_index(b):
    return parse_tbi(b) if b[:3] == b"TBI" else parse_csi(b)


def reg2bins(beg, end, depth):
    end -= 1
    out, s, t = [], 14 + 3 * depth, 0
    for lv in range(depth + 1):
        out += list(range(t + (beg >> s), t + (end >> s) + 1))
        t += 1 << (3 * lv)
        s -= 3
    return out


def query(idx, tid, beg, end):
    """the merged chunks that can hold lines overlapping [beg, end): the region's bins, cut at the smallest offset as htslib's lookup finds it -- TBI: the linear
    index's value of beg's window; CSI: the loffset of beg's leaf bin or, while that bin is absent, of the bin to its left among its siblings, else of its parent"""
    r = idx["refs"][tid]
    if not r["bins"] or end <= beg:
        return []
    depth = idx["depth"]
    if idx["fmt"] == TBI:
        lin = r["lin"]
        min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    else:
        b = ((1 << (3 * depth)) - 1) // 7 + (beg >> 14)
        while b and b not in r["loff"]:
            parent = (b - 1) >> 3
            b = b - 1 if b > (parent << 3) + 1 else parent
        min_off = r["loff"].get(b, 0)
    ch = sorted(c for b in reg2bins(beg, end, depth) for c in r["bins"].get(b, ()) if c[1] > min_off)
    merged = []
    for s, e in ch:
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return merged


def lines_through_index(scan, idx, tid, beg, end):
    """the data lines (indices) a reader finds: it seeks to each chunk's begin, reads lines until the chunk's end, keeps those of the contig that overlap"""
    by_v = {}
    for i, x in enumerate(scan["lines"]):
        by_v.setdefault(x["vbeg"], i)
    got = []
    for s, e in query(idx, tid, beg, end):
        assert s in by_v, "a chunk does not begin at a line"
        i = by_v[s]
        while i < len(scan["lines"]) and scan["lines"][i]["vbeg"] < e:
            x = scan["lines"][i]
            if x["tid"] == tid and x["beg"] < end and x["end"] > beg:
                got.append(i)
            i += 1
    return got


def lines_by_scan(scan, tid, beg, end):
    return [i for i, x in enumerate(scan["lines"]) if x["tid"] == tid and x["beg"] < end and x["end"] > beg]


def regions_for(rng, scan, tid, n_random):
    """whole contig, single bases, windows aligned to 2^14 and to 2^14 +- 1, random ones, and regions past the contig's last line: (beg, end) 0-based half-open"""
    ln = max(x["end"] for x in scan["lines"] if x["tid"] == tid) + 40000
    out = [(0, ln), (ln - 30000, ln), (ln + 5, ln + 100000)]
    for _ in range(n_random // 4):
        p = int(rng.integers(0, ln)); out.append((p, p + 1))
    for _ in range(n_random // 4):
        w = int(rng.integers(0, (ln >> 14) + 1)) << 14
        d0, d1 = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
        b = max(0, w + d0); out.append((b, max(b + 1, w + (int(rng.integers(1, 4)) << 14) + d1)))
    for _ in range(n_random // 2):
        b = int(rng.integers(0, ln)); out.append((b, b + int(rng.integers(1, 60000))))
    return out


# ---------------------------------------------------------------- seeded files ----------------------------------------------------------------
HEADER = b"##fileformat=VCFv4.2\n##source=test\n"
COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"


def header(contigs=()):
    """contigs: [(name, length or None)]"""
    h = HEADER
    for nm, ln in contigs:
        h += b"##contig=<ID=" + nm + (b",length=%d" % ln if ln is not None else b"") + b">\n"
    return h + COLS


def line(chrom, pos, ref=b"A", alt=b"C", info=b"DP=10", tail=b"\tGT\t0|1"):
    return b"\t".join([chrom, b"%d" % pos, b".", ref, alt, b"30", b"PASS", info]) + tail + b"\n"


def seeded_text(seed, n=300, contig_lengths=True):
    """n data lines over four contigs (a fifth is named in the header and stays empty): SNVs, short indels, deletions with END up to 150 kb, an ALT of a few kb now
    and then, dense stretches and sparse ones (unset windows), a meta line in the middle"""
    rng = np.random.default_rng(seed)
    ctg = [(b"chr1", 3000000), (b"chrEmpty", 50000), (b"chr2", 900000), (b"chrUn_x", 120000), (b"chrM", 16569)]
    out = header([(nm, ln if contig_lengths else None) for nm, ln in ctg])
    share = rng.multinomial(n, [0.5, 0.3, 0.15, 0.05])
    for (nm, ln), k in zip([ctg[0], ctg[2], ctg[3], ctg[4]], share):
        pos = np.sort(np.concatenate([rng.integers(1, ln, k - k // 3), rng.integers(ln // 3, ln // 3 + 3000, k // 3)]))
        for i, p in enumerate(pos):
            kind = rng.random()
            if kind < 0.6:
                out += line(nm, int(p), b"ACGT"[int(rng.integers(0, 4))::4] or b"A", b"T")
            elif kind < 0.8:
                out += line(nm, int(p), b"A" * int(rng.integers(2, 40)), b"A", info=b"SVTYPE=DEL;CIEND=-5,5")
            elif kind < 0.95:
                out += line(nm, int(p), b"N", b"<DEL>", info=b"SVTYPE=DEL;SVLEN=-1;END=%d" % (int(p) + int(rng.choice([50, 20000, 150000]))))
            else:
                out += line(nm, int(p), b"G", b"G" + b"ACGT" * int(rng.integers(200, 1500)), info=b"END=%d;SVTYPE=INS" % int(p), tail=b"\tGT:ALTREADS\t1|0:" + b"r1,r2," * 50)
            if i == k // 2 and nm == b"chr2":
                out += b"##a meta line between data lines\n"
    return out


def seeded_gz(seed, n=300, contig_lengths=True):
    return build_gz(seeded_text(seed, n, contig_lengths), rng=np.random.default_rng(seed + 1000))


SEEDS = list(range(201, 209))


# ---------------------------------------------------------------- named cases ----------------------------------------------------------------
# a case -> (gz bytes, format, predicate(scan, parsed index) or None, refusal (code, data line or None) or None)
def _n_members(s, x):
    return sum(1 for _c, u, n in s["tab"] if n and u < x["u1"] and u + n > x["u0"])


def _case_count(n):
    def make():
        text = header([(b"c1", 1 << 20)]) + b"".join(line(b"c1", 10 + 37 * i) for i in range(n))
        return build_gz(text, payloads=[4000]), TBI, (lambda s, idx: len(s["lines"]) == n and len(idx["refs"]) == (1 if n else 0) and (n == 0 or idx["refs"][0]["meta"]["n"] == n)), None
    return make


def _case_member_end():
    ls = [line(b"c1", 100 * (i + 1)) for i in range(6)]
    h = header()
    o = np.cumsum([len(h)] + [len(x) for x in ls])
    gz = build_gz(h + b"".join(ls), cuts=[int(o[2]), int(o[4])])
    def pred(s, idx):
        r, starts = s["lines"], {c for c, _u, _n in s["tab"]}
        return all(r[i]["vend"] & 0xffff == 0 and (r[i]["vend"] >> 16) in starts and r[i]["vend"] == r[i + 1]["vbeg"] for i in (1, 3))
    return gz, TBI, pred, None


def _case_last_byte():
    ls = [line(b"c1", 100 * (i + 1)) for i in range(4)]
    h = header()
    o = np.cumsum([len(h)] + [len(x) for x in ls])
    gz = build_gz(h + b"".join(ls), cuts=[int(o[2]) + 1])
    def pred(s, idx):
        x = s["lines"][2]
        m = [(c, u, n) for c, u, n in s["tab"] if u <= x["u0"] < u + n][0]
        return x["u0"] == m[1] + m[2] - 1 and _n_members(s, x) == 2
    return gz, TBI, pred, None


def _case_long_line():
    text = header() + line(b"c1", 50) + line(b"c1", 60, b"A", b"A" + b"ACGT" * 50000) + line(b"c1", 70)
    return build_gz(text), TBI, (lambda s, idx: _n_members(s, s["lines"][1]) == 4 and s["lines"][1]["u1"] - s["lines"][1]["u0"] > 200000), None


def _case_straddle():
    text = header() + b"".join(line(b"c1", 10 * (i + 1), b"A" * 700) for i in range(12))
    return build_gz(text, payloads=[1000]), TBI, (lambda s, idx: sum(_n_members(s, x) >= 2 for x in s["lines"]) >= 6), None


def _case_no_newline():
    text = header() + line(b"c1", 5) + line(b"c2", 9)[:-1]
    return build_gz(text), TBI, (lambda s, idx: s["stream"][-1:] != b"\n" and len(s["lines"]) == 2 and s["lines"][1]["vend"] == s["tab"][-1][0] << 16), None


def _case_info_forms():
    text = header() + b"".join([
        line(b"c1", 1000, info=b"END=5000;SVTYPE=DEL"), line(b"c1", 2000, info=b"SVTYPE=DEL;END=7000"), line(b"c1", 3000, info=b"CIEND=-9,9;SVEND=99999"),
        line(b"c1", 4000, info=b"END=.;X=1;END=90000"), line(b"c1", 5000, info=b"A=1;END=4000"), line(b"c1", 6000, info=b"END=6001"),
        line(b"c1", 7000, b"ACGT", info=b"X;END=9000", tail=b""), line(b"c1", 8000, info=b"SVEND=5;END=8500;END=99")])
    want = [(999, 5000), (1999, 7000), (2999, 3000), (3999, 4000), (4999, 5000), (5999, 6001), (6999, 9000), (7999, 8500)]
    return build_gz(text), TBI, (lambda s, idx: [(x["beg"], x["end"]) for x in s["lines"]] == want), None


def _case_deletion():
    text = header() + line(b"c1", (5 << 14) + 1, b"N", b"<DEL>", info=b"END=%d" % ((5 << 14) + 100000)) + line(b"c1", (13 << 14) + 6)
    def pred(s, idx):
        lin, v0, v1 = idx["refs"][0]["lin"], s["lines"][0]["vbeg"], s["lines"][1]["vbeg"]
        return len(lin) == 14 and lin[:5] == [0] * 5 and lin[5:12] == [v0] * 7 and lin[12] == v0 and lin[13] == v1 and 73 in idx["refs"][0]["bins"] and 4681 + 13 in idx["refs"][0]["bins"]
    return build_gz(text), TBI, pred, None


def _case_pos0():
    text = header() + line(b"c1", 0) + line(b"c1", 1)
    return build_gz(text), TBI, (lambda s, idx: [(x["beg"], x["end"]) for x in s["lines"]] == [(0, 1), (0, 1)]), None


def _case_window0_after_many():
    text = header() + b"".join(line(b"c1", (i << 14) + 3) for i in range(40)) + line(b"c2", 7)
    return build_gz(text), TBI, (lambda s, idx: len(idx["refs"][0]["lin"]) == 40 and len(idx["refs"][1]["lin"]) == 1 and idx["refs"][1]["lin"][0] == s["lines"][40]["vbeg"]), None


def _case_meta_between():
    text = header() + line(b"c1", 5) + b"##late meta line\n" + line(b"c1", 6) + b"#another\n" + line(b"c2", 1)
    return build_gz(text), TBI, (lambda s, idx: s["n_meta"] == 5 and len(s["lines"]) == 3 and len(idx["refs"][0]["bins"][4681]) == 1), None


def _case_70_contigs():
    text = header() + b"".join(line(b"ctg%d" % i, 100 + i) for i in range(70))
    return build_gz(text), TBI, (lambda s, idx: len(idx["refs"]) == 70 and idx["hdr"]["names"][69] == b"ctg69"), None


def _case_csi_depth6():
    text = header([(b"big", 3000000000)]) + line(b"big", 100) + line(b"big", (1 << 29) + 50) + line(b"big", 2900000000, b"N", b"<DEL>", info=b"END=2900200000")
    return build_gz(text), CSI, (lambda s, idx: idx["depth"] == 6 and len(idx["refs"][0]["bins"]) == 3), None


def _case_csi_no_lengths():
    text = header([(b"big", None)]) + line(b"big", 100) + line(b"big", (1 << 30) + 50)
    return build_gz(text), CSI, (lambda s, idx: idx["depth"] == 6 and s["max_clen"] == 0), None


def _case_csi_small():
    return seeded_gz(77, 120), CSI, (lambda s, idx: idx["depth"] == 5 and s["max_clen"] == 3000000), None


def _refusal(body, fmt, code, no):
    return lambda: (build_gz(header() + body), fmt, None, (code, no))


CASES = {f"lines_{n}": _case_count(n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097)}
CASES.update({
    "line_ends_at_member_end": _case_member_end, "line_starts_at_last_byte_of_member": _case_last_byte, "line_200kb_over_four_members": _case_long_line,
    "lines_straddle_slab_borders": _case_straddle, "last_line_without_newline": _case_no_newline, "info_forms": _case_info_forms,
    "deletion_100kb_seven_windows": _case_deletion, "pos_0": _case_pos0, "window0_contig_after_many_windows": _case_window0_after_many,
    "meta_line_between_data_lines": _case_meta_between, "seventy_contigs": _case_70_contigs, "csi_depth6_from_header": _case_csi_depth6,
    "csi_depth6_from_largest_end": _case_csi_no_lengths, "csi_seeded_depth5": _case_csi_small,
    "refused_pos_decreasing": _refusal(line(b"c1", 500) + line(b"c1", 700) + line(b"c1", 699), TBI, ERR_ORDER, 2),
    "refused_contig_reappears": _refusal(line(b"c1", 500) + line(b"c2", 5) + line(b"c1", 900), TBI, ERR_ORDER, 2),
    "refused_seven_columns": _refusal(line(b"c1", 500) + b"c1\t600\t.\tA\tC\t30\tPASS\n", TBI, ERR_LINE, 1),
    "refused_pos_not_a_number": _refusal(line(b"c1", 500) + line(b"c1", 600).replace(b"600", b"6x0"), TBI, ERR_LINE, 1),
    "refused_end_over_2_29_tbi": _refusal(line(b"c1", 100) + line(b"c1", (1 << 29) + 5), TBI, ERR_CSI, 1),
})
