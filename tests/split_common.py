"""The per-haplotype read sets (lcd_chunk_split_reads, split_kernel.hip) restated in Python from their rules (include/lcd_hotpath.h): split_text formats the
records of a chunk's table that a plan names as three FASTQ byte strings and the haplotag list, with the statistics lcd_split_stats_t must show.  Beside it the
records the tests are made of, a table of named cases, and what reads an output BAM back into the streams a run must have written.  There is no reference
implementation: the rules are the project's.

Conventions: `table` is a chunk's record table as bam_out_common.region_records gives it, [(record body without its block_size word, chunk read id | -1)];
haps / phase_sets are per chunk read id; streams are 0 = none, 1, 2; the list has no header line (HEADER is the file writer's)."""
import struct

import numpy as np

import bam_out_common as bo
from bam_src_common import CONTIG, aux_walk, record, write_bam  # noqa: F401

NIB = "=ACMGRSVTWYHKDBN"
NIB_COMP = "=TGKCYSBAWRDMHVN"
HEADER = b"#readname\thaplotype\tphaseset\tchromosome\n"
STAT_KEYS = ("n_records", "n_selected", "n_hap", "n_not_primary", "n_filtered_primary", "n_reverse", "n_no_seq", "n_bad_layout", "bytes_fastq", "bytes_list")
EOF_MEMBER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
TLEN = 60000


# ---------------- one record ----------------
def parse(body):
    """-> dict(flag, refid, lseq, ok (the layout fits), qname (b"*" for an empty name), nibbles, quals); the last three only with ok"""
    refid, _pos, lname, _mapq, _bin, nc, flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    a_seq = 32 + lname + 4 * nc
    x = dict(flag=flag, refid=refid, lseq=lseq, ok=lseq >= 0 and a_seq + (lseq + 1) // 2 + lseq <= len(body))
    if x["ok"]:
        x["qname"] = body[32:32 + lname].split(b"\0")[0] or b"*"
        sq = body[a_seq:a_seq + (lseq + 1) // 2]
        x["nibbles"] = [(sq[q >> 1] >> (0 if q & 1 else 4)) & 15 for q in range(lseq)]
        x["quals"] = list(body[a_seq + (lseq + 1) // 2:a_seq + (lseq + 1) // 2 + lseq])
    return x


def seq_qual(x):
    """the read as sequenced: SEQ and QUAL text of a parsed record with bases"""
    nib, q = x["nibbles"], x["quals"]
    bang = q[0] == 0xff
    if x["flag"] & 0x10:
        seq = "".join(NIB_COMP[n] for n in reversed(nib)); q = q[::-1]
    else:
        seq = "".join(NIB[n] for n in nib)
    return seq.encode(), bytes(33 if bang else min(b, 93) + 33 for b in q)


def revcomp_body(body):
    """the record with its bases reverse-complemented, its qualities reversed and flag 0x10 toggled: it must give the entry of the original with 0x10 toggled twice"""
    x = parse(body)
    refid, pos, lname, mapq, bin_, nc, flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    a_seq = 32 + lname + 4 * nc
    comp = [NIB.index(NIB_COMP[n]) for n in reversed(x["nibbles"])] + [0]
    packed = bytes((comp[2 * k] << 4) | comp[2 * k + 1] for k in range((lseq + 1) // 2))
    return struct.pack("<iiBBHHHi", refid, pos, lname, mapq, bin_, nc, flag ^ 0x10, lseq) + body[20:a_seq] + packed + bytes(reversed(x["quals"])) + body[a_seq + (lseq + 1) // 2 + lseq:]


def fastq_entry(x, hap, ps, comment):
    name = x["qname"]
    if comment:
        name += (b"\tHP:i:%d" % hap if hap != 0 else b"") + (b"\tPS:i:%d" % ps if ps > 0 else b"")
    seq, qual = seq_qual(x)
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def list_line(x, hap, ps, names):
    nm = [n if isinstance(n, bytes) else n.encode() for n in names]
    chrom = nm[x["refid"]] if 0 <= x["refid"] < len(nm) and nm[x["refid"]] else b"*"
    return b"\t".join([x["qname"], b"H%d" % hap if hap else b"none", b"%d" % ps if ps > 0 else b"none", chrom]) + b"\n"


def split_text(table, haps, phase_sets, skip=None, order=None, names=None, comment=False):
    """-> ([FASTQ of stream 0, 1, 2], the list's lines (b"" without names), statistics)"""
    n = len(table)
    picked = [i for i in range(n) if skip is None or not skip[i]] if order is None else [int(i) for i in order if i >= 0]
    assert sorted(picked) == [i for i in range(n) if skip is None or not skip[i]]
    fq, lst = [[], [], []], []
    st = dict(n_records=len(picked), n_selected=0, n_hap=[0, 0, 0], n_not_primary=0, n_filtered_primary=0, n_reverse=0, n_no_seq=0, n_bad_layout=0)
    for i in picked:
        body, r = table[i]
        x = parse(body)
        if x["flag"] & 0x900:
            st["n_not_primary"] += 1; continue
        if not x["ok"]:
            st["n_bad_layout"] += 1; continue
        hap, ps = (int(haps[r]), int(phase_sets[r])) if r >= 0 else (0, 0)
        assert hap in (0, 1, 2)
        st["n_selected"] += 1; st["n_hap"][hap] += 1; st["n_filtered_primary"] += r < 0; st["n_reverse"] += bool(x["flag"] & 0x10)
        if x["lseq"] == 0:
            st["n_no_seq"] += 1
        else:
            fq[hap].append(fastq_entry(x, hap, ps, comment))
        if names is not None:
            lst.append(list_line(x, hap, ps, names))
    fq = [b"".join(f) for f in fq]
    st["bytes_fastq"] = [len(f) for f in fq]; st["bytes_list"] = sum(len(ln) for ln in lst)
    return fq, b"".join(lst), st


def offsets(stream, fq_len, list_len):
    """lcd_split_offsets in Python"""
    tot, fo, lo = [0, 0, 0, 0], [], []
    for s, f, ln in zip(stream, fq_len, list_len):
        fo.append(tot[s] if s >= 0 else 0); lo.append(tot[3])
        if s >= 0:
            tot[s] += f; tot[3] += ln
    return fo, lo, tot


def paths(prefix, gz=False):
    return [prefix + s + (".fastq.gz" if gz else ".fastq") for s in (".none", ".h1", ".h2")]


# ---------------- reading a run's own output back ----------------
def tags_of(body):
    """(HP, PS) of a written record: its first HP / PS field as an integer, 0 where there is none"""
    a0 = bo.parse(body)["aux0"]
    out = {}
    for tag, ty, val in aux_walk(body[a0:]):
        if tag in (b"HP", b"PS") and tag not in out:
            out[tag] = bo.aux2i(ty, val)
    return out.get(b"HP", 0), out.get(b"PS", 0)


def streams_of_bam(bodies, names, comment=False):
    """the records of an output BAM, in file order -> what the run's read sets and list must be: the primary records grouped by their HP tag"""
    table, haps, pss = [], [], []
    for b in bodies:
        hp, ps = tags_of(b)
        table.append((b, len(haps))); haps.append(hp); pss.append(ps)
    return split_text(table, haps, pss, names=names, comment=comment)


def fastq_entries(text):
    """a FASTQ byte string -> its entries (four lines each)"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines) - 1, 4)]


# ---------------- records ----------------
def pack_nibbles(nib):
    nib = list(nib) + [0]
    return np.array([(nib[2 * k] << 4) | nib[2 * k + 1] for k in range((len(nib) - 1 + 1) // 2)], np.uint8)


def make(name, pos1, nibbles, quals, flag=0, mapq=60, hap=0, ps=0):
    """a record at 1-based pos1 whose CIGAR is <l_seq>M (none for an empty read), with the given base codes and quality bytes"""
    n = len(nibbles)
    assert len(quals) == n
    a = dict(name=name, pos0=pos1 - 1, flag=flag, qlen=n, bseq=pack_nibbles(nibbles), qual=np.asarray(quals, np.uint8))
    r = record(a, [(n << 4) | 0] if n else [], [("NM", "i", 0)], mapq=mapq)
    r["end"] = min(r["end"], TLEN); r["hap"] = hap; r["ps"] = ps
    return r


def broken(name, pos1):
    """a record whose l_seq says more bases than its block holds"""
    r = make(name, pos1, [1, 2, 4, 8], [30] * 4)
    b = r["body"]
    r["body"] = b[:16] + struct.pack("<i", 4000) + b[20:]
    return r


REG_BEG = 2001
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 20000)
NAME_LENGTHS = (1, 63, 64, 65, 254)
PHASE_SETS = (1, 9, 10, (1 << 31) - 1, (1 << 32) + 5)


def case_table(with_broken=True):
    """[dict(name, rec)] in position order.  with_broken=False leaves the record out that no chunk can hold: the loader refuses a file with it"""
    rng = np.random.default_rng(2026)
    T, pos = [], [REG_BEG + 50]

    def add(name, **kw):
        n = kw.pop("n", 40)
        nib = kw.pop("nibbles", None)
        nib = [int(v) for v in rng.choice([1, 2, 4, 8], n)] if nib is None else nib
        q = kw.pop("quals", None)
        q = [int(v) for v in rng.integers(0, 94, len(nib))] if q is None else q
        rname = kw.pop("rname", name.encode())
        T.append(dict(name=name, rec=make(rname, pos[0], nib, q, **kw)))
        pos[0] += 7

    for k, n in enumerate(LENGTHS):
        for rev in (0, 0x10):
            add("len_%d_%s" % (n, "rev" if rev else "fwd"), n=n, flag=rev, hap=1 + k % 2, ps=REG_BEG)
    for rev in (0, 0x10):
        add("all_nibbles_%s" % ("rev" if rev else "fwd"), nibbles=list(range(16)) + list(range(15, -1, -1)) + [3], flag=rev, hap=2, ps=7)
        add("quals_edge_%s" % ("rev" if rev else "fwd"), nibbles=[1, 2, 4, 8, 15, 1, 2], quals=[0, 93, 94, 255, 1, 92, 200], flag=rev, hap=1, ps=7)
        add("quals_ff_first_%s" % ("rev" if rev else "fwd"), nibbles=[1, 2, 4, 8, 15], quals=[255, 0, 40, 93, 94], flag=rev, hap=0)
    for n in NAME_LENGTHS:
        add("name_%d" % n, rname=bytes(33 + (k * 7) % 90 for k in range(n)), n=5, hap=1, ps=3)
    add("name_empty", rname=b"", n=5, hap=2, ps=3)
    add("name_nul_inside", rname=b"ab\0cd", n=5, flag=0x10, hap=2, ps=3)
    for ps in PHASE_SETS:
        add("ps_%d" % ps, n=9, hap=1, ps=ps)
    add("ps_negative", n=9, hap=2, ps=-5)
    add("hap0_with_ps", n=9, hap=0, ps=12)
    add("hap2_no_ps", n=9, hap=2, ps=0)
    add("secondary", n=9, flag=0x100, hap=1)
    add("supplementary", n=9, flag=0x800 | 0x10, hap=1)
    add("unmapped_with_position", n=9, flag=0x4, hap=1, ps=5)
    add("low_mapq", n=9, mapq=3, hap=1, ps=5)
    add("low_mapq_reverse", n=9, mapq=3, flag=0x10, hap=2, ps=5)
    if with_broken:
        T.append(dict(name="broken_layout", rec=broken(b"broken", pos[0])))
        pos[0] += 7
    return T


def build_cases(with_broken=True):
    """-> dict(cases, recs, table (the chunk's record table of [REG_BEG, reg_end]), haps, phase_sets per kept read, reg_beg, reg_end)"""
    cases = case_table(with_broken)
    recs = [c["rec"] for c in cases]
    assert all(a["pos0"] < b["pos0"] for a, b in zip(recs, recs[1:]))
    reg_end = REG_BEG + 30000
    return dict(cases=cases, recs=recs, reg_beg=REG_BEG, reg_end=reg_end, **table_of(recs, REG_BEG, reg_end))


def table_of(recs, reg_beg, reg_end, min_mapq=30):
    """the region's record table with the records' own haplotypes and phase sets for its kept reads"""
    by_body = {id(r["body"]): r for r in recs}
    table = bo.region_records([r["body"] for r in recs], reg_beg, reg_end, min_mapq)
    kept = [by_body[id(b)] for b, k in table if k >= 0]
    return dict(table=table, haps=[r["hap"] for r in kept], phase_sets=[r["ps"] for r in kept])


def seeded_chunk(seed, n_rec=200):
    """random records of every kind around a region -> (recs, reg_beg, reg_end)"""
    rng = np.random.default_rng(seed)
    reg_beg, recs = 5000, []
    for i in range(n_rec):
        n = int(rng.choice([0, 1, 3, 62, 64, 66, 130, 300, 1000]))
        nib = [int(v) for v in rng.integers(0, 16, n)]
        q = [255] * n if rng.integers(0, 8) == 0 else [int(v) for v in rng.integers(0, 256, n)]
        recs.append(make(b"s%03d" % i + b"x" * int(rng.integers(0, 70)), reg_beg - 100 + 5 * i, nib, q, flag=int(rng.choice([0, 0, 0x10, 0x10, 0x100, 0x800, 0x4, 0x14])),
                         mapq=int(rng.choice([60, 60, 60, 5])), hap=int(rng.integers(0, 3)), ps=int(rng.choice([0, 1, 5000, 123456789012]))))
    return recs, reg_beg, reg_beg + 5 * n_rec
