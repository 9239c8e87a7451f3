"""Helpers of the several-input tests (lcd_chunk_open_from_bams, lcd_merged_record_plan, lcd_call_files): one sample's reads dealt out to several BAMs, and the
rules of include/lcd_hotpath.h ("one sample from several alignment files") restated in Python:
  1 a chunk's reads: for file 0, then file 1, ... the region iterator's records in file order with the flag / MAPQ filter -- the read ids and the record table are
    file-major;
  4 a record, kept or filtered, is left out of the alignment output if and only if it overlaps the region of the chunk before it on the same contig;
  5 sort_output: the records to be written in (pos0, file index, position in the file) order.
The BAM writer is call_file_common.write_multi_bam with a flag, a MAPQ and a name per record (that one writes MAPQ 60 and the strand flag only)."""
import struct

import numpy as np

import call_chunks_common as kc
import call_file_common as fc
from test_io import _bgzf, _write_bai

FILTER_FLAGS = 0x4 | 0x100 | 0x800
MIN_MAPQ = 30


def rec_flag(r):
    return int(r.get("flag", 16 if r["is_rev"] else 0))


def rec_kept(r, min_mapq=MIN_MAPQ):
    return not (rec_flag(r) & FILTER_FLAGS) and int(r.get("mapq", 60)) >= min_mapq


def write_bam(path, contigs, header_text=fc.DEFAULT_HEADER, block=30000):
    """contigs: [(name, length, reads)] in header order; reads: dicts with name, pos0, cigar, bseq (4-bit packed), qual, is_rev[, flag, mapq], sorted by pos0.
    Writes path and path + '.bai'; -> the record bodies in file order"""
    hdr = header_text
    d = b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", len(contigs))
    for nm, ln, _ in contigs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    recs, bodies = [], []
    for tid, (nm, _ln, reads) in enumerate(contigs):
        assert all(a["pos0"] <= b["pos0"] for a, b in zip(reads[:-1], reads[1:])), "records must be sorted"
        for r in reads:
            name = r["name"].encode() + b"\0"
            cig = np.asarray(r["cigar"], "<u4"); qlen = len(r["qual"])
            body = struct.pack("<iiBBHHHiiii", tid, r["pos0"], len(name), int(r.get("mapq", 60)), 4680, len(cig), rec_flag(r), qlen, -1, -1, 0) + name + cig.tobytes() + \
                np.asarray(r["bseq"], np.uint8).tobytes() + np.asarray(r["qual"], np.uint8).tobytes()
            u0 = len(d)
            d += struct.pack("<i", len(body)) + body
            bodies.append(body)
            recs.append(dict(tid=tid, pos=r["pos0"], end=max(kc.read_end(r), r["pos0"] + 1), u0=u0, u1=len(d)))
    coffs = []
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    coffs.append(coffs[-1] + 1)
    for x in recs:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", len(contigs), recs)
    return bodies


def deal(reads, contig, n_files=2, borders=(), filtered=True):
    """a contig's reads (sorted) dealt out: read i goes to file i % n_files, named <contig>_f<file>_r<i>.  With `filtered`, every file also gets, per border b (the
    last position of a chunk), two records the loader filters that straddle it: a copy of the file's first read over the border with the secondary flag and a copy of
    its last one with MAPQ 10, each right behind its original (equal pos0: the file stays sorted)"""
    files = [[] for _ in range(n_files)]
    for i, r in enumerate(reads):
        files[i % n_files].append(dict(r, name=f"{contig}_f{i % n_files}_r{i}"))
    if filtered:
        for f in range(n_files):
            for b in borders:
                over = [r for r in files[f] if r["pos0"] + 1 <= b and kc.read_end(r) >= b + 1 and "mapq" not in r and "flag" not in r]
                if not over:
                    continue
                for src, extra in ((over[0], dict(flag=0x100 | (16 if over[0]["is_rev"] else 0))), (over[-1], dict(mapq=10))):
                    k = max(i for i, r in enumerate(files[f]) if r is src or r.get("copy_of") == src["name"])
                    files[f].insert(k + 1, dict(src, name=src["name"] + ("_sec" if "flag" in extra else "_lowq"), copy_of=src["name"], **extra))
    return files


# ---------------- rules 1, 4 and 5 ----------------
def chunk_table(files, reg_beg, reg_end, min_mapq=MIN_MAPQ):
    """rule 1: files = per file its records of the contig in file order -> (rows, reads): rows = the chunk's record table, file-major, dicts(file, idx = position in
    the file's list, pos0, end = bam_endpos, read = chunk read id or -1); reads = the kept records in read-id order.  Sorted input: a file's walk stops at the first
    record at or behind reg_end"""
    rows, reads = [], []
    for f, recs in enumerate(files):
        for i, r in enumerate(recs):
            end = max(kc.read_end(r), r["pos0"] + 1)
            if r["pos0"] >= reg_end:
                break
            if end <= reg_beg - 1:
                continue
            kept = rec_kept(r, min_mapq)
            rows.append(dict(file=f, idx=i, pos0=int(r["pos0"]), end=int(end), read=len(reads) if kept else -1))
            if kept:
                reads.append(r)
    return rows, reads


def python_plan(rows, has_prev, prev_beg, prev_end, sort_output):
    """rules 4 and 5 -> (skip mask, the rows to write in output order)"""
    skip = [bool(has_prev) and not (r["end"] < prev_beg or r["pos0"] + 1 > prev_end) for r in rows]
    order = [i for i in range(len(rows)) if not skip[i]]
    if sort_output:
        order.sort(key=lambda i: (rows[i]["pos0"], rows[i]["file"], rows[i]["idx"]))
    return skip, order


def plan_of(lcd, rows, has_prev, prev_beg, prev_end, sort_output, with_files=True):
    """lcd_merged_record_plan on the table -> (skip mask, order) as lists"""
    skip, order = lcd.merged_record_plan([r["file"] for r in rows] if with_files else None, [r["pos0"] for r in rows], [r["end"] for r in rows], has_prev, prev_beg,
                                         prev_end, sort_output)
    return skip.tolist(), order.tolist()


def seeded_contigs():
    """the contigs of the whole-file tests: chr1 / chr2 = the seeded 12 kb diploid contigs of kc.two_chunks, chr3 = 18 kb"""
    import clean_vars_common as cc
    return dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12),
                chr3=cc.make_diploid_chunk(41, ref_len=18000, depth=12))


def regions_of(length, chunk_len=6000):
    return [(b, min(b + chunk_len - 1, length)) for b in range(1, length + 1, chunk_len)]
