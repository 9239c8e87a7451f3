"""Helpers of the whole-file tests (lcd_plan_chunks, lcd_call_files): a multi-contig BAM + .bai writer and a multi-contig FASTA + .fai writer built from the
writers of tests/test_io.py, and the chunk plan restated in Python from the rules of include/lcd_hotpath.h (collect_regions, src/call_var_main.c:404-634)."""
import struct

import numpy as np

from test_io import _bgzf, _write_bai

CTG_AUTOSOME_XY, CTG_AUTOSOME, CTG_ALL = 0, 1, 2
DEFAULT_HEADER = b"@HD\tVN:1.6\tSO:coordinate\n"


def m_cigar(cig):
    """an EQX CIGAR as minimap2 writes it without --eqx: '=' and 'X' runs joined into 'M' (tests/test_gpu_call_chunks.py)"""
    out = []
    for c in cig:
        op, ln = int(c) & 0xf, int(c) >> 4
        op = 0 if op in (7, 8) else op
        if out and out[-1][0] == op:
            out[-1][1] += ln
        else:
            out.append([op, ln])
    return np.array([(ln << 4) | op for op, ln in out], np.uint32)


def write_multi_bam(path, contigs, header_text=DEFAULT_HEADER, block=30000):
    """contigs: [(name, length, reads)] in header order; reads: dicts with pos0, cigar, bseq (4-bit packed), qual, is_rev, sorted by pos0.  Read names are
    <contig>_r<i>.  Writes path and path + '.bai'."""
    hdr = header_text
    d = b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", len(contigs))
    for nm, ln, _ in contigs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    recs = []
    for tid, (nm, _ln, reads) in enumerate(contigs):
        for i, r in enumerate(reads):
            name = f"{nm}_r{i}".encode() + b"\0"
            cig = np.asarray(r["cigar"], "<u4"); qlen = len(r["qual"])
            flag = 16 if r["is_rev"] else 0
            body = struct.pack("<iiBBHHHiiii", tid, r["pos0"], len(name), 60, 4680, len(cig), flag, qlen, -1, -1, 0) + name + cig.tobytes() + \
                np.asarray(r["bseq"], np.uint8).tobytes() + np.asarray(r["qual"], np.uint8).tobytes()
            u0 = len(d)
            d += struct.pack("<i", len(body)) + body
            rl = sum(int(c) >> 4 for c in cig if (int(c) & 0xf) in (0, 2, 3, 7, 8))
            recs.append(dict(tid=tid, pos=r["pos0"], end=r["pos0"] + max(rl, 1), u0=u0, u1=len(d)))
    coffs = []
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    coffs.append(coffs[-1] + 1)
    for x in recs:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", len(contigs), recs)


def write_multi_fasta(path, contigs, width=60):
    """contigs: [(name, codes 0-4 as a uint8 array)] -> path and path + '.fai'"""
    fai, off = [], 0
    with open(path, "w") as f:
        for nm, seq in contigs:
            text = np.frombuffer(b"ACGTN", np.uint8)[np.asarray(seq, np.uint8)].tobytes().decode()
            head = f">{nm}\n"
            f.write(head); off += len(head)
            fai.append(f"{nm}\t{len(text)}\t{off}\t{width}\t{width + 1}\n")
            for i in range(0, len(text), width):
                line = text[i:i + width] + "\n"
                f.write(line); off += len(line)
    with open(path + ".fai", "w") as f:
        f.write("".join(fai))


# ---------------- the plan, from the rules ----------------
def classify(name):
    """0 autosome, 1 sex chromosome, 2 other"""
    s = name.split(":")[0]
    if s.startswith("chr"):
        s = s[3:]
    if s in ("X", "Y"):
        return 1
    if s in ("M", "MT"):
        return 2
    t = s.lstrip(" \t\n\v\f\r")                       # strtol skips leading white space, takes a sign and digits and must consume the whole name
    body = t[1:] if t[:1] in ("+", "-") else t
    if body.isascii() and body.isdigit() and int(t) >= 1:
        return 0
    return 2


def _kept(name, mode, exclude):
    t = classify(name)
    if mode == CTG_AUTOSOME and t != 0:
        return False
    if mode == CTG_AUTOSOME_XY and t not in (0, 1):
        return False
    return name not in exclude


def _cut(tid, beg, end, L):
    return [(tid, b, min(b + L - 1, end)) for b in range(beg, end + 1, L)]


def _atoi(s):
    """C's atoi: optional white space and sign, then the leading digits; 0 without any"""
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def python_plan(contigs, mode=CTG_AUTOSOME_XY, exclude=(), regions=(), bed_text=None, chunk_len=0):
    """-> ([(tid, reg_beg, reg_end)], fallback)"""
    L = chunk_len or 500000
    names = [c[0] for c in contigs]; lens = [c[1] for c in contigs]
    regs = None
    if regions:
        regs = []
        for s in regions:
            if s in names:
                regs.append((names.index(s), 1, lens[names.index(s)])); continue
            if ":" not in s:
                continue
            nm, iv = s.rsplit(":", 1)
            if nm not in names:
                continue
            tid = names.index(nm)
            parts = iv.replace(",", "").split("-", 1)
            try:
                beg = int(parts[0]); end = int(parts[1]) if len(parts) > 1 and parts[1] != "" else lens[tid]
            except ValueError:
                continue
            regs.append((tid, beg, end))
    elif bed_text is not None:
        regs = []
        for line in bed_text.split("\n"):
            line = line.rstrip("\r")
            if not line or line.startswith("#"):
                continue
            col = [c for c in line.split("\t") if c != ""]
            if not col or col[0] not in names:
                continue
            tid = names.index(col[0])
            beg, end = 1, lens[tid]
            if len(col) > 1:
                beg = _atoi(col[1]) + 1
                if len(col) > 2:
                    end = _atoi(col[2])
            if beg > end or beg <= 0 or end <= 0:
                continue
            regs.append((tid, beg, end))
    plan = []
    if regs is None:
        for tid, nm in enumerate(names):
            if _kept(nm, mode, exclude):
                plan += _cut(tid, 1, lens[tid], L)
    else:
        keep = []
        for tid, beg, end in regs:
            if names[tid] in exclude:
                continue
            beg, end = max(1, beg), min(end, lens[tid])
            if beg <= end:
                keep.append((tid, beg, end))
        keep.sort(key=lambda r: (r[0], r[1]))                 # (Python's sort is stable)
        merged = []
        for tid, beg, end in keep:
            if merged and merged[-1][0] == tid and beg <= merged[-1][2]:
                merged[-1] = (tid, merged[-1][1], max(merged[-1][2], end))
            else:
                merged.append((tid, beg, end))
        for tid, beg, end in merged:
            plan += _cut(tid, beg, end, L)
    if plan:
        return plan, 0
    for tid, nm in enumerate(names):
        if nm not in exclude:
            plan += _cut(tid, 1, lens[tid], L)
    return plan, 1
