"""Shared by the GPU tests of the refined one-call drivers: the two-chunk seeded BAM of tests/call_chunks_common.py written in the four spellings a read's alignment
comes in (EQX CIGAR; 'M' CIGAR + cs; 'M' CIGAR + MD; plain 'M'), and the oracle of a refined run composed from the existing oracles: per chunk the digars of each
record's own source, the first round, the rounds with their refine log (refine_common.oracle_rounds_log), the log applied in order, and the records rewritten from
the final digars (refine_common.refined_stream) under the writer's skip rule."""
import numpy as np

import bam_out_common as bo
import bam_src_common as bs
import call_chunks_common as kc
import clean_vars_common as cc
import refine_common as rc

CHROM = bs.CONTIG
KINDS = ("eqx", "cs", "md", "ref")


def cigar_digars(pos0, cigar):
    out, p, q = [], pos0 + 1, 0
    for w in cigar:
        o, l = int(w) & 0xf, int(w) >> 4
        out.append([p, o, l, q, 0])
        if o in (7, 8):
            p += l; q += l
        elif o == 2:
            p += l
        elif o in (1, 4):
            q += l
    return out


def m_cigar(cigar):
    out = []
    for w in cigar:
        o, l = int(w) & 0xf, int(w) >> 4
        o = 0 if o in (7, 8) else o
        if out and out[-1][0] == o == 0:
            out[-1][1] += l
        else:
            out.append([o, l])
    return np.array([(l << 4) | o for o, l in out], np.uint32)


def spelled_records(whole, kind):
    """the chunk's reads as bam_src_common.record()s of one spelling; read i is named r<i>"""
    ref, rb = whole["ref"], whole["ref_beg"]
    out = []
    for i, r in enumerate(whole["reads"]):
        a = dict(name=b"r%d" % i, pos0=int(r["pos0"]), flag=16 if r["is_rev"] else 0, qlen=len(r["qual"]), bseq=r["bseq"], qual=r["qual"])
        d = cigar_digars(a["pos0"], r["cigar"])
        far = rb + len(ref) + 1
        f = [("cs", "Z", rc.digars_cs(d, r["seq"], ref, rb, far))] if kind == "cs" else [("MD", "Z", rc.digars_md(d, ref, rb, far))] if kind == "md" else []
        out.append(bs.record(a, r["cigar"] if kind == "eqx" else m_cigar(r["cigar"]), f))
    return out


def write_inputs(tmp, seed, kind):
    whole = cc.make_diploid_chunk(seed, ref_len=12000, depth=12)
    recs = spelled_records(whole, kind)
    bam, fa = str(tmp / (kind + ".bam")), str(tmp / "ref.fa")
    bs.write_bam(bam, recs, block=30000, tlen=whole["whole_ref_len"])
    kc.write_fasta(fa, CHROM, whole)
    return whole, recs, bam, fa


def oracle_refined(lcd, oracle, whole, recs, regions, got_chunks, max_len):
    """-> (the record stream behind the header, [per chunk dict(log, final digars, states, stats)]) for the haplotypes / phase sets / read order the call arrived at"""
    letters = bytes(b"ACGTN"[b] for b in whole["ref"])
    rb, re_ = whole["ref_beg"], whole["ref_beg"] + len(whole["ref"]) - 1
    bodies = [r["body"] for r in recs]
    index_of = {b: i for i, b in enumerate(bodies)}
    stream, per = b"", []
    for c, (reg_beg, reg_end) in enumerate(regions):
        rr = bo.region_records(bodies, reg_beg, reg_end, 30)
        idx = [index_of[b] for b, r in rr if r >= 0]
        digs = [bs.expected(oracle, recs[i], letters, rb, re_, reg_beg, reg_end, 0)[2] for i in idx]
        ch = dict(whole, reads=[whole["reads"][i] for i in idx], reg_beg=reg_beg, reg_end=reg_end)
        g = got_chunks[c]
        ordered = np.asarray(g["ordered_read_ids"], np.int32)
        first = kc.first_round_chain(lcd, oracle, ch, digs, ordered)
        assert first["is_skipped"].tolist() == np.asarray(g["is_skipped"]).tolist()
        _, log, _, final = rc.oracle_rounds_log(oracle, ch, digs, first["cv"], first["state"], ordered, first["is_skipped"], max_len=max_len)
        skip = np.zeros(len(rr), np.uint8)
        if c:
            pb, pe = regions[c - 1]
            for k, (b, _r) in enumerate(rr):
                x = bo.parse(b)
                skip[k] = not (x["end"] < pb or x["pos0"] + 1 > pe)
        s, n, st, states = rc.refined_stream(rr, final, first["is_skipped"], whole["ref"], rb, re_, g["haps"], g["phase_sets"], skip)
        stream += s
        per.append(dict(log=log, final=final, digs=digs, states=states, stats=st, skip=skip, records=rr, n=n))
    return stream, per
