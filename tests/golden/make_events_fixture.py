"""Builds tests/golden/testdata_events.npz from the reference's bundled real input:
    /root/reference/test_data/chr11_2M.fa + HG002_chr11_hifi_test.bam   (HG002 HiFi, EQX CIGARs)
Run in the build container only (`python tests/golden/make_events_fixture.py`); the GPU box has no /root/reference.

DATA only: per read (primary, mapped, chr11, file order) its position, flag and EQX CIGAR; the bases and qualities at every X / I operation; the
qualities on either side of every D (the only ones collect_digar_from_eqx_cigar and get_digar_ave_qual read, src/bam_utils.c:258-280, :701-842);
and the reference slice the reads cover.  Everything else is rebuilt by tests/clean_vars_common.events_chunk: '=' bases are the reference's bases
(what '=' means), soft-clipped bases N, every other quality 30.  The generator checks that the digars of every rebuilt record equal those of the
full record (oracle/digar.c), and that the rebuilt '=' bases equal the record's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
TD = "/root/reference/test_data"
OUT = os.path.join(ROOT, "tests", "golden", "testdata_events.npz")
NT16 = np.array([4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4], np.uint8)


def read_bam_full(path):
    import gzip, struct
    d = gzip.open(path).read()
    lt, = struct.unpack_from("<i", d, 4)
    o = 8 + lt
    nref, = struct.unpack_from("<i", d, o); o += 4
    names, lens = [], []
    for _ in range(nref):
        ln, = struct.unpack_from("<i", d, o); o += 4
        names.append(d[o:o + ln - 1].decode()); o += ln
        lens.append(struct.unpack_from("<i", d, o)[0]); o += 4
    reads = []
    while o < len(d):
        bs, = struct.unpack_from("<i", d, o); o += 4
        refid, pos, lname, mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiBBHHHi", d, o)
        p = o + 32 + lname
        cig = np.frombuffer(d, "<u4", ncig, p).copy(); p += 4 * ncig
        bseq = np.frombuffer(d, np.uint8, (lseq + 1) // 2, p).copy(); p += (lseq + 1) // 2
        qual = np.frombuffer(d, np.uint8, lseq, p).copy()
        o += bs
        if flag & 0x904 or refid < 0 or names[refid] != "chr11":
            continue
        seq = NT16[(bseq[np.arange(lseq) >> 1] >> ((~np.arange(lseq) & 1) << 2)) & 0xf]
        reads.append(dict(pos0=pos, flag=flag, cigar=cig, seq=seq, qual=qual))
    return reads, lens[names.index("chr11")]


def main():
    from make_testdata_fixture import read_fasta
    from oracle import pyoracle as orc
    import clean_vars_common as cc
    orc.build()
    ref_all = read_fasta(os.path.join(TD, "chr11_2M.fa"))
    reads, tlen = read_bam_full(os.path.join(TD, "HG002_chr11_hifi_test.bam"))
    ref_beg = max(1, min(r["pos0"] for r in reads) + 1 - 100)
    ends = []
    ev_seq, ev_qual, del_qual = [], [], []
    n_ev, n_del = [], []
    for r in reads:
        pos, qi, es, eq, dq = r["pos0"] + 1, 0, [], [], []
        for c in r["cigar"]:
            op, ln = int(c & 0xf), int(c >> 4)
            if op in (8, 1):
                es += r["seq"][qi:qi + ln].tolist(); eq += r["qual"][qi:qi + ln].tolist()
            if op == 2:
                dq += [int(r["qual"][qi - 1]) if qi > 0 else 30, int(r["qual"][qi]) if qi < len(r["qual"]) else 30]
            if op in (7, 8, 2, 3):
                pos += ln
            if op in (7, 8, 1, 4):
                qi += ln
        ends.append(pos - 1)
        ev_seq += es; ev_qual += eq; del_qual += dq; n_ev.append(len(es)); n_del.append(len(dq) // 2)
    ref_end = min(len(ref_all), max(ends) + 100)
    z = dict(ref_beg=np.int64(ref_beg), ref=ref_all[ref_beg - 1:ref_end].astype(np.uint8), whole_ref_len=np.int64(tlen),
             pos0=np.array([r["pos0"] for r in reads], np.int64), flag=np.array([r["flag"] for r in reads], np.int32),
             cigar_off=np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]).astype(np.int64),
             cigar=np.concatenate([r["cigar"] for r in reads]).astype(np.uint32),
             ev_off=np.concatenate([[0], np.cumsum(n_ev)]).astype(np.int64), ev_seq=np.array(ev_seq, np.uint8), ev_qual=np.array(ev_qual, np.uint8),
             del_off=np.concatenate([[0], np.cumsum(n_del)]).astype(np.int64), del_qual=np.array(del_qual, np.uint8))
    np.savez_compressed(OUT, **z)
    ch = cc.events_chunk(OUT)
    reg_beg, reg_end = ch["reg_beg"], ch["reg_end"]
    for r, full in zip(ch["reads"], reads):
        a = orc.collect_digar_from_eqx_cigar(r["pos0"], r["cigar"], r["qual"], reg_beg, reg_end, tlen)
        b = orc.collect_digar_from_eqx_cigar(full["pos0"], full["cigar"], full["qual"], reg_beg, reg_end, tlen)
        assert a["rc"] == b["rc"] and (a["digars"] == b["digars"]).all() and (a["noisy"] == b["noisy"]).all() and a["beg"] == b["beg"] and a["end"] == b["end"]
        aligned = np.ones(len(full["seq"]), bool)
        qi = 0
        for c in full["cigar"]:
            op, ln = int(c & 0xf), int(c >> 4)
            if op == 4:
                aligned[qi:qi + ln] = False
            if op in (7, 8, 1, 4):
                qi += ln
        assert (r["seq"][aligned] == full["seq"][aligned]).all()
    print(f"{OUT}: {len(reads)} reads, {os.path.getsize(OUT)} bytes, region {reg_beg}-{reg_end}")


if __name__ == "__main__":
    main()
