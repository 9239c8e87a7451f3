"""Measurement of the SAM text output's GPU side on ONE chunk of HiFi shape: a synthetic sorted BAM (reads of ~15 kb with an EQX CIGAR, RG / NM / np / rq fields and,
for every fourth read, a kinetics array as long as the read) through chunk creation, a fixed haplotype state and the writer -- lcd_write_phased's ms_measure,
ms_emit, text GB/s and the download + write, with the BAM path's ms_tag + ms_deflate + download for the same chunk beside them.  Prints one JSON line; no
threshold is set on any number.
usage: python tools/bench_sam_out.py [reads, default 2000] [repeats, default 3]"""
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from longcalld_amd import align  # noqa: E402
from bam_src_common import CONTIG, record, write_bam  # noqa: E402


def source_hash():
    h = hashlib.sha1()
    for f in ("bam_sam_kernel.hip", "sam_fmt.h", "bam_aux_hop.h", "wave_copy.h", "lcd_bam_out.cpp", "lcd_call.cpp"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def hifi_records(n, rng):
    out = []
    for i in range(n):
        qlen = int(rng.integers(12000, 18000))
        words, left = [], qlen
        while left > 0:                                     # '=' runs with an X / I / D between them, about one event per 100 bases
            run = min(left, int(rng.integers(20, 200)))
            words.append((run << 4) | 7); left -= run
            if left > 0:
                op = (8, 1, 2)[int(rng.integers(0, 3))]
                words.append((1 << 4) | op); left -= 1 if op != 2 else 0
        nib = (1 << rng.integers(0, 4, qlen + (qlen & 1))).astype(np.uint8)               # A C G T as 1 2 4 8
        a = dict(name=b"m84011_220902_175841_s1/%d/ccs" % (1000 + 7 * i), pos0=250 * i, flag=16 * (i & 1), qlen=qlen, bseq=(nib[0::2] << 4) | nib[1::2],
                 qual=rng.integers(2, 94, qlen).astype(np.uint8))
        f = [("RG", "Z", b"a1b2c3d4"), ("NM", "i", len(words) // 2), ("np", "i", int(rng.integers(4, 30))), ("rq", "f", float(np.float32(0.99 + 0.0099 * rng.random())))]
        if i % 4 == 0:
            f.append(("fi", "B", ("C", rng.integers(0, 256, qlen).tolist())))
        out.append(record(a, words, f))
    return out


def best_of(reps, fn, key):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        st = fn()
        st["call_ms"] = (time.perf_counter() - t0) * 1e3
        if best is None or key(st) < key(best):
            best = st
    return best


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rng = np.random.default_rng(17)
    recs = hifi_records(n, rng)
    span = 250 * n + 20000
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "in.bam")
        write_bam(bam, recs, block=0xff00, tlen=span)
        ch = align.DeviceChunk.from_bam(bam, bam + ".bai", CONTIG, 1, span, min_mapq=30)
        chunk = [dict(chunk=ch, haps=[1 + (i & 1) for i in range(ch.n)], phase_sets=[1000] * ch.n, reg_beg=1, reg_end=span)]
        align.write_phased_sam(bam, chunk, os.path.join(tmp, "warm.sam"))                       # first touch: allocations, code objects
        align.write_phased_sam(bam, chunk, os.path.join(tmp, "warm.bam"), aln_format="bam")
        s = best_of(reps, lambda: align.write_phased_sam(bam, chunk, os.path.join(tmp, "o.sam")), lambda st: st["sam"]["ms_measure"] + st["sam"]["ms_emit"])
        b = best_of(reps, lambda: align.write_phased_sam(bam, chunk, os.path.join(tmp, "o.bam"), aln_format="bam"),
                    lambda st: st["bam_out"]["ms_tag"] + st["bam_out"]["ms_deflate"] + st["bam_out"]["ms_download_write"])
        ch.close()
    sam, so, bo = s["sam"], s["bam_out"], b["bam_out"]
    r3 = lambda x: round(x, 3)
    print(json.dumps(dict(
        source=source_hash(), reads=n, n_records=sam["n_records"], mb_records=round(sam["bytes_records"] / 2**20, 1), mb_text=round(sam["bytes_text"] / 2**20, 1),
        n_float_values=sam["n_float_values"],
        sam=dict(ms_tag=r3(so["ms_tag"]), ms_measure=r3(sam["ms_measure"]), ms_emit=r3(sam["ms_emit"]), ms_download_write=r3(sam["ms_download_write"]),
                 text_GBps_emit=r3(sam["bytes_text"] / sam["ms_emit"] / 1e6), text_GBps_measure_and_emit=r3(sam["bytes_text"] / (sam["ms_measure"] + sam["ms_emit"]) / 1e6),
                 download_GBps=r3(sam["bytes_text"] / sam["ms_download_write"] / 1e6), call_ms=round(s["call_ms"], 1)),
        bam=dict(ms_tag=r3(bo["ms_tag"]), ms_deflate=r3(bo["ms_deflate"]), ms_download_write=r3(bo["ms_download_write"]), mb_file=round(bo["bytes_file"] / 2**20, 1),
                 sum_ms=r3(bo["ms_tag"] + bo["ms_deflate"] + bo["ms_download_write"]), call_ms=round(b["call_ms"], 1)))))


if __name__ == "__main__":
    main()
