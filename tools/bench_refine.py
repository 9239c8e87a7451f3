"""Measurement of the refined alignment rewrite (lcd_chunk_refine_records, bam_refine_kernel.hip) against the HP / PS rewrite it extends (lcd_chunk_tag_records_sel,
bam_tag_kernel.hip) on the same device-resident chunk: the seeded 30 kb / 60-read BAM of tests/bam_src_common.py, every record repeated, in its plain-'M' spelling
(every CIGAR changes: M -> = / X, no tags to compare), its MD + cs spelling (texts generated, compared and replaced) and its EQX spelling (every CIGAR identical: the
cost of looking).  A quarter of the reads is handed over as touched reads, to show the upload.  Then the whole-file run (whole_file below).  Prints one JSON line; no threshold is set on any number.
usage: python tools/bench_refine.py [copies of every record, default 20] [repeats, default 5]"""
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
import bam_src_common as bs  # noqa: E402


def source_hash():
    h = hashlib.sha1()
    for f in ("bam_refine_kernel.hip", "bam_tag_kernel.hip", "bam_aux_hop.h", "wave_copy.h", "lcd_bam_out.cpp"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def best_ms(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), r


def one(kind, copies, reps, tmp):
    ref, al = bs.seeded()
    recs = []
    for r in bs.records_as(kind, sa=False):
        if kind == "md":                                   # MD + cs on an 'M' CIGAR: both texts are made and compared
            r = bs.record(r["a"], r["a"]["mcig"], [("MD", "Z", r["a"]["md"]), ("cs", "Z", r["a"]["cs"]), ("NM", "i", 0)])
        recs += [r] * copies
    path = os.path.join(tmp, kind + ".bam")
    bs.write_bam(path, recs, block=60000)
    ch = align.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, 1, bs.TLEN, min_mapq=0, src=(bs.ref_letters(ref), 1, bs.TLEN, 0))
    hp = np.arange(ch.n, dtype=np.int32) % 3; ps = np.where(hp > 0, 4000, 0).astype(np.int64)
    dg = ch.digars()
    st = ch.read_info()["status"]
    touched = {r: dg[r] for r in range(0, ch.n, 4) if st[r] == 0}
    t_tag, (tagged, n_rec) = best_ms(lambda: ch.tag_records_sel(hp, ps), reps)
    t_ref, (out, n_out, stats) = best_ms(lambda: ch.refine_records(hp, ps, None, ref, 1, bs.TLEN), reps)
    t_tch, (out2, _, stats2) = best_ms(lambda: ch.refine_records(hp, ps, touched, ref, 1, bs.TLEN), reps)
    assert n_out == n_rec and out2 == out                  # (the touched lists are the chunk's own: the same records)
    mb = len(tagged) / 2**20
    ch.close()
    return dict(kind=kind, records=n_rec, reads=ch.n, digars=int(sum(len(d) for d in dg)), inflated_mb=round(mb, 2), out_mb=round(len(out) / 2**20, 2),
                tag_call_ms=round(t_tag, 3), refine_call_ms=round(t_ref, 3), refine_call_ms_touched=round(t_tch, 3), refine_ms_per_mb=round(t_ref / mb, 3),
                tag_ms_per_mb=round(t_tag / mb, 3), ms_measure=round(stats["ms_measure"], 3), ms_emit=round(stats["ms_emit"], 3),
                n_refined=stats["n_refined"], n_identical=stats["n_identical"], n_unrefined=stats["n_unrefined"], n_md_replaced=stats["n_md_replaced"],
                n_cs_replaced=stats["n_cs_replaced"], bytes_ref_up=stats["bytes_ref_up"], touched_reads=len(touched), bytes_digars_up=stats2["bytes_digars_up"])


def whole_file(n_contigs=6, contig_kb=24, repeats=3):
    """tools/bench_call_file.py's seeded file (6 contigs of 24 kb, 12x, chunk_len 6000), as EQX and as plain-'M' records, through lcd_call_files with and without
    refine: wall time, the writer's ms_tag (without refine it is lcd_chunk_tag_records_sel, the writer as it was), the logs' bytes down, the digars' bytes up"""
    import call_file_common as fc
    import clean_vars_common as cc
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    cfg = align.call_cfg(0, pass_=dict(max_noisy_reg_len=600))
    out = []
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "ref.fa")
        fc.write_multi_fasta(fa, [(n, c["ref"]) for n, c in zip(names, chs)])
        for kind in ("eqx", "m"):
            bam = os.path.join(d, kind + ".bam")
            fc.write_multi_bam(bam, [(n, len(c["ref"]), c["reads"] if kind == "eqx" else [dict(r, cigar=fc.m_cigar(r["cigar"])) for r in c["reads"]]) for n, c in zip(names, chs)])
            row = dict(kind=kind)
            for refine in (False, True):
                best = None
                for _ in range(repeats + 1):
                    st = align.call_file(bam, fa, chunk_len=6000, vcf_path=os.path.join(d, "o.vcf"), bam_out=dict(path=os.path.join(d, "o.bam")), cfg=cfg, contig_mode=2,
                                         refine=refine)
                    if best is None or st["ms_wall"] < best["ms_wall"]:
                        best = st
                tag = "refine" if refine else "plain"
                row.update({f"{tag}_ms_wall": round(best["ms_wall"], 1), f"{tag}_ms_call": round(best["ms_call"], 1), f"{tag}_ms_write": round(best["ms_write"], 1),
                            f"{tag}_ms_tag": round(best["bam_out"]["ms_tag"], 2), "records_out": best["bam_out"]["n_records_out"],
                            "inflated_mb": round(best["bam_out"]["bytes_inflated"] / 2**20, 2), "n_chunks": best["n_planned"]})
                if refine:
                    r = best["refine"]
                    row.update({k: r[k] for k in ("n_refined", "n_identical", "n_unrefined", "n_pos_moved", "n_touched", "n_log_entries", "bytes_log_down", "bytes_digars_up",
                                                  "bytes_ref_up", "n_log_rejected")})
                    row.update(refine_ms_measure=round(r["ms_measure"], 2), refine_ms_emit=round(r["ms_emit"], 2))
            out.append(row)
    return out


def main():
    copies = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    with tempfile.TemporaryDirectory() as tmp:
        print(json.dumps(dict(source=source_hash(), copies=copies, runs=[one(k, copies, reps, tmp) for k in ("ref", "md", "eqx")], whole_file=whole_file())))


if __name__ == "__main__":
    main()
