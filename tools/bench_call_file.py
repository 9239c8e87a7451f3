#!/usr/bin/env python
"""bench_call_file.py [n_contigs] [contig_kb] [repeats] -- the whole-file run (lcd_call_files) on a seeded multi-contig HiFi-shape file: wall time and the busy time of
the three stages for overlap 0 / 1, loader_threads 1 / 2 / 4 and a few window sizes, and the same file through lcd_call_bam_regions per contig (the two-pass
wrapper: what a caller had before).  Prints one JSON line; the reading is in profiles/NOTES_call_file.md.  The file is synthetic (tests' generator: 12x depth,
2 - 6 kb reads, chunk_len 6000), so the chunks are a hundredth of a real 500 kb chunk: the figures compare schedules, they are not throughput."""
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")


def source_hash():
    h = hashlib.sha256()
    for f in ("lcd_call_file.cpp", "lcd_call.cpp", "lcd_chunk.cpp", "lcd_bam_out.cpp", "lcd_emit.cpp"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def main():
    n_contigs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    contig_kb = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    import call_file_common as fc
    import clean_vars_common as cc
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_call_file_")
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    fc.write_multi_bam(bam, [(n, len(c["ref"]), c["reads"]) for n, c in zip(names, chs)])
    fc.write_multi_fasta(fa, [(n, c["ref"]) for n, c in zip(names, chs)])
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=600))
    chunk_len = 6000
    contigs = lcd.bam_contigs(bam)
    plan, _ = lcd.plan_chunks(contigs, chunk_len=chunk_len)

    def one(**kw):
        best = None
        for _ in range(repeats):
            st = lcd.call_file(bam, fa, chunk_len=chunk_len, vcf_path=os.path.join(d, "o.vcf"), bam_out=dict(path=os.path.join(d, "o.bam")), cfg=cfg, **kw)
            if best is None or st["ms_wall"] < best["ms_wall"]:
                best = st
        return {k: round(best[k], 1) if isinstance(best[k], float) else best[k] for k in ("ms_wall", "ms_load", "ms_call", "ms_write", "n_windows", "n_region_loads", "peak_device_bytes")}

    one(window_chunks=4, overlap=0)                                                    # warm-up: allocations, code objects
    runs = []
    for window in (2, 8, 0):
        for overlap, threads in ((0, 1), (0, 4), (1, 1), (1, 2), (1, 4)):
            runs.append(dict(window_chunks=window, overlap=overlap, loader_threads=threads, **one(window_chunks=window, overlap=overlap, loader_threads=threads)))
    t0 = time.perf_counter()
    n_rec = 0
    for tid, (name, _ln) in enumerate(contigs):                                        # the two-pass wrapper, one call per contig, alignment output included
        mine = [(b, e) for t, b, e in plan if t == tid]
        r = lcd.call_bam_regions(bam, bam + ".bai", fa, name, [b for b, _ in mine], [e for _, e in mine], cfg=cfg, bam_out=dict(path=os.path.join(d, f"y{tid}.bam")))
        n_rec += len(r["records"])
    per_contig_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(source=source_hash(), n_contigs=n_contigs, contig_kb=contig_kb, chunk_len=chunk_len, n_chunks=len(plan), n_records=n_rec, repeats=repeats,
                          call_bam_regions_per_contig_ms=round(per_contig_ms, 1), runs=runs)), flush=True)


if __name__ == "__main__":
    main()
