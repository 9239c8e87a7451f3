#!/usr/bin/env python
"""bench_vcf_fields.py [--root DIR] [n_contigs] [contig_kb] [repeats] -- what the supporting read names (--out-var-rnames / --out-sv-rnames) cost the whole-file run:
tools/bench_call_file.py's seeded file (12x depth, 2 - 6 kb reads, chunk_len 6000) through lcd_call_files with no options, rnames="sv" and rnames="all", each as plain
VCF and as -O z, with a TE library of three seeded sequences where the options are on.  Per run ms_write, ms_wall (the best of `repeats` by wall time) and the VCF's
bytes.  --root DIR imports the package of another checkout (a build of the parent commit): only the no-options runs are made there.  Prints one JSON line; the
reading is in profiles/NOTES_vcf_fields.md.  The chunks are a hundredth of a real 500 kb chunk: the figures compare runs of this file, they are not throughput."""
import inspect
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
if argv[:1] == ["--root"]:
    ROOT, argv = os.path.abspath(argv[1]), argv[2:]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")


def main():
    n_contigs = int(argv[0]) if len(argv) > 0 else 6
    contig_kb = int(argv[1]) if len(argv) > 1 else 24
    repeats = int(argv[2]) if len(argv) > 2 else 3
    import numpy as np
    import call_file_common as fc
    import clean_vars_common as cc
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_vcf_fields_")
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    bam, fa, te = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "te.fa")
    fc.write_multi_bam(bam, [(n, len(c["ref"]), c["reads"]) for n, c in zip(names, chs)])
    fc.write_multi_fasta(fa, [(n, c["ref"]) for n, c in zip(names, chs)])
    rng = np.random.default_rng(2024)
    with open(te, "w") as f:
        for i in range(3):
            f.write(f">TE{i}\n" + "".join("ACGT"[x] for x in rng.integers(0, 4, 300)) + "\n")
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=600))
    has_fields = "rnames" in inspect.signature(lcd.call_file).parameters

    def one(bgzf, **kw):
        best, walls, vcf = None, [], os.path.join(d, "o.vcf.gz" if bgzf else "o.vcf")
        for _ in range(repeats):
            st = lcd.call_file(bam, fa, chunk_len=6000, vcf_path=vcf, vcf_bgzf=bgzf, bam_out=dict(path=os.path.join(d, "o.bam")), cfg=cfg, **kw)
            walls.append(round(st["ms_wall"], 1))
            if best is None or st["ms_wall"] < best["ms_wall"]:
                best = st
        return dict(ms_wall_all=walls, ms_write=round(best["ms_write"], 1), ms_wall=round(best["ms_wall"], 1), ms_call=round(best["ms_call"], 1), vcf_bytes=os.path.getsize(vcf),
                    n_vcf_lines=best["n_vcf_lines"])

    one(0)                                                                             # warm-up: allocations, code objects
    runs = []
    for label, kw in (("none", {}), ("sv", dict(rnames="sv", te_fasta=te)), ("all", dict(rnames="all", te_fasta=te))):
        if kw and not has_fields:
            continue
        for bgzf in (0, 1):
            runs.append(dict(options=label, out_type="z" if bgzf else "v", **one(bgzf, **kw)))
    print(json.dumps(dict(root=os.path.basename(ROOT), n_contigs=n_contigs, contig_kb=contig_kb, chunk_len=6000, repeats=repeats, runs=runs)), flush=True)


if __name__ == "__main__":
    main()
