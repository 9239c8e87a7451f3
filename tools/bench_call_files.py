#!/usr/bin/env python
"""bench_call_files.py [n_contigs] [contig_kb] [repeats] [--root DIR] -- one sample from several BAMs (lcd_call_files) on the seeded file of tools/bench_call_file.py:
the one BAM holding all reads through lcd_call_files without an input list, the same file through lcd_call_files with n = 1, and the reads dealt out to 2 and to 4 files (read i of a contig
goes to file i % n).  Per run the best of `repeats` wall times with its ms_load / ms_call / ms_write, n_region_loads and peak_device_bytes.  Prints one JSON line;
the reading is in profiles/NOTES_call_files.md.
--root DIR measures the library and the Python mirror of another checkout of this project (one that has been built), e.g. the parent commit: a tree without
lcd_call_files records the one-file run only.  The data is written by this tree's test helpers in either case, so both trees read the same bytes.
The file is synthetic (12x depth, 2 - 6 kb reads, chunk_len 6000): the chunks are a hundredth of a real 500 kb chunk, which was NOT measured."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")


def main():
    argv = sys.argv[1:]
    root = HERE
    if "--root" in argv:
        i = argv.index("--root"); root = os.path.abspath(argv[i + 1]); del argv[i:i + 2]
    n_contigs = int(argv[0]) if len(argv) > 0 else 6
    contig_kb = int(argv[1]) if len(argv) > 1 else 24
    repeats = int(argv[2]) if len(argv) > 2 else 5
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, root)                                                          # longcalld_amd of the tree under measurement
    import clean_vars_common as cc
    import call_file_common as fc
    import multi_bam_common as mb
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_call_files_")
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    fa = os.path.join(d, "ref.fa")
    fc.write_multi_fasta(fa, [(n, c["ref"]) for n, c in zip(names, chs)])
    inputs = {}
    for n_files in (1, 2, 4):
        dealt = [mb.deal(c["reads"], n, n_files, filtered=False) for n, c in zip(names, chs)]
        inputs[n_files] = [os.path.join(d, f"in{n_files}_{f}.bam") for f in range(n_files)]
        for f, path in enumerate(inputs[n_files]):
            mb.write_bam(path, [(n, len(c["ref"]), dealt[k][f]) for k, (n, c) in enumerate(zip(names, chs))])
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=600))
    keys = ("ms_wall", "ms_load", "ms_call", "ms_write", "n_windows", "n_region_loads", "peak_device_bytes", "n_reads", "n_records")

    def best_of(fn):
        runs = [fn() for _ in range(repeats)]
        best = min(runs, key=lambda s: s["ms_wall"])
        out = {k: round(best[k], 1) if isinstance(best[k], float) else best[k] for k in keys}
        out["ms_wall_all"] = sorted(round(s["ms_wall"], 1) for s in runs)              # the run-to-run spread
        if "bam_out" in best:
            out["n_records_out"] = best["bam_out"]["n_records_out"]
        return out

    common = dict(chunk_len=6000, vcf_path=os.path.join(d, "o.vcf"), bam_out=dict(path=os.path.join(d, "o.bam")), cfg=cfg, window_chunks=0, overlap=0)
    lcd.call_file(inputs[1][0], fa, **common)                                          # warm-up: allocations, code objects
    res = dict(root=os.path.relpath(root, HERE), n_contigs=n_contigs, contig_kb=contig_kb, chunk_len=6000, repeats=repeats, runs={})
    res["runs"]["call_file"] = best_of(lambda: lcd.call_file(inputs[1][0], fa, **common))
    if hasattr(lcd, "call_files"):
        for n_files in (1, 2, 4):
            res["runs"][f"call_files_n{n_files}"] = best_of(lambda: lcd.call_files(inputs[n_files], fa, **common))
        res["runs"]["call_files_n4_sorted"] = best_of(lambda: lcd.call_files(inputs[4], fa, sort_output=True, index=dict(write_out_bai=1), **common))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
