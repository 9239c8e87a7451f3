#!/usr/bin/env python
"""bench_split.py [reads, default 2000] [repeats, default 5] [--rounds N] [--other-root DIR] -- the per-haplotype read sets (lcd_chunk_split_reads,
split_kernel.hip) on the HiFi-shape chunk of bench_sam_out.py (reads of ~15 kb, every second one on the reverse strand): ms and output GB/s of the measure and
the emit pass, for all records, for the forward records alone and for the reverse records alone (the plan's skip array picks them from the one chunk), every
figure the best and the spread of `repeats` calls after a warm-up; beside them lcd_tagged_to_sam's emit pass on the same records, the nearest existing kernel
with the same access pattern.  Then the wall time of call_file on the seeded two-contig file of bench_depth.py with and without split= (FASTQ .gz + list), each
run in a fresh child process (warm-up run, then the timed one), the variants alternating round by round.  --other-root DIR: another build of the project (a
checkout with its library built); the run without the option is timed on it too.  Prints one JSON line; no threshold is set on any number.  The reading is in
profiles/NOTES_split.md."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_LEN = 6000


def source_hash():
    h = hashlib.sha256()
    for f in ("split_kernel.hip", "lcd_split.cpp", "lcd_split_format.cpp", "wave_copy.h", "sam_fmt.h"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def child(root, with_split, d):
    """one process: call_file twice on d/in.bam, the second run timed -> one JSON line"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import call_chunks_common as kc
    from longcalld_amd import align as lcd
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    out = None
    for k in range(2):
        pre = os.path.join(d, f"child_{os.getpid()}")
        kw = dict(split=dict(prefix=pre, gz=True, haplotag_list=pre + ".tsv")) if with_split else {}
        t0 = time.perf_counter()
        st = lcd.call_file(os.path.join(d, "in.bam"), os.path.join(d, "ref.fa"), chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=pre + ".vcf", no_vcf_header=1, cfg=cfg, **kw)
        out = dict(ms=(time.perf_counter() - t0) * 1e3, ms_write=st["ms_write"], split_reads=st["split"]["n_selected"] if with_split else 0,
                   split_ms={k: round(st["split"][k], 2) for k in ("ms_measure", "ms_emit", "ms_deflate", "ms_download_write")} if with_split else None,
                   vcf=hashlib.sha256(open(pre + ".vcf", "rb").read()).hexdigest()[:12])
    print(json.dumps(out), flush=True)


def spread(xs):
    return dict(best=round(min(xs), 3), median=round(statistics.median(xs), 3), worst=round(max(xs), 3))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] == "1", sys.argv[4])
    args = list(sys.argv[1:])
    rounds, other = 5, None
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    if "--other-root" in args:
        i = args.index("--other-root"); other = os.path.abspath(args[i + 1]); del args[i:i + 2]
    n = int(args[0]) if len(args) > 0 else 2000
    reps = int(args[1]) if len(args) > 1 else 5
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import call_file_common as fc
    import clean_vars_common as cc
    import mods_common as mc
    from bam_src_common import CONTIG, write_bam
    from bench_sam_out import hifi_records
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_split_")
    # ---- the chunk call alone
    recs = hifi_records(n, np.random.default_rng(17))
    span = 250 * n + 20000
    bam = os.path.join(d, "hifi.bam")
    write_bam(bam, recs, block=0xff00, tlen=span)
    ch = lcd.DeviceChunk.from_bam(bam, bam + ".bai", CONTIG, 1, span, min_mapq=30)
    haps, pss = [1 + (i & 1) for i in range(ch.n)], [1000] * ch.n
    fwd_only = [int(bool(r["flag"] & 16)) for r in recs]                         # skip arrays over the record table (every record of the file is in it)
    rev_only = [1 - s for s in fwd_only]
    per = {}
    for label, skip in (("all", None), ("forward", fwd_only), ("reverse", rev_only)):
        lcd.chunk_split_reads(ch, haps, pss, skip=skip, names=[CONTIG], comment=True, list=True)     # warm-up: allocations, code objects
        runs = [lcd.chunk_split_reads(ch, haps, pss, skip=skip, names=[CONTIG], comment=True, list=True)[1] for _ in range(reps)]
        out_bytes = sum(runs[0]["bytes_fastq"]) + runs[0]["bytes_list"]
        em, me = [r["ms_emit"] for r in runs], [r["ms_measure"] for r in runs]
        per[label] = dict(n_selected=runs[0]["n_selected"], n_reverse=runs[0]["n_reverse"], mb_out=round(out_bytes / 2**20, 1), ms_measure=spread(me), ms_emit=spread(em),
                          GBps_emit_best=round(out_bytes / min(em) / 1e6, 2), GBps_measure_and_emit_best=round(out_bytes / (min(me) + min(em)) / 1e6, 2))
    per["reverse_over_forward_emit"] = round(per["reverse"]["ms_emit"]["median"] / per["forward"]["ms_emit"]["median"], 3)
    lcd.tagged_to_sam(ch, haps, pss, [CONTIG])
    sam = [lcd.tagged_to_sam(ch, haps, pss, [CONTIG])[2] for _ in range(reps)]
    em = [s["ms_emit"] for s in sam]
    per["sam_emit"] = dict(mb_text=round(sam[0]["bytes_text"] / 2**20, 1), ms_emit=spread(em), ms_measure=spread([s["ms_measure"] for s in sam]), GBps_emit_best=round(sam[0]["bytes_text"] / min(em) / 1e6, 2))
    ch.close()
    # ---- the file driver with and without the option, fresh processes, alternating
    chs = [cc.make_diploid_chunk(100 + i, ref_len=48000, depth=12) for i in range(2)]
    names = ["chr1", "chr2"]
    mc.write_multi_bam_aux(os.path.join(d, "in.bam"), [(nm, len(c["ref"]), c["reads"]) for nm, c in zip(names, chs)])
    fc.write_multi_fasta(os.path.join(d, "ref.fa"), [(nm, c["ref"]) for nm, c in zip(names, chs)])
    variants = [("without", ROOT, "0"), ("with_split_gz", ROOT, "1")] + ([("other_without", other, "0")] if other else [])
    res = {v[0]: [] for v in variants}
    for _ in range(rounds):
        for name, root, flag in variants:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, flag, d], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:]); sys.exit(1)                   # (nothing more is started after a failed run)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert len({x["vcf"] for v in res.values() for x in v}) == 1, "the variants wrote different VCFs"
    wall = {k: dict(median_ms=round(statistics.median(x["ms"] for x in v), 1), min_ms=round(min(x["ms"] for x in v), 1), max_ms=round(max(x["ms"] for x in v), 1),
                    median_ms_write=round(statistics.median(x["ms_write"] for x in v), 2), split_reads=v[0]["split_reads"], split_ms=v[-1]["split_ms"]) for k, v in res.items()} if rounds else {}
    print(json.dumps(dict(source=source_hash(), reads=n, repeats=reps, rounds=rounds, chunk_call=per, call_file_wall=wall)), flush=True)


if __name__ == "__main__":
    main()
