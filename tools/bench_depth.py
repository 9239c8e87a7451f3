#!/usr/bin/env python
"""bench_depth.py [n_contigs] [contig_kb] [--rounds N] [--other-root DIR] -- the per-haplotype depth track (lcd_chunk_depth, depth_kernel.hip) on the seeded
HiFi-shape file of bench_mods.py: per chunk the wall-clock split of the call (ms_mark: upload, memset and the mark launch; ms_rows: tile partials, scan, rows and
their download), the rows and the bytes brought down, intervals per record; then the wall time of call_file on the same file with and without depth=, each run in
a fresh child process (warm-up run, then the timed one), the variants alternating round by round.  --other-root DIR: another build of the project (a checkout with
its library built); the run without the option is timed on it too, in the same alternation.  Prints one JSON line; no threshold is set on any number.  The
reading is in profiles/NOTES_depth.md."""
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
    for f in ("depth_kernel.hip", "lcd_depth.cpp", "lcd_depth_format.cpp", "bam_aux_hop.h"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def child(root, with_depth, d):
    """one process: call_file twice on d/in.bam, the second run timed -> one JSON line"""
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import call_chunks_common as kc
    from longcalld_amd import align as lcd
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    out = None
    for k in range(2):
        kw = dict(depth=dict(path=os.path.join(d, f"child_{os.getpid()}.bed"))) if with_depth else {}
        t0 = time.perf_counter()
        st = lcd.call_file(os.path.join(d, "in.bam"), os.path.join(d, "ref.fa"), chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=os.path.join(d, f"child_{os.getpid()}.vcf"), no_vcf_header=1,
                           cfg=cfg, **kw)
        out = dict(ms=(time.perf_counter() - t0) * 1e3, ms_write=st["ms_write"], ms_call=st["ms_call"], depth_rows=st["depth"]["n_rows"] if with_depth else 0,
                   vcf=hashlib.sha256(open(os.path.join(d, f"child_{os.getpid()}.vcf"), "rb").read()).hexdigest()[:12])
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] == "1", sys.argv[4])
    args = [a for a in sys.argv[1:]]
    rounds, other = 5, None
    if "--rounds" in args:
        i = args.index("--rounds"); rounds = int(args[i + 1]); del args[i:i + 2]
    if "--other-root" in args:
        i = args.index("--other-root"); other = os.path.abspath(args[i + 1]); del args[i:i + 2]
    n_contigs = int(args[0]) if len(args) > 0 else 2
    contig_kb = int(args[1]) if len(args) > 1 else 48
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import call_file_common as fc
    import clean_vars_common as cc
    import depth_common as dc
    import mods_common as mc
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_depth_")
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    bam = os.path.join(d, "in.bam")
    bodies = mc.write_multi_bam_aux(bam, [(n, len(c["ref"]), c["reads"]) for n, c in zip(names, chs)])
    fc.write_multi_fasta(os.path.join(d, "ref.fa"), [(n, c["ref"]) for n, c in zip(names, chs)])
    plan, _ = lcd.plan_chunks([(n, len(c["ref"])) for n, c in zip(names, chs)], contig_mode=2, chunk_len=CHUNK_LEN)
    # ---- the chunk call alone: the planned chunks, and every contig as ONE chunk
    per = {}
    for label, regs in (("planned", plan), ("whole_contig", [(t, 1, len(chs[t]["ref"])) for t in range(n_contigs)])):
        tot = dict(n_chunks=len(regs), positions=0, ms_mark=0.0, ms_rows=0.0, wall_ms=0.0, n_records=0, n_intervals=0, n_rows=0)
        for tid, rb, re_ in regs:
            ref = chs[tid]["ref"]
            ch = lcd.DeviceChunk.from_bam(bam, bam + ".bai", names[tid], rb, re_, src=(ref, 1, len(ref), 0))
            haps = [k % 3 for k in range(ch.n)]
            ch.depth(haps)                                                       # warm-up
            best = None
            for _ in range(3):
                t0 = time.perf_counter(); rows, st = ch.depth(haps); ms = (time.perf_counter() - t0) * 1e3
                if best is None or ms < best[0]:
                    best = (ms, rows, st)
            ms, rows, st = best
            assert (rows, {k: st[k] for k in dc.STAT_KEYS}) == dc.depth_rows(bodies, rb, re_, haps, refid=tid)
            tot["positions"] += re_ - rb + 1; tot["wall_ms"] += ms
            for k in ("ms_mark", "ms_rows", "n_records", "n_intervals", "n_rows"):
                tot[k] += st[k]
            ch.close()
        tot["bytes_down"] = tot["n_rows"] * 24 + tot["n_chunks"] * 68              # the rows (24 B each), eight statistics and the row count per chunk
        tot["intervals_per_record"] = round(tot["n_intervals"] / max(1, tot["n_records"]), 3)
        per[label] = {k: round(v, 3) if isinstance(v, float) else v for k, v in tot.items()}
    # ---- the file driver with and without the option, fresh processes, alternating
    variants = [("without", ROOT, "0"), ("with_depth", ROOT, "1")] + ([("other_without", other, "0")] if other else [])
    res = {v[0]: [] for v in variants}
    for _ in range(rounds):
        for name, root, flag in variants:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, flag, d], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:]); sys.exit(1)                   # (nothing more is started after a failed run)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert len({x["vcf"] for v in res.values() for x in v}) == 1, "the variants wrote different VCFs"
    wall = {n: dict(median_ms=round(statistics.median(x["ms"] for x in v), 1), min_ms=round(min(x["ms"] for x in v), 1), max_ms=round(max(x["ms"] for x in v), 1),
                    median_ms_write=round(statistics.median(x["ms_write"] for x in v), 2), depth_rows=v[0]["depth_rows"]) for n, v in res.items()}
    print(json.dumps(dict(source=source_hash(), n_contigs=n_contigs, contig_kb=contig_kb, chunk_len=CHUNK_LEN, rounds=rounds, tile=lcd.depth_tile(), chunk_call=per, call_file_wall=wall)), flush=True)


if __name__ == "__main__":
    main()
