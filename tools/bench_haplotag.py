#!/usr/bin/env python
"""lcd_chunk_haplotag on a synthetic chunk set: N seeded diploid chunks (tests/haplotag_common.py simulate: het SNV / INS / DEL sites about every 90 bases, reads with
exact CIGARs) against their phased VCF.  Reports reads per second of the haplotag stage, its launch times (measure + scan, mark, reduce: the medians over the
repeats, summed over the chunks), the agreement of the haplotypes with the simulation's truth and, for orientation, the load time of the chunks.  The measuring
runs in a child process under a time limit of its own (--step-timeout seconds); the parent prints the child's one JSON line.
usage: bench_haplotag.py [--chunks 8] [--reads 400] [--length 30000] [--repeats 5] [--step-timeout 300]"""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(a):
    import numpy as np
    from longcalld_amd import align as lcd
    import haplotag_common as hc
    from bam_src_common import CONTIG
    d = tempfile.mkdtemp(prefix="bench_haplotag_")
    sets = []
    t0 = time.perf_counter()
    for i in range(a.chunks):
        sim = hc.simulate(100 + i, n_reads=a.reads, length=a.length, read_len=(2000, min(15000, a.length // 2)))
        bam, vcf = os.path.join(d, f"c{i}.bam"), os.path.join(d, f"c{i}.vcf")
        hc.write_bam(bam, sim["recs"], block=30000, tlen=a.length)
        open(vcf, "w").write(sim["vcf"])
        sets.append((sim, bam, vcf))
    ms_make = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    work = []
    for sim, bam, vcf in sets:
        ref = np.array(["ACGT".index(c) for c in sim["ref"]], np.uint8)
        work.append((sim, lcd.DeviceChunk.from_bam(bam, bam + ".bai", CONTIG, 1, a.length, min_mapq=30, src=(ref, 1, a.length, 0)), lcd.phased_vcf_read(vcf, ["sim"])))
    ms_load = (time.perf_counter() - t0) * 1e3
    for _, ch, v in work:
        lcd.chunk_haplotag(ch, v, 0)                                              # warm-up: the site tables go up here
    wall, stage = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = [lcd.chunk_haplotag(ch, v, 0) for _, ch, v in work]
        wall.append((time.perf_counter() - t0) * 1e3)
        stage.append([sum(r["stats"][k] for r in res) for k in ("ms_measure", "ms_mark", "ms_reduce")])
    n_reads = sum(ch.n for _, ch, _ in work)
    voted = right = 0
    for (sim, _, _), r in zip(work, res):
        for h, n1, n2, rec in zip(r["haps"], r["n1"], r["n2"], sim["recs"]):
            if n1 + n2:
                voted += 1; right += h == rec["true_hap"]
    med = lambda x: float(np.median(x))
    print(json.dumps(dict(bench="haplotag", chunks=a.chunks, n_reads=n_reads, n_pairs=sum(r["stats"]["n_pairs"] for r in res), n_sites=sum(v.stats["n_sites"] for _, _, v in work),
                          ms_wall=round(med(wall), 3), reads_per_s=round(n_reads / (med(wall) / 1e3)), ms_measure=round(med([s[0] for s in stage]), 3),
                          ms_mark=round(med([s[1] for s in stage]), 3), ms_reduce=round(med([s[2] for s in stage]), 3), ms_load_chunks=round(ms_load, 1), ms_make_inputs=round(ms_make, 1),
                          reads_with_votes=voted, agree_with_truth=right, repeats=a.repeats)), flush=True)
    for _, ch, v in work:
        ch.close(); v.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8); ap.add_argument("--reads", type=int, default=400); ap.add_argument("--length", type=int, default=30000)
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--step-timeout", type=int, default=300); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
    else:
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"])
        sys.exit(r.returncode)
