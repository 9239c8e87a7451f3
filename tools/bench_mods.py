#!/usr/bin/env python
"""bench_mods.py [n_contigs] [contig_kb] -- the methylation pile-up (lcd_chunk_mod_pileup, mods_kernel.hip) on the seeded HiFi-shape file of bench_call_file.py with
MM / ML added to every read (tests/mods_common.add_calls), chunk by chunk, beside two baselines on the same device-resident chunks: the HP / PS rewrite of the
chunk's records (lcd_chunk_tag_records: the existing one-wavefront-per-record pass over the same auxiliary fields, the stage the file driver reports as ms_tag) and
the Python oracle.  Best of 2 runs after a warm-up; prints one JSON line, no threshold is set on any number.  The reading is in profiles/NOTES_mods.md."""
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def source_hash():
    h = hashlib.sha256()
    for f in ("mods_kernel.hip", "lcd_mods.cpp", "lcd_mods_format.cpp", "bam_aux_hop.h", "bam_tag_kernel.hip", "lcd_bam_out.cpp"):
        h.update(open(os.path.join(ROOT, "longcalld_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def main():
    n_contigs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    contig_kb = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    import numpy as np
    import bam_out_common as bo
    import clean_vars_common as cc
    import mods_common as mc
    from longcalld_amd import align as lcd
    d = tempfile.mkdtemp(prefix="bench_mods_")
    rng = np.random.default_rng(9)
    chs = [cc.make_diploid_chunk(100 + i, ref_len=contig_kb * 1000, depth=12) for i in range(n_contigs)]
    names = [f"chr{i + 1}" for i in range(n_contigs)]
    bam = os.path.join(d, "in.bam")
    bodies = mc.write_multi_bam_aux(bam, [(n, len(c["ref"]), [mc.add_calls(rng, r) for r in c["reads"]]) for n, c in zip(names, chs)])
    chunk_len = 6000
    plan, _ = lcd.plan_chunks([(n, len(c["ref"])) for n, c in zip(names, chs)], chunk_len=chunk_len)
    chunks = []
    for tid, rb, re_ in plan:
        ref = chs[tid]["ref"]
        ch = lcd.DeviceChunk.from_bam(bam, bam + ".bai", names[tid], rb, re_, src=(ref, 1, len(ref), 0))
        chunks.append((ch, tid, rb, re_, [k % 3 for k in range(ch.n)]))

    def best_of_2(f):
        f()
        best = None
        for _ in range(2):
            t0 = time.perf_counter(); r = f(); ms = (time.perf_counter() - t0) * 1e3
            if best is None or ms < best[0]:
                best = (ms, r)
        return best

    def pile():
        tot = dict(ms_site_map=0.0, ms_pileup=0.0, ms_compact=0.0, n_records=0, n_counted=0, n_rows=0, n_sites=0)
        for ch, tid, rb, re_, haps in chunks:
            _, st = ch.mod_pileup(haps, chs[tid]["ref"], 1, len(chs[tid]["ref"]))
            for k in tot:
                tot[k] += st[k]
        return tot

    def tag():
        n = 0
        for ch, tid, rb, re_, haps in chunks:
            n += ch.tag_records(haps, [1000 * (h > 0) for h in haps])[1]
        return n

    def oracle():
        n = 0
        for ch, tid, rb, re_, haps in chunks:
            n += mc.pileup(bodies, chs[tid]["ref"], 1, rb, re_, haps, refid=tid)[1]["n_counted"]
        return n

    ms_pile, st = best_of_2(pile)
    ms_tag, n_tagged = best_of_2(tag)
    t0 = time.perf_counter(); n_oracle = oracle(); ms_oracle = (time.perf_counter() - t0) * 1e3
    assert n_oracle == st["n_counted"]
    bases = sum(len(r["qual"]) for c in chs for r in c["reads"])
    print(json.dumps(dict(source=source_hash(), n_contigs=n_contigs, contig_kb=contig_kb, chunk_len=chunk_len, n_chunks=len(plan), read_bases=bases, records=st["n_records"],
                          records_tagged=n_tagged, calls_counted=st["n_counted"], sites=st["n_sites"], rows=st["n_rows"], mod_pileup_wall_ms=round(ms_pile, 2),
                          mod_pileup_site_map_ms=round(st["ms_site_map"], 2), mod_pileup_kernel_ms=round(st["ms_pileup"], 2), mod_pileup_compact_ms=round(st["ms_compact"], 2),
                          tag_records_wall_ms=round(ms_tag, 2), python_oracle_ms=round(ms_oracle, 1))), flush=True)
    for ch, *_ in chunks:
        ch.close()


if __name__ == "__main__":
    main()
