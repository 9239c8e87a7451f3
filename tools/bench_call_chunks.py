#!/usr/bin/env python
"""lcd_chunks_call (chunks -> stitched genotype records and VCF body lines) on N chunks of one seeded HiFi-shape contig (tests/clean_vars_common.py
make_diploid_chunk of N x ref_len bases, cut into N regions): the call as a whole, and the same chain stepped through the stage exports with a wall-clock timer
around each -- first round (lcd_chunks_first_round), rounds (lcd_chunks_noisy_rounds), stitch (lcd_flip_variant_hap), records + text (lcd_make_variants,
lcd_annotate_te, lcd_format_vcf_te per chunk; one timer: the mirror makes both in one call).  All times are through the Python mirror (host arrays in and out).
Asserts that the whole call equals the stepped chain.  Prints one JSON line.
usage: bench_call_chunks.py [N=8] [ref_len=30000]"""
import ctypes as C, hashlib, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from longcalld_amd import _lib, align as lcd
from oracle import pyoracle as oracle
import call_chunks_common as kc
import clean_vars_common as cc

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
ref_len = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
oracle.build()                                                                    # (emit_common's structs; nothing of the oracle is timed or compared)
prod = C.CDLL(_lib.LIB_PATH)
whole = cc.make_diploid_chunk(300, ref_len=n * ref_len)
chs = kc.split_chunk(whole, [ref_len * (i + 1) for i in range(n - 1)])
devs = []
for ch in chs:
    r = ch["reads"]
    devs.append(lcd.DeviceChunk([x["pos0"] for x in r], [x["cigar"] for x in r], [x["qual"] for x in r], [x["bseq"] for x in r], ch["reg_beg"], ch["reg_end"], ch["whole_ref_len"]))
items = [dict(ref=ch["ref"], ref_beg=ch["ref_beg"], reg_beg=ch["reg_beg"], reg_end=ch["reg_end"], ordered_read_ids=np.arange(len(ch["reads"]), dtype=np.int32),
              is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8)) for ch in chs]
cfg = lcd.call_cfg(0)

lcd.chunks_call(devs, items, cfg)                                                 # warm-up
ts = []
for _ in range(3):
    t0 = time.perf_counter(); whole_res = lcd.chunks_call(devs, items, cfg); ts.append(time.perf_counter() - t0)
ms_call = float(np.median(ts)) * 1e3

def stepped():
    T = {}
    t0 = time.perf_counter(); first = lcd.chunks_first_round(devs, items); T["first_round"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rounds = lcd.chunks_noisy_rounds(devs, [dict(cv=f["cv"], state=f["state"], ordered_read_ids=f["ordered_read_ids"], is_skipped=f["is_skipped"], ref=ch["ref"], ref_beg=ch["ref_beg"])
                                            for f, ch in zip(first, chs)])
    T["rounds"] = time.perf_counter() - t0
    finals = [dict(cv=r["cv"], state=r["state"], n_passes=r["n_passes"], ordered=f["ordered_read_ids"], skipped=f["is_skipped"]) for r, f in zip(rounds, first)]
    t0 = time.perf_counter(); flips = kc.stitch(prod, "lcd_", chs, finals); T["stitch"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    records, text = [], ""
    for ch, f, fl in zip(chs, finals, flips):
        recs, t = kc.emit_records(prod, "lcd_", ch, f["cv"], f["state"], f["ordered"], f["skipped"])
        f["flip"], f["n_records"] = fl, len(recs)
        records += recs; text += t
    T["records_and_text"] = time.perf_counter() - t0
    return dict(chunks=finals, records=records, vcf_body=text), T
stepped()
runs = [stepped() for _ in range(3)]
kc.same_call(whole_res, runs[-1][0], state_keys=("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps", "var_phase_set", "hap_to_cons_alle", "hap_to_alle_profile"))
stages = {k: round(float(np.median([r[1][k] for r in runs])) * 1e3, 2) for k in runs[0][1]}

commit = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
h = hashlib.sha256()   # the measured code itself: the library's sources and the public header
for d in ("include", os.path.join("longcalld_amd", "csrc")):
    for f in sorted(os.listdir(os.path.join(ROOT, d))):
        if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(ROOT, d, f), "rb").read())
print(json.dumps(dict(tool="bench_call_chunks", commit=commit, source_sha256=h.hexdigest()[:16], n_chunks=n, ref_len=ref_len, reads_per_chunk=[len(ch["reads"]) for ch in chs],
                      passes_per_chunk=[c["n_passes"] for c in whole_res["chunks"]], flips=[c["flip_hap"] for c in whole_res["chunks"]],
                      joined=[int(c["flip_pre_PS"] != -1) for c in whole_res["chunks"]], vars_final=int(sum(c["cv"]["n_vars"] for c in whole_res["chunks"])),
                      records=len(whole_res["records"]), vcf_lines=whole_res["vcf_body"].count("\n"), ms_call=round(ms_call, 2), ms_stepped_stages=stages,
                      ms_stepped_total=round(sum(stages.values()), 2), parity=True)), flush=True)
for d in devs:
    d.close()
