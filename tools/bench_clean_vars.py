#!/usr/bin/env python
"""lcd_chunk_clean_vars_batch throughput (steps 1.2 - 3.1 of collect_var_main on device-resident chunks): N synthetic 500 kb chunks of configs[1] shape
(30x HiFi, 15 kb reads) and one ONT-shaped set (30x, 25 kb reads, 0.5 % errors), against the C oracle (tests/c/clean_vars_oracle.c) run on 16 host threads over
the same chunks.  The chunks of a set share one seeded record set (generated once), each uploaded as a chunk of its own.  Prints one JSON line.
usage: bench_clean_vars.py [N=16] [ref_kb=500]"""
import json, os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from longcalld_amd import align
from longcalld_amd._lib import LcdCleanVars
from oracle import pyoracle
import clean_vars_common as cc


def one_set(n, ref_kb, is_ont, read_len, err, seed):
    ch = cc.make_diploid_chunk(seed, ref_len=ref_kb * 1000, depth=30, read_len=read_len, is_ont=is_ont, err=err)
    digs = cc.read_digars(ch, pyoracle, is_ont)
    low = align.sdust(ch["ref"])
    ci = cc.chunk_inputs(ch, digs)
    pre = align.pre_process_noisy_regs(ci["chunk_noisy"], low, ci["read_beg"], ci["read_end"], ci["read_ivs"])
    r = ch["reads"]
    args = dict(ordered_read_ids=np.arange(len(r), dtype=np.int32), ref=ch["ref"], ref_beg=1, ref_end=len(ch["ref"]), reg_beg=ch["reg_beg"], reg_end=ch["reg_end"],
                pre_regs=pre, low_comp=low, is_rev=np.array([x["is_rev"] for x in r], np.uint8))
    devs = [align.DeviceChunk([x["pos0"] for x in r], [x["cigar"] for x in r], [x["qual"] for x in r], [x["bseq"] for x in r], ch["reg_beg"], ch["reg_end"],
                              ch["whole_ref_len"], is_ont=is_ont) for _ in range(n)]
    opt = align.clean_opt(is_ont)
    align.chunk_clean_vars_batch(devs, [args] * n, opt)          # warm-up (and the host-array chunks' one quality upload)
    reps = 3; t0 = time.perf_counter()
    for _ in range(reps):
        res = align.chunk_clean_vars_batch(devs, [args] * n, opt)
    t = (time.perf_counter() - t0) / reps
    ref = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low)
    cc.same_clean_vars(res[0], ref)
    call = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low, call_only=True)
    L = cc.oracle_lib()
    def job(_):
        o = LcdCleanVars(); rc = call(o); L.cvo_clean_vars_free(o); return rc
    with ThreadPoolExecutor(16) as ex:
        c0 = time.perf_counter(); list(ex.map(job, range(n))); c = time.perf_counter() - c0
    for d in devs:
        d.close()
    return dict(n_chunks=n, n_reads=len(r), n_vars=res[0]["n_vars"], n_regs=len(res[0]["regs"]), profile_cells=int(res[0]["allele_off"][-1]),
                ms_per_chunk=round(t * 1e3 / n, 3), chunks_per_s=round(n / t, 1), ms_batch=round(t * 1e3, 2), oracle_16t_ms_batch=round(c * 1e3, 2),
                speedup_vs_oracle_16t=round(c / t, 2), parity_chunk0=True)


n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
kb = int(sys.argv[2]) if len(sys.argv) > 2 else 500
commit = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
# the measured code itself: sha256 over the library's sources and the public header (identifies a tree that is not, or not yet, a commit)
import hashlib
h = hashlib.sha256()
for d in ("include", os.path.join("longcalld_amd", "csrc")):
    for f in sorted(os.listdir(os.path.join(ROOT, d))):
        if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(ROOT, d, f), "rb").read())
out = dict(tool="bench_clean_vars", commit=commit, source_sha256=h.hexdigest()[:16], ref_kb=kb,
           hifi=one_set(n, kb, 0, (12000, 18000), 0.001, 1), ont=one_set(n, kb, 1, (20000, 30000), 0.005, 2))
print(json.dumps(out), flush=True)
