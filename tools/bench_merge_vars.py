#!/usr/bin/env python
"""lcd_merge_region_vars_batch (a pass's noisy-region variants folded into the chunk, merge_var_profile) on N chunks of the tests' seeded shape B scaled to
1 000 reads, 1 000 current variants and 35 regions, against the pure-Python oracle (tests/merge_vars_common.py) on the same chunks.  The chunks share one seeded
state (generated once).  Beside it: the time N chunks spend in the lcd_batch_region_vars calls that hand over such a pass's region variants (35 synthetic
regions through the hot path once, then the per-region calls N times, bare C calls).  Prints one JSON line.
usage: bench_merge_vars.py [N=16]"""
import ctypes as C
import hashlib, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from longcalld_amd import align, jobs
from longcalld_amd._lib import LcdNoisyVar
import merge_vars_common as mc

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N_REGIONS = 35
cv, regions, ordered, skipped = mc.make_case(seed=12, n_reads=1000, n_vars=1000, n_regions=N_REGIONS, span=30)
args = ([cv] * n, [regions] * n, [ordered] * n, [skipped] * n)
align.merge_region_vars_batch(*args)                                   # warm-up
ts = []
for _ in range(3):
    t0 = time.perf_counter(); res = align.merge_region_vars_batch(*args); ts.append(time.perf_counter() - t0)
t = float(np.median(ts))
t0 = time.perf_counter(); want = mc.oracle_merge(cv, regions, ordered, skipped); t_oracle = (time.perf_counter() - t0) * n
mc.same_merge(res[0], want)
for r in res[1:]:
    mc.same_merge(r, res[0])

# the producer of a pass's region variants: lcd_batch_region_vars per region of a downloaded batch
bopt = align.default_opt(); bopt.collect_noisy_vars = 1
b = align.RegionBatch(bopt)
for r in jobs.make_regions(12, N_REGIONS):
    b.add_region(r)
b.upload(); b.run(); b.download()
lib, i32p = b.lib, C.POINTER(C.c_int)
cref = np.zeros(16, np.uint8)
def region_vars_calls():
    for k in range(N_REGIONS):
        vp = C.POINTER(LcdNoisyVar)(); nrows = C.c_int(0); ids, ps, pe, pa = i32p(), i32p(), i32p(), i32p()
        nv = lib.lcd_batch_region_vars(b.h, k, 1, None, 1, 0, C.byref(vp), C.byref(nrows), C.byref(ids), C.byref(ps), C.byref(pe), C.byref(pa))
        assert nv >= 0, nv
        for i in range(nv):
            if vp[i].alt_seq:
                align._libc.free(C.cast(vp[i].alt_seq, C.c_void_p))
        for p in (vp, ids, ps, pe, pa):
            if p:
                align._libc.free(C.cast(p, C.c_void_p))
region_vars_calls()
tr = []
for _ in range(3):
    t0 = time.perf_counter()
    for _ in range(n):
        region_vars_calls()
    tr.append(time.perf_counter() - t0)
b.close()

commit = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
h = hashlib.sha256()   # the measured code itself: the library's sources and the public header
for d in ("include", os.path.join("longcalld_amd", "csrc")):
    for f in sorted(os.listdir(os.path.join(ROOT, d))):
        if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(ROOT, d, f), "rb").read())
print(json.dumps(dict(tool="bench_merge_vars", commit=commit, source_sha256=h.hexdigest()[:16], n_chunks=n, n_reads=cv["n_reads"], n_vars=cv["n_vars"],
                      n_regions=N_REGIONS, n_vars_merged=res[0][0]["n_vars"], cells_before=int(cv["allele_off"][-1]), cells_after=int(res[0][0]["allele_off"][-1]),
                      ms_batch=round(t * 1e3, 2), ms_per_chunk=round(t * 1e3 / n, 3), ms_region_vars_calls=round(float(np.median(tr)) * 1e3, 2),
                      oracle_py_ms_batch=round(t_oracle * 1e3, 2), slower_than_oracle=bool(t > t_oracle), parity=True)), flush=True)
