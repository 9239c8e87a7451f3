#!/usr/bin/env python
"""lcd_chunks_noisy_rounds (collect_var_main's noisy-region loop on device-resident chunks) on N seeded HiFi-shape chunks (tests/clean_vars_common.py
make_diploid_chunk): passes per chunk, the driver call as a whole, the same loop stepped through the batch exports with a timer around every stage (plan, hot
path = add + upload + run_many + download, region variants, merge, carry + K5), and the plan call alone against the host-pair path it replaces (lcd_chunk_read_info
-> pairs in Python -> lcd_chunk_region_slices -> per-region lcd_batch_add_region_from_chunk_dev), both ending with the first pass's regions in a batch.  All times
are through the Python mirror (host arrays in and out).  Prints one JSON line.
usage: bench_noisy_rounds.py [N=16] [ref_len=30000]"""
import hashlib, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from longcalld_amd import align as lcd, jobs
from oracle import pyoracle as oracle
import clean_vars_common as cc
import pass_plan_common as pc

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ref_len = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
oracle.build()
popt = lcd.pass_opt()

# ---- first round per chunk (not timed): records -> device chunk -> clean vars -> K5 over the clean categories
chunks = []
for i in range(n):
    ch = cc.make_diploid_chunk(300 + i, ref_len=ref_len)
    digs = cc.read_digars(ch, oracle)
    low = lcd.sdust(ch["ref"], 5, 20)
    low_cr = np.stack([ch["ref_beg"] + low[:, 0] - 1, ch["ref_beg"] + low[:, 1] - 1], 1).astype(np.int64)
    ci = cc.chunk_inputs(ch, digs)
    pre = lcd.pre_process_noisy_regs(ci["chunk_noisy"], low_cr, ci["read_beg"], ci["read_end"], ci["read_ivs"])
    r = ch["reads"]
    dev = lcd.DeviceChunk([x["pos0"] for x in r], [x["cigar"] for x in r], [x["qual"] for x in r], [x["bseq"] for x in r], ch["reg_beg"], ch["reg_end"], ch["whole_ref_len"])
    ordered = np.arange(len(r), dtype=np.int32)
    cv = dev.clean_vars(ordered, ch["ref"], ch["ref_beg"], ch["ref_beg"] + len(ch["ref"]) - 1, ch["reg_beg"], ch["reg_end"], pre, low_cr,
                        is_rev=np.array([x["is_rev"] for x in r], np.uint8))
    skipped = np.array([d["rc"] != 0 for d in digs], np.uint8)
    st = lcd.assign_hap_germline(lcd.clean_vars_hap_problem(cv, ordered, skipped), jobs.GERMLINE_CLEAN)
    chunks.append(dict(ch=ch, dev=dev, cv=cv, st=st, ordered=ordered, skipped=skipped, ref=ch["ref"], ref_beg=ch["ref_beg"]))
items = [dict(cv=c["cv"], state=c["st"], ordered_read_ids=c["ordered"], is_skipped=c["skipped"], ref=c["ref"], ref_beg=c["ref_beg"]) for c in chunks]
devs = [c["dev"] for c in chunks]

# ---- the driver
lcd.chunks_noisy_rounds(devs, items, popt=popt)                                   # warm-up
ts = []
for _ in range(3):
    t0 = time.perf_counter(); res = lcd.chunks_noisy_rounds(devs, items, popt=popt); ts.append(time.perf_counter() - t0)
ms_driver = float(np.median(ts)) * 1e3

# ---- the same loop through the batch exports, a timer per stage and pass
bopt = lcd.default_opt(); bopt.collect_noisy_vars = 2
cur = [dict(cv=c["cv"], st=c["st"], done=np.zeros(len(c["cv"]["regs"]), np.int32), order=lcd.sort_noisy_regs(c["cv"]["regs"]), passes=0, live=len(c["cv"]["regs"]) > 0) for c in chunks]
passes = []
while any(x["live"] for x in cur):
    A = [i for i, x in enumerate(cur) if x["live"]]
    T = dict(plan=0.0, hot_path=0.0, region_vars=0.0, merge=0.0, carry_k5=0.0)
    t0 = time.perf_counter()
    plans = lcd.plan_pass_batch([devs[i] for i in A], [dict(regs=cur[i]["cv"]["regs"], done=cur[i]["done"], ordered_read_ids=chunks[i]["ordered"], is_skipped=chunks[i]["skipped"],
                                                            ref_beg=chunks[i]["ref_beg"], ref_end=chunks[i]["ref_beg"] + len(chunks[i]["ref"]) - 1) for i in A], popt)
    T["plan"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    bs, idxs = [], []
    for i, p in zip(A, plans):
        b = lcd.RegionBatch(bopt)
        idxs.append(b.add_planned(devs[i], p, cur[i]["st"]["haps"], cur[i]["st"]["phase_sets"], chunks[i]["ref"], chunks[i]["ref_beg"]))
        bs.append(b)
    run = [b for b, ix in zip(bs, idxs) if (ix >= 0).any()]
    for b in run:
        b.upload()
    lcd.RegionBatch.run_many(run)
    for b in run:
        b.download()
    T["hot_path"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    gots, newdone = [], []
    for i, p, b, ix in zip(A, plans, bs, idxs):
        got, nd = [], False
        for k in cur[i]["order"]:
            if p["status"][k] in (pc.SKIP_LONG, pc.SKIP_DEEP):
                cur[i]["done"][k] = 1; nd = True
            if p["status"][k] != pc.SUBMIT or b.n_cons(int(ix[k])) == 0:
                continue
            cur[i]["done"][k] = 1; nd = True
            got.append(b.region_vars(int(ix[k]), int(p["beg"][k]), chunks[i]["ref"], chunks[i]["ref_beg"]))
        gots.append(got); newdone.append(nd)
    T["region_vars"] = time.perf_counter() - t0
    for b in bs:
        b.close()
    M = [q for q, got in enumerate(gots) if any(v["n_vars"] > 0 for v in got)]
    if M:
        t0 = time.perf_counter()
        merged = lcd.merge_region_vars_batch([cur[A[q]]["cv"] for q in M], [gots[q] for q in M], [chunks[A[q]]["ordered"] for q in M], [chunks[A[q]]["skipped"] for q in M])
        T["merge"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        sts = [lcd.hap_state_carry(cur[A[q]]["st"], m[0]["n_vars"], m[1]) for q, m in zip(M, merged)]
        probs = [lcd.clean_vars_hap_problem(m[0], chunks[A[q]]["ordered"], chunks[A[q]]["skipped"]) for q, m in zip(M, merged)]
        sts = lcd.assign_hap_batch(probs, [pc.GERMLINE_ALL] * len(M), sts)
        T["carry_k5"] = time.perf_counter() - t0
        for q, m, s in zip(M, merged, sts):
            cur[A[q]]["cv"], cur[A[q]]["st"] = m[0], s
    for i, nd in zip(A, newdone):
        cur[i]["passes"] += 1
        cur[i]["live"] = nd
    passes.append(dict(chunks=len(A), regions_submitted=int(sum((p["status"] == pc.SUBMIT).sum() for p in plans)), pairs=int(sum(len(p["read_ids"]) for p in plans)),
                       **{k: round(v * 1e3, 2) for k, v in T.items()}))
for x, r in zip(cur, res):                                                          # the stepped loop and the driver agree
    assert x["passes"] == r["n_passes"] and (x["done"] == r["done"]).all()
    cc.same_clean_vars(x["cv"], r["cv"]); pc.same_state(x["st"], r["state"])

# ---- the first pass's regions into batches: the plan call against the host-pair path (both on every chunk, chunk by chunk for the host-pair path as a caller
# without the plan has to; regions of the first pass, all pending)
def with_plan():
    plans = lcd.plan_pass_batch(devs, [dict(regs=c["cv"]["regs"], done=np.zeros(len(c["cv"]["regs"]), np.int32), ordered_read_ids=c["ordered"], is_skipped=c["skipped"],
                                            ref_beg=c["ref_beg"], ref_end=c["ref_beg"] + len(c["ref"]) - 1) for c in chunks], popt)
    t_plan = time.perf_counter()
    bs = []
    for c, p in zip(chunks, plans):
        b = lcd.RegionBatch(bopt); b.add_planned(c["dev"], p, c["st"]["haps"], c["st"]["phase_sets"], c["ref"], c["ref_beg"]); bs.append(b)
    return bs, t_plan
def host_pairs():
    bs = []
    t_pairs = 0.0
    for c in chunks:
        t0 = time.perf_counter()
        info = c["dev"].read_info()
        used = []
        rb, re_ = c["ref_beg"], c["ref_beg"] + len(c["ref"]) - 1
        for beg, end, _ in c["cv"]["regs"]:
            beg, end = max(int(beg), rb), min(int(end), re_)
            if end - beg + 1 > popt.max_noisy_reg_len:
                continue
            ids = np.array([r for r in c["ordered"] if not c["skipped"][r] and not (info["beg"][r] > end or info["end"][r] <= beg)], np.int32)
            if 0 < len(ids) <= popt.max_noisy_reg_cov:
                used.append((beg, end, ids))
        if used:
            pr = np.concatenate([u[2] for u in used]); pb = np.concatenate([[u[0]] * len(u[2]) for u in used]); pe = np.concatenate([[u[1]] * len(u[2]) for u in used])
            srb, sre, scv = c["dev"].region_slices(pr, pb, pe, popt.noisy_reg_flank_len)
        t_pairs += time.perf_counter() - t0
        b = lcd.RegionBatch(bopt); at = 0
        for beg, end, ids in used:
            k = len(ids)
            c["dev"].add_region(b, beg, end, ids, srb[at:at + k], sre[at:at + k], scv[at:at + k], c["st"]["haps"][ids], c["st"]["phase_sets"][ids], c["ref"][beg - rb:end - rb + 1])
            at += k
        bs.append(b)
    return bs, t_pairs
def timed(f):
    out = []
    for k in range(4):
        t0 = time.perf_counter(); bs, mark = f(); t1 = time.perf_counter()
        n_regs = sum(len(b.n_reads) for b in bs)
        for b in bs:
            b.close()
        if k:
            out.append((t1 - t0, mark - t0 if f is with_plan else mark, n_regs))
    return float(np.median([o[0] for o in out])) * 1e3, float(np.median([o[1] for o in out])) * 1e3, out[0][2]
ms_plan_path, ms_plan_only, nr1 = timed(with_plan)
ms_host_path, ms_host_pairs_only, nr2 = timed(host_pairs)
assert nr1 == nr2

commit = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
h = hashlib.sha256()   # the measured code itself: the library's sources and the public header
for d in ("include", os.path.join("longcalld_amd", "csrc")):
    for f in sorted(os.listdir(os.path.join(ROOT, d))):
        if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile":
            h.update(f.encode()); h.update(open(os.path.join(ROOT, d, f), "rb").read())
print(json.dumps(dict(tool="bench_noisy_rounds", commit=commit, source_sha256=h.hexdigest()[:16], n_chunks=n, ref_len=ref_len, reads_per_chunk=len(chunks[0]["ch"]["reads"]),
                      regions_per_chunk=[len(c["cv"]["regs"]) for c in chunks], passes_per_chunk=[r["n_passes"] for r in res],
                      vars_first_round=int(sum(c["cv"]["n_vars"] for c in chunks)), vars_final=int(sum(r["cv"]["n_vars"] for r in res)), ms_driver=round(ms_driver, 2),
                      stepped_passes=passes, first_pass_regions=nr1, ms_plan_then_add=round(ms_plan_path, 2), ms_plan_call=round(ms_plan_only, 2),
                      ms_host_pairs_then_add=round(ms_host_path, 2), ms_host_pairs_and_slices=round(ms_host_pairs_only, 2),
                      plan_beats_host_pairs=bool(ms_plan_only < ms_host_pairs_only), parity=True)), flush=True)
