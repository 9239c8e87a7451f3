"""Shared by tests/test_pass_plan.py, tests/test_gpu_pass_plan.py, tests/test_gpu_noisy_rounds.py and tools/bench_noisy_rounds.py: a pure-Python oracle of the
plan of one noisy-region pass, written from the reference's statements (collect_noisy_vars1 src/collect_var.c:2650-2663, collect_reg_ref_bseq src/seq.c:415-426,
collect_noisy_reg_reads1 src/collect_var.c:1047-1061), the K5 state's way across a merge, and the loop of collect_var_main (:2946-2977) composed from the
existing oracles: oracle.read_region_slice, oracle.collect_noisy_reg_aln_strs, oracle.make_vars_from_msa_cons_aln, merge_vars_common.oracle_merge and
oracle.assign_hap_germline."""
import numpy as np

import merge_vars_common as mc

DONE_BEFORE, SKIP_LONG, SKIP_DEEP, NO_READS, SUBMIT = range(5)
GERMLINE_ALL = 0x004 | 0x008 | 0x080 | 0x100 | 0x200   # LONGCALLD_CAND_GERMLINE_VAR_CATE, src/collect_var.h:25
STATE_KEYS = ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle")


def oracle_plan(regs, done, ordered, skipped, read_beg, read_end, ref_beg, ref_end, max_len=50000, max_cov=1000):
    """-> (status, beg, end, [read ids per region]) for every region of regs (n, 3) start / end / label"""
    status, begs, ends, lists = [], [], [], []
    for (s, e, _), d in zip(np.asarray(regs, np.int64).reshape(-1, 3), done):
        beg, end = max(int(s), int(ref_beg)), min(int(e), int(ref_end))
        begs.append(beg); ends.append(end)
        ids = []
        if d:
            st = DONE_BEFORE
        elif end - beg + 1 > max_len:
            st = SKIP_LONG
        else:
            ids = [int(r) for r in ordered if not skipped[r] and not (read_beg[r] > end or read_end[r] <= beg)]
            st = SKIP_DEEP if len(ids) > max_cov else NO_READS if not ids else SUBMIT
            if st != SUBMIT:
                ids = []
        status.append(st); lists.append(ids)
    return np.array(status, np.int32), np.array(begs, np.int64), np.array(ends, np.int64), lists


def same_plan(plan, want):
    status, begs, ends, lists = want
    assert (plan["status"] == status).all(), (plan["status"], status)
    assert (plan["beg"] == begs).all() and (plan["end"] == ends).all()
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    assert (plan["read_off"] == off).all(), (plan["read_off"], off)
    flat = np.array([r for x in lists for r in x], np.int32)
    assert (plan["read_ids"] == flat).all()
    assert len(plan["read_beg"]) == len(plan["read_end"]) == len(plan["cover"]) == len(flat)


def plan_pairs(plan):
    """-> (pair_read, pair_beg, pair_end): the plan's pairs as lcd_chunk_region_slices takes them"""
    n = np.diff(plan["read_off"])
    return plan["read_ids"], np.repeat(plan["beg"], n), np.repeat(plan["end"], n)


def sort_noisy_regs(regs):
    """sort_noisy_regs (src/collect_var.c:2745-2769): the exchange sort by label, then end - start, with its own swap sequence"""
    regs = np.asarray(regs, np.int64).reshape(-1, 3)
    o = list(range(len(regs)))
    key = lambda i: (int(regs[i][2]), int(regs[i][1] - regs[i][0]))
    for i in range(len(o)):
        for j in range(i + 1, len(o)):
            if key(o[i]) > key(o[j]):
                o[i], o[j] = o[j], o[i]
    return o


def fresh_state(R, V):
    return dict(haps=np.zeros(R, np.int32), phase_sets=np.full(R, -1, np.int64), n_clean_agree_snps=np.zeros(R, np.int32), n_clean_conflict_snps=np.zeros(R, np.int32),
                var_phase_set=np.full(V, -1, np.int64), hap_to_cons_alle=np.full(V * 3, -1, np.int32), hap_to_alle_profile=np.zeros(6 * V, np.int32))


def carry(state, n_merged, c2m):
    """K5's state on the merged table: per-read arrays as they are, per-variant arrays through cur_to_merged; variants that came from a region keep the fresh
    values (-1, -1, 0)"""
    out = fresh_state(len(state["haps"]), n_merged)
    for k in ("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps"):
        out[k] = state[k].copy()
    c2m = np.asarray(c2m, np.int64)
    out["var_phase_set"][c2m] = state["var_phase_set"]
    out["hap_to_cons_alle"].reshape(-1, 3)[c2m] = state["hap_to_cons_alle"].reshape(-1, 3)
    out["hap_to_alle_profile"].reshape(3, -1, 2)[:, c2m, :] = state["hap_to_alle_profile"].reshape(3, -1, 2)   # [hap][variant][allele]
    return out


def same_state(a, b, keys=None):
    for k in keys or fresh_state(0, 0).keys():
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x == y).all(), k


def py_hap_problem(cv, ordered, skipped, is_ont=0):
    """the K5 layout over a clean_vars_dict, written out independently of lcd_clean_vars_hap_problem"""
    V, R = cv["n_vars"], cv["n_reads"]
    return dict(n_reads=R, n_vars=V, is_ont=is_ont, var_pos=cv["pos"], var_type=cv["var_type"], var_cate=cv["cate"], is_homopolymer_indel=cv["is_homopolymer_indel"],
                total_cov=cv["total_cov"], alle_off=(2 * np.arange(V + 1)).astype(np.int32), alle_covs=cv["alle_covs"], start_var_idx=cv["start_var_idx"],
                end_var_idx=cv["end_var_idx"], allele_off=np.asarray(cv["allele_off"]).astype(np.int32), alleles=cv["alleles"],
                ordered_read_ids=np.asarray(ordered, np.int32), is_skipped=np.asarray(skipped, np.uint8), cr_read=cv["cr_read"])


def oracle_region(oracle, ch, digs, beg, end, ids, state, flank=10):
    """one submitted region through the oracles -> (n_cons, region variants dict or None)"""
    ref, o = ch["ref"], ch["ref_beg"]
    seqs, quals, covers = [], [], []
    for r in ids:
        rd = ch["reads"][r]
        r0, r1, cv = oracle.read_region_slice(digs[r]["digars"][:, :4], len(rd["qual"]), beg, end, flank)
        seqs.append(rd["seq"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
        quals.append(rd["qual"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
        covers.append(cv)
    ids = np.asarray(ids, np.int32)
    reg = dict(reg_len=end - beg + 1, read_ids=ids, seqs=seqs, quals=quals, covers=np.asarray(covers, np.int32), haps=state["haps"][ids],
               phase_sets=state["phase_sets"][ids], ref=ref[beg - o:end - o + 1])
    res = oracle.collect_noisy_reg_aln_strs(reg)
    if res["n_cons"] == 0:
        return 0, None
    v = oracle.make_vars_from_msa_cons_aln(res, beg, ref, o)
    v["row_read_ids"] = np.concatenate([np.asarray(res["clu_read_ids"][c], np.int32) for c in range(res["n_cons"])] + [np.zeros(0, np.int32)])
    return res["n_cons"], v


def oracle_rounds(oracle, ch, digs, cv, state, ordered, skipped, max_len=50000, max_cov=1000, flank=10, max_passes=20):
    """collect_var_main's loop (src/collect_var.c:2946-2977) from "first round done" to its fixed point
    -> dict(cv, state, done, n_passes, first_to_final, productive: passes that merged a variant, resolved: regions resolved per pass)"""
    rb = [d["beg"] for d in digs]; re_ = [d["end"] for d in digs]
    o, ref = ch["ref_beg"], ch["ref"]
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    order = sort_noisy_regs(regs)
    done = np.zeros(len(regs), np.int32)
    f2f = np.arange(cv["n_vars"], dtype=np.int32)
    n_passes, productive, resolved = 0, 0, []
    state = {k: v.copy() for k, v in state.items()}
    while len(regs) and n_passes < max_passes:
        n_passes += 1
        status, begs, ends, lists = oracle_plan(regs, done, ordered, skipped, rb, re_, o, o + len(ref) - 1, max_len, max_cov)
        new_done, got = False, []
        for i in order:
            if status[i] in (SKIP_LONG, SKIP_DEEP):
                done[i] = 1; new_done = True
            if status[i] != SUBMIT:
                continue
            n_cons, v = oracle_region(oracle, ch, digs, int(begs[i]), int(ends[i]), lists[i], state, flank)
            if n_cons == 0:
                continue
            done[i] = 1; new_done = True
            got.append(v)
        resolved.append(len(got))
        if any(v["n_vars"] > 0 for v in got):
            productive += 1
            merged, c2m, _ = mc.oracle_merge(cv, got, ordered, skipped)
            state = carry(state, merged["n_vars"], c2m)
            state = oracle.assign_hap_germline(py_hap_problem(merged, ordered, skipped, ch.get("is_ont", 0)), GERMLINE_ALL, state=state)
            cv, f2f = merged, np.asarray(c2m, np.int32)[f2f]
        if not new_done:
            break
    return dict(cv=cv, state=state, done=done, n_passes=n_passes, first_to_final=f2f, productive=productive, resolved=resolved)


def stepped_rounds(lcd, dev, cv, state, ordered, skipped, ref, ref_beg, popt, is_ont=0, max_passes=20):
    """the same loop through the library's single exports: sort_noisy_regs -> plan_pass -> RegionBatch.add_planned -> run -> region_vars -> merge_region_vars ->
    hap_state_carry -> clean_vars_hap_problem -> assign_hap_germline"""
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    order = lcd.sort_noisy_regs(regs)
    done = np.zeros(len(regs), np.int32)
    f2f = np.arange(cv["n_vars"], dtype=np.int32)
    bopt = lcd.default_opt(); bopt.collect_noisy_vars = 2
    n_passes = 0
    while len(regs) and n_passes < max_passes:
        n_passes += 1
        plan = lcd.plan_pass(dev, regs, done, ordered, skipped, ref_beg, ref_beg + len(ref) - 1, popt)
        new_done, got = False, []
        b = lcd.RegionBatch(bopt)
        idx = b.add_planned(dev, plan, state["haps"], state["phase_sets"], ref, ref_beg)
        if (idx >= 0).any():
            b.upload(); b.run(); b.download()
        for i in order:
            if plan["status"][i] in (SKIP_LONG, SKIP_DEEP):
                done[i] = 1; new_done = True
            if plan["status"][i] != SUBMIT or b.n_cons(int(idx[i])) == 0:
                continue
            done[i] = 1; new_done = True
            got.append(b.region_vars(int(idx[i]), int(plan["beg"][i]), ref, ref_beg))
        b.close()
        if any(v["n_vars"] > 0 for v in got):
            merged, c2m, _ = lcd.merge_region_vars(cv, got, ordered, skipped)
            state = lcd.hap_state_carry(state, merged["n_vars"], c2m)
            state = lcd.assign_hap_germline(lcd.clean_vars_hap_problem(merged, ordered, skipped, is_ont), GERMLINE_ALL, state=state)
            cv, f2f = merged, np.asarray(c2m, np.int32)[f2f]
        if not new_done:
            break
    return dict(cv=cv, state=state, done=done, n_passes=n_passes, first_to_final=f2f)


def same_rounds(got, want):
    import clean_vars_common as cc
    assert got["n_passes"] == want["n_passes"], (got["n_passes"], want["n_passes"])
    assert (np.asarray(got["done"]) == np.asarray(want["done"])).all()
    assert (np.asarray(got["first_to_final"]) == np.asarray(want["first_to_final"])).all()
    cc.same_clean_vars(got["cv"], want["cv"])
    same_state(got["state"], want["state"], STATE_KEYS)


def two_pass_chunk(seed=5):
    """a seeded chunk whose second pass resolves a region the first one leaves open.  Haplotype 1 carries two clusters of 8 SNPs in 64 bp (two noisy regions),
    1 500 bp apart, and there is no clean heterozygous variant, so the first K5 call phases nothing.  Ten reads (five per haplotype) cover the first cluster:
    enough full-cover reads (min_dp 5) for the unphased path, which yields heterozygous variants, and K5 over all germline categories then phases every read.
    Only four of the reads (two per haplotype) reach the second cluster: unphased, that region has neither a phase set with both haplotypes nor five full-cover
    reads (n_cons == 0, not done); in the second pass the four reads are phased and the region is resolved.  The third pass finds nothing to do."""
    import clean_vars_common as cc
    rng = np.random.default_rng(seed)
    L = 6000
    ref = rng.integers(0, 4, L).astype(np.uint8)
    hap1 = {}
    for base in (2000, 3500):
        for k in range(8):
            p = base + 8 * k
            hap1[p] = ("X", int((ref[p] + 1 + k % 3) % 4))
    hom = {1000: ("X", int((ref[1000] + 1) % 4))}
    reads = []
    for i in range(10):
        end = 4200 if i < 4 else 3300 - 20 * i
        s = 500 + 30 * i
        ev = dict(hom); ev.update(hap1 if i % 2 == 0 else {})
        reads.append(cc.read_from_hap(ref, s, end - s, ev))
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=L, whole_ref_len=L, is_ont=0)
