"""The real HG002 chunk one step past tests/test_gpu_chunk_first_round.py: the first pass's noisy-region variants are merged into the chunk
(lcd_sort_noisy_regs -> lcd_merge_region_vars) and K5 runs again over all germline categories, as collect_var_main does (src/collect_var.c:2946-2977).
    BAM --> digars in HBM --> lcd_chunk_clean_vars --> K5 (clean categories) --> the region hot path --> lcd_batch_region_vars
        --lcd_merge_region_vars--> merged variant table + profile --lcd_clean_vars_hap_problem + lcd_assign_hap_germline(GERMLINE_ALL)--> haplotypes
The merge equals the pure-Python oracle on the oracle's own region variants, the second K5 equals oracle/assign_hap.c on the oracle-merged problem."""
import numpy as np
import pytest

import clean_vars_common as cc
import merge_vars_common as mc
from test_gpu_chunk_first_round import _py_hap_problem
from test_gpu_clean_vars import write_chunk_bam
from test_gpu_vars import same_vars

pytestmark = pytest.mark.gpu


def _carry(state, fresh, c2m):
    """the first call's K5 state on the merged table: per-read arrays as they are, per-variant arrays through cur_to_merged; variants that came from a
    region keep the fresh values"""
    out = {k: v.copy() for k, v in fresh.items()}
    for k in ("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps"):
        out[k] = state[k].copy()
    out["var_phase_set"][c2m] = state["var_phase_set"]
    out["hap_to_cons_alle"].reshape(-1, 3)[c2m] = state["hap_to_cons_alle"].reshape(-1, 3)
    out["hap_to_alle_profile"].reshape(3, -1, 2)[:, c2m, :] = state["hap_to_alle_profile"].reshape(3, -1, 2)   # [hap][variant][allele], two alleles each
    return out


def test_first_noisy_pass_merge_and_second_k5(lcd, oracle, tmp_path):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")
    from longcalld_amd import align, jobs
    ch = cc.events_chunk()
    o, ref = ch["ref_beg"], ch["ref"]
    path = str(tmp_path / "hg002.bam")
    write_chunk_bam(ch, path)
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", ch["reg_beg"], ch["reg_end"], min_mapq=0)
    digs = cc.read_digars(ch, oracle)
    info, ivs = dev.read_info(), dev.intervals()
    n = dev.n
    low = lcd.sdust(ref, 5, 20)
    low_cr = np.stack([o + low[:, 0] - 1, o + low[:, 1] - 1], 1).astype(np.int64)
    kept = [i for i in range(n) if info["status"][i] != -1]
    chunk_noisy = np.concatenate([ivs[i][0][ivs[i][1]] for i in kept])
    rb, re_, rivs = [info["beg"][i] for i in kept], [info["end"][i] for i in kept], [ivs[i][0] for i in kept]
    pre = lcd.pre_process_noisy_regs(chunk_noisy, low_cr, rb, re_, rivs)
    ordered = np.arange(n, dtype=np.int32)
    is_rev = (np.asarray(dev.meta["flag"]) & 0x10 != 0).astype(np.uint8)
    opt = lcd.clean_opt(0)
    cv = dev.clean_vars(ordered, ref, o, o + len(ref) - 1, ch["reg_beg"], ch["reg_end"], pre, low_cr, is_rev=is_rev, opt=opt)
    want = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low_cr)
    cc.same_clean_vars(cv, want)
    skipped = (info["status"] == -1).astype(np.uint8)
    prob = lcd.clean_vars_hap_problem(cv, ordered, skipped)
    ref_prob = _py_hap_problem(want, ordered, skipped)
    st = lcd.assign_hap_germline(prob, jobs.GERMLINE_CLEAN)
    ex = oracle.assign_hap_germline(ref_prob, jobs.GERMLINE_CLEAN)
    for k in ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle"):
        assert (st[k] == ex[k]).all(), k
    # the used regions in the order collect_var_main processes them
    used = []
    for ri in lcd.sort_noisy_regs(cv["regs"]):
        beg, end = int(cv["regs"][ri][0]), int(cv["regs"][ri][1])
        if end - beg + 1 > 3000:
            continue
        ids = np.array([i for i in kept if not (info["beg"][i] > end or info["end"][i] <= beg)], np.int32)
        if len(ids) >= 5:
            used.append((beg, end, ids))
    assert len(used) >= 8
    labels = [int(cv["regs"][ri][2]) for ri in lcd.sort_noisy_regs(cv["regs"])]
    assert labels == sorted(labels)
    pr = np.concatenate([u[2] for u in used]); pb = np.concatenate([[u[0]] * len(u[2]) for u in used]); pe = np.concatenate([[u[1]] * len(u[2]) for u in used])
    srb, sre, scv = dev.region_slices(pr, pb, pe, 10)
    bopt = lcd.default_opt(); bopt.collect_noisy_vars = 1
    b = lcd.RegionBatch(bopt)
    at = 0
    for beg, end, ids in used:
        k = len(ids)
        dev.add_region(b, beg, end, ids, srb[at:at + k], sre[at:at + k], scv[at:at + k], st["haps"][ids], st["phase_sets"][ids], ref[beg - o:end - o + 1])
        at += k
    b.upload(); b.run(); b.download()
    got_regs, exp_regs = [], []
    at = 0
    for k, (beg, end, ids) in enumerate(used):
        seqs, qs = [], []
        for j, i in enumerate(ids):
            r0, r1 = srb[at + j], sre[at + j]
            seqs.append(ch["reads"][i]["seq"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
            qs.append(ch["reads"][i]["qual"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
        reg = dict(reg_len=end - beg + 1, read_ids=ids, seqs=seqs, quals=qs, covers=np.asarray(scv[at:at + len(ids)], np.int32), haps=st["haps"][ids],
                   phase_sets=st["phase_sets"][ids], ref=ref[beg - o:end - o + 1])
        at += len(ids)
        exp_res = oracle.collect_noisy_reg_aln_strs(reg)
        exp_v = oracle.make_vars_from_msa_cons_aln(exp_res, beg, ref, o)
        # the oracle's rows: the reads of cluster 0, then of cluster 1, in its own clu_read_ids order
        exp_v["row_read_ids"] = np.concatenate([np.asarray(exp_res["clu_read_ids"][c], np.int32) for c in range(exp_res["n_cons"])] + [np.zeros(0, np.int32)])
        got_v = b.region_vars(k, beg, ref, o)
        same_vars(exp_v, got_v)
        assert len(exp_v["row_read_ids"]) == exp_v["n_rows"]
        got_regs.append(got_v); exp_regs.append(exp_v)
    b.close(); dev.close()
    # merge: the library on its own region variants == the oracle merge of the oracle's region variants
    got = lcd.merge_region_vars(cv, got_regs, ordered, skipped)
    exp = mc.oracle_merge(want, exp_regs, ordered, skipped)
    mc.same_merge(got, exp)
    merged, c2m, _ = got
    assert merged["n_vars"] > cv["n_vars"]
    # K5 again over all germline categories, the first call's state carried through cur_to_merged on both sides
    prob2 = lcd.clean_vars_hap_problem(merged, ordered, skipped)
    ref_prob2 = _py_hap_problem(exp[0], ordered, skipped)
    for k, x in ref_prob2.items():
        assert np.array_equal(np.asarray(prob2[k]), np.asarray(x)), k
    st2 = lcd.assign_hap_germline(prob2, jobs.GERMLINE_ALL, state=_carry(st, align._hap_state(prob2), c2m))
    ex2 = oracle.assign_hap_germline(ref_prob2, jobs.GERMLINE_ALL, state=_carry(ex, align._hap_state(ref_prob2), exp[1]))
    for k in ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle"):
        assert (st2[k] == ex2[k]).all(), k
