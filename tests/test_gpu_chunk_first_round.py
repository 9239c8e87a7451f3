"""The real HG002 chunk from BAM records to noisy-region variants with nothing approximated in between:
    BAM --lcd_chunk_create_from_bam--> digars in HBM --lcd_sdust / lcd_pre_process_noisy_regs--> pre-processed regions
        --lcd_chunk_clean_vars--> candidate variants, final noisy regions, read x variant profile
        --lcd_clean_vars_hap_problem + lcd_assign_hap_germline (K5)--> haplotypes
        --the produced regions: lcd_chunk_region_slices + lcd_batch_add_region_from_chunk_dev--> K1..K4 --> lcd_batch_region_vars
Every stage equals its oracle on the same inputs (the reference's own sdust / cgranges where oracle/_ref is built, tests/c/clean_vars_oracle.c, oracle/)."""
import numpy as np
import pytest

import clean_vars_common as cc
from conftest import same_result
from test_gpu_clean_vars import write_chunk_bam
from test_gpu_vars import same_vars

pytestmark = pytest.mark.gpu


def _py_hap_problem(cv, ordered, skipped):
    """the K5 layout written out independently of lcd_clean_vars_hap_problem"""
    V, R = cv["n_vars"], cv["n_reads"]
    return dict(n_reads=R, n_vars=V, is_ont=0, var_pos=cv["pos"], var_type=cv["var_type"], var_cate=cv["cate"], is_homopolymer_indel=cv["is_homopolymer_indel"],
                total_cov=cv["total_cov"], alle_off=(2 * np.arange(V + 1)).astype(np.int32), alle_covs=cv["alle_covs"], start_var_idx=cv["start_var_idx"],
                end_var_idx=cv["end_var_idx"], allele_off=cv["allele_off"].astype(np.int32), alleles=cv["alleles"], ordered_read_ids=np.asarray(ordered, np.int32),
                is_skipped=np.asarray(skipped, np.uint8), cr_read=cv["cr_read"])


def test_bam_to_region_variants_through_the_first_round(lcd, oracle, tmp_path):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")
    from longcalld_amd import jobs
    ch = cc.events_chunk()
    o, ref = ch["ref_beg"], ch["ref"]
    path = str(tmp_path / "hg002.bam")
    write_chunk_bam(ch, path)
    # 1. records -> digars in HBM (== the oracle's digars of the same records)
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", ch["reg_beg"], ch["reg_end"], min_mapq=0)
    digs = cc.read_digars(ch, oracle)
    info, ivs = dev.read_info(), dev.intervals()
    n = dev.n
    assert n == len(ch["reads"])
    for i in range(n):
        assert (info["status"][i], info["beg"][i], info["end"][i], info["n_digars"][i]) == (digs[i]["rc"], digs[i]["beg"], digs[i]["end"], len(digs[i]["digars"]))
        assert (ivs[i][0] == digs[i]["noisy"]).all()
    # 2. low-complexity intervals, 3. pre-processed noisy regions
    low = lcd.sdust(ref, 5, 20)
    assert (low == oracle.ref_sdust(ref, 5, 20)).all()
    low_cr = np.stack([o + low[:, 0] - 1, o + low[:, 1] - 1], 1).astype(np.int64)
    kept = [i for i in range(n) if info["status"][i] != -1]
    chunk_noisy = np.concatenate([ivs[i][0][ivs[i][1]] for i in kept])
    rb, re_, rivs = [info["beg"][i] for i in kept], [info["end"][i] for i in kept], [ivs[i][0] for i in kept]
    pre = lcd.pre_process_noisy_regs(chunk_noisy, low_cr, rb, re_, rivs)
    assert (pre == oracle.ref_pre_process_noisy_regs(chunk_noisy, low_cr, rb, re_, rivs)).all()
    # 4. the first round
    ordered = np.arange(n, dtype=np.int32)
    is_rev = (np.asarray(dev.meta["flag"]) & 0x10 != 0).astype(np.uint8)
    opt = lcd.clean_opt(0)
    cv = dev.clean_vars(ordered, ref, o, o + len(ref) - 1, ch["reg_beg"], ch["reg_end"], pre, low_cr, is_rev=is_rev, opt=opt)
    want = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low_cr)
    cc.same_clean_vars(cv, want)
    # 5. K5 on the produced profile, through the C view
    skipped = (info["status"] == -1).astype(np.uint8)
    prob = lcd.clean_vars_hap_problem(cv, ordered, skipped)
    ref_prob = _py_hap_problem(want, ordered, skipped)
    for k, x in ref_prob.items():
        assert np.array_equal(np.asarray(prob[k]), np.asarray(x)), k
    st = lcd.assign_hap_germline(prob, jobs.GERMLINE_CLEAN)
    ex = oracle.assign_hap_germline(ref_prob, jobs.GERMLINE_CLEAN)
    for k in ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle"):
        assert (st[k] == ex[k]).all(), k
    assert (st["haps"] > 0).sum() > n // 2
    # 6. the produced regions (post_process_noisy_regs already applied: [start, end] as collect_noisy_vars1 reads them) through the hot path
    used, pr, pb, pe = [], [], [], []
    for s_, e_, _ in cv["regs"]:
        beg, end = int(s_), int(e_)
        if end - beg + 1 > 3000:
            continue
        ids = np.array([i for i in kept if not (info["beg"][i] > end or info["end"][i] <= beg)], np.int32)  # collect_noisy_reg_reads1
        if len(ids) < 5:
            continue
        used.append((beg, end, ids)); pr += list(ids); pb += [beg] * len(ids); pe += [end] * len(ids)
    assert len(used) >= 8
    srb, sre, scv = dev.region_slices(pr, pb, pe, 10)
    digars4 = [d["digars"][:, :4] for d in digs]
    bopt = lcd.default_opt(); bopt.collect_noisy_vars = 1
    b = lcd.RegionBatch(bopt)
    at = 0
    for beg, end, ids in used:
        k = len(ids)
        dev.add_region(b, beg, end, ids, srb[at:at + k], sre[at:at + k], scv[at:at + k], st["haps"][ids], st["phase_sets"][ids], ref[beg - o:end - o + 1])
        at += k
    b.upload(); b.run(); b.download()
    at = n_vars = 0
    for k, (beg, end, ids) in enumerate(used):
        seqs, qs, covers = [], [], []
        for j, i in enumerate(ids):
            r0, r1, c = oracle.read_region_slice(digars4[i], len(ch["reads"][i]["qual"]), beg, end, 10)
            assert (r0, r1, c) == (srb[at + j], sre[at + j], scv[at + j])
            seqs.append(ch["reads"][i]["seq"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
            qs.append(ch["reads"][i]["qual"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8)); covers.append(c)
        at += len(ids)
        reg = dict(reg_len=end - beg + 1, read_ids=ids, seqs=seqs, quals=qs, covers=np.array(covers, np.int32), haps=st["haps"][ids], phase_sets=st["phase_sets"][ids],
                   ref=ref[beg - o:end - o + 1])
        exp = oracle.collect_noisy_reg_aln_strs(reg)
        same_result(exp, b.result(k))
        got_v = b.region_vars(k, beg, ref, o)
        same_vars(oracle.make_vars_from_msa_cons_aln(exp, beg, ref, o), got_v)
        n_vars += got_v["n_vars"]
    assert n_vars > 0
    b.close(); dev.close()
