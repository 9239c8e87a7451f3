"""SURVEY 8(f) f1 on the GPU: candidate variants + read x variant profile of a region (stage S6, vars_kernel.hip through
lcd_batch_region_vars) vs the oracle's restatement of make_vars_from_msa_cons_aln (src/collect_var.c:2279) run on the oracle's strings --
every field bit-identical, on seeded synthetic regions (HiFi / ONT shapes, K1 and K2 branches), on the reference's bundled real chunk and on the
planted-variant cases of tests/vars_cases.py (tests/test_vars_cases_oracle.py shows on the CPU which edge each of those reaches)."""
import functools

import numpy as np
import pytest

import testdata_common as tc
import vars_cases as vc

pytestmark = pytest.mark.gpu

KEYS = ("pos", "var_type", "ref_len", "alt_len", "cate", "from_cons", "is_homopolymer_indel", "ref_base", "alt_ref_base", "total_cov")


def same_vars(exp, got, ids=None):
    assert exp["n_vars"] == got["n_vars"]
    for k in KEYS:
        assert (exp[k] == got[k]).all(), (k, exp[k], got[k])
    assert (exp["alle_covs"] == got["alle_covs"]).all()
    for a, b in zip(exp["alt_seqs"], got["alt_seqs"]):
        assert a.tobytes() == b.tobytes()
    assert exp["n_rows"] == got["n_rows"]
    assert (exp["prof_start"] == got["prof_start"]).all() and (exp["prof_end"] == got["prof_end"]).all()
    assert (exp["prof_alleles"] == got["prof_alleles"]).all()
    if ids is not None:
        assert (np.concatenate(ids) == got["row_read_ids"]).all()


def _opt(lcd, mode):
    o = lcd.default_opt()
    o.collect_noisy_vars = mode
    return o


@pytest.mark.parametrize("shape,seed,n", [("hifi", 11, 40), ("ont", 12, 12)])
def test_vars_match_oracle_synthetic(lcd, oracle, shape, seed, n):
    from longcalld_amd import jobs
    regs = jobs.make_regions(seed, n, jobs.HIFI if shape == "hifi" else jobs.ONT)
    rng = np.random.default_rng(seed)
    b = lcd.RegionBatch(_opt(lcd, 1))
    for r in regs:
        b.add_region(r)
    b.upload(); b.run(); b.download()
    n_vars = n_hom = 0
    for k, r in enumerate(regs):
        beg = 100000 + 5000 * k
        cref = np.concatenate([r["ref"], rng.integers(0, 4, 8).astype(np.uint8)])   # chunk reference continues past the region
        res = oracle.collect_noisy_reg_aln_strs(r)
        exp = oracle.make_vars_from_msa_cons_aln(res, beg, cref, beg)
        got = b.region_vars(k, beg, cref, beg)
        ids = [res["clu_read_ids"][c] for c in range(res["n_cons"])] if res["n_cons"] else None
        same_vars(exp, got, ids)
        n_vars += got["n_vars"]; n_hom += int((got["cate"] == 0x200).sum())
    assert n_vars > n
    assert b.stats()["ms_vars"] > 0
    b.close()


def test_vars_only_download(lcd, oracle):
    """opt.collect_noisy_vars == 2: the strings stay in HBM, the variants are the same, lcd_batch_region_result refuses"""
    from longcalld_amd import jobs
    regs = jobs.make_regions(21, 12, jobs.HIFI)
    b = lcd.RegionBatch(_opt(lcd, 2))
    for r in regs:
        b.add_region(r)
    b.upload(); b.run(); b.download()
    for k, r in enumerate(regs):
        res = oracle.collect_noisy_reg_aln_strs(r)
        same_vars(oracle.make_vars_from_msa_cons_aln(res, 1000, r["ref"], 1000), b.region_vars(k, 1000, r["ref"], 1000))
    with pytest.raises(Exception):
        b.result(0)
    b.close()


def test_vars_on_real_chunk(lcd, oracle):
    """K5 haplotypes -> K1 -> strings -> variants, on the reference's bundled HG002 reads"""
    ch = tc.Chunk()
    haps, pss = ch.z["exp_haps"], ch.z["exp_phase_sets"]
    views, keep = lcd.make_read_views(ch.digars, ch.bseq, ch.qual, ch.qlen, haps, pss)
    b = lcd.RegionBatch(_opt(lcd, 1))
    for k, (beg, end) in enumerate(ch.regions):
        b.add_region_from_chunk(views, beg, end, ch.reg_reads(k), ch.ref_slice(k))
    b.upload(); b.run(); b.download()
    o = int(ch.z["ref_beg"])
    tot = het = 0
    for k, (beg, end) in enumerate(ch.regions):
        res = oracle.collect_noisy_reg_aln_strs(ch.region_dict(oracle, k, haps, pss))
        exp = oracle.make_vars_from_msa_cons_aln(res, beg, ch.z["ref"], o)
        got = b.region_vars(k, beg, ch.z["ref"], o)
        same_vars(exp, got, [res["clu_read_ids"][c] for c in range(res["n_cons"])])
        tot += got["n_vars"]; het += int((got["cate"] == 0x100).sum())
    assert tot == int(ch.z["exp_n_noisy_vars"]) and het > 0
    b.close()
    del keep


def test_vars_joint_submission(lcd, oracle):
    """lcd_batch_run_many with stage S6: two batches in one set of launches, each gets its own variants"""
    from longcalld_amd import jobs
    sets = [jobs.make_regions(31, 10, jobs.HIFI), jobs.make_regions(32, 7, jobs.HIFI)]
    bs = []
    for regs in sets:
        b = lcd.RegionBatch(_opt(lcd, 1))
        for r in regs:
            b.add_region(r)
        b.upload(); bs.append(b)
    lcd.RegionBatch.run_many(bs)
    for b in bs:
        b.download()
    for b, regs in zip(bs, sets):
        for k, r in enumerate(regs):
            res = oracle.collect_noisy_reg_aln_strs(r)
            same_vars(oracle.make_vars_from_msa_cons_aln(res, 500, r["ref"], 500), b.region_vars(k, 500, r["ref"], 500))
    for b in reversed(bs):
        b.close()


# ---------------------------------------------------------------- planted-variant cases (tests/vars_cases.py) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(oracle, name, gap_aln):
    """the oracle's (variants, row read ids) of a case, computed once and shared"""
    res, exp = vc.through_oracle(oracle, vc.cases()[name], gap_aln)
    return exp, [res["clu_read_ids"][c] for c in range(res["n_cons"])]


def _case_opt(lcd, mode, gap_aln=1):
    o = _opt(lcd, mode)
    o.gap_aln = gap_aln
    return o


def _same_case(oracle, b, k, name, gap_aln=1):
    case = vc.cases()[name]
    exp, ids = _expected(oracle, name, gap_aln)
    same_vars(exp, b.region_vars(k, case["beg"], case["chunk_ref"], case["chunk_ref_beg"]), ids)


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_vars_planted_case(lcd, oracle, name):
    """one case, one batch, with the gap side the case asks for: every field and row_read_ids as the oracle has them"""
    case = vc.cases()[name]
    b = lcd.RegionBatch(_case_opt(lcd, 1, case["gap_aln"]))
    b.add_region(case["region"])
    b.upload(); b.run(); b.download()
    _same_case(oracle, b, 0, name, case["gap_aln"])
    b.close()


def test_vars_planted_cases_share_launches(lcd, oracle):
    """every case in one batch (many scan and profile jobs per launch, packed work buffers; the one-consensus and the no-variant regions sit between the
    others), then the same cases dealt over two batches of one lcd_batch_run_many, once with collect_noisy_vars == 1 and once with == 2 (strings left in
    HBM): each region's result is what the region gives alone.  The batches of one joint submission share their options (lcd_batch_run_many checks it before
    anything is launched), so a pair with 1 and 2 mixed is refused and the two modes take one submission each."""
    from longcalld_amd._lib import LcdError
    names = list(vc.CASE_NAMES)
    b = lcd.RegionBatch(_case_opt(lcd, 1))
    for name in names:
        b.add_region(vc.cases()[name]["region"])
    b.upload(); b.run(); b.download()
    for k, name in enumerate(names):
        _same_case(oracle, b, k, name)
    b.close()
    halves = [names[0::2], names[1::2]]

    def pair(modes):
        bs = []
        for mode, part in zip(modes, halves):
            b = lcd.RegionBatch(_case_opt(lcd, mode))
            for name in part:
                b.add_region(vc.cases()[name]["region"])
            b.upload(); bs.append(b)
        return bs

    for mode in (1, 2):
        bs = pair((mode, mode))
        lcd.RegionBatch.run_many(bs)
        for b in bs:
            b.download()
        for b, part in zip(bs, halves):
            for k, name in enumerate(part):
                _same_case(oracle, b, k, name)
        for b in reversed(bs):
            b.close()
    bs = pair((1, 2))
    with pytest.raises(LcdError, match="different options"):
        lcd.RegionBatch.run_many(bs)
    for b in reversed(bs):
        b.close()
