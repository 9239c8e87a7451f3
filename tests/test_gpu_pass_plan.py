"""lcd_chunk_plan_pass / lcd_chunk_plan_pass_batch / lcd_batch_add_planned on the MI355X: the plan of one noisy-region pass computed on the chunk's reads in HBM
(plan_kernel.hip) against literal expectations on a hand-built chunk, against the Python oracle (pass_plan_common.oracle_plan) and DeviceChunk.region_slices on
seeded HiFi / ONT chunks, a batch against single calls, and planned regions against regions added one by one."""
import numpy as np
import pytest

import clean_vars_common as cc
import pass_plan_common as pc
from test_gpu_clean_vars import chunk_args, device_chunk

pytestmark = pytest.mark.gpu

REF_LEN = 8000
A, D, E, F, G, H, L1, L2, C = range(9)
REGS = np.array([[1000, 1100, 1], [3000, 3050, 1], [3500, 3550, 1], [4000, 4050, 1], [5000, 5100, 1], [1000, 1100, 2], [6000, 6300, 1], [6000, 6299, 1], [-20, 50, 1]], np.int64)
DONE = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], np.int32)


def hand_chunk():
    """266 error-free reads: 0-3 around region A's ends, 4 inside A (skipped by the caller), 5-69 (65) over D, 70-133 (64) over E, 134-263 (130) over F,
    264 inside L1 / L2, 265 at the reference's first base"""
    ref = np.random.default_rng(7).integers(0, 4, REF_LEN).astype(np.uint8)
    spans = [(899, 101), (899, 102), (1099, 60), (1100, 60), (1020, 60)] + [(2990, 100)] * 65 + [(3490, 100)] * 64 + [(3990, 100)] * 130 + [(6100, 60), (0, 60)]
    reads = [cc.record(p, [(7, l)], ref[p:p + l], np.full(l, 30, np.uint8)) for p, l in spans]
    ch = dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=REF_LEN, whole_ref_len=REF_LEN, is_ont=0)
    skipped = np.zeros(len(reads), np.uint8); skipped[4] = 1
    return ch, np.arange(len(reads) - 1, -1, -1).astype(np.int32), skipped          # ordered_read_ids: the reverse, so the output has to follow it


def _lists(plan):
    return [plan["read_ids"][plan["read_off"][i]:plan["read_off"][i + 1]].tolist() for i in range(len(plan["status"]))]


def _same_slices(dev, plan, flank=10):
    pr, pb, pe = pc.plan_pairs(plan)
    rb, re_, cv = dev.region_slices(pr, pb, pe, flank)
    assert (plan["read_beg"] == rb).all() and (plan["read_end"] == re_).all() and (plan["cover"] == cv).all()


def test_hand_built_chunk_plan_equals_literal_expectations(lcd):
    ch, ordered, skipped = hand_chunk()
    dev = device_chunk(lcd, ch)
    info = dev.read_info()
    assert (info["status"] == 0).all() and info["beg"][:4].tolist() == [900, 900, 1100, 1101] and info["end"][:4].tolist() == [1000, 1001, 1159, 1160]
    before = lcd.copy_counters()
    p = lcd.plan_pass(dev, REGS, DONE, ordered, skipped, 1, REF_LEN, lcd.pass_opt(max_noisy_reg_len=300, max_noisy_reg_cov=64))
    S = pc
    assert p["status"].tolist() == [S.SUBMIT, S.SKIP_DEEP, S.SUBMIT, S.SKIP_DEEP, S.NO_READS, S.DONE_BEFORE, S.SKIP_LONG, S.SUBMIT, S.SUBMIT]
    assert p["beg"].tolist() == [1000, 3000, 3500, 4000, 5000, 1000, 6000, 6000, 1] and p["end"].tolist() == [1100, 3050, 3550, 4050, 5100, 1100, 6300, 6299, 50]
    got = _lists(p)
    # read.end == reg_beg (read 0) is out, read.beg == reg_end (read 2) is in, read.beg == reg_end + 1 (read 3) is out, read 4 is skipped
    assert got[A] == [2, 1]
    assert got[E] == list(range(133, 69, -1)) and got[L2] == [264] and got[C] == [265]
    assert got[D] == got[F] == got[G] == got[H] == got[L1] == []
    assert p["read_off"].tolist() == [0, 2, 2, 66, 66, 66, 66, 66, 67, 68]
    _same_slices(dev, p)
    k = int(p["read_off"][E])          # an error-free read from 3491 over [3500, 3550]: bases 9 .. 59, both ends covered
    assert (p["read_beg"][k], p["read_end"][k], p["cover"][k]) == (9, 59, 12)
    # 65 and 130 reads (two and three 64-lane steps) are submitted once the coverage limit allows them
    p2 = lcd.plan_pass(dev, REGS, DONE, ordered, skipped, 1, REF_LEN, lcd.pass_opt(max_noisy_reg_len=300))
    got2 = _lists(p2)
    assert p2["status"][[D, F]].tolist() == [S.SUBMIT, S.SUBMIT] and got2[D] == list(range(69, 4, -1)) and got2[F] == list(range(263, 133, -1))
    assert got2[A] == [2, 1] and got2[E] == got[E]
    _same_slices(dev, p2)
    # a region clamped at both ends of the reference window; D cut at its right end
    p3 = lcd.plan_pass(dev, [[2950, 3100, 1], [3000, 3050, 1]], [0, 0], ordered, skipped, 3000, 3040)
    assert p3["beg"].tolist() == [3000, 3000] and p3["end"].tolist() == [3040, 3040] and _lists(p3) == [got2[D], got2[D]]
    _same_slices(dev, p3)
    pc.same_plan(p2, pc.oracle_plan(REGS, DONE, ordered, skipped, info["beg"], info["end"], 1, REF_LEN, max_len=300))
    assert lcd.copy_counters() == before          # no digar and no base crossed PCIe
    from longcalld_amd._lib import LcdError
    bad = ordered.copy(); bad[17] = len(ordered)
    with pytest.raises(LcdError, match=r"outside \[0, n_reads\)"):
        lcd.plan_pass(dev, REGS, DONE, bad, skipped, 1, REF_LEN)
    dev.close()


def _seeded(lcd, oracle, seed, is_ont=0, **kw):
    ch = cc.make_diploid_chunk(seed, is_ont=is_ont, **kw)
    digs = cc.read_digars(ch, oracle, is_ont=is_ont)
    a = chunk_args(lcd, ch, digs)
    dev = device_chunk(lcd, ch)
    cv = dev.clean_vars(**a, opt=lcd.clean_opt(is_ont))
    skipped = np.array([d["rc"] != 0 for d in digs], np.uint8)
    return ch, digs, a, dev, cv, skipped


@pytest.mark.parametrize("seed,is_ont,kw", [(3, 0, {}), (41, 1, dict(depth=40, err=0.004))])
def test_seeded_chunk_plan_equals_the_oracle_and_region_slices(lcd, oracle, seed, is_ont, kw):
    ch, digs, a, dev, cv, skipped = _seeded(lcd, oracle, seed, is_ont, **kw)
    regs = cv["regs"]
    assert len(regs) >= 3
    rng = np.random.default_rng(seed)
    ordered = rng.permutation(len(ch["reads"])).astype(np.int32)
    skipped = skipped | (rng.random(len(skipped)) < 0.1)
    done = (rng.random(len(regs)) < 0.2).astype(np.int32); done[0], done[1] = 1, 0
    rb, re_ = [d["beg"] for d in digs], [d["end"] for d in digs]
    before = lcd.copy_counters()
    seen = set()
    for popt, kwo in ((lcd.pass_opt(), {}), (lcd.pass_opt(max_noisy_reg_len=120, max_noisy_reg_cov=12, noisy_reg_flank_len=3), dict(max_len=120, max_cov=12))):
        p = lcd.plan_pass(dev, regs, done, ordered, skipped, a["ref_beg"], a["ref_end"], popt)
        want = pc.oracle_plan(regs, done, ordered, skipped, rb, re_, a["ref_beg"], a["ref_end"], **kwo)
        pc.same_plan(p, want)
        _same_slices(dev, p, popt.noisy_reg_flank_len)
        seen |= set(want[0].tolist())
    assert {pc.DONE_BEFORE, pc.SUBMIT} <= seen and seen & {pc.SKIP_LONG, pc.SKIP_DEEP}      # the small limits give long / deep regions beside submitted ones
    assert lcd.copy_counters() == before
    dev.close()


def test_batch_of_8_plans_equals_8_single_calls(lcd, oracle):
    made = [_seeded(lcd, oracle, 100 + i, ref_len=15000) for i in range(8)]
    devs = [m[3] for m in made]
    rng = np.random.default_rng(5)
    args = []
    for ch, digs, a, dev, cv, skipped in made:
        n = len(ch["reads"])
        args.append(dict(regs=cv["regs"], done=(rng.random(len(cv["regs"])) < 0.25).astype(np.int32), ordered_read_ids=rng.permutation(n).astype(np.int32),
                         is_skipped=skipped, ref_beg=a["ref_beg"], ref_end=a["ref_end"] - int(rng.integers(0, 3000))))
    popt = lcd.pass_opt(max_noisy_reg_len=400, max_noisy_reg_cov=20)
    batch = lcd.plan_pass_batch(devs, args, popt)
    assert sum(len(b["read_ids"]) for b in batch) > 100
    for dev, a, b in zip(devs, args, batch):
        s = lcd.plan_pass(dev, a["regs"], a["done"], a["ordered_read_ids"], a["is_skipped"], a["ref_beg"], a["ref_end"], popt)
        for k in s:
            assert (s[k] == b[k]).all(), k
    for d in devs:
        d.close()


def test_add_planned_equals_adding_the_regions_one_by_one(lcd, oracle):
    from longcalld_amd import jobs
    ch, digs, a, dev, cv, skipped = _seeded(lcd, oracle, 3)
    n = len(ch["reads"])
    ordered = np.arange(n, dtype=np.int32)
    st = lcd.assign_hap_germline(lcd.clean_vars_hap_problem(cv, ordered, skipped), jobs.GERMLINE_CLEAN)
    plan = lcd.plan_pass(dev, cv["regs"], np.zeros(len(cv["regs"]), np.int32), ordered, skipped, a["ref_beg"], a["ref_end"], lcd.pass_opt(max_noisy_reg_len=1000))
    sub = np.flatnonzero(plan["status"] == pc.SUBMIT)
    assert len(sub) >= 3
    bopt = lcd.default_opt(); bopt.collect_noisy_vars = 1
    b1, b2 = lcd.RegionBatch(bopt), lcd.RegionBatch(bopt)
    idx = b1.add_planned(dev, plan, st["haps"], st["phase_sets"], ch["ref"], ch["ref_beg"])
    assert idx[sub].tolist() == list(range(len(sub))) and (np.delete(idx, sub) == -1).all()
    for i in sub:
        lo, hi = int(plan["read_off"][i]), int(plan["read_off"][i + 1])
        ids = plan["read_ids"][lo:hi]
        beg, end = int(plan["beg"][i]), int(plan["end"][i])
        dev.add_region(b2, beg, end, ids, plan["read_beg"][lo:hi], plan["read_end"][lo:hi], plan["cover"][lo:hi], st["haps"][ids], st["phase_sets"][ids],
                       ch["ref"][beg - ch["ref_beg"]:end - ch["ref_beg"] + 1])
    for b in (b1, b2):
        b.upload(); b.run(); b.download()
    assert b1.digest() == b2.digest()
    n_vars = 0
    for k, i in enumerate(sub):
        x, y = b1.region_vars(k, int(plan["beg"][i]), ch["ref"], ch["ref_beg"]), b2.region_vars(k, int(plan["beg"][i]), ch["ref"], ch["ref_beg"])
        assert b1.n_cons(k) == b2.n_cons(k)
        assert x["n_vars"] == y["n_vars"] and x["n_rows"] == y["n_rows"]
        for f in ("pos", "var_type", "ref_len", "alt_len", "cate", "total_cov", "alle_covs", "row_read_ids", "prof_start", "prof_end", "prof_alleles", "is_homopolymer_indel"):
            assert (np.asarray(x[f]) == np.asarray(y[f])).all(), f
        n_vars += x["n_vars"]
    assert n_vars > 0
    b1.close(); b2.close(); dev.close()
