"""Branches of a joint submission (lcd_batch_run_many) that the digest tests of test_gpu_region.py do not reach: where the short stages run (side by side
or one after the other), host retries whose bookkeeping spans several batches, and the retry policy the submission shares with lcd_poa_batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SETS = {}


def _sets(shape, seeds, n):
    """the batches' regions, made once per module"""
    from longcalld_amd import jobs
    key = (shape, tuple(seeds), n)
    if key not in _SETS:
        _SETS[key] = [jobs.make_regions(s, n, jobs.HIFI if shape == "hifi" else jobs.ONT) for s in seeds]
    return _SETS[key]


def _opt(lcd, shape):
    o = lcd.default_opt(); o.is_ont = 0 if shape == "hifi" else 1
    return o


def _submit(lcd, sets, opt, joint=True):
    """one joint submission of the batches (or every batch on its own) -> digests, statistics"""
    bs = []
    for regs in sets:
        b = lcd.RegionBatch(opt)
        for r in regs:
            b.add_region(r)
        b.upload()
        bs.append(b)
    if joint:
        lcd.RegionBatch.run_many(bs)
    else:
        for b in bs:
            b.run(); b.download()
    for b in bs:          # (the ref<->cons rows live in the leader's buffers: everything is downloaded before a batch is closed)
        b.download()
    out = [b.digest() for b in bs], [b.stats() for b in bs]
    for b in bs:
        b.close()
    return out


@pytest.mark.parametrize("shape,n", [("hifi", 150), ("ont", 60)])
def test_stage_placement_switches_keep_the_digests(lcd, monkeypatch, shape, n):
    """K4 beside K3 in the anchor stage, the strings stage beside the ref<->cons WFA stage and the WFA classes over the side streams are placements only:
    each of LCD_ANCHOR_SEQ / LCD_STRINGS_SEQ / LCD_WFA_SEQ, and all three, leave every batch's digest as it is"""
    sets, opt = _sets(shape, (51, 52), n), _opt(lcd, shape)
    d_ref, st = _submit(lcd, sets, opt)
    assert all(d != 0 for d in d_ref)
    for s in st:    # the anchor stage really has K4 and K3 jobs, the WFA stage more than one job per region: side by side against sequential is a real difference
        assert s["n_anchor_jobs"] > 0 and s["n_edlib_jobs"] > 0 and s["n_wfa_jobs"] > s["n_regions_resolved"] > 0
    switches = ["LCD_STRINGS_SEQ", "LCD_ANCHOR_SEQ", "LCD_WFA_SEQ"]
    for on in [[s] for s in switches] + [switches]:
        with monkeypatch.context() as m:
            for s in on:
                m.setenv(s, "1")
            d, _ = _submit(lcd, sets, opt)
        assert d == d_ref, on


@pytest.mark.parametrize("shape,n", [("hifi", 60), ("ont", 24)])
def test_joint_host_retries_over_several_batches(lcd, monkeypatch, shape, n):
    """DP regions far too small and no spare pool: chains of BOTH batches of a joint submission come back and are re-run by the host, some with a larger graph
    and a fresh output block of their batch -- the digests are those of each batch alone and of the unshrunk run"""
    sets, opt = _sets(shape, (40, 41), n), _opt(lcd, shape)
    d_ref, _ = _submit(lcd, sets, opt)
    monkeypatch.setenv("LCD_CELL_SHRINK", "24")
    monkeypatch.setenv("LCD_SPARE_GB", "0")
    d_joint, st = _submit(lcd, sets, opt)
    d_alone, _ = _submit(lcd, sets, opt, joint=False)
    assert all(d != 0 for d in d_ref)
    assert d_joint == d_alone == d_ref
    for s in st:
        assert s["poa_retries"] > 0 and s["poa_grown"] == 0


@pytest.mark.parametrize("shape,n", [("hifi", 60), ("ont", 24)])
def test_retry_policy_is_the_same_through_lcd_poa_batch(lcd, monkeypatch, shape, n):
    """the K2 chains of a batch (regions without a phase set: every full-cover read, in the region's sorted order) through lcd_poa_batch and through the region
    batch, both with DP regions far too small and no spare pool: the same consensus sequences and clusters per chain"""
    from longcalld_amd import jobs
    regs, opt = _sets(shape, (40, 41), n)[0], _opt(lcd, shape)
    monkeypatch.setenv("LCD_CELL_SHRINK", "24")
    monkeypatch.setenv("LCD_SPARE_GB", "0")
    b = lcd.RegionBatch(opt)
    for r in regs:
        b.add_region(r)
    b.upload(); b.run(); b.download()
    assert b.stats()["poa_retries"] > 0
    chains, where = [], []
    for i, r in enumerate(regs):
        if (np.asarray(r["haps"]) != 0).any():
            continue
        ids = list(r["read_ids"])
        members = [int(rid) for rid in b.sorted_ids(i) if r["covers"][ids.index(rid)] == jobs.BOTH and len(r["seqs"][ids.index(rid)]) > 0]
        if len(members) < opt.min_dp:
            continue
        chains.append(dict(mode=1, reads=[r["seqs"][ids.index(rid)] for rid in members]))
        where.append((i, members))
    assert len(chains) >= 3
    got = lcd.poa_batch(chains, opt)
    n_cons = 0
    for g, (i, members) in zip(got, where):
        res = b.result(i)
        assert g["status"] == 0 and g["n_cons"] == res["n_cons"]
        for c in range(g["n_cons"]):
            rc = res["aln_strs"][c][0]
            assert (g["cons"][c] == rc["query"][rc["query"] != 5]).all() and len(g["cons"][c]) == int((rc["query"] != 5).sum())
            assert [members[k] for k in g["clu"][c]] == list(res["clu_read_ids"][c])
            n_cons += 1
    b.close()
    assert n_cons > 0
