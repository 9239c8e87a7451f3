"""lcd_chunks_first_round on the MI355X: the head of collect_var_main (src/collect_var.c:2897-2945) for several device chunks in one call -- is_skipped, the
low-complexity intervals of the region window (src/bam_utils.c:1573-1581), pre_process_noisy_regs from the chunk handles with one batched read-support launch,
the clean-region variants and the first K5 call -- against the chain of existing oracles (the reference's own sdust / cgranges where oracle/_ref is built, the C
oracle of the first round, the K5 oracle) and against the same chain stepped through the library's single exports."""
import numpy as np
import pytest

import clean_vars_common as cc
import pass_plan_common as pc
from call_chunks_common import first_round_chain as chain, low_comp_of
from test_gpu_clean_vars import device_chunk

pytestmark = pytest.mark.gpu


def same_first_round(got, want, state_keys=None):
    assert got["is_skipped"].tolist() == want["is_skipped"].tolist()
    assert got["low_comp"].tolist() == want["low_comp"].tolist()
    assert got["pre_regs"].tolist() == want["pre_regs"].tolist()
    cc.same_clean_vars(got["cv"], want["cv"])
    assert got["cv"]["alt_ref_base"].tolist() == [4] * got["cv"]["n_vars"]
    pc.same_state(got["state"], want["state"], state_keys)


def item_of(ch, ordered=None):
    return dict(ref=ch["ref"], ref_beg=ch["ref_beg"], reg_beg=ch["reg_beg"], reg_end=ch["reg_end"], is_ont=ch.get("is_ont", 0),
                ordered_read_ids=np.arange(len(ch["reads"]), dtype=np.int32) if ordered is None else ordered, is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8))


def need_ref(oracle):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")


def test_three_chunks_in_one_call_equal_the_oracle_chain_the_stepped_chain_and_single_calls(lcd, oracle):
    need_ref(oracle)
    chs = [cc.make_diploid_chunk(seed, ref_len=12000) for seed in (3, 17, 29)]
    digs = [cc.read_digars(ch, oracle) for ch in chs]
    rng = np.random.default_rng(1)
    # the second chunk in an order of its own: the order reaches pre_process_noisy_regs (cr_add order), the pile-up and K5
    orders = [np.arange(len(ch["reads"]), dtype=np.int32) for ch in chs]
    orders[1] = rng.permutation(len(chs[1]["reads"])).astype(np.int32)
    devs = [device_chunk(lcd, ch) for ch in chs]
    before = lcd.copy_counters()
    got = lcd.chunks_first_round(devs, [item_of(ch, o) for ch, o in zip(chs, orders)])
    after = lcd.copy_counters()
    assert after[0] == before[0] and after[1] == before[1]                       # no digar crossed PCIe, either way
    n_regs = 0
    for ch, dg, o, dev, g in zip(chs, digs, orders, devs, got):
        assert g["ordered_read_ids"].tolist() == o.tolist()
        same_first_round(g, chain(lcd, oracle, ch, dg, o), pc.STATE_KEYS)
        same_first_round(g, chain(lcd, oracle, ch, dg, o, dev))
        same_first_round(g, lcd.chunks_first_round([dev], [item_of(ch, o)])[0])
        assert g["cv"]["n_vars"] > 5 and len(g["low_comp"]) > 0
        n_regs += len(g["pre_regs"])
    assert n_regs > 0 and any((g["state"]["haps"] > 0).any() for g in got)
    for d in devs:
        d.close()


def test_real_hg002_chunk_equals_the_oracle_chain(lcd, oracle):
    need_ref(oracle)
    ch = cc.events_chunk()
    digs = cc.read_digars(ch, oracle)
    o = np.arange(len(ch["reads"]), dtype=np.int32)
    dev = device_chunk(lcd, ch)
    got = lcd.chunks_first_round([dev], [item_of(ch)])[0]
    same_first_round(got, chain(lcd, oracle, ch, digs, o), pc.STATE_KEYS)
    same_first_round(got, chain(lcd, oracle, ch, digs, o, dev))
    assert got["is_skipped"].sum() == sum(d["rc"] != 0 for d in digs) and len(got["pre_regs"]) > 10 and got["cv"]["n_vars"] > 100
    dev.close()


def flat_chunk(n_reads=6, ref_len=4000):
    """every read equals the reference: no variant, no noisy window"""
    rng = np.random.default_rng(8)
    ref = rng.integers(0, 4, ref_len).astype(np.uint8)
    reads = []
    for i in range(n_reads):
        p, ln = 100 + 300 * i, 1500
        seq = ref[p:p + ln].copy()
        reads.append(cc.record(p, [(7, ln)], seq, np.full(ln, 30, np.uint8), is_rev=i & 1))
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=50, reg_end=ref_len - 50, whole_ref_len=ref_len, is_ont=0)


def test_chunk_identical_to_the_reference_comes_back_empty_with_the_initial_state(lcd, oracle):
    ch = flat_chunk()
    dev = device_chunk(lcd, ch)
    got = lcd.chunks_first_round([dev], [item_of(ch)])[0]
    R = len(ch["reads"])
    assert got["cv"]["n_vars"] == 0 and len(got["pre_regs"]) == 0 and len(got["cv"]["regs"]) == 0 and got["is_skipped"].tolist() == [0] * R
    pc.same_state(got["state"], pc.fresh_state(R, 0))
    assert got["low_comp"].tolist() == low_comp_of(lcd.sdust, ch).tolist()
    dev.close()


def test_regions_without_a_clean_variant_keep_the_initial_state(lcd, oracle):
    """a cluster of mismatches in every read makes a noisy region and nothing else: 0 variants, >= 1 region, no K5 call"""
    need_ref(oracle)
    ch = flat_chunk()
    for r in ch["reads"][:5]:
        ops, seq, at = [], r["seq"].copy(), 1200 - r["pos0"]
        if at < 10 or at + 40 > len(seq):
            continue
        pos = list(range(at, at + 40, 4))                                   # ten mismatches within 40 bases, the same sites in every read that spans them
        last = 0
        for p in pos:
            ops += [(7, p - last), (8, 1)]; seq[p] = (seq[p] + 1) & 3; last = p + 1
        ops.append((7, len(seq) - last))
        r.update(cc.record(r["pos0"], ops, seq, r["qual"], is_rev=r["is_rev"]))
    digs = cc.read_digars(ch, oracle)
    dev = device_chunk(lcd, ch)
    o = np.arange(len(ch["reads"]), dtype=np.int32)
    got = lcd.chunks_first_round([dev], [item_of(ch)])[0]
    want = chain(lcd, oracle, ch, digs, o)
    same_first_round(got, want)
    assert got["cv"]["n_vars"] == 0 and len(got["pre_regs"]) >= 1 and len(got["cv"]["regs"]) >= 1
    pc.same_state(got["state"], pc.fresh_state(len(ch["reads"]), 0))
    dev.close()


def test_chunk_without_reads_is_legal(lcd, tmp_path):
    import call_chunks_common as kc
    path = str(tmp_path / "e.bam")
    kc.write_aux_bam(path, kc.nm_records())
    empty = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", 50000, 60000, min_mapq=30)
    full = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", 1, 5000, min_mapq=30)
    assert empty.n == 0 and full.n == 16
    ref = np.zeros(12000, np.uint8)
    got = lcd.chunks_first_round([empty, full], [dict(ref=ref, ref_beg=49001, reg_beg=50000, reg_end=60000), dict(ref=ref[:6000], ref_beg=1, reg_beg=1, reg_end=5000)])
    e = got[0]
    assert e["cv"]["n_vars"] == 0 and e["cv"]["n_reads"] == 0 and len(e["pre_regs"]) == 0 and len(e["ordered_read_ids"]) == 0 and len(e["state"]["haps"]) == 0
    assert len(e["low_comp"]) >= 1                                              # 10 kb of one base is low-complexity
    assert got[1]["cv"]["n_reads"] == 16
    empty.close(); full.close()


def test_malformed_input_is_refused_before_any_launch(lcd):
    ch = flat_chunk()
    dev = device_chunk(lcd, ch)
    bad_order = np.arange(len(ch["reads"]), dtype=np.int32); bad_order[2] = len(ch["reads"])
    twice = np.arange(len(ch["reads"]), dtype=np.int32); twice[3] = 0
    for it in (item_of(ch, bad_order), item_of(ch, twice), dict(item_of(ch), ref_end=0), dict(item_of(ch), reg_beg=0), dict(item_of(ch), reg_end=ch["reg_beg"] - 1)):
        before = lcd.copy_counters()
        with pytest.raises(lcd.LcdError, match="-4"):
            lcd.chunks_first_round([dev], [it])
        assert lcd.copy_counters() == before
    with pytest.raises(lcd.LcdError, match="-4"):
        lcd.chunks_first_round([dev, None], [item_of(ch), item_of(ch)])
    with pytest.raises(lcd.LcdError, match="-2"):
        lcd.chunks_first_round([dev], [item_of(ch)], opt=lcd.clean_opt(0, out_somatic=1))
    assert lcd.chunks_first_round([], []) == []
    dev.close()
