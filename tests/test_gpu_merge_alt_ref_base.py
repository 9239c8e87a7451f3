"""cand_var_t.alt_ref_base through the chunk's variant table: 4 for every first-round variant (src/collect_var.c:44), carried by lcd_merge_region_vars for a kept
table entry, taken from the region's variant by make_cand_vars0's rule (:1755-1756: 0 for an X variant, the given base for an insertion / deletion) for a kept
region entry, the table's value where the two are equal -- what make_variants (:1544) writes in front of a gap record's ALT."""
import numpy as np
import pytest

import call_chunks_common as kc
import clean_vars_common as cc
import merge_vars_common as mc

pytestmark = pytest.mark.gpu


def with_arb(reg, values):
    reg = dict(reg)
    reg["alt_ref_base"] = np.array(values, np.int32)
    return reg


def hand_case(table_arb):
    """a table of four variants and two regions: region 0 adds an X (given base 3: the rule makes it 0), an insertion with anchor 2 and repeats the table's
    insertion at 120 with another anchor (equal: dropped); region 1 adds a deletion with anchor 1, a deletion with an unknown anchor and repeats region 0's insertion"""
    cv, o, s = mc.make_cv([mc.X(100, 0), mc.INS(120, [1, 1]), mc.DEL(140, 2), mc.X(160, 3)], [(0, [1, 0, 1, 0]), (1, [1, 1]), None])
    if table_arb is not None:
        cv["alt_ref_base"] = np.array(table_arb, np.uint8)
    r0 = with_arb(mc.make_reg([mc.X(105, 1), mc.INS(110, [2, 2, 2]), mc.INS(120, [1, 1])], [(0, 0, 2, [1, 1, 0]), (2, 0, 1, [0, 1, -1])]), [3, 2, 0])
    r1 = with_arb(mc.make_reg([mc.INS(110, [2, 2, 2]), mc.DEL(130, 4), mc.DEL(150, 1)], [(1, 0, 2, [1, 0, 1])], cate=0x200), [3, 1, 4])
    return cv, [r0, r1], o, s


@pytest.mark.parametrize("single", [True, False])
def test_hand_case_table_and_region_values(lcd, single):
    cv, regions, o, s = hand_case([4, 2, 4, 4])
    f = (lambda *a: lcd.merge_region_vars(*a)) if single else (lambda c, r, oo, ss: lcd.merge_region_vars_batch([c], [r], [oo], [ss])[0])
    st, c2m, r2m = f(cv, regions, o, s)
    mc.same_merge((st, c2m, r2m), mc.oracle_merge({k: v for k, v in cv.items() if k != "alt_ref_base"}, regions, o, s))
    assert st["pos"].tolist() == [100, 105, 110, 120, 130, 140, 150, 160]
    #                             X    X(0)  I(2)  I tab D(1)  D tab D(4)  X
    assert st["alt_ref_base"].tolist() == [4, 0, 2, 2, 1, 4, 4, 4]
    assert r2m[0].tolist() == [1, 2, -1] and r2m[1].tolist() == [-1, 4, 6]      # the equal entries were dropped: the table's 2 at 120 and region 0's 2 at 110 stay
    assert st["alt_ref_base"].tolist() == kc.merged_alt_ref_base(cv, regions, c2m, r2m, st["n_vars"]).tolist()


def test_table_without_the_member_counts_as_all_4(lcd):
    cv, regions, o, s = hand_case(None)
    assert "alt_ref_base" not in cv                                              # the mirror leaves the member NULL
    for got in (lcd.merge_region_vars(cv, regions, o, s), lcd.merge_region_vars_batch([cv], [regions], [o], [s])[0]):
        assert got[0]["alt_ref_base"].tolist() == [4, 0, 2, 4, 1, 4, 4, 4]
    explicit = dict(cv, alt_ref_base=np.full(4, 4, np.uint8))
    assert lcd.merge_region_vars(explicit, regions, o, s)[0]["alt_ref_base"].tolist() == [4, 0, 2, 4, 1, 4, 4, 4]
    none = lcd.merge_region_vars(cv, [], o, s)[0]                                # no region: the table comes back, all 4
    assert none["alt_ref_base"].tolist() == [4, 4, 4, 4]


def test_seeded_batch_with_and_without_the_member(lcd):
    """three seeded chunks in one batch call (one without the member, one with an empty table): the column follows the maps, the batch equals single calls"""
    cases = []
    for i in range(3):
        cv, regions, o, s = mc.make_case(seed=300 + i, n_reads=30 + 20 * i, n_vars=(0 if i == 2 else 15 + 10 * i), n_regions=3 + i, span=6, p_tie=0.4)
        rng = np.random.default_rng(900 + i)
        regions = [with_arb(g, rng.integers(0, 5, max(0, int(g["n_vars"])))) for g in regions]
        if i != 1:
            cv["alt_ref_base"] = rng.integers(0, 5, cv["n_vars"]).astype(np.uint8)
        cases.append((cv, regions, o, s))
    got = lcd.merge_region_vars_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    n_drop = n_ins = 0
    for (cv, regions, o, s), (st, c2m, r2m) in zip(cases, got):
        want = kc.merged_alt_ref_base(cv, regions, c2m, r2m, st["n_vars"])
        assert st["alt_ref_base"].tolist() == want.tolist()
        assert lcd.merge_region_vars(cv, regions, o, s)[0]["alt_ref_base"].tolist() == want.tolist()
        mc.same_merge((st, c2m, r2m), mc.oracle_merge({k: v for k, v in cv.items() if k != "alt_ref_base"}, regions, o, s))
        n_drop += sum(int((m < 0).sum()) for m in r2m)
        n_ins += sum(1 for g, m in zip(regions, r2m) for j in range(len(m)) if m[j] >= 0 and int(g["var_type"][j]) != kc.CDIFF)
    assert n_drop > 0 and n_ins > 0                                              # equal entries and kept gap entries both occurred


def test_first_round_table_is_all_4_and_survives_the_k5_view(lcd, oracle):
    from test_gpu_clean_vars import chunk_args, device_chunk
    ch = cc.make_diploid_chunk(3, ref_len=12000)
    digs = cc.read_digars(ch, oracle)
    a = chunk_args(lcd, ch, digs)
    dev = device_chunk(lcd, ch)
    single = dev.clean_vars(**a, opt=lcd.clean_opt(0))
    batch = lcd.chunk_clean_vars_batch([dev], [a], lcd.clean_opt(0))[0]
    for got in (single, batch):
        assert got["n_vars"] > 5 and got["alt_ref_base"].tolist() == [4] * got["n_vars"]
    cc.same_clean_vars(single, cc.run_oracle(ch, digs, lcd.clean_opt(0), pre_regs=a["pre_regs"], low_comp=a["low_comp"], ordered=a["ordered_read_ids"]))
    dev.close()
