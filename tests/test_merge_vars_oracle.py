"""lcd_merge_region_vars without a device: the pure-Python oracle (tests/merge_vars_common.py) on hand-built cases whose results are written out,
its independence of the region order for comparator-sorted distinct lists, lcd_sort_noisy_regs (host code) through the library, and the argument
checks of lcd_merge_region_vars, which return before anything touches a device."""
import numpy as np
import pytest

import merge_vars_common as mc


@pytest.mark.parametrize("name", sorted(mc.hand_cases()))
def test_oracle_on_hand_built_cases(name):
    cv, regions, ordered, skipped, exp = mc.hand_cases()[name]
    mc.check_expected(mc.oracle_merge(cv, regions, ordered, skipped), exp)


def test_hand_built_region_list_is_out_of_comparator_order():
    reg = mc.hand_cases()["out_of_comparator_order"][1][0]
    keys = [mc.var_key(reg["pos"][j], reg["var_type"][j], reg["ref_len"][j], reg["alt_len"][j], reg["alt_seqs"][j]) for j in range(2)]
    assert keys[0] > keys[1] and keys[0][0] == keys[1][0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_region_order_does_not_matter_for_sorted_distinct_lists(seed):
    cv, regions, ordered, skipped = mc.make_case(seed, n_reads=40, n_vars=25, n_regions=5, span=6, p_tie=0.0, sorted_regions=True)
    # pairwise distinct across the regions and against the current table: nothing is dropped, so no cell competes with another one
    seen = {mc.var_key(cv["pos"][i], cv["var_type"][i], cv["ref_len"][i], cv["alt_len"][i], mc._alts(cv)[i]) for i in range(cv["n_vars"])}
    kept = []
    for g in regions:
        ks = [mc.var_key(g["pos"][j], g["var_type"][j], g["ref_len"][j], g["alt_len"][j], g["alt_seqs"][j]) for j in range(g["n_vars"])]
        if not seen.intersection(ks):
            seen.update(ks); kept.append(g)
    assert len(kept) >= 3
    base, _, base_maps = mc.oracle_merge(cv, kept, ordered, skipped)
    perm = np.random.default_rng(seed).permutation(len(kept))
    other, _, maps = mc.oracle_merge(cv, [kept[i] for i in perm], ordered, skipped)
    for k in mc.FIELDS:
        assert np.array_equal(np.asarray(base[k]), np.asarray(other[k])), k
    for at, i in enumerate(perm):
        assert np.array_equal(maps[at], base_maps[i])


def test_sort_noisy_regs_is_the_exchange_sort(lcd):
    # labels (2, 2, 1), equal lengths: i = 0 meets j = 2 and swaps -> (2, 1, 0); a stable sort would give (2, 0, 1)
    regs = [(100, 150, 2), (300, 350, 2), (500, 550, 1)]
    assert list(lcd.sort_noisy_regs(regs)) == [2, 1, 0]
    # by label first, then by end - start
    assert list(lcd.sort_noisy_regs([(0, 90, 3), (0, 50, 3), (0, 70, 1), (0, 10, 5)])) == [2, 1, 0, 3]
    assert list(lcd.sort_noisy_regs([])) == []


def _case():
    cv, ordered, sk = mc.make_cv([mc.X(100, 0), mc.X(110, 1)], [(0, [1, 0]), None])
    return cv, ordered, sk


@pytest.mark.parametrize("rows, what", [
    ([(2, 0, 0, [1])], "read id"), ([(-1, 0, 0, [1])], "read id"),        # a row read id outside [0, n_reads)
    ([(0, 0, 1, [1])], "span"),                                              # a span outside [0, n_vars)
    ([(1, 0, 0, [1]), (1, 0, 0, [0])], "twice"),                             # a read twice in one region
])
def test_malformed_regions_are_refused(lcd, rows, what):
    from longcalld_amd._lib import LcdError
    cv, ordered, sk = _case()
    with pytest.raises(LcdError, match=what):
        lcd.merge_region_vars(cv, [mc.make_reg([mc.X(105, 2)], rows)], ordered, sk)


def test_negative_region_count_is_refused(lcd):
    from longcalld_amd._lib import LcdError
    cv, ordered, sk = _case()
    with pytest.raises(LcdError, match="n_regions"):
        lcd.merge_region_vars(cv, [], ordered, sk, n_regions=-1)


def test_exports_and_struct_layout(lcd):
    import ctypes as C
    from longcalld_amd import _lib
    assert {"lcd_merge_region_vars", "lcd_merge_region_vars_batch", "lcd_sort_noisy_regs"} <= set(_lib.EXPORTS)
    assert C.sizeof(_lib.LcdRegionVars) == 56
