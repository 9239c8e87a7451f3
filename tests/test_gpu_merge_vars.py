"""lcd_merge_region_vars on the device against the pure-Python oracle (tests/merge_vars_common.py): every field of the result and both maps, on the hand-built
cases, on seeded shapes sized to the kernels' paths, and a batch of 8 different chunks against 8 single calls."""
import pytest

import merge_vars_common as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(mc.hand_cases()))
def test_hand_built_cases(lcd, name):
    cv, regions, ordered, skipped, exp = mc.hand_cases()[name]
    got = lcd.merge_region_vars(cv, regions, ordered, skipped)
    mc.check_expected(got, exp)
    mc.same_merge(got, mc.oracle_merge(cv, regions, ordered, skipped))


@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_seeded_shapes(lcd, shape):
    cv, regions, ordered, skipped = mc.make_case(**mc.SHAPES[shape])
    want = mc.oracle_merge(cv, regions, ordered, skipped)
    got = lcd.merge_region_vars(cv, regions, ordered, skipped)
    mc.same_merge(got, want)
    assert got[0]["n_vars"] > cv["n_vars"] and any((m < 0).any() for m in got[2])
    if shape == "B":
        assert int(got[0]["allele_off"][-1]) > 8000 and cv["n_reads"] > 256     # the offset scan crossed a workgroup boundary
    if shape == "C":
        assert sum(1 for m in got[2] if len(m) and (m < 0).all()) >= 3           # regions whose rows lose every cell


def test_result_feeds_the_k5_view(lcd):
    cv, regions, ordered, skipped = mc.make_case(**mc.SHAPES["A"])
    st, _, _ = lcd.merge_region_vars(cv, regions, ordered, skipped)
    prob = lcd.clean_vars_hap_problem(st, ordered, skipped)
    assert prob["n_vars"] == st["n_vars"] and (prob["alleles"] == st["alleles"]).all() and (prob["cr_read"] == st["cr_read"]).all()
    assert (prob["allele_off"] == st["allele_off"].astype("int32")).all() and (prob["var_cate"] == st["cate"]).all()


def test_batch_of_8_chunks_equals_8_single_calls(lcd):
    cases = [mc.make_case(seed=100 + i, n_reads=40 + 37 * i, n_vars=(0 if i == 3 else 20 + 9 * i), n_regions=2 + i, span=5 + 3 * i, p_profile=0.5 + 0.06 * i)
             for i in range(8)]
    got = lcd.merge_region_vars_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    assert len(got) == 8
    for c, g in zip(cases, got):
        mc.same_merge(g, lcd.merge_region_vars(*c))
        mc.same_merge(g, mc.oracle_merge(*c))
