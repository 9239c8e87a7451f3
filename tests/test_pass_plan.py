"""Host-side pieces of the noisy-region rounds (no GPU): lcd_hap_state_carry against the rule written out in pass_plan_common.carry, its refusals, and the
argument checks of lcd_chunk_plan_pass / lcd_chunk_plan_pass_batch / lcd_chunks_noisy_rounds, which answer before any device call."""
import numpy as np
import pytest

import pass_plan_common as pc


def _random_state(rng, R, V):
    return dict(haps=rng.integers(0, 3, R).astype(np.int32), phase_sets=rng.integers(-1, 5000, R).astype(np.int64),
                n_clean_agree_snps=rng.integers(0, 40, R).astype(np.int32), n_clean_conflict_snps=rng.integers(0, 9, R).astype(np.int32),
                var_phase_set=rng.integers(-1, 5000, V).astype(np.int64), hap_to_cons_alle=rng.integers(-1, 2, 3 * V).astype(np.int32),
                hap_to_alle_profile=rng.integers(0, 30, 6 * V).astype(np.int32))


@pytest.mark.parametrize("seed,R,V,M", [(1, 40, 25, 25), (2, 7, 12, 30), (3, 0, 5, 9), (4, 13, 0, 6), (5, 64, 100, 164)])
def test_hap_state_carry_equals_the_rule_on_random_maps(lcd, seed, R, V, M):
    rng = np.random.default_rng(seed)
    st = _random_state(rng, R, V)
    c2m = np.sort(rng.choice(M, V, replace=False)).astype(np.int32)      # increasing, as a merge makes it
    got = lcd.hap_state_carry(st, M, c2m)
    pc.same_state(got, pc.carry(st, M, c2m))
    assert len(got["var_phase_set"]) == M and len(got["hap_to_cons_alle"]) == 3 * M and len(got["hap_to_alle_profile"]) == 6 * M


def test_hap_state_carry_with_a_region_variant_in_front_of_index_0(lcd):
    rng = np.random.default_rng(9)
    st = _random_state(rng, 5, 3)
    c2m = np.array([1, 2, 4], np.int32)                                  # merged variants 0 and 3 came from a region
    got = lcd.hap_state_carry(st, 5, c2m)
    pc.same_state(got, pc.carry(st, 5, c2m))
    assert got["var_phase_set"][0] == -1 and got["var_phase_set"][3] == -1 and (got["var_phase_set"][c2m] == st["var_phase_set"]).all()
    assert (got["hap_to_cons_alle"][0:3] == -1).all() and (got["hap_to_cons_alle"][9:12] == -1).all()
    prof = got["hap_to_alle_profile"].reshape(3, 5, 2)
    assert (prof[:, [0, 3], :] == 0).all() and (prof[:, c2m, :] == st["hap_to_alle_profile"].reshape(3, 3, 2)).all()
    for k in ("haps", "phase_sets", "n_clean_agree_snps", "n_clean_conflict_snps"):
        assert (got[k] == st[k]).all()


def test_hap_state_carry_refuses_duplicate_and_out_of_range_targets(lcd):
    from longcalld_amd._lib import LcdError
    st = _random_state(np.random.default_rng(0), 4, 3)
    for bad, word in (([0, 1, 1], "two variants"), ([0, 1, 3], "outside"), ([-1, 1, 2], "outside")):
        with pytest.raises(LcdError, match=word):
            lcd.hap_state_carry(st, 3, np.array(bad, np.int32))
    pc.same_state(lcd.hap_state_carry(st, 3, np.array([0, 1, 2], np.int32)), st)   # the identity map changes nothing


def test_plan_argument_checks_answer_without_a_device(lcd):
    from longcalld_amd._lib import LcdError
    regs = np.array([[100, 200, 1]], np.int64)
    a = dict(regs=regs, done=[0], ordered_read_ids=[], is_skipped=[], ref_beg=1, ref_end=1000)
    with pytest.raises(LcdError, match="n_regs < 0"):
        lcd.plan_pass(None, regs, [0], [], [], 1, 1000, n_regs=-1)
    with pytest.raises(LcdError, match="ref_end < ref_beg"):
        lcd.plan_pass(None, regs, [0], [], [], 1000, 999)
    with pytest.raises(LcdError, match="NULL chunk"):
        lcd.plan_pass(None, regs, [0], [], [], 1, 1000)
    with pytest.raises(LcdError, match="chunk 1: n_regs < 0"):
        lcd.plan_pass_batch([None, None], [a, a], n_regs=[1, -3])
    with pytest.raises(LcdError, match="chunk 1: ref_end < ref_beg"):
        lcd.plan_pass_batch([None, None], [a, dict(a, ref_beg=5, ref_end=4)])
    assert lcd.plan_pass_batch([], []) == []


def test_pass_opt_defaults_match_reference(lcd):
    """src/call_var_main.h:36-42"""
    o = lcd.pass_opt()
    assert (o.max_noisy_reg_len, o.max_noisy_reg_cov, o.noisy_reg_flank_len) == (50000, 1000, 10)


def test_rounds_driver_refuses_somatic_mode_and_bad_counts(lcd):
    import ctypes as C
    from longcalld_amd._lib import LcdRoundsChunk
    lib = lcd.load_library()
    opt = lcd.default_opt(); opt.collect_ref_read_aln_str = 1
    popt = lcd.pass_opt()
    arr = (LcdRoundsChunk * 1)()
    assert lib.lcd_chunks_noisy_rounds(1, arr, C.byref(opt), C.byref(popt)) == -2
    assert b"somatic" in lib.lcd_last_error()
    opt.collect_ref_read_aln_str = 0
    assert lib.lcd_chunks_noisy_rounds(-1, arr, C.byref(opt), C.byref(popt)) == -4
    assert lib.lcd_chunks_noisy_rounds(1, arr, C.byref(opt), C.byref(popt)) == -4      # NULL members
    assert lib.lcd_chunks_noisy_rounds(0, arr, C.byref(opt), C.byref(popt)) == 0


def test_plan_oracle_on_written_out_cases():
    """the Python plan oracle itself on a few literal cases (the boundary tests of the reference's asymmetric overlap test)"""
    rb = [900, 900, 1100, 1101, 1000]; re_ = [1000, 1001, 1200, 1200, 1050]
    st, b, e, lists = pc.oracle_plan([[1000, 1100, 1]], [0], [4, 3, 2, 1, 0], [0, 0, 0, 0, 1], rb, re_, 1, 5000)
    assert st.tolist() == [pc.SUBMIT] and lists == [[2, 1]]
    st, b, e, lists = pc.oracle_plan([[-5, 300, 1], [4000, 9000, 1], [10, 20, 1]], [0, 0, 1], [0], [0], [1], [10], 1, 5000, max_len=1000)
    assert st.tolist() == [pc.SUBMIT, pc.SKIP_LONG, pc.DONE_BEFORE] and b.tolist() == [1, 4000, 10] and e.tolist() == [300, 5000, 20]
    assert pc.sort_noisy_regs([[0, 50, 2], [0, 10, 2], [0, 99, 1]]) == [2, 1, 0]
