"""lcd_sdust / lcd_sdust_batch (sdust_kernel.hip: one automaton per segment) on sequences in which runs of N are dense: every case of tests/sdust_cases.py
equals the sequential model of tests/sdust_model.py -- and the reference's own sdust() where oracle/_ref is built; tests/test_sdust_cases_oracle.py proves
the two equal on the CPU -- one call per case and all cases of a (T, W) in one launch.  No case is left out of a comparison."""
import numpy as np
import pytest

import sdust_cases as SC
import sdust_model as M
from call_chunks_common import low_comp_of

pytestmark = pytest.mark.gpu


def _arr(seq):
    return np.frombuffer(seq, np.uint8) if isinstance(seq, bytes) else seq


def _pairs(a):
    return [tuple(int(v) for v in x) for x in np.asarray(a).reshape(-1, 2)]


def _diff(name, exp, got):
    return (name, [x for x in exp if x not in got], [x for x in got if x not in exp])


@pytest.mark.parametrize("T,W", SC.PARAMS)
def test_every_case_equals_the_sequential_model(lcd, oracle, T, W):
    cs = SC.by_params()[(T, W)]
    full = SC.full_runs()
    ref = oracle.ref_cgranges() is not None
    bad = []
    single = {}
    for c in cs:
        exp = full[c["name"]][0]
        got = single[c["name"]] = _pairs(lcd.sdust(_arr(c["seq"]), T, W))
        if got != exp:
            bad.append(_diff(c["name"], exp, got))
        if ref:
            assert _pairs(oracle.ref_sdust(_arr(c["seq"]), T, W)) == exp, c["name"]
    # one launch: a sequence with intervals at or past its end directly in front of another sequence of the pool
    past_end = {c["name"] for c in cs if full[c["name"]][1].get("past_end", 0) > 0}
    order = SC.pack_order(cs, past_end)
    if W > 4:
        assert past_end and any(x["name"] in past_end and y["name"] not in past_end for x, y in zip(order, order[1:]))
    got = lcd.sdust_batch([_arr(c["seq"]) for c in order], T, W)
    assert len(got) == len(order)
    for c, g in zip(order, got):
        if _pairs(g) != single[c["name"]] or _pairs(g) != full[c["name"]][0]:
            bad.append(_diff(c["name"] + " (batch)", full[c["name"]][0], _pairs(g)))
    assert not bad, (len(bad), len(cs), bad[:12])


def test_first_round_low_comp_with_dense_n_at_reg_end(lcd):
    """chunk->low_comp_cr as lcd_first_round.cpp fills it: sdust over the bases of [reg_beg, reg_end] only, so an N-dense stretch that straddles reg_end is an
    N-dense END of the sequence the kernel sees"""
    ch = SC.first_round_chunk()
    cen = {}
    model = lambda s, T, W: np.array(M.sdust_full(s, T, W, cen), np.int64).reshape(-1, 2)
    exp = low_comp_of(model, ch)
    assert cen["past_end"] > 0 and cen["displaced"] > 0 and len(exp) >= 4
    assert low_comp_of(lcd.sdust, ch).tolist() == exp.tolist()
