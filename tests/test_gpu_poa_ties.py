"""Parity of the POA chain kernel with the oracle on TIE-DENSE chains (tests/tie_cases.py), row variant by row variant.

The kernel's direction codes exist to replay the tie decisions of oracle/poa.c's backtrack; reads of iid bases hardly decide any (tests/test_tie_cases_oracle.py
holds the census, and checks on the CPU that every chain here lands in the class its table row names).  Every row of POA_CASES runs through lcd.poa_batch under
its environment and under each of its further environments, and EVERY run is compared with the oracle: status, n_cons, msa_len, every consensus, every cluster,
every MSA row byte for byte."""
import pytest

import tie_cases as T

pytestmark = pytest.mark.gpu

_SWITCHES = sorted({k for c in T.POA_CASES for env in [c["env"]] + c["also"] for k in env})


def _same(got, exp, what):
    assert got["status"] == 0, what
    assert got["n_cons"] == exp["n_cons"] and got["msa_len"] == exp["msa_len"], (what, got["n_cons"], exp["n_cons"], got["msa_len"], exp["msa_len"])
    for c in range(exp["n_cons"]):
        assert len(got["cons"][c]) == len(exp["cons"][c]) and (got["cons"][c] == exp["cons"][c]).all(), (what, "consensus", c)
        assert len(got["clu"][c]) == len(exp["clu"][c]) and (got["clu"][c] == exp["clu"][c]).all(), (what, "cluster", c)
    assert len(got["msa"]) == len(exp["msa"]), what
    for r, (a, b) in enumerate(zip(got["msa"], exp["msa"])):
        assert (a == b).all(), (what, "msa row", r)


@pytest.mark.parametrize("case", T.POA_CASES, ids=[c["name"] for c in T.POA_CASES])
def test_poa_tie_chain_matches_oracle(lcd, oracle, case, monkeypatch):
    exp, census = T.case_oracle(case)
    if case["mode"] == 0:
        assert exp["n_cons"] == 1
    opt = lcd.default_opt()
    for k, v in case["scoring"].items():
        setattr(opt, k, v)
    opt.is_ont = case["is_ont"]
    job = [dict(mode=case["mode"], reads=T.case_reads(case))]
    for env in [case["env"]] + case["also"]:
        with monkeypatch.context() as m:
            for k in _SWITCHES:
                m.delenv(k, raising=False)
            for k, v in env.items():      # (the switches are read at every call)
                m.setenv(k, v)
            got = lcd.poa_batch(job, opt)[0]
        _same(got, exp, (case["name"], env, census))
