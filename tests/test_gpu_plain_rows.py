"""Parity of the POA chain kernel with the oracle on chains made for the PLAIN rows of the single-wavefront rows (tests/plain_row_cases.py).

Every row of CASES runs through lcd.poa_batch under its environment and under each of its further environments, and EVERY run is compared with the oracle: status,
n_cons, msa_len, every consensus, every cluster, every MSA row byte for byte.  The same job then runs under LCD_DBG=8 on top of that environment (the generic
rows instead of the lean ones) and must give the same bytes again.  tests/test_plain_row_cases_oracle.py checks on the CPU that the chains land in the class
their table row names and that their graphs span more than two plan windows."""
import pytest

import plain_row_cases as R

pytestmark = pytest.mark.gpu


def _same(got, exp, what):
    assert got["status"] == 0, what
    assert got["n_cons"] == exp["n_cons"] and got["msa_len"] == exp["msa_len"], (what, got["n_cons"], exp["n_cons"], got["msa_len"], exp["msa_len"])
    for c in range(exp["n_cons"]):
        assert len(got["cons"][c]) == len(exp["cons"][c]) and (got["cons"][c] == exp["cons"][c]).all(), (what, "consensus", c)
        assert len(got["clu"][c]) == len(exp["clu"][c]) and (got["clu"][c] == exp["clu"][c]).all(), (what, "cluster", c)
    assert len(got["msa"]) == len(exp["msa"]), what
    for r, (a, b) in enumerate(zip(got["msa"], exp["msa"])):
        assert (a == b).all(), (what, "msa row", r)


def _run(lcd, monkeypatch, job, opt, env):
    with monkeypatch.context() as m:
        for k in R.SWITCHES:
            m.delenv(k, raising=False)
        for k, v in env.items():      # (the switches are read at every call)
            m.setenv(k, v)
        return lcd.poa_batch(job, opt)[0]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_plain_row_chain_matches_oracle_and_generic_rows(lcd, oracle, case, monkeypatch):
    exp = R.case_oracle(case)
    assert exp["n_cons"] == 1
    opt = lcd.default_opt()
    job = [dict(mode=case["mode"], reads=R.case_reads(case))]
    for env in [case["env"]] + [dict(case["env"], **e) for e in case["also"]]:
        got = _run(lcd, monkeypatch, job, opt, env)
        _same(got, exp, (case["name"], env))
        generic = _run(lcd, monkeypatch, job, opt, dict(env, LCD_DBG="8"))
        _same(generic, exp, (case["name"], env, "generic rows"))
        _same(got, generic, (case["name"], env, "lean rows against generic rows"))
