"""Conditions on the plain-row chains of tests/plain_row_cases.py, checked without a GPU: the planner's probe puts every case in the 64-thread class with the
window its table row names (so the chain runs in the single-wavefront rows, one cell per lane first), the oracle's MSA is longer than 128 columns (the graph spans
more than two 64-row plan windows), and the reads are what the table says they are.  The kernel's parity on the same chains is tests/test_gpu_plain_rows.py."""
import os

import pytest

import chain_plan_cases as P
import plain_row_cases as R

_IDS = [c["name"] for c in R.CASES]


@pytest.fixture(scope="module")
def plan_lib():
    from longcalld_amd import _lib
    return P.open_lib(_lib.LIB_PATH)


def _probe(plan_lib, monkeypatch, case, env):
    for k in [k for k in os.environ if k.startswith("LCD_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert not any(k in P.PROCESS_SWITCHES for k in env)
    return dict(zip(P.CHAIN_OUT, P.probe(plan_lib, R.plan_case(case, env))))


@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_plain_row_case_lands_in_the_single_wavefront_class(plan_lib, case, monkeypatch):
    """under the row's environment and under each further one (the switches are read per call)"""
    for env in [case["env"]] + [dict(case["env"], **e) for e in case["also"]]:
        got = _probe(plan_lib, monkeypatch, case, env)
        assert got["threads"] == 64
        assert {k: got[k] for k in case["planned"]} == case["planned"], (case["name"], env, max(len(r) for r in R.case_reads(case)))


@pytest.mark.parametrize("case", R.CASES, ids=_IDS)
def test_plain_row_case_spans_more_than_two_plan_windows(oracle, case):
    exp = R.case_oracle(case)
    assert exp["n_cons"] == 1 and exp["msa_len"] > 128, (case["name"], exp["msa_len"])
    assert all(130 <= len(r) <= 200 for r in R.case_reads(case))


def test_shrunk_regions_run_out_inside_the_second_plan_window(plan_lib, monkeypatch):
    """LCD_CELL_SHRINK as the table sets it: the code region holds the rows of the first plan window (64 rows of at most 64 code bytes would not fit, but rows of
    this band do: the planner's own figure for a K1 band is w = 10 + length / 100 = 11, 2 w + 1 = 23 columns, padded to 24 or 28 bytes) and not the read (at
    least 24 bytes for each of its rows away from the ends), and a region eight times as large -- the next size a chain is given -- holds every read of the
    chain at 64 bytes a row"""
    for case in R.CASES:
        for e in case["also"]:
            assert e == R.SHRINK
            full = _probe(plan_lib, monkeypatch, case, case["env"])["cell_cap"]
            cap = _probe(plan_lib, monkeypatch, case, dict(case["env"], **e))["cell_cap"]
            rows = min(len(r) for r in R.case_reads(case))
            assert 64 * 28 < cap < 24 * (rows - 24) and cap < full, (case["name"], cap, full)
            assert 8 * cap > 64 * (max(len(r) for r in R.case_reads(case)) + 2), (case["name"], cap)


def test_plain_row_reads_are_what_the_table_says():
    h = R.case_reads(R.CASES[0])[0]
    assert len(h) == R.L and (h[1:] != h[:-1]).all()
    assert all((r == h).all() for r in R.READS["identical"]())
    assert sorted(len(r) for r in R.READS["indel12"]()) == [R.L - 12] + [R.L] * 4 + [R.L + 12]
    snps = R.READS["snps"]()
    assert [int((r != h).sum()) for r in snps] == [0, 1, 1, 1, 1, 1] and len({int((r != h).argmax()) for r in snps[1:]}) == 5
    ins = R.READS["ins40"]()
    assert sorted(len(r) for r in ins) == [150] * 5 + [190]
    assert {c["reads"] for c in R.CASES if c["also"]} == {"identical", "snps"} and {c["mode"] for c in R.CASES} == {0, 1}
