"""Are the S6 GPU cases aimed correctly?  Every case of tests/vars_cases.py is run through the oracle (collect_noisy_reg_aln_strs, then oracle/cand_vars.c) and
must reach the conditions it names; every condition of the table must be reached by some case.  No GPU needed: this file says what the planted-variant tests
of tests/test_gpu_vars.py exercise."""
import functools

import numpy as np
import pytest

import vars_cases as vc


@functools.lru_cache(maxsize=None)
def _seen(oracle, name):
    case = vc.cases()[name]
    return vc.Seen(case, *vc.through_oracle(oracle, case))


def test_table_is_consistent():
    assert set(vc.cases()) == set(vc.CASE_NAMES)
    named = {w for c in vc.cases().values() for w in c["want"]}
    assert named == set(vc.CONDITIONS), set(vc.CONDITIONS) ^ named


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_case_reaches_its_conditions(oracle, name):
    s = _seen(oracle, name)
    missed = [w for w in s.case["want"] if not vc.CONDITIONS[w](s)]
    assert not missed, (name, missed)


def test_every_condition_is_reached(oracle):
    reached = {w for name in vc.CASE_NAMES for w in vc.cases()[name]["want"] if vc.CONDITIONS[w](_seen(oracle, name))}
    assert reached == set(vc.CONDITIONS), set(vc.CONDITIONS) - reached


def test_consensus_is_the_planted_haplotype(oracle):
    """tagged cases: cluster c holds exactly the reads tagged c + 1, in the sorted order the region driver leaves them, and the strings de-gap to the inputs"""
    from conftest import check_invariants
    for name, case in vc.cases().items():
        reg = case["region"]
        res, exp = vc.through_oracle(oracle, case)
        assert res["n_cons"] == (1 if name == "one_consensus" else 2), name
        assert check_invariants(reg, res) == len(reg["seqs"])
        assert exp["n_rows"] == len(reg["seqs"])
        if reg["haps"].any():
            for c in range(2):
                assert set(res["clu_read_ids"][c].tolist()) == set(reg["read_ids"][reg["haps"] == c + 1].tolist())


def test_columns_restate_the_variant_starts(oracle):
    """the column walk of vars_cases.runs and the oracle's variant list agree: per consensus the same (offset, type, lengths) in the same order"""
    for name in vc.CASE_NAMES:
        s = _seen(oracle, name)
        for c in range(s.n_cons):
            mine = [(v["off"], v["type"], v["ref_len"] if v["type"] != vc.INS else v["alt_len"]) for v in s.v if s.n_cons == 1 or v["src"] & (c + 1)]
            walk = [(r["ref_off"], {1: vc.SNP, 2: vc.INS, 3: vc.DEL}[r["cls"]], r["end"] - r["col"] + 1) for r in s.starts[c]]
            assert sorted(mine) == sorted(walk), (name, c)


def test_partial_reads_have_short_rows(oracle):
    """runs_over_step: the two reads that stop or start inside the insertion and the one that stops inside the other haplotype's deletion have -1 cells and
    a span shorter than the variant list; every full read spans all variants"""
    s = _seen(oracle, "runs_over_step")
    reg = s.case["region"]
    ids = np.concatenate([s.res["clu_read_ids"][c] for c in range(2)])
    partial = np.isin(ids, reg["read_ids"][reg["covers"] != vc.BOTH])
    assert partial.sum() == 3
    span = s.exp["prof_end"] - s.exp["prof_start"] + 1
    assert (span[~partial] == s.n).all() and (span[partial] < s.n).all()
    assert ((s.exp["prof_alleles"][partial] == -1).sum(1) >= 1).all() and (s.exp["prof_alleles"][~partial] >= 0).all()
