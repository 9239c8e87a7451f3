"""Parity of the WFA and edlib kernels with the oracle / the reference's edlib on TIE-DENSE pairs (tests/tie_cases.py tie_pairs): tandem repeats, indels of exactly
the length at which the two gap pieces cost the same, long tandem-repeat insertions, homopolymer and dinucleotide runs at edlib's word, tile and Hirschberg edges.
tests/test_tie_cases_oracle.py checks on the CPU that left- and right-aligned rows differ on these pairs and that the edlib vectors equal the oracle."""
import json
import os

import numpy as np
import pytest

import tie_cases as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

_WIDE = {"LCD_WFA_LDS_MAX_KB": "0", "LCD_WFA_WIDE_KB": "1", "LCD_WFA_WIDE_MIN": "1"}     # (tests/test_gpu_kernels.py::test_wfa_wide_instantiation_matches_oracle)
_VARIANTS = {"default": ({}, None), "hbm_ring": ({"LCD_WFA_LDS_MAX_KB": "0"}, None), "wide": (_WIDE, "wide"), "small_blocks": ({"LCD_WFA_BLOCK_KB": "8"}, None)}
_SWITCHES = sorted({k for env, _ in _VARIANTS.values() for k in env})
_expected = {}


def _pairs(pen, only):
    return T.tie_pairs("wide") + T.tie_pairs("str")[:4] if only == "wide" else T.wfa_pairs(pen)


def _oracle_rows(oracle, pen, ga):
    """the oracle's alignments of one scoring and gap_aln: computed once, shared by the variants"""
    if (pen, ga) not in _expected:
        b, q, e, q2, e2 = pen
        _expected[(pen, ga)] = {id_: oracle.wfa_end2end_aln(p, t, ga, b, q, e, q2, e2) for id_, (p, t) in _keyed(T.wfa_pairs(pen))}
    return _expected[(pen, ga)]


def _keyed(pairs):
    return [((p.tobytes(), t.tobytes()), (p, t)) for p, t in pairs]


def _check(lcd, oracle, pen, only, what):
    b, q, e, q2, e2 = pen
    pairs = _pairs(pen, only)
    for ga in (1, 2):
        exp_all = _oracle_rows(oracle, pen, ga)
        got = lcd.wfa_batch(pairs, gap_aln=ga, b=b, q=q, e=e, q2=q2, e2=e2)
        for i, (key, (p, t)) in enumerate(_keyed(pairs)):
            exp = exp_all[key]
            assert got[i]["score"] == exp["score"], (what, ga, i, len(p), len(t))
            assert len(got[i]["cigar"]) == len(exp["cigar"]) and (got[i]["cigar"] == exp["cigar"]).all(), (what, ga, i, len(p), len(t))
            assert len(got[i]["pattern_alg"]) == len(exp["pattern_alg"]) and (got[i]["pattern_alg"] == exp["pattern_alg"]).all(), (what, ga, i)
            assert (got[i]["text_alg"] == exp["text_alg"]).all(), (what, ga, i)
            if only == "wide" and i < len(T.tie_pairs("wide")):     # (the pair's last rows are batched ones: >= 2 048 diagonals)
                assert exp["score"] >= 1524 and min(len(p), len(t)) + min(exp["score"], max(len(p), len(t))) + 1 >= 2048, i


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_wfa_tie_pairs_match_oracle(lcd, oracle, variant, monkeypatch):
    """score, CIGAR and both rows, left- and right-aligned, at the default penalties: the default classes, every job in the HBM-ring class, the instantiation with
    four diagonals per thread in flight (on the long-insertion pairs, whose rows have >= 2 048 diagonals), and blocks of 8 KB of decisions"""
    env, only = _VARIANTS[variant]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(lcd, oracle, T.WFA_PENALTIES[0], only, variant)


@pytest.mark.parametrize("pen", T.WFA_PENALTIES[1:], ids=lambda p: "_".join(map(str, p)))
def test_wfa_tie_pairs_other_penalties_match_oracle(lcd, oracle, pen, monkeypatch):
    """other penalties, with indels of THEIR crossover length (18 and 22 bases)"""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _check(lcd, oracle, pen, None, pen)


def _golden(key):
    with open(os.path.join(ROOT, "tests", "golden", "edlib_tie_golden.json")) as f:
        cases = json.load(f)[key]
    arr = lambda s: np.frombuffer(s.encode(), np.uint8) - ord("0")
    return cases, [(arr(c["target"]), arr(c["query"])) for c in cases]


def test_edlib_kernel_matches_reference_tie_vectors(lcd):
    """the K4 kernel against the reference's own edlib on homopolymer / dinucleotide pairs (nearly every traceback step a tie): distance, xgaps, =/XID counts"""
    cases, pairs = _golden("tie_cases")
    assert len(cases) >= 16
    got = lcd.edlib_batch(pairs)
    for i, c in enumerate(cases):
        assert (got["dist"][i], got["xgaps"][i], got["n_eq"][i], got["n_xid"][i]) == (c["dist"], c["xgaps"], c["n_eq"], c["n_xid"]), (i, len(pairs[i][0]))


def test_edlib_hw_kernel_matches_reference_tie_vectors(lcd):
    """... and in HW (infix) mode: distance, the target stretch, and the path-dependent counts"""
    cases, pairs = _golden("tie_hw_cases")
    assert len(cases) >= 16
    got = lcd.edlib_batch_hw(pairs)
    for i, c in enumerate(cases):
        assert (got["dist"][i], got["start"][i], got["end"][i]) == (c["dist"], c["start"], c["end"]), (i, len(pairs[i][0]))
        assert (got["xgaps"][i], got["n_eq"][i], got["n_xid"][i]) == (c["xgaps"], c["n_eq"], c["n_xid"]), (i, len(pairs[i][0]))
