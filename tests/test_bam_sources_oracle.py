"""CPU side of the chunks-from-any-BAM tests (tests/bam_src_common.py): the Python restatements of the source selection rule and of the SA-tag palindrome rule
give what the named cases expect (flags worked out by hand, and the branch each case is named for), and the seeded file is worth running on the device: every
source class is populated, its oracle accepts most of its reads, noisy windows land in the chunk, palindromic reads change their digars -- and the plain-'M'
oracle agrees with the EQX oracle on these reads, which is what lets tests/test_gpu_bam_sources.py compare the first round of the two BAMs."""
import os

import numpy as np
import pytest

import bam_src_common as bs
from conftest import ROOT


@pytest.fixture(scope="module")
def orc(oracle):
    if not os.path.exists(os.path.join(ROOT, "oracle", "liblcd_oracle.so")):
        pytest.skip("oracle/liblcd_oracle.so not built")
    return oracle


# what each named case must exercise: name -> condition on the oracle's trace
SA_CONDITIONS = {
    "containment": lambda t: t[-1][0] == "contain",
    "left_partial": lambda t: t[-1][0] == "left_partial",
    "left_partial_too_short": lambda t: t[-1][0] == "left_partial",
    "left_of_the_primary": lambda t: t[-1][0] == "left_none",
    "right_partial": lambda t: t[-1][0] == "right_partial",
    "inside": lambda t: t[-1][0] == "inside",
    "right_of_the_primary": lambda t: t[-1][0] == "right_none",
    "exactly_0.9_len_1000": lambda t: t[-1][1] * 10 == 9 * 1000,
    "one_short_len_1000": lambda t: t[-1][1] == 899,
    "exactly_0.9_len_10": lambda t: t[-1][1] * 10 == 9 * 10,
    "one_short_len_10": lambda t: t[-1][1] == 8,
    "second_entry": lambda t: len(t) == 2 and t[0][1] == 0,
    "another_rname": lambda t: t[-1][0] == "contain",
    "plus_strand_entry": lambda t: t[-1][0] == "contain",
    "reverse_primary": lambda t: t[-1][0] == "contain",
    "ops_S_N_I_H_in_the_cigar": lambda t: t[-1][1] == 901,
    "N_is_not_counted": lambda t: t[-1][0] == "left_partial",
    "D_eq_X_are_counted": lambda t: t[-1][1] == 903,
    "letter_without_digits": lambda t: t[-1][1] == 901,
    "missing_cigar": lambda t: t == ["skipped"],
    "missing_strand_and_cigar": lambda t: t == ["skipped"],
    "empty_rname": lambda t: t == ["skipped"],
    "pos_not_a_number_then_a_good_entry": lambda t: t[0] == "skipped" and t[1][0] == "contain",
    "empty_pieces": lambda t: t.count("empty") >= 2,
    "SA_of_type_A": lambda t: t == "not_Z",
    "no_SA": lambda t: t == "no_tag",
    "is_ont_0": lambda t: t == "not_ont",
    "forward_primary": lambda t: t[-1][0] == "contain",
}


def test_named_sa_cases():
    assert 1000.0 * 0.9 == 900.0 and 10.0 * 0.9 == 9.0          # the two "exactly 0.9" cases sit on the boundary in double arithmetic as well
    recs = bs.sa_case_records()
    assert {c[0] for c, _ in recs} == set(SA_CONDITIONS) and len(recs) == len(SA_CONDITIONS)
    seen = set()
    for case, rec in recs:
        name, rlen, flag, is_ont, sa, want, trace = case
        assert rec["end"] - rec["pos0"] == rlen and rec["flag"] == flag
        fld = bs.first_field(bs.aux_walk(rec["aux"]), b"SA")
        assert (fld is None) == (sa is None)
        got, tr = bs.sa_rule(fld, rec["pos0"], rec["end"], flag, is_ont)
        assert got == want, name
        assert tr == trace, (name, tr)
        assert SA_CONDITIONS[name](tr), name
        if isinstance(tr, list):
            seen |= {x[0] for x in tr if isinstance(x, tuple)}
    assert seen == {"contain", "left_partial", "left_none", "right_partial", "inside", "right_none"}
    assert {c[5] for c, _ in recs} == {0, 1, 2}


def _rec(cig, fields):
    a = dict(pos0=100, flag=0, qlen=20, bseq=np.zeros(10, np.uint8), qual=np.full(20, 30, np.uint8), name=b"h")
    return bs.record(a, np.array(cig, np.uint32), fields)


def test_selection_rule_on_hand_built_records():
    M, EQ, X, I, S = 0, 7, 8, 1, 4
    w = lambda op, ln: (ln << 4) | op
    cs, md = ("cs", "Z", b":20"), ("MD", "Z", b"20")
    cases = [
        ([w(EQ, 10), w(X, 1), w(EQ, 9)], [cs, md], bs.SRC_EQX),                               # EQX CIGAR with cs + MD decoys
        ([w(M, 20)], [("NM", "i", 0), md, cs], bs.SRC_CS),                                     # 'M' with cs + MD: cs wins wherever it stands
        ([w(M, 20)], [("XZ", "Z", b"cs"), md], bs.SRC_MD),
        ([w(M, 20)], [("NM", "i", 0)], bs.SRC_REF),
        ([w(M, 20)], [], bs.SRC_REF),
        ([w(S, 5), w(I, 15)], [cs], bs.SRC_CS),                                                # none of = / X / M: "no"
        ([w(S, 5), w(I, 15)], [], bs.SRC_REF),
        ([w(M, 20)], [("cs", "i", 5), md], bs.SRC_CS),                                         # the first cs field decides, whatever its type (status -2 then)
        ([w(S, 2), w(M, 10), w(EQ, 8)], [md], bs.SRC_MD),                                      # the FIRST of = / X / M
        ([w(S, 2), w(X, 1), w(M, 17)], [cs], bs.SRC_EQX),
        ([w(M, 20)], [md, (None, None, b"XBBi" + b"\x64\0\0\0" + b"\1\0\0\0"), cs], bs.SRC_MD),   # a B array that runs past the record: cs behind it does not exist
        ([w(M, 20)], [(None, None, b"XBBi" + b"\x64\0\0\0" + b"\1\0\0\0"), md], bs.SRC_REF),      # ... nor MD
        ([w(M, 20)], [md, (None, None, b"XZZno-nul")], bs.SRC_MD),                             # a Z value without its NUL ends the walk silently
        ([w(M, 20)], [("MD", "Z", b"20"), (None, None, b"cs")], bs.SRC_MD),                    # two bytes left: not a field
    ]
    for cig, fields, want in cases:
        r = _rec(cig, fields)
        src, fld = bs.select_source(r["cig"], r["aux"])
        assert src == want, (cig, fields)
        if want == bs.SRC_CS:
            assert fld[0] == fields[[f[0] for f in fields].index("cs")][1]
    # every field type is stepped over
    rng = np.random.default_rng(1)
    dz = bs.decoys(rng)
    assert {f[1] for f in dz} == set("AcCsSiIfZHB") and {f[2][0] for f in dz if f[1] == "B"} == set("cCsSiIf")
    r = _rec([w(M, 20)], dz + [md])
    assert [t for t, _, _ in bs.aux_walk(r["aux"])] == [f[0].encode() for f in dz] + [b"MD"] and bs.select_source(r["cig"], r["aux"])[0] == bs.SRC_MD


def _same(a, b, what):
    assert a["rc"] == b["rc"], what
    for k in ("digars", "noisy", "chunk_noisy"):
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)
    assert (a["beg"], a["end"], a["n_cand"]) == (b["beg"], b["end"], b["n_cand"]), what


def test_seeded_file_is_worth_running(orc):
    ref, al = bs.seeded()
    letters = bs.ref_letters(ref)
    recs = bs.records_as("mixed")
    assert len(recs) == 60 and all(2000 <= r["end"] - r["pos0"] < 6000 for r in recs) and all(recs[i]["pos0"] <= recs[i + 1]["pos0"] for i in range(59))
    for is_ont in (0, 1):
        ok, win, n = [0] * 4, [0] * 4, [0] * 4
        n_pal = 0
        for i, r in enumerate(recs):
            src, fl, e = bs.expected(orc, r, letters, 1, bs.TLEN, 3000, 27000, is_ont)
            assert src == i % 4
            n[src] += 1; ok[src] += e["rc"] == 0; win[src] += len(e["chunk_noisy"])
            if fl:
                a = r["a"]
                clip = r["cig"][0] if fl == 1 else r["cig"][-1]
                _, _, plain = bs.expected(orc, r, letters, 1, bs.TLEN, 3000, 27000, is_ont, pal=0)
                if int(clip) >> 4 > bs.END_CLIP_REG and int(clip) & 0xf in (4, 5) and (plain["digars"].shape != e["digars"].shape or (plain["digars"] != e["digars"]).any() or
                                                                                           len(plain["noisy"]) != len(e["noisy"])):
                    n_pal += 1
        assert min(n) >= 10 and min(ok) >= 8 and min(win) >= 1, (n, ok, win)
        assert n_pal >= (3 if is_ont else 0) and (is_ont or n_pal == 0)


def test_plain_m_and_eqx_oracles_agree_on_the_seeded_reads(orc):
    """the condition behind tests/test_gpu_bam_sources.py::test_plain_m_bam_through_the_first_round: the reads lie inside the reference window, away from the contig
    ends, so collect_digar_from_ref_seq on the 'M' CIGARs and collect_digar_from_eqx_cigar on the EQX CIGARs give identical digars, windows and counters"""
    ref, al = bs.seeded()
    letters = bs.ref_letters(ref)
    n_win = 0
    for a in al:
        assert a["pos0"] > 200 and a["pos0"] + a["rlen"] < bs.TLEN - 200
        args = (1, bs.TLEN, bs.TLEN, orc.digar_opt(0), 0, 0)
        e = orc.collect_digar_from_eqx_cigar(a["pos0"], a["eqx"], a["qual"], *args)
        _same(e, orc.collect_digar_from_ref_seq(a["pos0"], a["mcig"], a["bseq"], a["qual"], letters, 1, bs.TLEN, *args), "ref")
        _same(e, orc.collect_digar_from_cs_tag(a["pos0"], a["mcig"], a["cs"], a["qual"], *args), "cs")
        _same(e, orc.collect_digar_from_MD_tag(a["pos0"], a["mcig"], a["md"], a["qual"], *args), "MD")
        n_win += len(e["chunk_noisy"])
    assert n_win > 20
