"""The refined alignment output on the CPU: the case table reaches every condition it names (proved from the oracle's own trace), and a refined record still
describes the alignment its digars describe -- its CIGAR re-expanded against the window and its bases, its NM, its MD and its cs."""
import re
import struct

import numpy as np
import pytest

import bam_out_common as bo
import refine_cases as cases
import refine_common as rc


@pytest.fixture(scope="module")
def table(oracle):
    cs = cases.build()
    digars_of, skipped, touched, kept = cases.resolve(cs, oracle)
    return cs, digars_of, skipped, touched, kept


def _one(c, d, skipped, trace):
    kept = not (c["rec"]["flag"] & cases.FILTER_FLAGS)
    return rc.refine_record(c["rec"]["body"], kept, d, skipped, cases.WIN, cases.REF_BEG, cases.REF_END, c["hap"], c["ps"], trace)


def test_c1_every_named_condition_is_reached(table):
    cs, digars_of, skipped, touched, kept = table
    read_of = {i: r for r, i in enumerate(kept)}
    seen = set()
    for i, c in enumerate(cs):
        r = read_of.get(i)
        t = []
        _, state = _one(c, digars_of[r] if r is not None else None, skipped[r] if r is not None else False, t)
        assert state == c["state"], (c["name"], state, t)
        for w in c["want"]:
            assert w in t, (c["name"], w, t)
        seen.add(state)
    assert seen == {"filtered", "changed", "identical"} | set(rc.REASONS)
    n = {c["name"]: len(digars_of[read_of[i]]) for i, c in enumerate(cs) if i in read_of}
    assert [n["digars_%d" % k] for k in (1, 63, 64, 65, 130)] == [1, 63, 64, 65, 130] and n["unrefined_too_many_ops"] == 65536
    assert any(isinstance(c["digars"], str) for c in cs) and len(touched) > 20                  # both digar sources
    assert len({(len(c["rec"]["body"]) + 4) % 2 for c in cs}) == 2                             # records start at odd and even offsets


def test_c1_named_texts(table):
    """the bytes that make a case what it says it is, worked out by hand"""
    cs, digars_of, skipped, touched, kept = table
    by = {c["name"]: (c, digars_of[r]) for r, c in ((r, cs[i]) for r, i in enumerate(kept))}
    L = lambda p: bytes([b"ACGT"[cases.REF[p - 1]]])
    E = cases.REF_END
    md = lambda n: rc.digars_md(by[n][1], cases.WIN, cases.REF_BEG, cases.REF_END)
    csx = lambda n: rc.digars_cs(by[n][1], rc.read_codes(by[n][0]["rec"]["body"]), cases.WIN, cases.REF_BEG, cases.REF_END)
    assert md("window_first_base_X") == b"1N" + L(1003) + b"50" and md("window_first_base_D") == b"2^N" + L(1003) + b"50"
    assert md("window_last_base_X") == b"10" + L(E - 1) + b"NN30" and md("window_last_base_D") == b"9^" + L(E - 1) + b"NN30"
    assert csx("window_last_base_D") == b":9-" + L(E - 1).lower() + b"nn:30"
    assert re.fullmatch(rb":1\*n[acgt]\*" + L(1003).lower() + rb"[acgt]:50", csx("window_first_base_X"))
    assert md("adjacent_eq_all_three_equal").startswith(b"20") and csx("adjacent_eq_all_three_equal").startswith(b":12:8*")
    assert md("decimal_widths").split(b"^")[0][:2] == b"9" + L(by["decimal_widths"][0]["rec"]["pos0"] + 10) and b"10" in md("decimal_widths") and b"99^" in md("decimal_widths") and b"100" in md("decimal_widths")
    assert b":9*" in csx("decimal_widths") and b":10*" in csx("decimal_widths") and b":99-" in csx("decimal_widths") and b":100*" in csx("decimal_widths")
    d = by["md_eq_len_over_insertion_and_64"][1]
    assert (d[62][1], d[63][1], d[64][1], d[65][1]) == (7, 1, 7, 8) and md("md_eq_len_over_insertion_and_64").endswith(b"%d" % (d[62][2] + d[64][2]) + L(d[65][0]) + b"4")
    d = by["eq_run_merged_across_64"][1]
    w = rc.digars_cigar(d)
    assert d[63][1] == d[64][1] == 7 and (5 << 4 | 7) in w and len(w) == len(d) - 1
    w = rc.digars_cigar(by["hard_to_soft_both_ends"][1])
    assert w[0] == (7 << 4 | 4) and w[-1] == (9 << 4 | 4)


def test_c3_a_refined_record_describes_its_digars(table):
    cs, digars_of, skipped, touched, kept = table
    n = 0
    for r, i in enumerate(kept):
        c, d = cs[i], digars_of[r]
        if c["state"] != "changed" or c["name"].startswith("window_"):         # (outside the window the texts say N: nothing to parse back)
            continue
        new, _ = _one(c, d, skipped[r], [])
        x = rc.core(new)
        want = rc.digar_events(d)
        bases = rc.read_codes(new)
        assert (bases == rc.read_codes(c["rec"]["body"])).all()
        got = rc.expand_cigar(x["pos"], x["cig"], bases, cases.REF, 1)
        assert got == want, c["name"]
        assert sum(1 for k, *_ in want if k != "=") == rc.digars_nm(d)
        # the texts, regenerated for every such record whatever tags it carries, parse back to the same columns
        md = rc.md_ref_events(rc.digars_md(d, cases.WIN, cases.REF_BEG, cases.REF_END))
        cst = rc.cs_events(rc.digars_cs(d, bases, cases.WIN, cases.REF_BEG, cases.REF_END))
        ref_cols = [(k, p) for k, p, _ in want if k != "I"]
        assert len(md) == len(ref_cols)
        for m, (k, p) in zip(md, ref_cols):
            assert (m == "=") if k == "=" else (m == (k, bytes([b"ACGT"[cases.REF[p - 1]]]))), c["name"]
        assert len(cst) == len(want)
        for e, (k, p, q) in zip(cst, want):
            rb, qb = bytes([b"acgt"[cases.REF[p - 1]]]), bytes([b"acgtn"[bases[q]]])
            assert e == {"=": "=", "X": ("X", rb, qb), "I": ("I", qb), "D": ("D", rb)}[k], c["name"]
        n += 1
    assert n >= 15


def test_stream_selection_and_stats(table):
    cs, digars_of, skipped, touched, kept = table
    recs = bo.region_records([c["rec"]["body"] for c in cs], 1, cases.TLEN, cases.MIN_MAPQ)
    assert [r for _, r in recs if r >= 0] == list(range(len(kept))) and sum(1 for _, r in recs if r < 0) == 1
    haps = [cs[i]["hap"] for i in kept]; ps = [cs[i]["ps"] for i in kept]
    out, n, st, states = rc.refined_stream(recs, digars_of, skipped, cases.WIN, cases.REF_BEG, cases.REF_END, haps, ps)
    assert n == len(cs) and states == [c["state"] for c in cs]
    assert st["n_unrefined"] == 6 and st["n_no_digars"] == 2 and st["n_identical"] == 3 and st["n_pos_moved"] == 5 and st["n_refined"] == len(cs) - 1 - 6 - 3
    _, bodies = bo.bam_split(b"BAM\x01" + struct.pack("<ii", 0, 0) + out)
    assert len(bodies) == n
    skip = np.zeros(len(recs), np.uint8); skip[[2, 5]] = 1
    order = [i for i in range(len(recs)) if not skip[i]][::-1]
    out2, n2, st2, _ = rc.refined_stream(recs, digars_of, skipped, cases.WIN, cases.REF_BEG, cases.REF_END, haps, ps, skip, order)
    _, b2 = bo.bam_split(b"BAM\x01" + struct.pack("<ii", 0, 0) + out2)
    assert n2 == n - 2 and b2 == [bodies[i] for i in order]
