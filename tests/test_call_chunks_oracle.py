"""The oracle side of the whole-path tests (tests/call_chunks_common.py), on the CPU: the overlap test of the stitch lists on hand cases, and proof from the oracles'
own output that the two-chunk seeds the GPU tests use reach the conditions they are named for -- a stitch that joins two chunks and swaps the second one's
haplotypes, and one that joins them as they are."""
import numpy as np
import pytest

import call_chunks_common as kc


def test_overlap_with_a_neighbouring_region_on_hand_cases():
    prev, nxt = (1000, 2000), (3001, 4000)
    assert kc.ovlp_with_region(2000, 2600, *prev)            # begins exactly at prev_end
    assert not kc.ovlp_with_region(2001, 2600, *prev)
    assert kc.ovlp_with_region(500, 1000, *prev)             # ends exactly at prev_beg
    assert not kc.ovlp_with_region(500, 999, *prev)
    assert kc.ovlp_with_region(2500, 3001, *nxt)             # ends exactly at next_beg
    assert not kc.ovlp_with_region(2500, 3000, *nxt)
    assert not kc.ovlp_with_region(2100, 2900, *prev) and not kc.ovlp_with_region(2100, 2900, *nxt)   # touches neither
    assert kc.ovlp_with_region(900, 4100, *prev) and kc.ovlp_with_region(900, 4100, *nxt)             # spans both


def test_split_chunks_share_their_reads_in_file_order():
    chs = kc.two_chunks(kc.SEED_FLIP)
    (_, down), (up, _) = kc.overlap_lists(chs)
    assert len(down) == len(up) > 5
    for i, j in zip(down, up):                               # the same records, pairwise
        a, b = chs[0]["reads"][i], chs[1]["reads"][j]
        assert a["pos0"] == b["pos0"] and a["cigar"].tolist() == b["cigar"].tolist()
    assert chs[0]["reg_end"] + 1 == chs[1]["reg_beg"] == 6001


@pytest.fixture(scope="module")
def oracle_results(lcd, oracle):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")
    return {seed: kc.oracle_call(lcd, oracle, kc.two_chunks(seed), max_len=kc.TWO_CHUNK_MAX_LEN) for seed in (kc.SEED_FLIP, kc.SEED_JOIN)}


def test_seed_flip_joins_and_swaps_the_haplotypes(oracle_results):
    w = oracle_results[kc.SEED_FLIP]
    flip_hap, pre_ps, cur_ps = w["chunks"][1]["flip"]
    assert flip_hap == 1 and pre_ps > 0 and cur_ps > 0 and pre_ps != cur_ps
    assert w["chunks"][0]["flip"] == (0, -1, -1)
    second = w["chunks"][1]
    assert (second["state"]["phase_sets"] == pre_ps).any() and not (second["state"]["phase_sets"] == cur_ps).any()      # the phase set was renamed
    assert (second["state"]["var_phase_set"] == pre_ps).any()
    assert any(c["n_passes"] > 0 for c in w["chunks"]) and any((c["cv"]["alt_ref_base"] != 4).any() for c in w["chunks"])
    assert len(w["records"]) > 15 and w["vcf_body"].count("\n") > 15
    assert sum(c["n_records"] for c in w["chunks"]) == len(w["records"])


def test_seed_join_joins_without_swapping(oracle_results):
    w = oracle_results[kc.SEED_JOIN]
    flip_hap, pre_ps, cur_ps = w["chunks"][1]["flip"]
    assert flip_hap == 0 and pre_ps > 0 and cur_ps > 0
    assert (w["chunks"][1]["state"]["phase_sets"] == pre_ps).any()
    assert any((c["cv"]["alt_ref_base"] != 4).any() for c in w["chunks"])


def test_records_of_one_phase_set_carry_the_first_chunks_name(oracle_results):
    for w in oracle_results.values():
        pre_ps = w["chunks"][1]["flip"][1]
        n0 = w["chunks"][0]["n_records"]
        assert any(r["PS"] == pre_ps for r in w["records"][:n0]) and any(r["PS"] == pre_ps for r in w["records"][n0:])


def test_planted_insertion_right_of_a_shared_snp_keeps_the_snp_as_its_anchor(lcd, oracle):
    if oracle.ref_cgranges() is None:
        pytest.skip("oracle/_ref/libcgranges_ref.so not built")
    ch, pos = kc.planted_anchor_chunk()
    w = kc.oracle_call(lcd, oracle, [ch])
    c = w["chunks"][0]
    assert len(c["cv"]["regs"]) == 1 and c["cv"]["regs"][0][0] < pos < c["cv"]["regs"][0][1] and c["n_passes"] == 2      # the site lies inside the one noisy region
    odd = kc.anchor_differs(w["records"])
    assert [r["pos"] for r in odd] == [pos] and odd[0]["type"] == kc.CINS and len(odd[0]["alt"][0]) == 6
    assert odd[0]["alt"][0][0] == c["cv"]["alt_ref_base"][odd[0]["cand_i"]] != ch["ref"][pos - 1] == odd[0]["ref"][0]
    line = [l.split("\t") for l in w["vcf_body"].splitlines() if l.split("\t")[1] == str(pos) and len(l.split("\t")[4]) == 6]
    assert len(line) == 1 and line[0][3][0] != line[0][4][0]                          # REF and ALT begin with different letters

