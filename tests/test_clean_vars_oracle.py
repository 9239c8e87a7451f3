"""The C oracle of lcd_chunk_clean_vars (tests/c/clean_vars_oracle.c) on hand-built chunks with the expected values written out, its cr_merge2 against the
reference's own cgranges (where oracle/_ref is built), and the ABI of the new entry points.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import clean_vars_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edge_chunk():
    """600 bp of reference, every read 30-quality unless said otherwise.  Returns (chunk, pre_regs, low_comp)."""
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 4, 600).astype(np.uint8)
    ref[150:160] = 2                                   # a homopolymer (G x 10) for the indel at 152
    reads = []
    def add(pos0, length, ev, rev=0, qual=None):
        r = cc.read_from_hap(ref, pos0, length, ev, qual=qual)
        r["is_rev"] = rev
        reads.append(r)
    ins = lambda n: ("I", [(k * 7 + n) % 4 for k in range(n)])
    # (a) a family of SV-size insertions at 100 (lengths 42, 45, 47 fuzzy-equal to 40; 60 is not, and one read is too few for a candidate)
    for n in (40, 40, 42, 45, 47, 60):
        add(0, 600, {99: ins(n)})
    # (b) N in the alt base of a SNP at 201 (two reads), A / C at the same place (two reads each)
    for b in (4, 4, (ref[200] + 1) % 4, (ref[200] + 1) % 4):
        add(0, 600, {200: ("X", int(b))})
    # (c) low-quality X and I digars at 251 / 261: base quality 5 in two reads, the same events at quality 30 in two others
    for q in (5, 5, 30, 30):
        r = cc.read_from_hap(ref, 0, 600, {250: ("X", int((ref[250] + 2) % 4)), 260: ("I", [1])})
        qq = r["qual"].copy(); qq[250] = q; qq[260] = q          # (the read starts at 0: query offset == reference offset up to the inserted base)
        r["qual"] = qq; r["is_rev"] = 0
        reads.append(r)
    # (d) two overlapping deletions: 3 bp at 301 and 5 bp at 302
    for ev in ({300: ("D", 3)}, {300: ("D", 3)}, {300: ("D", 3)}, {301: ("D", 5)}, {301: ("D", 5)}, {301: ("D", 5)}):
        add(0, 600, ev)
    # (e) variants within 6 bp of the reference ends: SNPs at 3 and 597, an insertion before 595
    for _ in range(3):
        add(0, 600, {2: ("X", int((ref[2] + 1) % 4)), 596: ("X", int((ref[596] + 1) % 4)), 594: ins(2)})
    # (f) a SNP inside the pre-processed noisy region (400, 420]
    for _ in range(3):
        add(0, 600, {410: ("X", int((ref[410] + 1) % 4))})
    # the homopolymer indel (REP_HET: a deletion of one G at 153)
    for _ in range(3):
        add(0, 600, {152: ("D", 1)})
    # (g) a read with a dense error cluster at 461-469 (its own noisy window); SNP at 480 in three other reads
    add(0, 600, {p: ("X", int((ref[p] + 1) % 4)) for p in range(460, 470, 2)} | {p + 1: ("D", 1) for p in range(460, 468, 4)})
    for _ in range(3):
        add(0, 600, {479: ("X", int((ref[479] + 1) % 4))})
    # (i) a read with a 40-base left soft clip at 391 and no event after it: its end-clip window (390, 491] (src/bam_utils.c:780-786); the walk meets no
    # difference, so every site of its span goes to the tail loop, which skips those inside the window (is_in_noisy_reg)
    reads.append(cc.record(390, [(4, 40), (7, 210)], np.concatenate([np.full(40, 1, np.uint8), ref[390:600]]), np.full(250, 30, np.uint8)))
    # (h) ONT strand bias: a SNP at 521 on 14 forward reads and none of the reverse ones (fisher(14, 0, 7, 7) < 0.01), one at 541 on 6 forward reads
    for k in range(14):
        add(0, 600, {520: ("X", int((ref[520] + 1) % 4)), 540: ("X", int((ref[540] + 1) % 4))} if k < 6 else {520: ("X", int((ref[520] + 1) % 4))})
    for k in range(12):
        add(0, 600, {}, rev=1)
    ch = dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=600, whole_ref_len=600, is_ont=0)
    return ch, np.array([[400, 420, 5]], np.int64), np.zeros((0, 2), np.int64)


@pytest.fixture(scope="module")
def edge(oracle):
    ch, pre, low = edge_chunk()
    digs = cc.read_digars(ch, oracle)
    return ch, digs, pre, low


def _span(ch, pos):
    """reads whose aligned span holds the 1-based position"""
    return sum(1 for r in ch["reads"] if r["pos0"] < pos <= r["pos0"] + sum(int(c) >> 4 for c in r["cigar"] if int(c) & 0xf in (2, 3, 7, 8)))


def _var(res, pos, vt, alt_len=None):
    k = [i for i in range(res["n_vars"]) if res["pos"][i] == pos and res["var_type"][i] == vt and (alt_len is None or res["alt_len"][i] == alt_len)]
    return k[0] if k else None


def test_sv_insertion_family_keeps_two_representatives(edge):
    """sorted by length, deduplicated against the last KEPT site: 40 swallows 42, 45, 47 (40 >= 0.8 * 47); 60 is a site of its own (one read: LOW_COV)"""
    ch, digs, pre, low = edge
    r = cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), pre, low)
    ins = [i for i in range(r["n_vars"]) if r["pos"][i] == 100 and r["var_type"][i] == cc.CINS]
    assert [int(r["alt_len"][i]) for i in ins] == [40]
    a = ins[0]
    n_reads = len(ch["reads"])
    assert list(r["alle_covs"][2 * a:2 * a + 2]) == [_span(ch, 100) - 5, 5]       # the 60-base read counts as reference for the 40-base site
    assert r["cate"][a] == cc.HET_INDEL                                   # 5 of 59 reads at min_af 0.01; too long for the homopolymer / repeat tests
    alt = r["alt_pool"][r["alt_off"][a]:r["alt_off"][a + 1]]
    assert list(alt) == [(k * 7 + 40) % 4 for k in range(40)]              # the representative's bases: the first 40-base insertion


def test_tail_walk_skips_the_reads_own_noisy_window(edge):
    ch, digs, pre, low = edge
    i = next(k for k, x in enumerate(ch["reads"]) if x["pos0"] == 390)
    assert digs[i]["rc"] == 0 and [tuple(v) for v in digs[i]["noisy"]] == [(390, 491, 0)]
    r = cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), pre, low)
    inside = [k for k in range(r["n_vars"]) if 391 <= r["pos"][k] < 491]
    after = [k for k in range(r["n_vars"]) if 491 <= r["pos"][k] <= 600]
    assert inside and after                                                # (480 inside; 521, 541, 595, 597 after)
    s, e = r["start_var_idx"][i], r["end_var_idx"][i]
    assert s == after[0] and e == after[-1]                                # the sites in the window never enter the read's profile
    assert list(r["alleles"][r["allele_off"][i]:r["allele_off"][i + 1]]) == [0] * len(after)
    j = next(k for k, x in enumerate(ch["reads"]) if k != i and x["pos0"] == 0 and len(digs[k]["noisy"]) == 0)
    assert r["start_var_idx"][j] <= inside[0] <= r["end_var_idx"][j]       # a read without the window reports them


def test_edge_chunk_expected_values(edge):
    ch, digs, pre, low = edge
    R = len(ch["reads"])
    # sites that only the thresholds or the pre-processed region remove: present without them
    loose = cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), (), low)
    k = _var(loose, 411, cc.CDIFF)
    assert k is not None and list(loose["alle_covs"][2 * k:2 * k + 2]) == [_span(ch, 411) - 3, 3] and loose["cate"][k] == cc.HET_SNP
    assert _var(cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), pre, low), 411, cc.CDIFF) is None
    r = cc.run_oracle(ch, digs, cc.default_opt(), pre, low)
    # (b) N alt: its own site, alt base code 4
    xs = [i for i in range(r["n_vars"]) if r["pos"][i] == 201 and r["var_type"][i] == cc.CDIFF]
    assert len(xs) == 0                                                    # 2 reads each: alt AF < 0.2 -> LOW_AF -> LOW_COV, compacted away
    # (c) low-quality digars are not sites; two reads at quality 30 are (LOW_AF as well)
    assert _var(r, 251, cc.CDIFF) is None
    # (f) inside the pre-processed noisy region: NON_VAR, compacted away
    assert _var(r, 411, cc.CDIFF) is None
    # every remaining variant is a candidate
    assert all(not (c & (cc.NON_VAR | cc.LOW_COV | cc.STRAND_BIAS)) for c in r["cate"])
    # profile layout: per read end - start + 1 entries
    for i in range(R):
        s, e = r["start_var_idx"][i], r["end_var_idx"][i]
        n = int(r["allele_off"][i + 1] - r["allele_off"][i])
        assert n == (e - s + 1 if s >= 0 else 0)


def test_low_af_thresholds_bring_the_small_sites_in(edge):
    """min_af 0.01: the N-alt SNP, the low-quality-masked SNP / insertion and both deletions become sites; overlapping sites open noisy regions"""
    ch, digs, pre, low = edge
    R = len(ch["reads"])
    r = cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), pre, low)
    # (b) N and C at 201 are two sites (alt codes 4 and 1 differ): they overlap each other -> a noisy region, both re-called there
    assert _var(r, 201, cc.CDIFF) is None and any(s < 201 and e >= 201 for s, e, _ in r["regs"])
    k = _var(r, 251, cc.CDIFF)
    assert k is not None and r["low_qual_cov"][k] == 2 and list(r["alle_covs"][2 * k:2 * k + 2]) == [_span(ch, 251) - 4, 2]
    k = _var(r, 262, cc.CINS) if _var(r, 262, cc.CINS) is not None else _var(r, 261, cc.CINS)
    assert k is not None and r["low_qual_cov"][k] == 2
    # (d) the two deletions overlap: var_pos_ovlp_n > 1 -> cr_add_var_cr with the noisy-reads ratio (6 noisy reads of 81 < 0.2: not added at min_af 0.2;
    # at min_af 0.01 it is): a noisy region covers 301-306 and both deletions are compacted away
    assert _var(r, 301, cc.CDEL) is None and _var(r, 302, cc.CDEL) is None
    assert any(s < 301 and e >= 306 for s, e, _ in r["regs"])


def test_homopolymer_and_chunk_end_windows(edge):
    ch, digs, pre, low = edge
    r = cc.run_oracle(ch, digs, cc.default_opt(min_af=0.01), pre, low)
    # the one-base deletion inside G x 10 is REP_HET -> an extra noisy region around it, the deletion itself is re-called there
    assert _var(r, 153, cc.CDEL) is None
    assert any(s < 153 and e >= 153 for s, e, _ in r["regs"])
    # SNPs 2 bp from the reference ends stay clean variants (var_is_homopolymer reads N past the ends)
    assert _var(r, 3, cc.CDIFF) is not None and _var(r, 597, cc.CDIFF) is not None


def test_ont_strand_bias_on_both_sides_of_the_threshold(edge):
    ch, digs, pre, low = edge
    L = cc.oracle_lib()
    p14, p12, p6 = L.cvo_fisher_exact_test(14, 0, 7, 7), L.cvo_fisher_exact_test(12, 0, 6, 6), L.cvo_fisher_exact_test(6, 0, 3, 3)
    assert p14 < 0.01 < p12 < p6
    hifi = cc.run_oracle(ch, digs, cc.default_opt(0, min_af=0.01), pre, low)
    ont = cc.run_oracle(ch, digs, cc.default_opt(1, min_af=0.01), pre, low)
    assert _var(hifi, 521, cc.CDIFF) is not None and _var(ont, 521, cc.CDIFF) is None    # 14 : 0 -> strand bias
    assert _var(hifi, 541, cc.CDIFF) is not None and _var(ont, 541, cc.CDIFF) is not None  # 6 : 0 -> p above 0.01
    k = _var(ont, 541, cc.CDIFF)
    assert list(ont["strand_alle_covs"][4 * k:4 * k + 4]) == [_span(ch, 541) - 12 - 6, 6, 12, 0]


def test_seeded_chunk_profile_is_consistent(oracle):
    ch = cc.make_diploid_chunk(7)
    digs = cc.read_digars(ch, oracle)
    r = cc.run_oracle(ch, digs, cc.default_opt())
    assert r["n_vars"] > 30
    # the profile's alt calls add up to alle_covs[1] minus the low-quality (-2) calls: both walks see the same digars
    alt = np.zeros(r["n_vars"], np.int64)
    for i in range(r["n_reads"]):
        s = r["start_var_idx"][i]
        if s < 0:
            continue
        a = r["alleles"][r["allele_off"][i]:r["allele_off"][i + 1]]
        for k, x in enumerate(a):
            if x == 1:
                alt[s + k] += 1
    snp = r["var_type"] == cc.CDIFF
    assert (alt[snp] == r["alle_covs"][1::2][snp]).all()
    assert sorted(r["cr_read"].tolist()) == [i for i in range(r["n_reads"]) if r["start_var_idx"][i] >= 0]


def test_cr_merge2_matches_the_reference_cgranges():
    so = os.path.join(ROOT, "oracle", "_ref", "libcgranges_ref.so")
    if not os.path.exists(so):
        pytest.skip("oracle/_ref/libcgranges_ref.so is built only where the reference tree exists")
    L = C.CDLL(so)
    if not hasattr(L, "cr_merge2"):
        pytest.skip("the reference build exports no cr_merge2")

    class Intv(C.Structure):
        _fields_ = [("x", C.c_uint64), ("y", C.c_uint32), ("label", C.c_int32)]

    class Cr(C.Structure):
        _fields_ = [("n_r", C.c_int64), ("m_r", C.c_int64), ("r", C.POINTER(Intv))]
    L.cr_init.restype = C.c_void_p
    L.cr_add.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
    L.cr_index.argtypes = [C.c_void_p]
    L.cr_merge2.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.cr_merge2.restype = C.c_void_p
    L.cr_destroy.argtypes = [C.c_void_p]
    rng = np.random.default_rng(11)
    for t in range(200):
        def ivs(n, lab):
            st = rng.integers(0, 5000, n)
            return np.stack([st, st + rng.integers(1, 300, n), lab(n)], 1).astype(np.int64)
        a = ivs(int(rng.integers(0, 40)), lambda n: rng.integers(1, 600, n))
        b = ivs(int(rng.integers(1, 90)), lambda n: np.ones(n, np.int64))
        crs = []
        for rows in (a, b):
            cr = L.cr_init()
            for s, e, l in rows:
                L.cr_add(cr, b"cr", int(s), int(e), int(l))
            L.cr_index(cr)
            crs.append(cr)
        # both inputs in their index order, as classify_cand_vars hands them over
        order = lambda cr: [(C.cast(cr, C.POINTER(Cr)).contents.r[i].x >> 32, C.cast(cr, C.POINTER(Cr)).contents.r[i].x & 0xffffffff,
                             C.cast(cr, C.POINTER(Cr)).contents.r[i].label) for i in range(C.cast(cr, C.POINTER(Cr)).contents.n_r)]
        ia, ib = order(crs[0]), order(crs[1])
        m = L.cr_merge2(crs[0], crs[1], -1, 500, 30)
        got = cc.cr_merge2(np.array(ia, np.int64).reshape(-1, 3), np.array(ib, np.int64).reshape(-1, 3), -1)
        want = np.array(order(m), np.int64).reshape(-1, 3)
        assert (got == want).all(), t


def test_abi_new_symbols_and_no_device():
    from longcalld_amd import _lib
    for name in ("lcd_clean_opt_default", "lcd_chunk_clean_vars", "lcd_chunk_clean_vars_batch", "lcd_clean_vars_free", "lcd_clean_vars_hap_problem"):
        assert name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = C.CDLL(_lib.LIB_PATH)
    for name in _lib.EXPORTS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read()
    assert "lcd_clean_vars_t" in hdr and "lcd_chunk_clean_vars_batch" in hdr
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a device is present: the no-device failure is not observable here")
    from longcalld_amd import align
    o = _lib.LcdCleanOpt()
    align.load_library().lcd_clean_opt_default(C.byref(o), 0)
    out = _lib.LcdCleanVars()
    rc = align.load_library().lcd_chunk_clean_vars(None, C.byref(o), None, None, None, 1, 1, 1, 1, None, 0, None, 0, C.byref(out))
    assert rc < 0                                                          # loud: no device, no host fallback
    assert align.load_library().lcd_last_error()


def test_hap_problem_view_is_the_k5_layout(oracle):
    """lcd_clean_vars_hap_problem (host code, no device needed) over the oracle's result: the K5 problem laid out as assign_hap_germline reads it"""
    from longcalld_amd import align
    ch = cc.make_diploid_chunk(7)
    digs = cc.read_digars(ch, oracle)
    r = cc.run_oracle(ch, digs, cc.default_opt())
    n = len(ch["reads"])
    ordered = np.arange(n, dtype=np.int32); skipped = np.array([d["rc"] == -1 for d in digs], np.uint8)
    p = align.clean_vars_hap_problem(r, ordered, skipped)
    V = r["n_vars"]
    assert p["n_vars"] == V and p["n_reads"] == n
    assert (p["alle_off"] == 2 * np.arange(V + 1)).all() and (p["alle_covs"] == r["alle_covs"]).all()
    assert (p["allele_off"] == r["allele_off"].astype(np.int64)).all() and (p["alleles"] == r["alleles"]).all()
    for k, f in (("var_pos", "pos"), ("var_type", "var_type"), ("var_cate", "cate"), ("total_cov", "total_cov"), ("start_var_idx", "start_var_idx"),
                 ("end_var_idx", "end_var_idx"), ("cr_read", "cr_read"), ("is_homopolymer_indel", "is_homopolymer_indel")):
        assert (p[k] == r[f]).all(), k
    assert (p["ordered_read_ids"] == ordered).all() and (p["is_skipped"] == skipped).all()
    # and K5 (the oracle) phases the reads on it
    from longcalld_amd import jobs
    st = oracle.assign_hap_germline(p, jobs.GERMLINE_CLEAN)
    assert (st["haps"] > 0).sum() > n // 2
