"""Chunks from ANY BAM on the MI355X (lcd_chunk_create_from_bam_src): every read from the digar source the reference chooses for it -- EQX CIGAR, cs tag, MD
tag, comparison with the reference (collect_digars_from_bam, src/collect_var.c:1072-1079) -- and, on ONT data, the SA-tag palindrome rule
(is_ont_palindrome_clip, src/bam_utils.c:642-698).  Every read of a seeded mixed file against the oracle of ITS source (oracle/digar_tags.c, oracle/digar.c)
through lcd_chunk_digars, the named SA cases, broken tags and records, the unchanged old entry point, and a plain-'M' BAM through the first round
(lcd_chunk_clean_vars) against the EQX BAM of the same alignments.  Inputs and the Python side of the rules: tests/bam_src_common.py; that they are worth
running, and the oracle agreement the first-round comparison rests on: tests/test_bam_sources_oracle.py."""
import numpy as np
import pytest

import bam_src_common as bs
import clean_vars_common as cc
import testdata_common as tc
from test_gpu_digar import _cigar_of

pytestmark = pytest.mark.gpu

RB, RE = 6000, 24000            # the chunk region of the seeded file: reads on either side of it, noisy windows inside and outside
WB, WE = 5000, 25000            # its reference window: the outermost reads stick out of it (bases stepped over without a digar)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_src")
    out = {}
    for kind in ("mixed", "eqx", "ref"):
        recs = bs.records_as(kind, sa=kind == "mixed")
        path = str(d / f"{kind}.bam")
        bs.write_bam(path, recs)
        out[kind] = (path, recs)
    return out


def _chunk(lcd, path, src, beg=RB, end=RE):
    return lcd.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, beg, end, min_mapq=30, src=src)


def _kept(recs, beg=RB, end=RE):
    return [r for r in recs if r["pos0"] < end and r["end"] > beg - 1]


def _same_read(e, i, info, ivs, dg, what):
    assert info["status"][i] == e["rc"], what
    if e["rc"] == -2:            # the reference stops the program there: nothing else is defined
        return
    assert dg[i].shape == e["digars"].shape and (dg[i] == e["digars"]).all(), what
    assert info["n_digars"][i] == len(e["digars"]) and (info["beg"][i], info["end"][i], info["n_cand"][i]) == (e["beg"], e["end"], e["n_cand"]), what
    noisy, inc = ivs[i]
    assert noisy.shape == e["noisy"].shape and (noisy == e["noisy"]).all(), what
    assert noisy[inc].reshape(-1, 3).shape == e["chunk_noisy"].shape and (noisy[inc].reshape(-1, 3) == e["chunk_noisy"]).all(), what


def _check_chunk(dev, orc, kept, ref, ref_beg, ref_end, beg, end, is_ont):
    so = dev.sources(); info = dev.read_info(); ivs = dev.intervals(); dg = dev.digars()
    assert dev.n == len(kept) and dev.meta["names"] == [r["a"]["name"].decode() for r in kept]
    tag_bytes = 0
    exp = []
    for i, r in enumerate(kept):
        src, fl, e = bs.expected(orc, r, ref, ref_beg, ref_end, beg, end, is_ont)
        assert so["source"][i] == src and so["is_ont_palindrome"][i] == (fl != 0), (i, src, fl)
        _same_read(e, i, info, ivs, dg, (r["a"]["name"], src, fl))
        fld = bs.select_source(r["cig"], r["aux"])[1]
        if src in (bs.SRC_CS, bs.SRC_MD) and fld[0] == "Z":
            tag_bytes += len(fld[1])
        exp.append((src, fl, e))
    assert so["tag_bytes_d2h"] == tag_bytes
    return exp, so


def test_every_source_equals_its_oracle(lcd, oracle, files):
    path, recs = files["mixed"]
    ref, _ = bs.seeded()
    window = bs.ref_letters(ref)[WB - 1:WE]
    kept = _kept(recs)
    assert 40 <= len(kept) < len(recs)
    for is_ont in (0, 1):
        c0 = lcd.copy_counters()
        dev = _chunk(lcd, path, (window, WB, WE, is_ont))
        assert lcd.copy_counters() == c0                                  # no digar, no base crossed PCIe while the chunk was made
        exp, so = _check_chunk(dev, oracle, kept, window, WB, WE, RB, RE, is_ont)
        assert lcd.copy_counters()[2:] == c0[2:]                          # (lcd_chunk_digars counts its download in [0])
        n_src = np.bincount(so["source"], minlength=4)
        assert n_src.min() >= 10 and so["tag_bytes_d2h"] > 0
        assert sum(len(e["chunk_noisy"]) for _, _, e in exp if e["rc"] == 0) > 20 and any(e["rc"] == -1 for _, _, e in exp)
        assert int(so["is_ont_palindrome"].sum()) == (sum(1 for r in kept if r["a"]["sa"] is not None and r["a"]["sa"].startswith(b"chrS")) if is_ont else 0)
        assert not is_ont or so["is_ont_palindrome"].sum() >= 3
        dev.close()


def test_sa_cases_on_the_device(lcd, oracle, tmp_path):
    cases = bs.sa_case_records()
    recs = [r for _, r in cases]
    path = str(tmp_path / "sa.bam")
    bs.write_bam(path, recs, block=5000)
    ref, _ = bs.seeded()
    letters = bs.ref_letters(ref)
    for is_ont in (1, 0):
        dev = _chunk(lcd, path, (letters, 1, bs.TLEN, is_ont), 1, bs.TLEN)
        exp, so = _check_chunk(dev, oracle, recs, letters, 1, bs.TLEN, 1, bs.TLEN, is_ont)
        dg = dev.digars()
        for i, (case, r) in enumerate(cases):
            name, rlen, flag, case_ont, sa, want, trace = case
            if case_ont == is_ont:                                        # the flag worked out by hand, not the Python oracle's
                assert exp[i][1] == want and so["is_ont_palindrome"][i] == (want != 0), name
                side = 0 if want == 1 else -1
                if want:                                                  # the palindromic side's clip is a hard-clip digar, its flank no noisy window
                    assert dg[i][side][1] == 5, name
        if not is_ont:
            assert not so["is_ont_palindrome"].any()
        else:
            assert so["is_ont_palindrome"].sum() == sum(1 for c, _ in cases if c[5] and c[3]) + 1   # (+ the is_ont = 0 case, which this run reads with is_ont = 1)
        dev.close()


def test_m_cigar_chunk_without_reference_and_bad_tags(lcd, oracle, tmp_path):
    ref, al = bs.seeded()
    letters = bs.ref_letters(ref)
    rng = np.random.default_rng(5)
    dz = bs.decoys(rng)
    w = lambda op, ln: (ln << 4) | op
    a = al[:13]
    bad_cs = a[1]["cs"][:40] + b"!" + a[1]["cs"][40:]
    broken_b = (None, None, b"XBBi" + (1 << 30).to_bytes(4, "little") + b"\1\0\0\0")   # a B,i array of 2^30 entries with one of them: it runs past the record
    si = dict(a[9]); si.update(qlen=20, bseq=a[9]["bseq"][:10], qual=a[9]["qual"][:20])
    recs = [
        bs.record(a[0], a[0]["mcig"], dz[:6]),                                                        # 0: plain 'M': REF
        bs.record(a[1], a[1]["mcig"], dz[:3] + [("cs", "Z", bad_cs)] + dz[3:5]),                      # 1: a foreign character in cs
        bs.record(a[2], a[2]["mcig"], [("MD", "Z", a[2]["md"][:-3])] + dz[:4]),                       # 2: MD shorter than its CIGAR
        bs.record(a[3], a[3]["mcig"], dz[:9] + [("cs", "Z", a[3]["cs"])]),                            # 3: a good cs read
        bs.record(a[4], a[4]["mcig"], [("MD", "Z", a[4]["md"])]),                                     # 4: a good MD read
        bs.record(a[5], a[5]["mcig"], dz[:2] + [("MD", "Z", a[5]["md"]), broken_b, ("cs", "Z", a[5]["cs"])]),   # 5: the aux block is cut off mid-field: no cs behind it
        bs.record(a[6], a[6]["mcig"], [broken_b, ("MD", "Z", a[6]["md"])]),                           # 6: ... in the first field: no tag at all
        bs.record(a[7], a[7]["mcig"], [("cs", "i", 5), ("MD", "Z", a[7]["md"])]),                     # 7: cs of type i decides, and is not a string
        bs.record(a[8], a[8]["eqx"], [("cs", "Z", b":1"), ("MD", "Z", b"1")] + dz[:5]),               # 8: EQX CIGAR: the (wrong) tags are not looked at
        bs.record(si, np.array([w(4, 5), w(1, 15)], np.uint32), [("cs", "Z", b"+" + b"a" * 15)]),     # 9: neither = / X nor M: "no", cs
        bs.record(a[10], a[10]["mcig"], []),                                                          # 10: no aux block at all
        bs.record(a[11], a[11]["mcig"], dz),                                                          # 11: every decoy type, no tag
        bs.record(a[12], a[12]["mcig"], [("cs", "Z", a[12]["cs"]), (None, None, b"XZZno-nul-before-the-record-ends")]),   # 12: a Z value cut off behind the tag that matters
    ]
    want_src = [3, 1, 2, 1, 2, 2, 3, 1, 0, 1, 3, 3, 1]
    path = str(tmp_path / "bad.bam")
    bs.write_bam(path, recs, block=7000)
    for have_ref in (False, True):
        src = (letters, 1, bs.TLEN, 0) if have_ref else (None, 0, -1, 0)
        dev = _chunk(lcd, path, src, 1, bs.TLEN)
        so = dev.sources(); info = dev.read_info(); ivs = dev.intervals(); dg = dev.digars()
        assert dev.n == len(recs) and list(so["source"]) == want_src
        for i, r in enumerate(recs):
            if i == 9:
                continue                                                  # (the rule is what this record is about: its reference span is empty)
            s, fl, e = bs.expected(oracle, r, letters if have_ref else None, 1, bs.TLEN, 1, bs.TLEN, 0)
            assert s == want_src[i]
            _same_read(e, i, info, ivs, dg, (i, have_ref))
        st = info["status"]
        assert st[1] == -2 and st[2] == -2 and st[7] == -2 and all(st[i] in (0, -1) for i in (3, 4, 5, 8, 12))
        assert all((st[i] == -2) == (not have_ref) for i in (0, 6, 10, 11))    # without a reference: -2 for the REF reads, and only for them
        dev.close()
    empty = _chunk(lcd, path, (letters, 5, 4, 0), 1, bs.TLEN)                 # an empty window is no reference either
    assert [empty.read_info()["status"][i] for i in (0, 6, 10, 11)] == [-2] * 4
    empty.close()


def test_old_entry_point_unchanged(lcd, files):
    path, recs = files["mixed"]
    ref, _ = bs.seeded()
    kept = _kept(recs)
    old = lcd.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30)
    new = _chunk(lcd, path, (bs.ref_letters(ref), 1, bs.TLEN, 0))
    assert old.n == new.n == len(kept)
    for k in ("pos0", "end_pos", "mapq", "flag", "n_cigar", "qlen"):
        assert (old.meta[k] == new.meta[k]).all()
    a, b = old.read_info(), new.read_info()
    ia, ib = old.intervals(), new.intervals()
    da, db = old.digars(), new.digars()
    src = new.sources()["source"]
    assert not old.sources()["source"].any() and old.sources()["tag_bytes_d2h"] == 0
    n_eqx = 0
    for i in range(old.n):
        if src[i] == bs.SRC_EQX:
            n_eqx += 1
            assert all(a[k][i] == b[k][i] for k in a) and a["status"][i] in (0, -1)
            assert (ia[i][0] == ib[i][0]).all() and (ia[i][1] == ib[i][1]).all() and (da[i] == db[i]).all() and len(da[i]) > 0
        else:
            assert a["status"][i] == -2                                   # an 'M' operation, whatever tags the read carries
    assert n_eqx >= 10
    old.close(); new.close()


def test_plain_m_bam_through_the_first_round(lcd, files):
    """valid because tests/test_bam_sources_oracle.py::test_plain_m_and_eqx_oracles_agree_on_the_seeded_reads holds for these reads"""
    ref, al = bs.seeded()
    letters = bs.ref_letters(ref)
    c0 = lcd.copy_counters()
    m = _chunk(lcd, files["ref"][0], (letters, 1, bs.TLEN, 0), 1, bs.TLEN)
    e = lcd.DeviceChunk.from_bam(files["eqx"][0], files["eqx"][0] + ".bai", bs.CONTIG, 1, bs.TLEN, min_mapq=30)
    assert m.n == e.n == len(al) and (m.sources()["source"] == bs.SRC_REF).all()
    info = e.read_info(); ivs = e.intervals()
    assert all((info[k] == m.read_info()[k]).all() for k in info)
    kept = [i for i in range(e.n) if info["status"][i] == 0]
    low = lcd.sdust(ref)
    pre = lcd.pre_process_noisy_regs(np.concatenate([ivs[i][0][ivs[i][1]] for i in kept]), low, [info["beg"][i] for i in kept], [info["end"][i] for i in kept],
                                     [ivs[i][0] for i in kept])
    args = dict(ordered_read_ids=np.arange(e.n, dtype=np.int32), ref=ref, ref_beg=1, ref_end=bs.TLEN, reg_beg=1, reg_end=bs.TLEN, pre_regs=pre, low_comp=low,
                is_rev=np.array([(a["flag"] >> 4) & 1 for a in al], np.uint8))
    got_m, got_e = m.clean_vars(**args), e.clean_vars(**args)
    print("first round: n_vars", got_e["n_vars"], "regs", len(got_e["regs"]), "alleles", len(got_e["alleles"]))
    assert got_e["n_vars"] >= 20 and len(got_e["alleles"]) > 0           # ~170 planted sites on two haplotypes at ~8x
    cc.same_clean_vars(got_m, got_e)
    c1 = lcd.copy_counters()
    assert c1[2:] == c0[2:] and c1[0] == c0[0]                            # no read base moved in either direction, no digar came down
    m.close(); e.close()


def test_real_chunk_as_plain_m_bam(lcd, tmp_path):
    """the bundled HG002 chunk written as an 'M'-CIGAR BAM without tags (only the stretches inside noisy regions carry bases, the rest is 'N': a dense stress of
    the comparison): digars == lcd_digar_batch_ref on the host arrays of the same reads, one launch each"""
    ch = tc.Chunk()
    o = int(ch.z["ref_beg"]); refc = np.asarray(ch.z["ref"], np.uint8)
    ref_end = o + len(refc) - 1
    order = sorted(range(ch.n_reads), key=lambda i: int(ch.digars[i][0][0]))
    recs, mc = [], []
    for i in order:
        m = []
        for wd in _cigar_of(ch.digars[i]):
            op = int(wd) & 0xf; l = int(wd) >> 4; o2 = 0 if op in (7, 8) else op
            if m and o2 == 0 and (m[-1] & 0xf) == 0:
                m[-1] += l << 4
            else:
                m.append((l << 4) | o2)
        mc.append(np.array(m, np.uint32))
        qlen = int(ch.qlen[i])
        a = dict(pos0=int(ch.digars[i][0][0]) - 1, flag=0, qlen=qlen, bseq=np.asarray(ch.bseq[i], np.uint8)[:(qlen + 1) // 2], qual=np.asarray(ch.qual[i], np.uint8), name=f"m/{i}/ccs".encode())
        recs.append(bs.record(a, mc[-1], [("NM", "i", 1)]))
    path = str(tmp_path / "real_m.bam")
    tlen = 135086622
    bs.write_bam(path, recs, block=65280, tlen=tlen)
    reg_beg, reg_end = o + 20000, o + 180000
    c0 = lcd.copy_counters()
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, reg_beg, reg_end, min_mapq=30, src=(refc, o, ref_end, 0))
    assert lcd.copy_counters() == c0
    kept = [k for k, r in enumerate(recs) if r["pos0"] < reg_end and r["end"] > reg_beg - 1]
    assert dev.n == len(kept) and len(kept) > 20 and (dev.sources()["source"] == bs.SRC_REF).all()
    got = lcd.digar_batch([recs[k]["pos0"] for k in kept], [mc[k] for k in kept], [recs[k]["a"]["qual"] for k in kept], reg_beg, reg_end, tlen,
                          seqs=[recs[k]["a"]["bseq"] for k in kept], ref=(refc.tobytes(), o, ref_end))
    info = dev.read_info(); ivs = dev.intervals(); dg = dev.digars()
    n_dig = 0
    for i in range(dev.n):
        _same_read(got[i], i, info, ivs, dg, i)
        n_dig += len(dg[i])
    assert n_dig > 100000
    dev.close()
