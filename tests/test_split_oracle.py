"""The oracle of the per-haplotype read sets (tests/split_common.py) against expectations written by hand, against itself under a double reverse-complement,
against the SAM oracle's SEQ / QUAL columns for forward records, and the host-only entry points lcd_split_offsets / lcd_split_paths against their Python
restatements (no GPU needed)."""
import numpy as np
import pytest

import sam_out_common as so
import split_common as sc

NAMES = [b"chrS", b""]


def _one(rec, hap=0, ps=0, kept=True, comment=False, names=None):
    fq, lst, st = sc.split_text([(rec["body"], 0 if kept else -1)], [hap], [ps], names=names, comment=comment)
    return fq, lst, st


def test_forward_by_hand():
    r = sc.make(b"read1", 100, [1, 2, 4, 8, 15, 0], [0, 10, 40, 93, 94, 200])
    fq, lst, st = _one(r, hap=1, ps=77)
    assert fq == [b"", b"@read1\nACGTN=\n+\n!+I~~~\n", b""] and lst == b""
    assert st == dict(n_records=1, n_selected=1, n_hap=[0, 1, 0], n_not_primary=0, n_filtered_primary=0, n_reverse=0, n_no_seq=0, n_bad_layout=0, bytes_fastq=[0, 23, 0], bytes_list=0)


def test_reverse_odd_by_hand():
    r = sc.make(b"r", 100, [1, 1, 2, 4, 8], [1, 2, 3, 4, 5], flag=0x10)       # stored AACGT -> sequenced ACGTT
    assert _one(r, hap=2)[0] == [b"", b"", b"@r\nACGTT\n+\n&%$#\"\n"]


def test_reverse_even_by_hand():
    r = sc.make(b"r", 100, [1, 2, 3, 15, 5, 10], [0, 0, 0, 0, 0, 60], flag=0x10)   # stored A C M N R Y -> complement of the reverse: R Y N K G T
    assert _one(r)[0][0] == b"@r\nRYNKGT\n+\n]!!!!!\n"


def test_comment_by_hand():
    r = sc.make(b"q", 100, [1], [5])
    assert _one(r, hap=1, ps=(1 << 32) + 5, comment=True)[0][1] == b"@q\tHP:i:1\tPS:i:4294967301\nA\n+\n&\n"
    assert _one(r, hap=0, ps=9, comment=True)[0][0] == b"@q\tPS:i:9\nA\n+\n&\n"
    assert _one(r, hap=2, ps=0, comment=True)[0][2] == b"@q\tHP:i:2\nA\n+\n&\n"
    assert _one(r, hap=2, ps=-5, comment=True)[0][2] == b"@q\tHP:i:2\nA\n+\n&\n"
    assert _one(r, hap=2, ps=3, kept=False, comment=True)[0] == [b"@q\nA\n+\n&\n", b"", b""]          # a filtered record: none, no tags


def test_ff_quality_by_hand():
    r = sc.make(b"q", 100, [1, 2, 4], [255, 10, 20])
    assert _one(r)[0][0] == b"@q\nACG\n+\n!!!\n"
    r = sc.make(b"q", 100, [1, 2, 4], [10, 255, 20])                             # 0xff behind the first byte is a quality like any other
    assert _one(r)[0][0] == b"@q\nACG\n+\n+~5\n"
    r = sc.make(b"q", 100, [1, 2, 4], [10, 20, 255], flag=0x10)                   # the FIRST stored byte decides, not the first printed one
    assert _one(r)[0][0] == b"@q\nCGT\n+\n~5+\n"


def test_list_lines_by_hand():
    r = sc.make(b"read1", 100, [1, 2], [1, 2])
    assert _one(r, hap=1, ps=2001, names=NAMES)[1] == b"read1\tH1\t2001\tchrS\n"
    assert _one(r, hap=0, ps=2001, names=NAMES)[1] == b"read1\tnone\t2001\tchrS\n"
    assert _one(r, hap=2, ps=0, names=NAMES)[1] == b"read1\tH2\tnone\tchrS\n"
    assert _one(r, hap=2, ps=5, kept=False, names=NAMES)[1] == b"read1\tnone\tnone\tchrS\n"
    assert _one(r, hap=1, ps=1, names=[])[1] == b"read1\tH1\t1\t*\n"
    empty = sc.make(b"", 100, [], [])
    fq, lst, st = _one(empty, hap=1, ps=4, names=NAMES)
    assert fq == [b"", b"", b""] and lst == b"*\tH1\t4\tchrS\n" and st["n_no_seq"] == 1 and st["n_selected"] == 1 and st["n_hap"] == [0, 1, 0]
    nul = sc.make(b"ab\0cd", 100, [1], [1])
    assert _one(nul, names=NAMES)[1] == b"ab\tnone\tnone\tchrS\n" and _one(nul)[0][0] == b"@ab\nA\n+\n\"\n"


def test_what_is_left_out():
    t = sc.build_cases()
    by = {c["name"]: c["rec"] for c in t["cases"]}
    for name, key in (("secondary", "n_not_primary"), ("supplementary", "n_not_primary"), ("broken_layout", "n_bad_layout")):
        fq, lst, st = _one(by[name], hap=1, names=NAMES)
        assert fq == [b"", b"", b""] and lst == b"" and st[key] == 1 and st["n_selected"] == 0 and st["n_records"] == 1, name


def test_the_case_table_holds_what_it_names():
    t = sc.build_cases()
    names = {c["name"] for c in t["cases"]}
    for n in sc.LENGTHS:
        assert {"len_%d_fwd" % n, "len_%d_rev" % n} <= names
    fq, lst, st = sc.split_text(t["table"], t["haps"], t["phase_sets"], names=[sc.CONTIG], comment=True)
    assert len(t["table"]) == len(t["recs"]) == st["n_records"] and st["n_not_primary"] == 2 and st["n_bad_layout"] == 1 and st["n_no_seq"] == 2
    assert st["n_filtered_primary"] == 3 and st["n_reverse"] > 10 and all(st["n_hap"]) and st["n_selected"] == sum(st["n_hap"]) == lst.count(b"\n")
    assert sum(len(sc.fastq_entries(f)) for f in fq) == st["n_selected"] - st["n_no_seq"]
    assert b"\tPS:i:4294967301\n" in fq[1] and b"\tPS:i:2147483647\n" in fq[1] and b"PS:i:-" not in b"".join(fq)
    # a stream that ends up empty: every record of haplotype 2 left out by the plan
    skip = [int(r >= 0 and t["haps"][r] == 2) for _, r in t["table"]]
    fq2, _, st2 = sc.split_text(t["table"], t["haps"], t["phase_sets"], skip=skip)
    assert fq2[2] == b"" and fq2[1] == sc.split_text(t["table"], t["haps"], t["phase_sets"])[0][1] and st2["n_hap"][2] == 0


def test_order_and_skip():
    t = sc.build_cases()
    n = len(t["table"])
    skip = [i % 2 for i in range(n)]
    order = [i for i in range(n) if not skip[i]][::-1]
    fq, lst, st = sc.split_text(t["table"], t["haps"], t["phase_sets"], skip=skip, order=order + [-1] * (n - len(order)), names=[sc.CONTIG])
    plain = sc.split_text(t["table"], t["haps"], t["phase_sets"], skip=skip, names=[sc.CONTIG])
    for s in range(3):
        assert sc.fastq_entries(fq[s]) == sc.fastq_entries(plain[0][s])[::-1]
    assert lst.splitlines() == plain[1].splitlines()[::-1] and st == plain[2]


def test_reverse_complementing_twice_is_the_identity():
    t = sc.build_cases(with_broken=False)
    for c in t["cases"]:
        b = c["rec"]["body"]
        x = sc.parse(b)
        if x["lseq"] == 0:
            continue
        once = sc.revcomp_body(b)
        assert sc.revcomp_body(once) == b, c["name"]
        # the mirrored record is the same read: its entry is the original's (the 0xff rule looks at the first STORED byte, so those records are left out here)
        if x["quals"][0] != 0xff and x["quals"][-1] != 0xff:
            assert sc.seq_qual(sc.parse(once)) == sc.seq_qual(x), c["name"]
    assert "".join(sc.NIB_COMP[sc.NIB.index(sc.NIB_COMP[k])] for k in range(16)) == sc.NIB


def test_forward_seq_and_qual_are_the_sam_oracle_s_columns():
    t = sc.build_cases(with_broken=False)
    n = 0
    for c in t["cases"]:
        b = c["rec"]["body"]
        x = sc.parse(b)
        if x["flag"] & 0x10 or x["lseq"] == 0 or max(x["quals"]) >= 94:
            continue
        cols = so.sam_line(b, [sc.CONTIG])[0].rstrip(b"\n").split(b"\t")
        assert (cols[9], cols[10]) == sc.seq_qual(x), c["name"]
        n += 1
    assert n >= 15


def test_offsets_through_the_library():
    from longcalld_amd import align
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 500):
        stream = [int(v) for v in rng.integers(-1, 3, n)]
        fl = [int(v) for v in rng.integers(0, 1 << 40, n)]; ll = [int(v) for v in rng.integers(0, 400, n)]
        assert align.split_offsets(stream, fl, ll) == tuple(sc.offsets(stream, fl, ll))
    assert align.split_offsets([1, -1, 1, 0], [10, 99, 5, 7], [3, 99, 4, 2]) == ([0, 0, 10, 0], [0, 3, 3, 7], [7, 15, 0, 9])
    for bad in ([3], [-2]):
        with pytest.raises(align.LcdError):
            align.split_offsets(bad, [1], [1])
    with pytest.raises(align.LcdError):
        align.split_offsets([0, 0], [(1 << 64) - 1, 1], [0, 0])


def test_paths_through_the_library():
    from longcalld_amd import align
    for gz in (False, True):
        assert align.split_paths("out/p", gz) == sc.paths("out/p", gz)
    assert align.split_paths("p", False, ["a.vcf", None, "-", "", "p.h1.fastq.gz", "-"]) == ["p.none.fastq", "p.h1.fastq", "p.h2.fastq"]
    assert align.split_paths(None, False, ["a", "b", None]) == []
    for prefix, gz, other in (("", False, []), ("-", False, []), ("p", False, ["p.h1.fastq"]), ("p", True, ["x", "p.none.fastq.gz"]), ("p", False, ["x", "y", "x"]), (None, False, ["l.tsv", "l.tsv"])):
        with pytest.raises(align.LcdError):
            align.split_paths(prefix, gz, other)
