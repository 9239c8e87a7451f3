"""The haplotag rules in Python (tests/haplotag_common.py) on their own: every named case reaches the condition it is named for; in the diploid simulator every read
with a vote gets the haplotype it came from; the reader counts the FIRST reason that holds for a line, normalises allele pairs as the header says, and builds the
tables from unsorted, interleaved input with and without PS (no GPU, no library)."""
import pytest

import bam_out_common as bo
import haplotag_common as hc


@pytest.fixture(scope="module")
def table():
    t = hc.build_cases()
    return t, hc.haplotag(t["table"], t["bodies"], t["reg_beg"], t["reg_end"])


def test_every_named_case_reaches_its_condition(table):
    t, out = table
    by = hc.case_results(t, out)
    assert len({c["name"] for c in t["cases"]}) == len(t["cases"]) > 20
    for c in t["cases"]:
        r = [by[bo.parse(x["body"])["name"]] for x in c["recs"] if bo.parse(x["body"])["name"] in by]
        assert c["pred"](r, t["table"]), c["name"]
    st = out["stats"]
    assert st["n_records"] == len(out["haps"]) and sum(st["n_tagged"]) == st["n_records"] and sum(st["n_verdict"]) == st["n_pairs"]
    assert all(st["n_verdict"][v] for v in (hc.NONE, hc.REF, hc.ALT, hc.OTHER)) and st["n_multi_ps"] >= 2 and st["n_cg"] == 1 and hc.NO_PAIR in out["verdict"]


def test_thresholds(table):
    t, out = table
    strict = hc.haplotag(t["table"], t["bodies"], t["reg_beg"], t["reg_end"], min_bq=20, min_diff=2)
    a, b = hc.case_results(t, out), hc.case_results(t, strict)
    assert (a[b"diff1"]["hap"], b[b"diff1"]["hap"]) == (1, 0) and b[b"diff1"]["ps"] == 0 and (b[b"diff1"]["n1"], b[b"diff1"]["n2"]) == (2, 1)
    assert [v for v in a[b"qlow"]["verdicts"] if v != hc.NO_PAIR] == [hc.ALT] and [v for v in b[b"qlow"]["verdicts"] if v != hc.NO_PAIR] == [hc.LOWQ]
    assert [v for v in b[b"qff"]["verdicts"] if v != hc.NO_PAIR] == [hc.ALT]              # absent qualities pass
    assert strict["stats"]["n_verdict"][hc.LOWQ] == 1 and strict["stats"]["n_tagged"][0] > out["stats"]["n_tagged"][0]


def test_records_without_bases_and_broken_layout(table):
    t, _ = table
    at = t["reg_beg"] + 100 + hc.SLOT * next(c["slot"] for c in t["cases"] if c["name"] == "ins_wrong_bases")
    recs = [hc.make_record(b"noseq", at, [(hc.EQ, 30)], no_seq=True), hc.make_record(b"noseq_i", at, [(hc.EQ, 10), (hc.I, 3), (hc.EQ, 10)], no_seq=True)]
    x = [hc.tag_record(t["table"], r["body"]) for r in recs]
    assert [x[0]["verdicts"], x[1]["verdicts"]] == [[hc.REF], [hc.OTHER]] and x[0]["no_seq"] and x[1]["no_seq"]      # covered: REF; the I operation cannot match
    at = t["reg_beg"] + 100 + hc.SLOT * next(c["slot"] for c in t["cases"] if c["name"] == "quality")
    y = hc.tag_record(t["table"], hc.make_record(b"noseq_s", at, [(hc.M, 30)], no_seq=True)["body"])
    assert y["verdicts"] == [hc.OTHER] and y["hap"] == 0
    good = hc.make_record(b"short", at, [(hc.M, 30)], edits={at + 10: hc.alt_base(at + 10)})["body"]
    assert hc.tag_record(t["table"], good)["hap"] == 1
    cut = hc.tag_record(t["table"], good[:len(good) - 20])
    assert cut["bad"] and cut["hap"] == 0 and cut["verdicts"] == []


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_simulated_reads_get_their_haplotype(seed):
    sim = hc.simulate(seed)
    tabs, st = hc.read_vcf(sim["vcf"].encode(), ["sim"])
    assert st["n_sites"] == len(sim["sites"]) == st["n_lines"] and st["n_ins"] > 5 and st["n_del"] > 5 and st["n_phase_sets"] == 2
    out = hc.haplotag(tabs[0], [r["body"] for r in sim["recs"]], 1, sim["length"])
    n_voted = 0
    for x, r in zip(out["recs"], sim["recs"]):
        if x["n1"] + x["n2"]:
            n_voted += 1
            assert x["hap"] == r["true_hap"] and x["ps"] in (1000, 1001) and min(x["n1"], x["n2"]) == 0, r["pos0"]
    assert n_voted > 150 and out["stats"]["n_verdict"][hc.OTHER] == 0 and out["stats"]["n_multi_ps"] > 5


def test_the_first_reason_is_the_one_counted():
    for line, key in hc.FIRST_REASON:
        _, st = hc.read_vcf((hc.HEAD2 + line).encode(), ["c1", "c2"])
        want = dict.fromkeys(hc.VCF_STAT_KEYS, 0)
        want["n_lines"] = 1; want[key] = 1
        if key in ("n_snv", "n_ins", "n_del"):
            want["n_sites"] = want["n_phase_sets"] = 1
        assert st == want, (line, key)
    _, st = hc.read_vcf((hc.HEAD2 + hc.line2("c1", 10, "AT", "A", "0|1")).encode(), ["c1"], snvs_only=True)
    assert st["n_indel_off"] == 1 and st["n_sites"] == 0
    _, st = hc.read_vcf((hc.HEAD2 + hc.line2("c1", 10, "A" + "C" * 51, "A", "0|1")).encode(), ["c1"], snvs_only=True)
    assert st["n_long_indel"] == 1 and st["n_indel_off"] == 0                                # the length rule comes first


def test_normalisation():
    for (ref, alt, gt), (pos, kind, ln, hap, ins) in hc.NORMALISE:
        tabs, st = hc.read_vcf((hc.HEAD2 + hc.line2("c1", 100, ref, alt, gt)).encode(), ["c1"])
        t = tabs[0]
        assert (t["pos"], t["kind"], t["len"], t["hap_of_alt"]) == ([pos], [kind], [ln], [hap]), (ref, alt, gt)
        assert "".join(hc.NT16[c] for c in t["pool"]) == ins and t["max_footprint"] == (1, 2, ln + 1)[kind]
        if kind == hc.SNV:
            assert (hc.NT16[t["ref_code"][0]], hc.NT16[t["alt_code"][0]]) == ("C", "T")


def test_missing_ps_unsorted_and_interleaved_contigs():
    files = {n: (d, kw) for n, d, kw in hc.crafted_files()}
    data, kw = files["interleaved_unsorted_missing_ps"]
    (c1, c2), st = hc.read_vcf(data, kw["names"])
    assert (c1["pos"], c1["kind"], c1["ps_idx"], c1["ps_value"]) == ([100, 100, 200, 300], [hc.INS, hc.SNV, hc.SNV, hc.SNV], [0, 0, 1, 1], [9, 200])
    assert (c2["pos"], c2["kind"], c2["ps_idx"], c2["ps_value"]) == ([50, 100, 300, 500], [hc.SNV, hc.DEL, hc.SNV, hc.SNV], [0, 1, 0, 1], [50, 7])
    assert c1["hap_of_alt"] == [2, 2, 1, 1] and c1["ins_off"] == [0, 0, 0, 0] and c1["pool"] == [8, 8] and (c1["max_footprint"], c2["max_footprint"]) == (2, 2)
    assert st["n_sites"] == 8 and st["n_phase_sets"] == 4
    (d1, d2), st2 = hc.read_vcf(*[files["second_sample"][0]], kw["names"], sample="S2")
    assert d1["ps_value"] == [44] and d2["ps_value"] == [50, 44] and set(d1["hap_of_alt"] + d2["hap_of_alt"]) == {1}
    for same in ("no_trailing_newline", "crlf", "gzip", "gzip_two_members"):
        import gzip
        raw = files[same][0]
        assert hc.read_vcf(gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw, kw["names"])[0] == [c1, c2], same
    with pytest.raises(hc.VcfError):
        hc.read_vcf(files["truncated_line"][0], kw["names"])
