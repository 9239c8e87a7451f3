"""lcd_call_bam_regions with refined alignments on the MI355X: the two-chunk seeded BAM in its EQX, cs, MD and plain-'M' spellings, called and written with refined alignments in one
call.  The VCF text and every read's HP / PS are those of the run without refine; every output record equals the oracle's (tests/refine_call_common.py); reads the
two chunks share are written once; nothing is left unrefined; and the classes of change -- a CIGAR changed inside a noisy region, 'M' -> '=' / 'X', POS moved -- are
shown on the oracle's output before anything is compared."""
import struct

import pytest

import bam_out_common as bo
import call_chunks_common as kc
import refine_call_common as rcc
import refine_common as rc

pytestmark = pytest.mark.gpu
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:test"


@pytest.mark.parametrize("kind", rcc.KINDS)
def test_g3_two_regions_refined_in_one_call(lcd, oracle, tmp_path, kind):
    whole, recs, bam, fa = rcc.write_inputs(tmp_path, kc.SEED_FLIP, kind)
    chs = kc.split_chunk(whole, [6000])
    begs, ends = [ch["reg_beg"] for ch in chs], [ch["reg_end"] for ch in chs]
    cfg = lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))
    plain_out, out = str(tmp_path / "plain.bam"), str(tmp_path / "out.bam")
    plain = lcd.call_bam_regions(bam, bam + ".bai", fa, rcc.CHROM, begs, ends, min_mapq=30, cfg=cfg, bam_out=dict(path=plain_out, pg_line=PG))
    got = lcd.call_bam_regions(bam, bam + ".bai", fa, rcc.CHROM, begs, ends, min_mapq=30, cfg=cfg, bam_out=dict(path=out, pg_line=PG), refine=True)
    assert plain["bam_out_rc"] == 0 and got["bam_out_rc"] == 0, got["bam_out_error"]
    # the call never sees a refined digar
    assert got["records"] == plain["records"] and got["vcf_body"] == plain["vcf_body"] and len(got["records"]) > 15
    for g, p in zip(got["chunks"], plain["chunks"]):
        assert g["haps"].tolist() == p["haps"].tolist() and g["phase_sets"].tolist() == p["phase_sets"].tolist()
    # the oracle first: the classes of change are there
    want, per = rcc.oracle_refined(lcd, oracle, whole, recs, list(zip(begs, ends)), got["chunks"], kc.TWO_CHUNK_MAX_LEN)
    n_log = sum(len(p["log"]) for p in per)
    n_noisy = sum(1 for p in per for r in {e["read_id"] for e in p["log"]} if rc.digars_cigar(p["final"][r]) != rc.digars_cigar(p["digs"][r]["digars"].tolist()))
    _, want_bodies = bo.bam_split(b"BAM\x01" + struct.pack("<ii", 0, 0) + want)
    in_by_name = {bo.parse(r["body"])["name"]: r["body"] for r in recs}
    n_m = sum(1 for b in want_bodies if any((w & 0xf) == 0 for w in rc.core(in_by_name[bo.parse(b)["name"]])["cig"]) and not any((w & 0xf) == 0 for w in rc.core(b)["cig"]))
    n_pos = sum(1 for b in want_bodies if bo.parse(b)["pos0"] != bo.parse(in_by_name[bo.parse(b)["name"]])["pos0"])
    st = {k: sum(p["stats"][k] for p in per) for k in per[0]["stats"]}
    print(kind, "log entries", n_log, "reads changed in a noisy region", n_noisy, "M -> =/X", n_m, "pos moved", n_pos, st)
    assert n_log > 0 and n_noisy >= 1 and st["n_unrefined"] == 0 and st["n_refined"] >= 1
    assert (n_m >= 1) == (kind != "eqx") and n_pos >= 1
    # the file
    hdr_in, _ = bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(bam, "rb").read())))
    stream = b"".join(m["payload"] for m in bo.bgzf_members(open(out, "rb").read()))
    head = bo.header_with_pg(hdr_in, PG.encode())
    assert stream.startswith(head)
    _, bodies = bo.bam_split(stream)
    assert len(bodies) == len(want_bodies) == len(recs)                    # every read once: the second chunk leaves out what the first wrote
    assert sorted(bo.parse(b)["name"] for b in bodies) == sorted(in_by_name)
    for b, w in zip(bodies, want_bodies):
        assert b == w, bo.parse(w)["name"]
    assert stream == head + want
    for k in ("n_records", "n_kept", "n_refined", "n_identical", "n_unrefined", "n_pos_moved", "n_nm_replaced", "n_md_replaced", "n_cs_replaced"):
        assert got["refine"][k] == st[k], k
    assert got["refine"]["n_log_entries"] == n_log and got["refine"]["bytes_log_down"] == 2 * sum(len(e["target"]) for p in per for e in p["log"])
    # HP / PS of every record are those of the run without refine
    _, plain_bodies = bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(open(plain_out, "rb").read())))
    tags = lambda b: [(t, ty, bytes(v)) for t, ty, v, *_ in bo.field_spans(b[bo.parse(b)["aux0"]:]) if t in (b"HP", b"PS")]
    assert [(bo.parse(b)["name"], tags(b)) for b in bodies] == [(bo.parse(b)["name"], tags(b)) for b in plain_bodies]
