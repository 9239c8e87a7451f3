"""lcd_call_files_ext2's methylation table (align.call_file(mods=...), --mods FILE) on the MI355X: a two-contig BAM whose reads carry MM / ML, called in windows of
chunks.  The yardstick is per contig: lcd_call_bam_regions_ext2 with the contig's planned regions returns every chunk's final haplotypes and writes the contig's
table; the oracle with EACH CHUNK'S OWN haplotypes must give that table, and the contigs' tables one after the other must be the file driver's, every column, with
and without combine_strands.  The table must not depend on window_chunks, overlap or the number of input files; its hap-free columns must be the oracle's from the
input file alone; with one chunk per contig the whole table must be the oracle's with the haplotypes the same run wrote into its phased BAM; the VCF and the BAM must
be the bytes of the run without the option; a failed run leaves no table."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import mods_common as mc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("mods_file")
    rng = np.random.default_rng(77)
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(41, ref_len=12000, depth=12))
    order = ["chr1", "chr2"]
    reads = {k: [mc.add_calls(rng, r) for r in chs[k]["reads"]] for k in order}
    refs = {k: chs[k]["ref"] for k in order}
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    bodies = mc.write_multi_bam_aux(bam, [(k, len(refs[k]), reads[k]) for k in order])
    halves = [str(d / "a.bam"), str(d / "b.bam")]
    for h, path in enumerate(halves):
        mc.write_multi_bam_aux(path, [(k, len(refs[k]), reads[k][h::2]) for k in order])
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in order])
    short = str(d / "short.fa")
    fc.write_multi_fasta(short, [("chr1", refs["chr1"])])
    return dict(dir=d, bam=bam, halves=halves, fa=fa, short=short, refs=refs, order=order, bodies=bodies)


def run(lcd, data, tag, mods=True, bam_out=True, bams=None, **kw):
    vcf, out, tab = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam"), str(data["dir"] / f"{tag}.tsv")
    kw.setdefault("chunk_len", CHUNK_LEN)
    args = dict(vcf_path=vcf, no_vcf_header=1, cfg=cfg_of(lcd), contig_mode=2, bam_out=dict(path=out, pg_line=PG) if bam_out else None, **kw)
    if mods:
        args["mods"] = dict(path=tab) if mods is True else dict(mods, path=tab)
    res = lcd.call_files(bams, data["fa"], **args) if bams else lcd.call_file(data["bam"], data["fa"], **args)
    res["vcf_bytes"] = open(vcf, "rb").read()
    res["bam_bytes"] = open(out, "rb").read() if bam_out else None
    res["table"] = open(tab).read() if mods else None
    return res


@pytest.fixture(scope="module")
def base(lcd, data):
    return run(lcd, data, "base")


def test_the_table_has_phased_rows_and_its_counters(base):
    rows = mc.parse_table(base["table"])
    assert len(rows) > 100 and base["mods"]["n_rows"] == len(rows)
    assert any(r[7] > 0 and r[9] > 0 for r in rows) and any(r[11] > 0 for r in rows) and {r[4] for r in rows} == {"+", "-"} and {r[0] for r in rows} == {"chr1", "chr2"}
    assert rows == sorted(rows, key=lambda r: (r[0], r[1]))                        # plan order, then position
    assert base["mods"]["n_records"] >= base["n_reads"] >= 80 and base["mods"]["n_counted"] == sum(r[5] + r[11] for r in rows)


@pytest.fixture(scope="module")
def yard(lcd, data):
    """per contig lcd_call_bam_regions_ext2 with the contig's planned regions: the chunks' final haplotypes, the contig's table (plain and combined)"""
    contigs = [(k, len(data["refs"][k])) for k in data["order"]]
    plan, _ = lcd.plan_chunks(contigs, contig_mode=2, chunk_len=CHUNK_LEN)
    assert [(t, e - b + 1) for t, b, e in plan] == [(0, 6000)] * 2 + [(1, 6000)] * 2
    out = dict(plan=plan, parts=[])
    for tid, name in enumerate(data["order"]):
        mine = [(b, e) for t, b, e in plan if t == tid]
        part = dict(regs=mine)
        for combine in (False, True):
            tab = str(data["dir"] / f"yard_{name}_{int(combine)}.tsv")
            res = lcd.call_bam_regions(data["bam"], data["bam"] + ".bai", data["fa"], name, [b for b, _ in mine], [e for _, e in mine], min_mapq=30, cfg=cfg_of(lcd),
                                       mods=dict(path=tab, combine_strands=combine))
            part[combine] = dict(text=open(tab).read(), chunks=res["chunks"], stats=res["mods"])
        out["parts"].append(part)
    return out


def test_the_yardstick_is_the_oracle_with_each_chunk_s_own_haplotypes(data, yard):
    flips, shared_differ = [], 0
    for tid, part in enumerate(yard["parts"]):
        name = data["order"][tid]
        for combine in (False, True):
            y = part[combine]
            tabs, n_counted = [], 0
            for (rb, re_), ch in zip(part["regs"], y["chunks"]):
                haps = [int(h) for h in ch["haps"]]
                assert len(haps) == sum(1 for _, r in bo.region_records(data["bodies"], rb, re_, 30, tid) if r >= 0)
                rows, st = mc.pileup(data["bodies"], data["refs"][name], 1, rb, re_, haps, refid=tid, combine=combine)
                tabs.append(rows); n_counted += st["n_counted"]
            assert y["text"] == mc.HEADER + mc.format_rows(mc.merge_rows(tabs), name), (name, combine)
            assert y["stats"]["n_counted"] == n_counted and y["stats"]["n_rows"] == y["text"].count("\n") - 1
        chunks = part[False]["chunks"]
        assert [[int(h) for h in c["haps"]] for c in chunks] == [[int(h) for h in c["haps"]] for c in part[True]["chunks"]]
        flips += [int(c["flip_hap"]) for c in chunks]
        # the reads two neighbouring chunks share: each chunk piles them up with its own array
        kept = [[b for b, r in bo.region_records(data["bodies"], rb, re_, 30, tid) if r >= 0] for rb, re_ in part["regs"]]
        both = {id(b) for b in kept[0]} & {id(b) for b in kept[1]}
        assert len(both) >= 5
        assert all({1, 2} <= {int(h) for h in c["haps"]} for c in chunks)                # phased chunks: both haplotypes present
    print("flips of the yardstick's chunks:", flips)
    assert any(flips), "no chunk of the yardstick had its haplotypes swapped by the stitch: a driver that piled up pre-flip haplotypes would pass"


@pytest.mark.parametrize("combine", [False, True])
def test_four_chunks_equal_the_per_contig_yardstick_in_every_column(lcd, data, yard, base, combine):
    want = mc.HEADER + "".join(p[combine]["text"][len(mc.HEADER):] for p in yard["parts"])
    got = base["table"] if not combine else run(lcd, data, "four_c", mods=dict(combine_strands=True), window_chunks=3)["table"]
    assert got == want
    rows = mc.parse_table(got)
    assert any(r[7] > 0 and r[9] > 0 for r in rows)


@pytest.mark.parametrize("window,overlap", [(1, 0), (1, 1), (4, 0), (4, 1)])
def test_windows_and_overlap_do_not_change_the_table(lcd, data, base, window, overlap):
    got = run(lcd, data, f"w{window}o{overlap}", window_chunks=window, overlap=overlap)
    assert got["table"] == base["table"] and got["vcf_bytes"] == base["vcf_bytes"]


def test_two_input_files_give_the_same_table(lcd, data, base):
    got = run(lcd, data, "two", bams=data["halves"], sort_output=True)
    assert got["n_reads"] == base["n_reads"] and got["vcf_bytes"] == base["vcf_bytes"]
    assert got["table"] == base["table"]


def test_the_other_outputs_are_the_bytes_of_the_run_without_the_option(lcd, data, base):
    plain = run(lcd, data, "plain", mods=False)
    assert "mods" not in plain and plain["vcf_bytes"] == base["vcf_bytes"] and plain["bam_bytes"] == base["bam_bytes"]
    alone = run(lcd, data, "alone", bam_out=False)                                 # the table without an alignment output
    assert alone["table"] == base["table"] and alone["vcf_bytes"] == base["vcf_bytes"]


def _oracle_tables(lcd, data, chunk_len, haps_of=None, **kw):
    contigs = [(k, len(data["refs"][k])) for k in data["order"]]
    plan, _ = lcd.plan_chunks(contigs, contig_mode=2, chunk_len=chunk_len)
    out = []
    for tid, rb, re_ in plan:
        n_kept = sum(1 for _, r in bo.region_records(data["bodies"], rb, re_, 30, tid) if r >= 0)
        haps = haps_of(tid, rb, re_) if haps_of else [0] * n_kept
        rows, _ = mc.pileup(data["bodies"], data["refs"][data["order"][tid]], 1, rb, re_, haps, refid=tid, **kw)
        out.append((data["order"][tid], rows))
    return plan, out


def test_the_hap_free_columns_are_the_oracle_s_from_the_input_alone(lcd, data, base):
    plan, tabs = _oracle_tables(lcd, data, CHUNK_LEN)
    assert len(plan) == 4
    want = [(c, p - 1, p, "m", s, sum(v[0:2]) + sum(v[3:5]) + sum(v[6:8]), v[0] + v[3] + v[6], v[2] + v[5] + v[8]) for c, rows in tabs for p, s, v in rows]
    got = [r[:7] + (r[11],) for r in mc.parse_table(base["table"])]
    assert got == want


def test_one_chunk_per_contig_equals_the_oracle_with_the_haplotypes_of_the_phased_bam(lcd, data):
    got = run(lcd, data, "whole", chunk_len=20000)
    _, bodies = bo.bam_split(b"".join(m["payload"] for m in bo.bgzf_members(got["bam_bytes"])))
    hp = {}
    for b in bodies:
        x = mc.parse_body(b)
        name = b[32:32 + b[8] - 1]
        hp[name] = next((struct.unpack("<i", v)[0] if ty == "i" else v[0] for t, ty, v in mc.aux_walk(x["aux"]) if t == b"HP"), 0)
    assert {1, 2} <= set(hp.values())

    def haps_of(tid, rb, re_):
        return [hp[b[32:32 + b[8] - 1]] for b, r in bo.region_records(data["bodies"], rb, re_, 30, tid) if r >= 0]
    for combine in (False, True):
        _, tabs = _oracle_tables(lcd, data, 20000, haps_of, combine=combine)
        want = mc.HEADER + "".join(mc.format_rows(rows, c) for c, rows in tabs)
        if combine:
            got = run(lcd, data, "whole_c", chunk_len=20000, mods=dict(combine_strands=True))
        assert got["table"] == want


@pytest.mark.parametrize("overlap", [0, 1])
def test_combine_strands_joins_the_rows_of_a_cpg_cut_by_a_chunk_end(lcd, data, base, overlap):
    got = run(lcd, data, f"comb{overlap}", mods=dict(combine_strands=True), window_chunks=1, overlap=overlap)      # (one chunk per window: a held row crosses windows)
    rows = mc.parse_table(got["table"])
    plain = mc.parse_table(base["table"])
    keys = [(r[0], r[1]) for r in rows]
    assert len(set(keys)) == len(keys) and all(r[4] == "." and r[2] == r[1] + 2 for r in rows)
    want = {}
    for r in plain:
        k = (r[0], r[1] if r[4] == "+" else r[1] - 1)
        want[k] = tuple(a + b for a, b in zip(want.get(k, (0,) * 7), r[5:]))
    assert {(r[0], r[1]): r[5:] for r in rows} == want


def test_a_failed_run_leaves_no_table(lcd, data):
    tab = str(data["dir"] / "fail.tsv")
    with pytest.raises(lcd.LcdError, match="no reference sequence|chr2"):            # the FASTA lacks chr2: the run fails at the load stage, after its outputs were created
        lcd.call_file(data["bam"], data["short"], chunk_len=CHUNK_LEN, contig_mode=2, vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), mods=dict(path=tab))
    assert not os.path.exists(tab)
    for bad in (dict(code="a"), dict(threshold=100), dict(threshold=256)):
        with pytest.raises(lcd.LcdError, match="code must be m or h"):
            lcd.call_file(data["bam"], data["fa"], vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), mods=dict(bad, path=tab))
        assert not os.path.exists(tab)
    with pytest.raises(lcd.LcdError, match="goes to a file"):
        lcd.call_file(data["bam"], data["fa"], vcf_path=str(data["dir"] / "fail.vcf"), cfg=cfg_of(lcd), mods=dict(path="-"))


def test_a_run_whose_vcf_cannot_be_closed_leaves_no_table(lcd, data):
    """the table is finished after the other outputs: a VCF on a full device fails when it is flushed -- at its close for a text this short -- and the table, complete
    by then, is removed with the run"""
    if not os.path.exists("/dev/full"):
        pytest.fail("/dev/full is needed to make the VCF's close fail")
    tab = str(data["dir"] / "full.tsv")
    with pytest.raises(lcd.LcdError, match="/dev/full"):
        lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, contig_mode=2, regions=["chr2:1-3000"], vcf_path="/dev/full", no_vcf_header=1, cfg=cfg_of(lcd), mods=dict(path=tab))
    assert not os.path.exists(tab)
    ok = lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, contig_mode=2, regions=["chr2:1-3000"], vcf_path=str(data["dir"] / "part.vcf"), no_vcf_header=1, cfg=cfg_of(lcd),
                       mods=dict(path=tab))
    assert os.path.exists(tab) and ok["mods"]["n_rows"] > 0 and 0 < ok["n_vcf_lines"] and os.path.getsize(str(data["dir"] / "part.vcf")) < 4096


def test_the_command_line(data, base):
    env = dict(os.environ, PYTHONPATH=ROOT)
    tab, vcf = str(data["dir"] / "cli.tsv"), str(data["dir"] / "cli.vcf")
    r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", "call", data["fa"], data["bam"], "--all-ctg", "-H", "-o", vcf, "--chunk-len", str(CHUNK_LEN), "--mods", tab],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tab).read() == base["table"] and open(vcf, "rb").read() == base["vcf_bytes"]
    assert f"{len(mc.parse_table(base['table']))} methylation rows" in r.stderr
