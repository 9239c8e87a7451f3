"""lcd_call_files on the MI355X: one sample from two BAMs (a contig's reads with even index in file A, the odd ones in file B, records the loader filters over every
chunk border in both) and a FASTA to one VCF and one phased BAM.  Records, VCF body, flips and n_passes against the composition of the oracles
(tests/call_chunks_common.py::oracle_call, the composition that pins lcd_call_bam_regions) on the planned chunks with their reads in file-major order; the output
BAM against the HP / PS rewrite of tests/bam_out_common.py applied through the Python plan of tests/multi_bam_common.py (rules 4 and 5)."""
import os
import shutil

import numpy as np
import pytest

import bai_common as bc
import bam_out_common as bo
import call_chunks_common as kc
import call_file_common as fc
import multi_bam_common as mb
from test_gpu_call_chunks import need_ref

pytestmark = pytest.mark.gpu

CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
EOF_MEMBER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HEADER_ARGS = dict(source_version="test-1", cmdline="call ref.fa in.bam", date_yyyymmdd="20240102")
ORDER = ["chr1", "chr2", "chr4"]


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


def inflated(path):
    return b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read()))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """chr1 / chr2: the seeded 12 kb contigs, dealt out to A and B; chr4: 12 kb without a read.  A carries @RG SM, B does not"""
    d = tmp_path_factory.mktemp("call_files")
    chs = {k: v for k, v in mb.seeded_contigs().items() if k in ("chr1", "chr2")}
    refs = dict({k: v["ref"] for k, v in chs.items()}, chr4=np.random.default_rng(4).integers(0, 4, 12000).astype(np.uint8))
    files = {k: mb.deal(chs[k]["reads"], k, 2, borders=[6000]) for k in chs}
    files["chr4"] = [[], []]
    a, b, fa = str(d / "a.bam"), str(d / "b.bam"), str(d / "ref.fa")
    bodies = {}
    for f, (path, text) in enumerate(((a, fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n"), (b, fc.DEFAULT_HEADER))):
        for body in mb.write_bam(path, [(k, len(refs[k]), files[k][f]) for k in ORDER], header_text=text, block=30000 if f == 0 else 11000):
            bodies[bo.parse(body)["name"].decode()] = body
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in ORDER])
    return dict(dir=d, a=a, b=b, fa=fa, refs=refs, files=files, bodies=bodies, contigs=[(k, len(refs[k])) for k in ORDER], header_a=bo.bam_split(inflated(a))[0])


@pytest.fixture(scope="module")
def want(lcd, oracle, data):
    """the oracle composition per contig on the planned chunks: reads = the file-major concatenation (rule 1), orders = kc.python_order"""
    need_ref(oracle)
    out = dict(records=[], text="", flips=[], n_passes=[], n_records=[], chunks=[])
    for tid, name in enumerate(ORDER):
        regs = mb.regions_of(len(data["refs"][name]), CHUNK_LEN)
        tabs = [mb.chunk_table(data["files"][name], rb, re_) for rb, re_ in regs]
        if name == "chr4":
            for (rb, re_), (rows, reads) in zip(regs, tabs):
                assert not rows
                out["flips"].append((0, -1, -1)); out["n_passes"].append(None); out["n_records"].append(0)
                out["chunks"].append(dict(tid=tid, reg=(rb, re_), rows=rows, reads=reads, names=[], order=[], haps=[], phase_sets=[]))
            continue
        chs = [dict(reads=reads, ref=data["refs"][name], ref_beg=1, reg_beg=rb, reg_end=re_, whole_ref_len=len(data["refs"][name]), is_ont=0) for (rb, re_), (_, reads) in zip(regs, tabs)]
        orders = [kc.python_order([r["pos0"] for r in ch["reads"]], [kc.read_end(r) for r in ch["reads"]], [0] * len(ch["reads"]), [r["name"] for r in ch["reads"]]) for ch in chs]
        res = kc.oracle_call(lcd, oracle, chs, max_len=kc.TWO_CHUNK_MAX_LEN, orders=orders)
        out["records"] += res["records"]
        out["text"] += "".join(name + l[len("chr11"):] + "\n" for l in res["vcf_body"].splitlines())
        for (rb, re_), (rows, reads), f, o in zip(regs, tabs, res["chunks"], orders):
            out["flips"].append(tuple(int(x) for x in f["flip"])); out["n_passes"].append(f["n_passes"]); out["n_records"].append(f["n_records"])
            out["chunks"].append(dict(tid=tid, reg=(rb, re_), rows=rows, reads=reads, names=[r["name"] for r in reads], order=o.tolist(),
                                      haps=np.asarray(f["state"]["haps"]).tolist(), phase_sets=np.asarray(f["state"]["phase_sets"]).tolist()))
    return out


def expected_bodies(data, want, sort_output):
    """the output BAM's record stream: per chunk the Python plan over its table, every written record through the rewrite oracle"""
    out = []
    for c, ch in enumerate(want["chunks"]):
        prev = want["chunks"][c - 1] if c > 0 and want["chunks"][c - 1]["tid"] == ch["tid"] else None
        skip, order = mb.python_plan(ch["rows"], prev is not None, *(prev["reg"] if prev else (0, 0)), sort_output)
        name = ORDER[ch["tid"]]
        for i in order:
            r = ch["rows"][i]
            body = data["bodies"][data["files"][name][r["file"]][r["idx"]]["name"]]
            k = r["read"]
            out.append(bo.tag_record(body, k >= 0, ch["haps"][k] if k >= 0 else 0, ch["phase_sets"][k] if k >= 0 else 0))
    return out


def run(lcd, data, tag, bams=None, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
    kw.setdefault("no_vcf_header", 1)
    res = lcd.call_files(bams or [data["a"], data["b"]], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), keep_records=True, **kw)
    res["text"] = open(vcf).read()
    res["vcf"], res["bam"] = vcf, out
    image = open(out, "rb").read()
    assert image.endswith(EOF_MEMBER)
    members = bo.bgzf_members(image)
    assert sum(1 for m in members if m["isize"] == 0) == 1                           # ONE EOF member, at the end
    res["bam_header"], res["bam_bodies"] = bo.bam_split(b"".join(m["payload"] for m in members))
    return res


@pytest.fixture(scope="module")
def merged(lcd, data, want):
    return run(lcd, data, "merged", window_chunks=2, overlap=0)


def test_the_oracle_side_takes_every_branch(want):
    print("flips:", want["flips"], "n_passes:", want["n_passes"], "records per chunk:", want["n_records"])
    assert any(f[0] == 1 for f in want["flips"])                                     # a chunk whose haplotypes were swapped
    assert any(f[1] > 0 and f[0] == 0 for f in want["flips"])                        # one joined as it is
    assert want["flips"][0] == want["flips"][2] == want["flips"][4] == (0, -1, -1)
    n_a = sum(1 for ch in want["chunks"] for r in ch["rows"] if r["file"] == 0 and r["read"] >= 0); n_b = sum(1 for ch in want["chunks"] for r in ch["rows"] if r["file"] == 1 and r["read"] >= 0)
    assert n_a > 50 and n_b > 50 and len(want["records"]) > 15
    for ch in want["chunks"][:4]:                                                    # file-major tables in which both files reach over the border behind them
        assert [r["file"] for r in ch["rows"]] == sorted(r["file"] for r in ch["rows"]) and {r["file"] for r in ch["rows"]} == {0, 1}
        assert sum(1 for r in ch["rows"] if r["read"] < 0) == 4                      # the secondary and the low-MAPQ copy of each file


def test_results_equal_the_oracle_composition(merged, want):
    got = merged
    assert got["n_planned"] == 6 == len(got["chunks"]) and got["n_windows"] == 3 and got["n_region_loads"] == 6 and got["n_empty"] == 2
    assert [(c["flip_hap"], c["flip_pre_PS"], c["flip_cur_PS"]) for c in got["chunks"]] == want["flips"]
    assert [c["n_passes"] for c in got["chunks"]][:4] == want["n_passes"][:4] and [c["n_records"] for c in got["chunks"]] == want["n_records"]
    assert len(got["records"]) == len(want["records"])
    for x, y in zip(got["records"], want["records"]):
        assert x == y, (x, y)
    assert got["text"] == want["text"] and got["n_vcf_lines"] == want["text"].count("\n")
    assert [c["n_reads"] for c in got["chunks"]] == [len(ch["reads"]) for ch in want["chunks"]]
    n_a = sum(1 for ch in want["chunks"] for r in ch["rows"] if r["file"] == 0 and r["read"] >= 0)
    assert got["n_reads_per_file"] == [n_a, got["n_reads"] - n_a] and got["n_reads"] == sum(len(ch["reads"]) for ch in want["chunks"])


def test_chunk_reads_and_their_order(lcd, data, want):
    """the chunk behind every planned region: read ids file-major, ordered_read_ids = sort_chunk_reads' order on them"""
    for ch in want["chunks"][:4]:
        c = lcd.chunk_open_from_bams([data["a"], data["b"]], None, ORDER[ch["tid"]], *ch["reg"], min_mapq=30)
        try:
            assert c.meta["names"] == ch["names"] and c.file_of_read.tolist() == [r["file"] for r in ch["rows"] if r["read"] >= 0]
            c.resolve((data["refs"][ORDER[ch["tid"]]], 1, 12000, 0))
            nm = lcd.chunk_read_nm(c)
            assert not nm.any()
            assert lcd.sort_chunk_reads(c.meta["pos0"], c.meta["end_pos"], nm, c.meta["names"]).tolist() == ch["order"]
        finally:
            c.close()


def test_bam_output_is_the_plan_over_the_rewrite(merged, data, want):
    got = merged
    exp = expected_bodies(data, want, 0)
    assert got["bam_bodies"] == exp
    assert got["bam_header"] == bo.header_with_pg(data["header_a"], PG.encode())                  # file 0's header plus @PG
    assert got["bam_out"]["n_records_out"] + got["bam_out"]["n_filtered_out"] == len(exp) and got["bam_out"]["n_filtered_out"] == 8
    names = sorted(bo.parse(b)["name"].decode() for b in got["bam_bodies"])
    assert names == sorted(data["bodies"])                                                        # every input record exactly once
    pos = [(bo.parse(b)["refid"], bo.parse(b)["pos0"]) for b in got["bam_bodies"]]
    assert pos != sorted(pos)                                                                     # the merged output is not coordinate-sorted
    assert any(b"HP" in b[bo.parse(b)["aux0"]:] for b in got["bam_bodies"])


def test_sorted_output_and_its_index(lcd, data, want, merged):
    got = run(lcd, data, "sorted", sort_output=True, window_chunks=0, overlap=0, index=dict(write_out_bai=1))
    assert got["bam_bodies"] == expected_bodies(data, want, 1)
    pos = [(bo.parse(b)["refid"], bo.parse(b)["pos0"]) for b in got["bam_bodies"]]
    assert pos == sorted(pos) and sorted(got["bam_bodies"]) == sorted(merged["bam_bodies"])
    assert got["text"] == merged["text"]
    assert got["index"]["wrote_out_bai"] == 1 and got["index"]["out_bai_skipped"] == 0
    s = bc.scan_bam(open(got["bam"], "rb").read())
    assert open(got["bam"] + ".bai", "rb").read() == bc.oracle_bai(len(s["refs"]), s["recs"])


def test_unsorted_output_completes_without_an_index(lcd, data, merged):
    from longcalld_amd import _lib
    got = run(lcd, data, "unsorted_idx", window_chunks=0, overlap=0, index=dict(write_out_bai=1))
    assert got["index"]["out_bai_skipped"] == _lib.LCD_ERR_BAI_ORDER and got["index"]["wrote_out_bai"] == 0 and got["index"]["out_bai_skip_reason"]
    assert got["bam_bodies"] == merged["bam_bodies"] and not os.path.exists(got["bam"] + ".bai")   # (run() checked the one EOF member)


@pytest.mark.parametrize("window,overlap", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_every_schedule_gives_the_same_files(lcd, data, merged, window, overlap):
    got = run(lcd, data, f"w{window}o{overlap}", window_chunks=window, overlap=overlap)
    assert got["text"] == merged["text"] and got["bam_bodies"] == merged["bam_bodies"] and got["bam_header"] == merged["bam_header"]
    assert got["records"] == merged["records"] and got["n_reads_per_file"] == merged["n_reads_per_file"]


def test_one_input_is_lcd_call_file_byte_for_byte(lcd, data):
    outs = {}
    for tag, fn, bam in (("one_files", lcd.call_files, [data["a"]]), ("one_file", lcd.call_file, data["a"])):
        vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
        st = fn(bam, data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), index=dict(write_out_bai=1), window_chunks=2, **HEADER_ARGS)
        assert st["index"]["wrote_out_bai"] == 1
        outs[tag] = (open(vcf, "rb").read(), open(out, "rb").read(), open(out + ".bai", "rb").read(), st["n_reads"], st["n_records"])
        if tag == "one_files":
            assert st["n_reads_per_file"] == [st["n_reads"]]
    assert outs["one_files"] == outs["one_file"] and len(outs["one_file"][0]) > 1000 and len(outs["one_file"][1]) > 10000


def test_header_mismatch_missing_and_built_indexes(lcd, data, merged, tmp_path):
    from longcalld_amd import _lib
    d = tmp_path
    a, b = str(d / "a.bam"), str(d / "b.bam")
    for src, dst in ((data["a"], a), (data["b"], b)):
        shutil.copy(src, dst); shutil.copy(src + ".bai", dst + ".bai")
    # B with one contig length changed: -54, no output file is created
    bad = str(d / "bad.bam")
    mb.write_bam(bad, [(k, 12000 if k != "chr2" else 12001, data["files"][k][1]) for k in ORDER])
    vcf, out = str(d / "o.vcf"), str(d / "o.bam")
    with pytest.raises(lcd.LcdError, match=r"-54.*bad\.bam.*entry 1 is chr2 \(12001\)"):
        lcd.call_files([a, bad], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out), cfg=cfg_of(lcd))
    assert _lib.LCD_ERR_INPUT_HEADERS == -54 and not os.path.exists(vcf) and not os.path.exists(out)
    # B.bai missing: -30 naming it; with build_missing_bai it is built, A.bai stays byte for byte, and the run equals the indexed one
    os.remove(b + ".bai")
    a_bai = open(a + ".bai", "rb").read()
    with pytest.raises(lcd.LcdError, match="-30.*b.bam.bai"):
        lcd.call_files([a, b], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, cfg=cfg_of(lcd))
    assert not os.path.exists(vcf)
    st = lcd.call_files([a, b], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), no_vcf_header=1, window_chunks=2,
                        index=dict(build_missing_bai=1))
    assert st["index"]["built_bai"] == 1 and os.path.exists(b + ".bai") and open(a + ".bai", "rb").read() == a_bai
    assert open(vcf).read() == merged["text"] and bo.bam_split(inflated(out))[1] == merged["bam_bodies"]


def test_sample_name(lcd, data):
    from test_gpu_call_file import header_text
    def head(bams, tag):
        vcf = str(data["dir"] / f"{tag}.vcf")
        lcd.call_files(bams, data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, cfg=cfg_of(lcd), regions=["chr4"], **HEADER_ARGS)
        return open(vcf).read()
    assert head([data["a"], data["b"]], "sm_a") == header_text(lcd, data["contigs"], "sample7")              # @RG SM in A only
    assert head([data["b"], data["a"]], "sm_ba") == header_text(lcd, data["contigs"], data["b"] + "," + data["a"])   # file 0 decides: no SM there, the paths joined
    nosm = str(data["dir"] / "nosm.bam")
    shutil.copy(data["b"], nosm); shutil.copy(data["b"] + ".bai", nosm + ".bai")
    t = head([data["b"], nosm], "sm_none")
    assert t == header_text(lcd, data["contigs"], data["b"] + "," + nosm) and t.splitlines()[-1].endswith("\t" + data["b"] + "," + nosm)
