"""The .bai rules without a device: the host finisher lcd_bai_from_records against the pure-Python oracle of tests/bai_common.py, byte for byte, on every named case
and on 20 seeded record tables; region queries through the product's index against a linear scan, through the oracle's reader and through the project's own
lcd_bam_load_region_indexed; the pin against the index samtools wrote for the reference's bundled test BAM (from the checkout where it exists, and from the
committed fixture tests/golden/bai_hg002.npz everywhere); the ABI of the new exports and the command line's new spellings."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bai_common as bc
from conftest import ROOT

REF_BAM = "/root/reference/test_data/HG002_chr11_hifi_test.bam"
FIXTURE = os.path.join(ROOT, "tests", "golden", "bai_hg002.npz")
NEW = ["lcd_bai_from_records", "lcd_bai_builder_create", "lcd_bai_builder_add_stream", "lcd_bai_builder_finish", "lcd_bai_builder_bytes", "lcd_bai_builder_destroy",
       "lcd_bai_build", "lcd_fai_build", "lcd_bam_writer_open", "lcd_call_files"]


@pytest.fixture(scope="module")
def seeded():
    """the 20 seeded files, scanned once: (bam bytes, scan)"""
    out = []
    for s in bc.SEEDS:
        bam = bc.seeded_bam(s)
        out.append((bam, bc.scan_bam(bam)))
    return out


@pytest.mark.parametrize("name", list(bc.CASES))
def test_named_case_is_reached_and_the_finisher_equals_the_oracle(lcd, name):
    bam, pred, refused = bc.CASES[name]()
    s = bc.scan_bam(bam)
    arrays = bc.table_arrays(s["recs"])
    if refused is not None:
        with pytest.raises(bc.BaiRefused) as e:
            bc.oracle_bai(len(s["refs"]), s["recs"])
        assert (e.value.code, e.value.recno) == refused                                  # the oracle itself proves that the case is reached
        with pytest.raises(lcd.LcdError) as pe:
            lcd.bai_from_records(len(s["refs"]), *arrays)
        assert f"error {refused[0]}:" in str(pe.value) and f"record {refused[1]} " in str(pe.value)
        if refused[0] == bc.ERR_CSI:
            assert "only BAI is supported, not CSI" in str(pe.value)
        return
    want = bc.oracle_bai(len(s["refs"]), s["recs"])
    assert pred(s, bc.parse_bai(want)), "the case is not reached"
    assert lcd.bai_from_records(len(s["refs"]), *arrays) == want


def test_seeded_tables_equal_the_oracle(lcd, seeded):
    for bam, s in seeded:
        assert len(s["recs"]) == 305 and sum(1 for x in s["recs"] if x["tid"] < 0) == 5
        want = bc.oracle_bai(len(s["refs"]), s["recs"])
        idx = bc.parse_bai(want)
        assert idx["n_no_coor"] == 5 and idx["refs"][1]["n_bin"] == 0 and all(idx["refs"][t]["n_bin"] > 1 for t in (0, 2, 3))
        assert any(len(ch) > 1 for r in idx["refs"] for ch in r["bins"].values())        # some bin has more than one chunk
        assert lcd.bai_from_records(len(s["refs"]), *bc.table_arrays(s["recs"])) == want


def _regions(seed, refs):
    rng = np.random.default_rng(1000 + seed)
    return [(t, b, e) for t in (0, 2, 3) for (b, e) in bc.regions_for(rng, refs, t, 68)] + [(1, 0, refs[1][1]), (1, 5, 6)]


def test_queries_through_the_products_index_equal_a_linear_scan(lcd, seeded):
    for seed, (bam, s) in zip(bc.SEEDS, seeded):
        idx = bc.parse_bai(lcd.bai_from_records(len(s["refs"]), *bc.table_arrays(s["recs"])))
        regs = _regions(seed, s["refs"])
        assert len(regs) >= 200
        hit = 0
        for t, b, e in regs:
            want = bc.records_by_scan(s, t, b, e)
            assert bc.records_through_index(s, idx, t, b, e) == want, (seed, t, b, e)
            hit += bool(want)
        assert 2 * hit >= len(regs), (seed, hit, len(regs))                              # at least half of the regions of every file are non-empty


def test_queries_through_the_projects_reader(lcd, seeded, tmp_path):
    from longcalld_amd._lib import LcdBamReads
    lib = lcd.load_library()
    lib.lcd_bam_load_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_bam_load_region_indexed.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_bam_reads_free.argtypes = [C.POINTER(LcdBamReads)]
    lib.lcd_io_last_error.restype = C.c_char_p

    def names(r, n):
        return [C.string_at(C.addressof(r.name_pool.contents) + r.name_off[i]).decode() for i in range(n)]
    for seed, (bam, s) in zip(bc.SEEDS, seeded):
        path = str(tmp_path / f"s{seed}.bam")
        open(path, "wb").write(bam)
        open(path + ".bai", "wb").write(lcd.bai_from_records(len(s["refs"]), *bc.table_arrays(s["recs"])))
        for t, b, e in _regions(seed, s["refs"]):
            a, q = LcdBamReads(), LcdBamReads()
            chrom = s["refs"][t][0].encode()
            n = lib.lcd_bam_load_region(path.encode(), chrom, b + 1, e, 0, 1, C.byref(a))
            m = lib.lcd_bam_load_region_indexed(path.encode(), (path + ".bai").encode(), chrom, b + 1, e, 0, C.byref(q))
            assert n >= 0 and m == n, (seed, t, b, e, lib.lcd_io_last_error())
            want = [s["recs"][i]["name"] for i in bc.records_by_scan(s, t, b, e) if not s["recs"][i]["flag"] & (4 | 256 | 2048)]
            assert names(a, n) == want and names(q, m) == want, (seed, t, b, e)
            lib.lcd_bam_reads_free(C.byref(a)); lib.lcd_bam_reads_free(C.byref(q))


# ---- the pin against htslib's output ----
def _compare_with_samtools(scan_recs, n_ref, ours_bytes, theirs_bytes, ref_lens):
    ours, theirs = bc.parse_bai(ours_bytes), bc.parse_bai(theirs_bytes)
    assert len(ours["refs"]) == len(theirs["refs"]) == n_ref
    assert theirs["n_no_coor"] is None or ours["n_no_coor"] == theirs["n_no_coor"]
    for a, b in zip(ours["refs"], theirs["refs"]):
        assert (a["meta"] is None) == (b["meta"] is None)
        if a["meta"]:
            assert a["meta"] == b["meta"]                                                # n_mapped, n_unmapped, off_beg, off_end
    s = dict(recs=scan_recs)
    rng = np.random.default_rng(7)
    t = max(range(n_ref), key=lambda k: sum(1 for x in scan_recs if x["tid"] == k))
    first, last = min(x["pos"] for x in scan_recs if x["tid"] == t), max(x["end"] for x in scan_recs if x["tid"] == t)
    hit = 0
    for _ in range(500):
        b = int(rng.integers(max(0, first - 20000), last + 20000)); e = min(ref_lens[t], b + int(rng.integers(1, 50000)))
        if e <= b:
            continue
        want = bc.records_by_scan(s, t, b, e)
        assert bc.records_through_index(s, ours, t, b, e) == want and bc.records_through_index(s, theirs, t, b, e) == want, (b, e)
        hit += bool(want)
    assert hit > 100


@pytest.mark.skipif(not os.path.exists(REF_BAM), reason="the reference's bundled test BAM exists in the build container only")
def test_oracle_index_of_the_bundled_bam_against_samtools():
    s = bc.scan_bam(open(REF_BAM, "rb").read())
    ours = bc.oracle_bai(len(s["refs"]), s["recs"])
    _compare_with_samtools(s["recs"], len(s["refs"]), ours, open(REF_BAM + ".bai", "rb").read(), [l for _n, l in s["refs"]])


def test_finisher_on_the_committed_record_table_against_samtools(lcd):
    z = np.load(FIXTURE)
    recs = [dict(tid=int(a), pos=int(b), end=int(c), flag=int(d), vbeg=int(e), vend=int(f)) for a, b, c, d, e, f in
            zip(z["tid"], z["pos"], z["end"], z["flag"], z["vbeg"], z["vend"])]
    # the committed offsets are the ones rule 5 gives on the committed member table
    tab = [tuple(int(v) for v in row) for row in z["members"]]
    assert [bc.voff(tab, int(z["fsize"]), int(u)) for u in z["u0"][:50]] == [r["vbeg"] for r in recs[:50]]
    ours = lcd.bai_from_records(int(z["n_ref"]), z["tid"], z["pos"], z["end"], z["flag"], z["vbeg"], z["vend"])
    assert ours == bc.oracle_bai(int(z["n_ref"]), recs)
    _compare_with_samtools(recs, int(z["n_ref"]), ours, z["samtools_bai"].tobytes(), [int(v) for v in z["ref_lens"]])


# ---- ABI and command line ----
def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib, align
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    for mirror in ("bai_build", "bai_from_records", "fai_build"):
        assert callable(getattr(align, mirror))
    import inspect
    assert inspect.signature(align.call_file).parameters["index"].default is None


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    from longcalld_amd import _lib
    exe = str(tmp_path / "index_abi")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "index_abi.c"), "-o", exe])
    want = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    mirrors = {"lcd_bai_member_t": _lib.LcdBaiMember, "lcd_bai_opt_t": _lib.LcdBaiOpt, "lcd_bai_stats_t": _lib.LcdBaiStats, "lcd_index_opt_t": _lib.LcdIndexOpt,
               "lcd_index_stats_t": _lib.LcdIndexStats}
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == int(want[name]), name
        fields = [k.split(".")[1] for k in want if k.startswith(name + ".")]
        assert fields == [f[0] for f in cls._fields_], name
        for f in fields:
            assert getattr(cls, f).offset == int(want[f"{name}.{f}"]), (name, f)
    assert (_lib.LCD_ERR_BAI_ORDER, _lib.LCD_ERR_BAI_CSI, _lib.LCD_ERR_FAI_FORMAT, _lib.LCD_ERR_BAI_CONTIG) == tuple(
        int(want[k]) for k in ("LCD_ERR_BAI_ORDER", "LCD_ERR_BAI_CSI", "LCD_ERR_FAI_FORMAT", "LCD_ERR_BAI_CONTIG"))


def test_c_round_trip(lcd, tmp_path):
    exe, fa = str(tmp_path / "index_roundtrip"), str(tmp_path / "r.fa")
    libdir = os.path.join(ROOT, "longcalld_amd")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "index_roundtrip.c"), "-L", libdir, "-llcd_hotpath",
                           "-Wl,-rpath," + libdir, "-o", exe])
    open(fa, "w").write(">a x\nACGT\nAC\n>b\nGG\n")
    out = dict(l.split(" ", 1) for l in subprocess.check_output([exe, fa], text=True).splitlines())
    recs = [dict(tid=0, pos=100, end=150, flag=0, vbeg=(98 << 16) | 7, vend=(98 << 16) | 300), dict(tid=0, pos=20000, end=20001, flag=4, vbeg=(98 << 16) | 300, vend=400 << 16)]
    want = bc.oracle_bai(2, recs)
    assert out["rc"] == f"0 n {len(want)}" and bytes.fromhex(out["bytes"]) == want
    assert out["refused"].startswith("-50 ") and "record 1 " in out["refused"]
    assert out["fai"] == "2" and open(fa + ".fai").read() == "a\t6\t5\t4\t5\nb\t2\t16\t2\t3\n"


def test_host_exports_refuse_bad_arguments(lcd):
    lib = lcd.load_library()
    assert lib.lcd_bai_from_records(1, 1, None, None, None, None, None, None, None, None) == -4
    assert lib.lcd_fai_build(None, None) == -4
    assert lib.lcd_bai_build(None, None, None, None) == -4
    assert lib.lcd_bai_builder_add_stream(None, 0, 0, 0, 0, None, 0, None) == -4 and lib.lcd_bai_builder_finish(None, None) == -4
    from longcalld_amd import _lib
    ist = _lib.LcdIndexStats()
    wo = _lib.LcdWriterOpt(write_index=1, idx_stats=C.pointer(ist))
    assert not lib.lcd_bam_writer_open(None, None, C.byref(wo))
    io = _lib.LcdIndexOpt()
    ro, out = _lib.LcdRunOpt(idx=C.pointer(io)), _lib.LcdRunOut(idx_stats=C.pointer(ist))
    assert lib.lcd_call_files(None, None, None, C.byref(ro), None, C.byref(out)) == -4


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def test_cli_parses_the_new_spellings(tmp_path):
    from longcalld_amd import cli as m
    o, pos = m.parse(["--make-index", "-o", "x.vcf", "ref.fa", "in.bam"])
    assert "--make-index" in o["flags"] and pos == ["ref.fa", "in.bam"]
    assert "--make-index" not in m.parse(["ref.fa", "in.bam"])[0]["flags"]
    assert m.parse_index(["index", "in.bam"]) == ("index", ["in.bam"]) and m.parse_index(["index", "in.bam", "o.bai"]) == ("index", ["in.bam", "o.bai"])
    assert m.parse_index(["faidx", "ref.fa"]) == ("faidx", ["ref.fa"])
    assert m.parse_index(["index"]) == 2 and m.parse_index(["faidx", "a", "b"]) == 2 and m.parse_index(["index", "--fast", "in.bam"]) == 2
    assert "--make-index" in m.USAGE and "index in.bam [out.bai]" in m.USAGE and "faidx ref.fa" in m.USAGE
    r = cli("sort", "in.bam")                                                            # anything else is still refused
    assert r.returncode == 2 and "unknown command sort" in r.stderr
    fa = str(tmp_path / "c.fa")
    open(fa, "w").write(">s1\nACGTACGT\nACG\n")
    r = cli("faidx", fa)                                                                 # host code: runs without a device
    assert r.returncode == 0 and open(fa + ".fai").read() == "s1\t11\t4\t8\t9\n"
    assert cli("faidx", str(tmp_path / "absent.fa")).returncode == 1
