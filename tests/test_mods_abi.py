"""The methylation table's entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported; the structs mirror the header as a C compiler
lays them out (tests/c/mods_abi.c); lcd_run_ext2_t starts with its own size and the older structs keep theirs; the host-only entry points and every refusal of the
device ones come back without a device (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

from conftest import ROOT

NEW = ["lcd_mods_opt_default", "lcd_mods_opt_check", "lcd_chunk_mod_pileup", "lcd_mods_n_rows", "lcd_mods_rows_to_host", "lcd_mods_free", "lcd_mods_combine_rows", "lcd_mods_format",
       "lcd_call_files_ext2", "lcd_call_bam_regions_ext2"]


def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def test_structs_mirror_the_header(tmp_path):
    from longcalld_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no host C compiler (the project's own build needs one)"
    exe = str(tmp_path / "mods_abi")
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "mods_abi.c"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    for name, T in (("lcd_mods_opt_t", _lib.LcdModsOpt), ("lcd_mods_stats_t", _lib.LcdModsStats), ("lcd_run_ext2_t", _lib.LcdRunExt2), ("lcd_run_ext_t", _lib.LcdRunExt),
                    ("lcd_run_opt_t", _lib.LcdRunOpt), ("lcd_run_out_t", _lib.LcdRunOut)):
        assert got[name] == C.sizeof(T), name
        for k, v in got.items():
            if k.startswith(name + "."):
                assert getattr(T, k.split(".")[1]).offset == v, k
    # the size-first rule, and the pinned sizes of the structs that came before
    assert got["lcd_run_ext2_t.size"] == 0 and _lib.LcdRunExt2._fields_[0] == ("size", C.c_size_t)
    assert (got["lcd_run_ext_t"], got["lcd_run_opt_t"], got["lcd_run_out_t"]) == (16, 24, 40)
    txt = open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read()
    m = re.search(r"typedef struct lcd_mods_stats_t \{(.*?)\} lcd_mods_stats_t;", txt, re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1)) == [f[0] for f in _lib.LcdModsStats._fields_]


def test_host_only_entry_points():
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    o = _lib.LcdModsOpt(); lib.lcd_mods_opt_default(C.byref(o))
    assert (o.code, o.threshold, o.combine_strands, o.ref_seq) == (ord("m"), 204, 0, None) and lib.lcd_mods_opt_check(C.byref(o)) == 0
    for code, thr, want in ((ord("h"), 128, 0), (ord("h"), 255, 0), (ord("a"), 204, -4), (0, 204, -4), (ord("m"), 127, -4), (ord("m"), 256, -4)):
        o.code, o.threshold = code, thr
        assert lib.lcd_mods_opt_check(C.byref(o)) == want, (code, thr)
    assert lib.lcd_mods_opt_check(None) == -4
    rows = [(1001, "-", (0, 0, 0, 1, 0, 0, 0, 0, 0)), (1200, "+", (1, 2, 3, 4, 5, 6, 7, 8, 9)), (1201, "-", (1, 0, 0, 0, 0, 0, 0, 0, 1))]
    assert align.mods_format(rows[:2], "chrS", "m", with_header=True) == ("#chrom\tstart\tend\tcode\tstrand\tn_all\tmod_all\tn_h1\tmod_h1\tn_h2\tmod_h2\tn_filtered\n"
                                                                          "chrS\t1000\t1001\tm\t-\t1\t1\t1\t1\t0\t0\t0\n" "chrS\t1199\t1200\tm\t+\t27\t12\t9\t4\t15\t7\t18\n")
    assert align.mods_format([], "c", "h", with_header=False) == ""
    assert align.mods_combine_rows(rows) == [(1000, ".", rows[0][2]), (1200, ".", (2, 2, 3, 4, 5, 6, 7, 8, 10))]
    assert align.mods_format([(7, ".", (0,) * 8 + (1,))], "c", "h") == "c\t6\t8\th\t.\t0\t0\t0\t0\t0\t0\t1\n"
    text = C.c_void_p(1)
    assert lib.lcd_mods_format(1, None, None, None, b"c", ord("m"), 0, C.byref(text)) == -4 and not text.value
    assert lib.lcd_mods_format(0, None, None, None, b"c", ord("x"), 0, C.byref(text)) == -4 and lib.lcd_mods_format(0, None, None, None, None, ord("m"), 0, C.byref(text)) == -4
    assert lib.lcd_mods_combine_rows(1, None, None, None) == -4 and lib.lcd_mods_combine_rows(-1, None, None, None) == -4 and lib.lcd_mods_combine_rows(0, None, None, None) == 0


def test_the_device_entry_points_refuse_without_a_device():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    st = _lib.LcdModsStats(); st.n_records = 7
    o = _lib.LcdModsOpt(); lib.lcd_mods_opt_default(C.byref(o))
    assert not lib.lcd_chunk_mod_pileup(None, None, C.byref(o), C.byref(st)) and b"not made from a BAM" in lib.lcd_last_error() and st.n_records == 0
    assert lib.lcd_mods_n_rows(None) == 0 and lib.lcd_mods_rows_to_host(None, None, None, None) == -4
    lib.lcd_mods_free(None)


def test_the_file_driver_keeps_its_refusals_and_gains_the_new_ones(tmp_path):
    """lcd_call_files_ext refuses and accepts what it did; lcd_call_files_ext2 with a NULL struct is that call; a size that does not reach the first option, a bad
    code / threshold and a table on stdout are -4 before a file is created; a struct LONGER than the library's is read as far as the library knows it"""
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.bam_path, job.fasta_path, job.vcf_path = b"missing_in.bam", b"missing_ref.fa", str(tmp_path / "o.vcf").encode()
    st = _lib.LcdFileStats()
    tab = str(tmp_path / "t.tsv").encode()
    base = (None, C.byref(job), C.byref(cfg), None, C.byref(st), None)
    assert lib.lcd_call_files_ext(*base, None) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert lib.lcd_call_files_ext2(*base, None, None) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    ext = _lib.LcdRunExt()
    assert lib.lcd_call_files_ext(*base, C.byref(ext)) == -30
    vio = _lib.LcdVcfIndexOpt(); ext.vcf_idx = C.pointer(vio)
    assert lib.lcd_call_files_ext(*base, C.byref(ext)) == -4 and b"vcf_idx" in lib.lcd_last_error()      # (an index needs a compressed VCF: as before)
    mk = lambda **kw: _lib.LcdRunExt2(**dict(dict(size=C.sizeof(_lib.LcdRunExt2), mods_path=tab), **kw))
    for x2, word in ((mk(size=0), b"size"), (mk(size=8), b"size"), (mk(mods_code=ord("a")), b"m or h"), (mk(mods_threshold=127), b"128"), (mk(mods_threshold=256), b"128"),
                     (mk(mods_path=b"-"), b"goes to a file"), (mk(mods_path=b""), b"goes to a file")):
        assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -4 and word in lib.lcd_last_error(), word
    ms = _lib.LcdModsStats(); ms.n_rows = 5
    for x2 in (mk(), mk(mods_code=ord("h"), mods_threshold=255, mods_combine_strands=1, mods_stats=C.pointer(ms)), mk(size=16), mk(size=4096), mk(mods_path=None)):
        assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert ms.n_rows == 0
    assert os.listdir(str(tmp_path)) == []


def test_the_per_contig_driver_takes_the_same_struct(tmp_path):
    """lcd_call_bam_regions_ext2 refuses what lcd_call_files_ext2 refuses of the struct, before anything else; with ext2 == NULL it is lcd_call_bam_regions"""
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    recs, n_recs, text = C.POINTER(_lib.LcdVar1)(), C.c_int(0), C.c_void_p()
    tab = str(tmp_path / "t.tsv").encode()
    args = (b"missing_in.bam", b"missing_in.bam.bai", b"missing_ref.fa", b"chr1", 0, None, None, 30, C.byref(cfg), None, C.byref(recs), C.byref(n_recs), C.byref(text), None, None, None)
    mk = lambda **kw: _lib.LcdRunExt2(**dict(dict(size=C.sizeof(_lib.LcdRunExt2), mods_path=tab), **kw))
    for x2, word in ((mk(size=8), b"size"), (mk(mods_code=ord("x")), b"m or h"), (mk(mods_threshold=300), b"128"), (mk(mods_path=b"-"), b"goes to a file")):
        assert lib.lcd_call_bam_regions_ext2(*args, C.byref(x2)) == -4 and word in lib.lcd_last_error(), word
    assert lib.lcd_call_bam_regions_ext2(*(args[:9] + (None,) + args[10:]), None) == lib.lcd_call_bam_regions(*(args[:9] + (None,) + args[10:]))
    assert os.listdir(str(tmp_path)) == []
