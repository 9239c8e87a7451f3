"""The depth track's entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported; the structs mirror the header as a C compiler lays
them out (tests/c/depth_abi.c); lcd_run_ext2_t still starts with its own size, its methylation members lie where they lay, and a caller that knows only those
gets a run without a depth track; every refusal comes back before a missing input is looked at (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

from conftest import ROOT

NEW = ["lcd_depth_opt_default", "lcd_depth_opt_check", "lcd_chunk_depth", "lcd_depth_n_rows", "lcd_depth_rows_to_host", "lcd_depth_free", "lcd_depth_tile", "lcd_depth_windows",
       "lcd_depth_format"]
# lcd_run_ext2_t as it was before the depth members: offsets on the LP64 targets the library is built for
OLD_EXT2 = {"size": 0, "mods_path": 8, "mods_code": 16, "mods_threshold": 20, "mods_combine_strands": 24, "reserved": 28, "mods_stats": 32}
OLD_EXT2_SIZE = 40


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
    exe = str(tmp_path / "depth_abi")
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "depth_abi.c"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    for name, T in (("lcd_depth_opt_t", _lib.LcdDepthOpt), ("lcd_depth_stats_t", _lib.LcdDepthStats), ("lcd_run_ext2_t", _lib.LcdRunExt2), ("lcd_mods_stats_t", _lib.LcdModsStats)):
        assert got[name] == C.sizeof(T), name
        n_members = 0
        for k, v in got.items():
            if k.startswith(name + "."):
                assert getattr(T, k.split(".")[1]).offset == v, k
                n_members += 1
        assert n_members == len(T._fields_) or name == "lcd_mods_stats_t", name
    # size first; the members that were there lie where they lay; the new ones begin where the old struct ended
    for k, v in OLD_EXT2.items():
        assert got["lcd_run_ext2_t." + k] == v, k
    assert got["lcd_run_ext2_t.depth_path"] == OLD_EXT2_SIZE and _lib.LcdRunExt2._fields_[0] == ("size", C.c_size_t)
    assert [f[0] for f in _lib.LcdRunExt2._fields_[:7]] == list(OLD_EXT2)
    assert (got["lcd_run_ext_t"], got["lcd_run_opt_t"], got["lcd_run_out_t"]) == (16, 24, 40)
    txt = open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read()
    m = re.search(r"typedef struct lcd_depth_stats_t \{(.*?)\} lcd_depth_stats_t;", txt, re.S)
    assert re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", m.group(1)) == [f[0] for f in _lib.LcdDepthStats._fields_]


def test_host_only_entry_points():
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    o = _lib.LcdDepthOpt(); o.skip_dels = o.window = 9
    lib.lcd_depth_opt_default(C.byref(o))
    assert (o.skip_dels, o.window, list(o.reserved)) == (0, 0, [0, 0]) and lib.lcd_depth_opt_check(C.byref(o)) == 0
    for w, want in ((0, 0), (1, 0), (1 << 30, 0), ((1 << 30) + 1, -4), (-1, -4)):
        o.window = w
        assert lib.lcd_depth_opt_check(C.byref(o)) == want, w
    assert lib.lcd_depth_opt_check(None) == -4
    assert lib.lcd_depth_tile() > 0
    rows = [(1001, 1010, (3, 2, 1)), (1011, 1011, (0, 0, 0))]
    assert align.depth_format(rows, "chrS", with_header=True) == ("#chrom\tstart\tend\tdepth_all\tdepth_h1\tdepth_h2\tdepth_unassigned\n" "chrS\t1000\t1010\t6\t2\t1\t3\n"
                                                                  "chrS\t1010\t1011\t0\t0\t0\t0\n")
    assert align.depth_windows(rows, 4) == [(1001, 1004, (12, 8, 4)), (1005, 1008, (12, 8, 4)), (1009, 1011, (6, 4, 2))]
    assert align.depth_format([(1, 4, (1 << 62, 5, 1 << 40))], "c", windows=True, with_header=True) == (
        "#chrom\tstart\tend\tbases_all\tbases_h1\tbases_h2\tbases_unassigned\n" f"c\t0\t4\t{(1 << 62) + 5 + (1 << 40)}\t5\t{1 << 40}\t{1 << 62}\n")
    text = C.c_void_p(1)
    assert lib.lcd_depth_format(1, None, None, None, None, b"c", 0, C.byref(text)) == -4 and not text.value
    assert lib.lcd_depth_format(0, None, None, None, None, None, 0, C.byref(text)) == -4 and lib.lcd_depth_format(0, None, None, None, None, b"c", 0, None) == -4
    p = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
    assert lib.lcd_depth_windows(1, None, None, None, 5, *[C.byref(x) for x in p]) == -4 and not any(x.value for x in p)
    assert lib.lcd_depth_windows(0, None, None, None, 0, *[C.byref(x) for x in p]) == -4
    assert lib.lcd_depth_windows(0, None, None, None, 5, *[C.byref(x) for x in p]) == 0 and all(x.value for x in p)
    for x in p:
        align._libc.free(x)


def test_the_device_entry_points_refuse_without_a_device():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    st = _lib.LcdDepthStats(); st.n_records = 7
    o = _lib.LcdDepthOpt()
    assert not lib.lcd_chunk_depth(None, None, C.byref(o), C.byref(st)) and b"not made from a BAM" in lib.lcd_last_error() and st.n_records == 0
    assert lib.lcd_depth_n_rows(None) == 0 and lib.lcd_depth_rows_to_host(None, None, None, None) == -4
    lib.lcd_depth_free(None)


def _file_base(tmp_path):
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.bam_path, job.fasta_path, job.vcf_path = b"missing_in.bam", b"missing_ref.fa", str(tmp_path / "o.vcf").encode()
    st = _lib.LcdFileStats()
    return lib, (None, C.byref(job), C.byref(cfg), None, C.byref(st), None), (job, cfg, st)


def test_the_file_driver_refuses_before_it_looks_at_the_input(tmp_path):
    """each refusal is -4 with its word although the input is missing (that would be -30); what is accepted goes on to the missing input; no file is created"""
    from longcalld_amd import _lib
    lib, base, _keep = _file_base(tmp_path)
    trk, tab = str(tmp_path / "d.bed").encode(), str(tmp_path / "t.tsv").encode()
    mk = lambda **kw: _lib.LcdRunExt2(**dict(dict(size=C.sizeof(_lib.LcdRunExt2), depth_path=trk), **kw))
    for x2, word in ((mk(depth_path=b""), b"goes to a file"), (mk(depth_path=b"-"), b"goes to a file"), (mk(depth_window=-1), b"window"), (mk(depth_window=(1 << 30) + 1), b"window"),
                     (mk(mods_path=trk), b"name one file"), (mk(size=8), b"size")):
        assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -4 and word in lib.lcd_last_error(), word
    ds = _lib.LcdDepthStats(); ds.n_rows = 5
    for x2 in (mk(), mk(depth_window=1 << 30, depth_skip_dels=1, depth_stats=C.pointer(ds)), mk(mods_path=tab), mk(depth_path=None, depth_window=-7), mk(size=4096)):
        assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert ds.n_rows == 0
    assert os.listdir(str(tmp_path)) == []


def test_a_caller_with_the_old_struct_gets_no_depth_track(tmp_path):
    """size = the offset of depth_path: what lies behind it -- here a path and a window that would both be refused -- is not read"""
    from longcalld_amd import _lib
    lib, base, _keep = _file_base(tmp_path)
    old = _lib.LcdRunExt2.depth_path.offset
    assert old == OLD_EXT2_SIZE
    ds = _lib.LcdDepthStats(); ds.n_rows = 5
    x2 = _lib.LcdRunExt2(size=old, mods_path=str(tmp_path / "t.tsv").encode(), depth_path=b"-", depth_window=-3, depth_skip_dels=77, depth_stats=C.pointer(ds))
    assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert ds.n_rows == 5                                                        # (not even zeroed: the library did not see the pointer)
    x2.size = old + 8                                                            # ... and one member further the path is read, and refused
    assert lib.lcd_call_files_ext2(*base, None, C.byref(x2)) == -4 and b"goes to a file" in lib.lcd_last_error()
    assert os.listdir(str(tmp_path)) == []


def test_the_per_contig_driver_takes_the_same_members(tmp_path):
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    recs, n_recs, text = C.POINTER(_lib.LcdVar1)(), C.c_int(0), C.c_void_p()
    trk = str(tmp_path / "d.bed").encode()
    args = (b"missing_in.bam", b"missing_in.bam.bai", b"missing_ref.fa", b"chr1", 1, (C.c_int64 * 1)(1), (C.c_int64 * 1)(100), 30, C.byref(cfg), (_lib.LcdCallChunk * 1)(), C.byref(recs),
            C.byref(n_recs), C.byref(text), None, None, None)
    mk = lambda **kw: _lib.LcdRunExt2(**dict(dict(size=C.sizeof(_lib.LcdRunExt2), depth_path=trk), **kw))
    for x2, word in ((mk(depth_path=b""), b"goes to a file"), (mk(depth_path=b"-"), b"goes to a file"), (mk(depth_window=-1), b"window"), (mk(depth_window=(1 << 30) + 1), b"window"),
                     (mk(mods_path=trk), b"name one file")):
        assert lib.lcd_call_bam_regions_ext2(*args, C.byref(x2)) == -4 and word in lib.lcd_last_error(), word
    assert lib.lcd_call_bam_regions_ext2(*args, C.byref(mk())) == -30
    assert lib.lcd_call_bam_regions_ext2(*args, C.byref(mk(size=_lib.LcdRunExt2.depth_path.offset, depth_path=b"-"))) == -30
    assert os.listdir(str(tmp_path)) == []
