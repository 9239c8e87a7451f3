"""The read sets' entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported; the structs mirror the header as a C compiler lays
them out (tests/c/split_abi.c); lcd_run_ext2_split_t is lcd_run_ext2_t grown at its end -- the older struct keeps its size, and a caller that hands in only that
gets a run without read sets; every refusal comes back before a missing input is looked at and before a device is touched (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

from conftest import ROOT

NEW = ["lcd_split_opt_default", "lcd_split_opt_check", "lcd_split_paths", "lcd_split_offsets", "lcd_chunk_split_reads", "lcd_split_size", "lcd_split_dev_ptr", "lcd_split_to_host",
       "lcd_split_free"]
OLD_EXT2_SIZE = 64


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
    exe = str(tmp_path / "split_abi")
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "split_abi.c"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    for name, T in (("lcd_split_opt_t", _lib.LcdSplitOpt), ("lcd_split_stats_t", _lib.LcdSplitStats), ("lcd_run_ext2_split_t", _lib.LcdRunExt2Split)):
        assert got[name] == C.sizeof(T), name
        n_members = 0
        for k, v in got.items():
            if k.startswith(name + "."):
                assert getattr(T, k.split(".")[1]).offset == v, k
                n_members += 1
        assert n_members == len(T._fields_), name
    # the older struct is the first member and keeps its size: the new members begin where it ended, as if it had grown at its end
    assert got["lcd_run_ext2_t"] == C.sizeof(_lib.LcdRunExt2) == OLD_EXT2_SIZE and got["lcd_run_ext2_split_t.x"] == 0 and got["lcd_run_ext2_split_t.split_prefix"] == OLD_EXT2_SIZE
    txt = open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read()
    m = re.search(r"typedef struct lcd_split_stats_t \{(.*?)\} lcd_split_stats_t;", txt, re.S)
    assert re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", m.group(1)) == [f[0] for f in _lib.LcdSplitStats._fields_]


def test_host_only_entry_points():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    o = _lib.LcdSplitOpt(); o.comment = o.list = 9
    assert lib.lcd_split_opt_check(C.byref(o)) == -4
    lib.lcd_split_opt_default(C.byref(o))
    assert (o.comment, o.list, list(o.reserved)) == (0, 0, [0, 0]) and lib.lcd_split_opt_check(C.byref(o)) == 0 and lib.lcd_split_opt_check(None) == -4
    o.comment = o.list = 1
    assert lib.lcd_split_opt_check(C.byref(o)) == 0
    tot = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert lib.lcd_split_offsets(1, None, None, None, None, None, tot) == -4 and list(tot) == [0, 0, 0, 0]
    assert lib.lcd_split_offsets(0, None, None, None, None, None, None) == -4 and lib.lcd_split_offsets(0, None, None, None, None, None, tot) == 0
    p = (C.c_void_p * 3)(1, 1, 1)
    assert lib.lcd_split_paths(b"", 0, 0, None, p) == -4 and not any(p)
    assert lib.lcd_split_paths(b"p", 0, 1, None, p) == -4 and lib.lcd_split_paths(b"p", 0, 0, None, None) == -4 and lib.lcd_split_paths(None, 0, 0, None, None) == 0


def test_the_device_entry_points_refuse_without_a_device():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    st = _lib.LcdSplitStats(); st.n_records = 7
    o = _lib.LcdSplitOpt()
    assert not lib.lcd_chunk_split_reads(None, None, None, None, None, None, C.byref(o), C.byref(st)) and b"not made from a BAM" in lib.lcd_last_error() and st.n_records == 0
    assert not lib.lcd_chunk_split_reads(None, None, None, None, None, None, None, None)
    assert lib.lcd_split_size(None, 0) == 0 and lib.lcd_split_dev_ptr(None, 3) == 0 and lib.lcd_split_to_host(None, 0, 0, 0, None) == -41
    lib.lcd_split_free(None)


def _file_base(tmp_path):
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.bam_path, job.fasta_path, job.vcf_path = b"missing_in.bam", b"missing_ref.fa", str(tmp_path / "o.vcf").encode()
    st = _lib.LcdFileStats()
    return lib, (None, C.byref(job), C.byref(cfg), None, C.byref(st), None), (job, cfg, st)


def _mk(tmp_path, **kw):
    from longcalld_amd import _lib
    x = dict(mods_path=None, depth_path=None)
    x.update({k: kw.pop(k) for k in list(kw) if k in ("mods_path", "depth_path", "size")})
    s = _lib.LcdRunExt2Split(**dict(dict(split_prefix=str(tmp_path / "p").encode()), **kw))
    s.x.size = x.get("size", C.sizeof(_lib.LcdRunExt2Split)); s.x.mods_path, s.x.depth_path = x["mods_path"], x["depth_path"]
    return s


def test_the_file_driver_refuses_before_it_looks_at_the_input(tmp_path):
    """each refusal is -4 with its word although the input is missing (that would be -30); what is accepted goes on to the missing input; no file is created"""
    lib, base, keep = _file_base(tmp_path)
    pre = str(tmp_path / "p")
    lst = str(tmp_path / "l.tsv").encode()
    bad = [(_mk(tmp_path, split_prefix=b""), b"go to files"), (_mk(tmp_path, split_prefix=b"-"), b"go to files"), (_mk(tmp_path, split_prefix=None, split_gz=1), b"need split_prefix"),
           (_mk(tmp_path, split_prefix=None, split_comment=1, haplotag_path=lst), b"need split_prefix"), (_mk(tmp_path, haplotag_path=b""), b"goes to a file"),
           (_mk(tmp_path, haplotag_path=b"-"), b"goes to a file"), (_mk(tmp_path, haplotag_path=(pre + ".h1.fastq").encode()), b"name one file"),
           (_mk(tmp_path, split_gz=1, haplotag_path=(pre + ".none.fastq.gz").encode()), b"name one file"), (_mk(tmp_path, mods_path=(pre + ".h2.fastq").encode()), b"name one file"),
           (_mk(tmp_path, depth_path=(pre + ".h2.fastq").encode()), b"name one file"), (_mk(tmp_path, split_prefix=None, haplotag_path=lst, depth_path=lst), b"name one file"),
           (_mk(tmp_path, split_prefix=None, haplotag_path=str(tmp_path / "o.vcf").encode()), b"name one file")]
    for s, word in bad:
        assert lib.lcd_call_files_ext2(*base, None, C.byref(s.x)) == -4 and word in lib.lcd_last_error(), word
    from longcalld_amd import _lib
    bo = _lib.LcdBamOut(); bo.path = (pre + ".h1.fastq").encode()
    keep[0].bam_out = C.pointer(bo)
    assert lib.lcd_call_files_ext2(*base, None, C.byref(_mk(tmp_path).x)) == -4 and b"name one file" in lib.lcd_last_error()
    keep[0].bam_out = None
    ss = _lib.LcdSplitStats(); ss.n_records = 5
    for s in (_mk(tmp_path), _mk(tmp_path, split_gz=1, split_comment=1, haplotag_path=lst, split_stats=C.pointer(ss)), _mk(tmp_path, split_prefix=None, haplotag_path=lst),
              _mk(tmp_path, split_prefix=None), _mk(tmp_path, haplotag_path=(pre + ".h1.fastq.gz").encode())):
        assert lib.lcd_call_files_ext2(*base, None, C.byref(s.x)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert ss.n_records == 0
    assert os.listdir(str(tmp_path)) == []


def test_a_caller_with_the_older_struct_gets_no_read_sets(tmp_path):
    """size = sizeof(lcd_run_ext2_t): what lies behind it -- here a prefix and a list path that would both be refused -- is not read"""
    from longcalld_amd import _lib
    lib, base, _keep = _file_base(tmp_path)
    ss = _lib.LcdSplitStats(); ss.n_records = 5
    s = _mk(tmp_path, size=OLD_EXT2_SIZE, split_prefix=b"-", haplotag_path=b"", split_gz=1, split_stats=C.pointer(ss))
    assert lib.lcd_call_files_ext2(*base, None, C.byref(s.x)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert ss.n_records == 5                                                      # (not even zeroed: the library did not see the pointer)
    s.x.size = OLD_EXT2_SIZE + 8                                                  # ... and one member further the prefix is read, and refused
    assert lib.lcd_call_files_ext2(*base, None, C.byref(s.x)) == -4 and b"go to files" in lib.lcd_last_error()
    assert os.listdir(str(tmp_path)) == []


def test_the_per_contig_driver_takes_the_same_members(tmp_path):
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    recs, n_recs, text = C.POINTER(_lib.LcdVar1)(), C.c_int(0), C.c_void_p()
    pre = str(tmp_path / "p")
    bo = _lib.LcdBamOut(); bo.path = (pre + ".none.fastq").encode()
    args = lambda b: (b"missing_in.bam", b"missing_in.bam.bai", b"missing_ref.fa", b"chr1", 1, (C.c_int64 * 1)(1), (C.c_int64 * 1)(100), 30, C.byref(cfg), (_lib.LcdCallChunk * 1)(), C.byref(recs),
                      C.byref(n_recs), C.byref(text), C.byref(b) if b is not None else None, None, None)
    for s, word in ((_mk(tmp_path, split_prefix=b""), b"go to files"), (_mk(tmp_path, split_prefix=None, split_gz=1), b"need split_prefix"), (_mk(tmp_path, haplotag_path=b"-"), b"goes to a file"),
                    (_mk(tmp_path, haplotag_path=(pre + ".h2.fastq").encode()), b"name one file")):
        assert lib.lcd_call_bam_regions_ext2(*args(None), C.byref(s.x)) == -4 and word in lib.lcd_last_error(), word
    assert lib.lcd_call_bam_regions_ext2(*args(bo), C.byref(_mk(tmp_path).x)) == -4 and b"name one file" in lib.lcd_last_error()
    assert lib.lcd_call_bam_regions_ext2(*args(None), C.byref(_mk(tmp_path).x)) == -30
    assert lib.lcd_call_bam_regions_ext2(*args(None), C.byref(_mk(tmp_path, size=OLD_EXT2_SIZE, split_prefix=b"-").x)) == -30
    assert os.listdir(str(tmp_path)) == []
