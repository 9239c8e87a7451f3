"""The haplotag entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported; the structs mirror the header as a C compiler lays them
out (tests/c/haplotag_abi.c); the host-only entry points work, and the device entry point refuses what it can refuse before any HIP call (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import haplotag_common as hc
from conftest import ROOT

NEW = ["lcd_hapvcf_opt_default", "lcd_phased_vcf_read", "lcd_phased_vcf_n_contigs", "lcd_phased_vcf_n_sites", "lcd_phased_vcf_n_phase_sets", "lcd_phased_vcf_pool_size",
       "lcd_phased_vcf_max_footprint", "lcd_phased_vcf_sites_to_host", "lcd_phased_vcf_free", "lcd_phased_vcf_errno", "lcd_phased_vcf_error", "lcd_haplotag_opt_default",
       "lcd_haplotag_opt_check", "lcd_chunk_haplotag", "lcd_haplotag_n_reads", "lcd_haplotag_n_records", "lcd_haplotag_to_host", "lcd_haplotag_n_candidates",
       "lcd_haplotag_pairs_to_host", "lcd_haplotag_free", "lcd_haplotag_files"]


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
    exe = str(tmp_path / "haplotag_abi")
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "haplotag_abi.c"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines())}
    for name, T in (("lcd_hapvcf_opt_t", _lib.LcdHapvcfOpt), ("lcd_hapvcf_stats_t", _lib.LcdHapvcfStats), ("lcd_haplotag_opt_t", _lib.LcdHaplotagOpt),
                    ("lcd_haplotag_stats_t", _lib.LcdHaplotagStats), ("lcd_haplotag_run_t", _lib.LcdHaplotagRun)):
        assert got[name] == C.sizeof(T), name
        members = [k for k in got if k.startswith(name + ".")]
        assert len(members) == len(T._fields_), name
        for k in members:
            assert getattr(T, k.split(".")[1]).offset == got[k], k
    assert tuple(f[0] for f in _lib.LcdHapvcfStats._fields_) == hc.VCF_STAT_KEYS == _lib.HAPVCF_STAT_KEYS
    assert _lib.LcdHaplotagRun._fields_[0] == ("size", C.c_size_t) and got["lcd_haplotag_run_t.size"] == 0 and got["lcd_haplotag_run_t.vcf_path"] == 8


def test_option_defaults_and_checks():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    v = _lib.LcdHapvcfOpt(); v.max_indel = v.snvs_only = 9
    lib.lcd_hapvcf_opt_default(C.byref(v))
    assert (v.max_indel, v.snvs_only, list(v.reserved)) == (50, 0, [0, 0])
    o = _lib.LcdHaplotagOpt(); o.min_bq = o.min_diff = 9
    lib.lcd_haplotag_opt_default(C.byref(o))
    assert (o.min_bq, o.min_diff, list(o.reserved)) == (0, 1, [0, 0]) and lib.lcd_haplotag_opt_check(C.byref(o)) == 0
    for bq, diff, want in ((0, 1, 0), (254, 7, 0), (0, 0, -4), (0, -1, -4), (-1, 1, -4), (255, 1, -4)):
        o.min_bq, o.min_diff = bq, diff
        assert lib.lcd_haplotag_opt_check(C.byref(o)) == want, (bq, diff)
    assert lib.lcd_haplotag_opt_check(None) == -4


def test_the_reader_through_the_library(tmp_path):
    """the library's reader (host only) against the Python reader on every crafted file: tables, statistics, error codes"""
    from longcalld_amd import align
    n_err = 0
    for name, data, kw in hc.crafted_files():
        path = str(tmp_path / (name + ".vcf"))
        open(path, "wb").write(data)
        try:
            want = hc.read_vcf(hc.vcf_bytes(path), kw["names"], kw["sample"], kw["max_indel"], bool(kw["snvs_only"]))
        except hc.VcfError as e:
            with pytest.raises(align.LcdError, match="error %d:" % e.code):
                align.phased_vcf_read(path, kw["names"], kw["sample"], kw["max_indel"], kw["snvs_only"])
            n_err += 1
            continue
        v = align.phased_vcf_read(path, kw["names"], kw["sample"], kw["max_indel"], kw["snvs_only"])
        assert v.stats == want[1], name
        assert [hc.table_of_lib(v.sites(c)) for c in range(len(kw["names"]))] == want[0], name
        with pytest.raises(align.LcdError):
            v.sites(len(kw["names"]))
        v.close()
    assert n_err >= 7
    with pytest.raises(align.LcdError, match="error -30: .*cannot open"):
        align.phased_vcf_read(str(tmp_path / "missing.vcf"), ["c1"])
    with pytest.raises(align.LcdError, match="error -4: .*line 3 has 10 columns, the #CHROM line 11"):
        align.phased_vcf_read(str(tmp_path / "short_line_in_the_middle.vcf"), ["c1"])
    with pytest.raises(align.LcdError, match="max_indel"):
        align.phased_vcf_read(str(tmp_path / "gzip.vcf"), ["c1"], max_indel=0)


def test_the_device_entry_point_refuses_without_a_device():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    st = _lib.LcdHaplotagStats(); st.n_records = 7
    assert not lib.lcd_chunk_haplotag(None, None, 0, None, C.byref(st)) and b"not made from a BAM" in lib.lcd_last_error() and st.n_records == 0
    assert lib.lcd_haplotag_n_reads(None) == 0 and lib.lcd_haplotag_n_records(None) == 0 and lib.lcd_haplotag_n_candidates(None) == 0
    assert lib.lcd_haplotag_to_host(None, None, None, None, None) == -4 and lib.lcd_haplotag_pairs_to_host(None, None, None, None) == -4
    lib.lcd_haplotag_free(None); lib.lcd_phased_vcf_free(None)
    assert lib.lcd_phased_vcf_n_contigs(None) == 0 and lib.lcd_phased_vcf_n_sites(None, 0) == -4


def _file_base(tmp_path, **job_kw):
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.bam_path, job.fasta_path = b"missing_in.bam", b"missing_ref.fa"
    bo = _lib.LcdBamOut(); bo.path = str(tmp_path / "o.bam").encode()
    job.bam_out = C.pointer(bo)
    for k, v in job_kw.items():
        setattr(job, k, v)
    st = _lib.LcdFileStats()
    return lib, job, cfg, st, bo


def test_the_file_driver_refuses_before_it_looks_at_the_input(tmp_path):
    """each refusal is -4 with its word although the input is missing (that would be -30); what is accepted goes on to the missing input; no file is created"""
    from longcalld_amd import _lib
    lib, job, cfg, st, bo = _file_base(tmp_path)
    hs = _lib.LcdHaplotagStats(); hs.n_records = 5
    mk = lambda **kw: _lib.LcdHaplotagRun(**dict(dict(size=C.sizeof(_lib.LcdHaplotagRun), vcf_path=b"missing.vcf", stats=C.pointer(hs)), **kw))
    run = lambda h, opt=None, x2=None: lib.lcd_haplotag_files(None, C.byref(job), C.byref(cfg), C.byref(h) if h is not None else None, opt, C.byref(st), None, x2)
    assert run(None) == -4 and b"NULL options" in lib.lcd_last_error()
    for h, word in ((mk(size=8), b"size"), (mk(vcf_path=None), b"no phased VCF"), (mk(min_diff=-1), b"min_diff"), (mk(max_indel=-1), b"max_indel"), (mk(min_bq=255), b"min_bq")):
        assert run(h) == -4 and word in lib.lcd_last_error(), word
    assert hs.n_records == 0
    ao = _lib.LcdAlnOpt(_lib.LCD_ALN_BAM, 1)
    assert run(mk(), C.byref(_lib.LcdRunOpt(aln=C.pointer(ao)))) == -4 and b"refine" in lib.lcd_last_error()
    vf = _lib.LcdVcfFields()
    assert run(mk(), C.byref(_lib.LcdRunOpt(fields=C.pointer(vf)))) == -4 and b"fields" in lib.lcd_last_error()
    job.vcf_path = str(tmp_path / "o.vcf").encode()
    assert run(mk()) == -4 and b"writes no VCF" in lib.lcd_last_error()
    job.vcf_path = None
    job.bam_out = None
    assert run(mk()) == -4 and b"no output requested" in lib.lcd_last_error()
    x2 = _lib.LcdRunExt2(size=C.sizeof(_lib.LcdRunExt2), depth_path=str(tmp_path / "d.bed").encode())
    assert run(mk(), None, C.byref(x2)) == -30 and b"missing_in.bam" in lib.lcd_last_error()       # an output of ext2 is an output
    job.bam_out = C.pointer(bo)
    for h in (mk(), mk(size=16), mk(min_diff=3, max_indel=9, snvs_only=1, sample=b"S")):
        assert run(h) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert os.listdir(str(tmp_path)) == []


def test_python_refuses_what_belongs_to_a_calling_run(tmp_path):
    from longcalld_amd import align
    with pytest.raises(ValueError, match="calling run"):
        align.haplotag_file("in.bam", "ref.fa", "p.vcf", no_vcf_header=1)
    with pytest.raises(align.LcdError, match="writes no VCF"):
        align.haplotag_file("in.bam", "ref.fa", "p.vcf", vcf_path=str(tmp_path / "o.vcf"), bam_out=dict(path=str(tmp_path / "o.bam")))
    with pytest.raises(align.LcdError, match="no output requested"):
        align.haplotag_file("in.bam", "ref.fa", "p.vcf")
    with pytest.raises(align.LcdError, match="refine"):
        align.haplotag_file("in.bam", "ref.fa", "p.vcf", refine=True, bam_out=dict(path=str(tmp_path / "o.bam")))
    assert os.listdir(str(tmp_path)) == []
