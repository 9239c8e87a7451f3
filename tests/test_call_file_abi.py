"""The whole-file entry points without a device: declared in include/lcd_hotpath.h, listed in the loader, exported; the ctypes mirrors against the C compiler's
layout (tests/c/call_file_abi.c); argument errors, refused settings, missing indexes; the BAM header readers; the command line's refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import call_file_common as fc
from conftest import ROOT

NEW = ["lcd_bam_contigs", "lcd_bam_contigs_free", "lcd_bam_sample_name", "lcd_plan_chunks", "lcd_chunk_plan_free", "lcd_stitch_chunks_carry", "lcd_stitch_carry_free",
       "lcd_chunk_open_from_bam", "lcd_chunk_resolve", "lcd_bam_writer_open", "lcd_bam_writer_append", "lcd_bam_writer_close", "lcd_bam_writer_abort", "lcd_vcf_writer_open",
       "lcd_vcf_writer_append", "lcd_vcf_writer_close", "lcd_vcf_writer_abort", "lcd_file_job_default", "lcd_call_files", "lcd_file_stats_free"]


def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib, align
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    for mirror in ("bam_contigs", "bam_sample_name", "plan_chunks", "stitch_chunks_carry", "vcf_write", "call_file"):
        assert callable(getattr(align, mirror))
    assert callable(align.DeviceChunk.open_from_bam) and callable(align.DeviceChunk.resolve)


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    from longcalld_amd import _lib
    exe = str(tmp_path / "call_file_abi")                                            # plain C against the public header: compiled here, no library needed
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "call_file_abi.c"), "-o", exe])
    want = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    mirrors = {"lcd_chunk_plan_t": _lib.LcdChunkPlan, "lcd_stitch_carry_t": _lib.LcdStitchCarry, "lcd_chunk_phase_t": _lib.LcdChunkPhase, "lcd_bam_out_t": _lib.LcdBamOut,
               "lcd_file_job_t": _lib.LcdFileJob, "lcd_file_stats_t": _lib.LcdFileStats}
    seen = 0
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == int(want[name]), name
        fields = [k.split(".")[1] for k in want if k.startswith(name + ".")]
        if name != "lcd_bam_out_t":
            assert fields == [f[0] for f in cls._fields_], name                       # every field, in order
        for f in fields:
            assert getattr(cls, f).offset == int(want[f"{name}.{f}"]), (name, f)
            seen += 1
    assert seen > 80
    assert (_lib.LCD_CTG_AUTOSOME_XY, _lib.LCD_CTG_AUTOSOME, _lib.LCD_CTG_ALL) == tuple(int(want[k]) for k in ("LCD_CTG_AUTOSOME_XY", "LCD_CTG_AUTOSOME", "LCD_CTG_ALL"))


@pytest.fixture()
def files(tmp_path):
    """a BAM without records, its .bai, a FASTA and its .fai"""
    import numpy as np
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    fc.write_multi_bam(bam, [("chr1", 100, []), ("chrM", 50, [])])
    fc.write_multi_fasta(fa, [("chr1", np.zeros(100, np.uint8)), ("chrM", np.ones(50, np.uint8))])
    return bam, fa


def run_file(lcd, bam, fa, cfg=None, **kw):
    from longcalld_amd import _lib
    lib = lcd.load_library()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    assert job.overlap == -1 and job.window_chunks == 0 and not job.bam_path
    job.bam_path = bam.encode() if bam else None; job.fasta_path = fa.encode() if fa else None
    for k, v in kw.items():
        setattr(job, k, v)
    st = _lib.LcdFileStats()
    cfg = cfg if cfg is not None else lcd.call_cfg()
    rc = lib.lcd_call_files(None, C.byref(job), C.byref(cfg), None, C.byref(st), None)
    msg = lib.lcd_last_error().decode()
    lib.lcd_file_stats_free(C.byref(st))
    return rc, msg


def test_argument_errors(lcd, files, tmp_path):
    from longcalld_amd import _lib
    bam, fa = files
    lib = lcd.load_library()
    assert lib.lcd_call_files(None, None, None, None, None, None) == -4
    assert run_file(lcd, None, fa)[0] == -4 and run_file(lcd, bam, None)[0] == -4
    for kw in (dict(window_chunks=-1), dict(loader_threads=-2), dict(chunk_len=-5), dict(overlap=2), dict(overlap=-2)):
        rc, msg = run_file(lcd, bam, fa, **kw)
        assert rc == -4 and "lcd_call_files" in msg, kw
    bo = _lib.LcdBamOut(); bo.path = None
    assert run_file(lcd, bam, fa, bam_out=C.pointer(bo))[0] == -4
    assert lib.lcd_chunk_resolve(None, None) == -4 and b"lcd_chunk_resolve" in lib.lcd_last_error()
    assert not lib.lcd_chunk_open_from_bam(None, None, None, None, 1, 2, 0, 0, None) and b"NULL" in lib.lcd_last_error()
    assert not lib.lcd_bam_writer_open(None, None, None) and b"NULL" in lib.lcd_last_error()
    assert lib.lcd_bam_writer_append(None, 0, None, None, None) == -4 and lib.lcd_bam_writer_close(None) == -4
    assert lib.lcd_vcf_writer_append(None, b"x") == -4 and lib.lcd_vcf_writer_close(None) == -4
    assert lib.lcd_bam_contigs(None, None, None, None) == -4 and lib.lcd_bam_sample_name(None, None) == -4
    assert lib.lcd_plan_chunks(1, None, None, 0, 0, None, 0, None, None, 0, None) == -4
    with pytest.raises(lcd.LcdError, match="-30"):
        lcd.bam_contigs(str(tmp_path / "absent.bam"))


def test_somatic_and_refine_settings_are_refused(lcd, files):
    bam, fa = files
    for cfg in (lcd.call_cfg(0, clean=dict(out_somatic=1)), lcd.call_cfg(0, opt=dict(collect_ref_read_aln_str=1))):
        rc, msg = run_file(lcd, bam, fa, cfg=cfg)
        assert rc == -2 and "not supported" in msg


def test_missing_indexes_name_their_path(lcd, files, tmp_path):
    bam, fa = files
    os.rename(bam + ".bai", bam + ".bai.away")
    rc, msg = run_file(lcd, bam, fa)
    assert rc == -30 and bam + ".bai" in msg
    other = str(tmp_path / "elsewhere.bai")
    rc, msg = run_file(lcd, bam, fa, bai_path=other.encode())
    assert rc == -30 and other in msg
    os.rename(bam + ".bai.away", bam + ".bai")
    os.remove(fa + ".fai")
    rc, msg = run_file(lcd, bam, fa)
    assert rc == -30 and fa + ".fai" in msg


HD = b"@HD\tVN:1.6\tSO:coordinate\n"


@pytest.mark.parametrize("text,want", [
    (HD, None),                                                                                   # no @RG
    (HD + b"@RG\tID:a\tPL:PACBIO\n", None),                                                       # an @RG without SM
    (HD + b"@RG\tID:a\tSM:HG002\tPL:x\n@RG\tID:b\tSM:HG002\n", "HG002"),                           # two equal SM
    (HD + b"@RG\tID:a\tPL:x\tSM:first\n@RG\tID:b\tSM:second\n", "first"),                          # two different SM: the first one is kept
    (HD + b"@RG\tID:a\n@RG\tID:b\tSM:late\n@PG\tID:p\tSM:nope\n", "late"),                         # the first @RG that has one
    (HD + b"@PG\tID:p\tCL:x SM:no\n@RG\tID:a\tDS:SM:not this\tSM:yes", "yes"),                     # fields are tab-separated; no final newline
])
def test_sample_name(lcd, tmp_path, text, want):
    bam = str(tmp_path / "h.bam")
    fc.write_multi_bam(bam, [("chr1", 10, [])], header_text=text)
    assert lcd.bam_sample_name(bam) == want


def test_bam_contigs(lcd, tmp_path):
    bam = str(tmp_path / "c.bam")
    ctg = [("chr1", 248956422), ("chrUn_x", 1), ("hs37d5", 35477943), ("chrM", 16569)]
    fc.write_multi_bam(bam, [(n, l, []) for n, l in ctg], header_text=HD + b"@SQ\tSN:ignored\tLN:5\n")    # the binary table counts, not the text
    assert lcd.bam_contigs(bam) == ctg
    empty = str(tmp_path / "e.bam")
    fc.write_multi_bam(empty, [], header_text=b"")
    assert lcd.bam_contigs(empty) == [] and lcd.bam_sample_name(empty) is None


def test_vcf_writer_plain_text(lcd, tmp_path):
    out = str(tmp_path / "o.vcf")
    lcd.vcf_write(out, ["chr1\t1\n", "", "chr1\t2\nchr2\t3\n"], header_text="##h\n#CHROM\n")
    assert open(out).read() == "##h\n#CHROM\nchr1\t1\nchr1\t2\nchr2\t3\n"
    lcd.vcf_write(out, ["x\n"])                                                       # -H: no header
    assert open(out).read() == "x\n"
    with pytest.raises(lcd.LcdError, match="cannot open"):
        lcd.vcf_write(str(tmp_path / "no" / "dir.vcf"), [])


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def test_cli_help_lists_the_reference_spellings():
    r = cli("--help")
    assert r.returncode == 0
    for o in ("--hifi", "--ont", "--region-file", "--autosome-XY", "--autosome", "--all-ctg", "-E", "-r", "-n", "-o", "-O", "-l", "-H", "--amb-base", "-b", "-c", "-d", "-a",
              "-M", "-B", "-C", "--window-chunks", "--no-overlap"):
        assert o in r.stdout, o
    assert cli("call", "--help").returncode == 0


@pytest.mark.parametrize("args", [["-s"], ["--refine-aln"], ["-L"], ["-X", "extra.bam"], ["-T", "te.fa"], ["-S", "out.sam"], ["-C", "out.cram"], ["--out-var-rnames"],
                                  ["--out-som-var-rnames"], ["--out-sv-rnames"]], ids=lambda a: a[0])
def test_cli_refuses_with_one_line_and_status_2(args):
    r = cli("call", *args, "ref.fa", "in.bam")
    assert r.returncode == 2 and r.stdout == ""
    assert len(r.stderr.strip().splitlines()) == 1 and "not supported" in r.stderr
