"""The several-input entry points without a device: declared in include/lcd_hotpath.h, listed in the loader, exported; lcd_inputs_t's ctypes mirror against the C
compiler's layout (tests/c/call_files_abi.c); argument errors; the header rule (LCD_ERR_INPUT_HEADERS) and the missing-index error, both raised before any output
file exists; the command line's input options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import call_file_common as fc
from conftest import ROOT
from test_call_file_abi import cli

NEW = ["lcd_chunk_open_from_bams", "lcd_chunk_n_files", "lcd_chunk_read_files", "lcd_merged_record_plan", "lcd_chunk_tag_records_sel", "lcd_bam_writer_open", "lcd_call_files"]


def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib, align
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    for mirror in ("chunk_open_from_bams", "merged_record_plan", "call_files"):
        assert callable(getattr(align, mirror))
    assert callable(align.DeviceChunk.open_from_bams) and callable(align.DeviceChunk.tag_records_sel)


def test_struct_mirror_has_the_compilers_layout(tmp_path):
    from longcalld_amd import _lib
    exe = str(tmp_path / "call_files_abi")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "call_files_abi.c"), "-o", exe])
    want = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert C.sizeof(_lib.LcdInputs) == int(want["lcd_inputs_t"])
    assert [f[0] for f in _lib.LcdInputs._fields_] == [k.split(".")[1] for k in want if k.startswith("lcd_inputs_t.")]
    for f, _t in _lib.LcdInputs._fields_:
        assert getattr(_lib.LcdInputs, f).offset == int(want[f"lcd_inputs_t.{f}"]), f
    # the structs the several-input run shares with the one-file run keep their layouts
    for name, cls in (("lcd_file_job_t", _lib.LcdFileJob), ("lcd_file_stats_t", _lib.LcdFileStats), ("lcd_index_opt_t", _lib.LcdIndexOpt), ("lcd_index_stats_t", _lib.LcdIndexStats)):
        assert C.sizeof(cls) == int(want[name]), name
    assert (_lib.LCD_MAX_INPUTS, _lib.LCD_ERR_INPUT_HEADERS) == (int(want["LCD_MAX_INPUTS"]), int(want["LCD_ERR_INPUT_HEADERS"])) == (64, -54)


@pytest.fixture()
def files(tmp_path):
    """two BAMs without records over the same reference table, their .bai, a FASTA and its .fai"""
    a, b, fa = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "ref.fa")
    for p in (a, b):
        fc.write_multi_bam(p, [("chr1", 100, []), ("chrM", 50, [])])
    fc.write_multi_fasta(fa, [("chr1", np.zeros(100, np.uint8)), ("chrM", np.ones(50, np.uint8))])
    return a, b, fa


def run_files(lcd, bams, fa, bais=None, sort_output=0, idx=None, n=None, **kw):
    from longcalld_amd import _lib
    lib = lcd.load_library()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.fasta_path = fa.encode() if fa else None
    for k, v in kw.items():
        setattr(job, k, v)
    inp = _lib.LcdInputs()
    arr = (C.c_char_p * max(1, len(bams)))(*[x.encode() if x is not None else None for x in bams])
    inp.n = len(bams) if n is None else n; inp.bam_paths = arr; inp.sort_output = sort_output
    if bais is not None:
        barr = (C.c_char_p * max(1, len(bais)))(*[x.encode() if x is not None else None for x in bais]); inp.bai_paths = barr
    st = _lib.LcdFileStats(); per = (C.c_int64 * max(1, len(bams)))()
    cfg = lcd.call_cfg()
    io = _lib.LcdIndexOpt(*idx) if idx else None
    ro, out = _lib.LcdRunOpt(idx=C.pointer(io) if io else None), _lib.LcdRunOut(n_reads_per_file=C.cast(per, C.POINTER(C.c_int64)))
    rc = lib.lcd_call_files(C.byref(inp), C.byref(job), C.byref(cfg), C.byref(ro), C.byref(st), C.byref(out))
    msg = lib.lcd_last_error().decode()
    lib.lcd_file_stats_free(C.byref(st))
    return rc, msg


def test_argument_errors_are_minus_4(lcd, files, tmp_path):
    from longcalld_amd import _lib
    a, b, fa = files
    lib = lcd.load_library()
    assert lib.lcd_call_files(None, None, None, None, None, None) == -4
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job)); job.fasta_path = fa.encode()
    st = _lib.LcdFileStats(); cfg = lcd.call_cfg()
    assert not job.bam_path                                                          # neither `in` nor job->bam_path
    assert lib.lcd_call_files(None, C.byref(job), C.byref(cfg), None, C.byref(st), None) == -4 and b"lcd_call_files" in lib.lcd_last_error()
    assert run_files(lcd, [], fa)[0] == -4                                            # n 0
    assert run_files(lcd, [a] * 65, fa)[0] == -4                                      # n > LCD_MAX_INPUTS
    assert run_files(lcd, [a, None], fa)[0] == -4 and run_files(lcd, [a, b], None)[0] == -4
    rc, msg = run_files(lcd, [a, b], fa, bam_path=b.encode())                          # job->bam_path differs from entry 0
    assert rc == -4 and "first input" in msg
    rc, msg = run_files(lcd, [a, b], fa, bais=[a + ".bai", None], bai_path=(b + ".bai").encode())
    assert rc == -4 and "index" in msg
    for kw in (dict(window_chunks=-1), dict(overlap=2), dict(chunk_len=-5)):
        assert run_files(lcd, [a, b], fa, **kw)[0] == -4, kw
    # the chunk level and the writer option
    assert not lib.lcd_chunk_open_from_bams(None, 0, None, None, None, 1, 2, 0, 0, None) and b"lcd_chunk_open_from_bams" in lib.lcd_last_error()
    opt = _lib.LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), 0)
    arr = (C.c_char_p * 65)(*[a.encode()] * 65)
    for n in (0, 65):
        assert not lib.lcd_chunk_open_from_bams(C.byref(opt), n, arr, None, b"chr1", 1, 2, 0, 0, None)
    arr[1] = None
    assert not lib.lcd_chunk_open_from_bams(C.byref(opt), 2, arr, None, b"chr1", 1, 2, 0, 0, None) and b"NULL path" in lib.lcd_last_error()
    wo = _lib.LcdWriterOpt(sort_output=1)
    assert not lib.lcd_bam_writer_open(None, None, C.byref(wo)) and b"lcd_bam_writer_open" in lib.lcd_last_error()
    assert lib.lcd_chunk_read_files(None, None) == -4 and lib.lcd_chunk_n_files(None) == 0
    assert not lib.lcd_chunk_tag_records_sel(None, None, None, None, None) and b"lcd_chunk_tag_records_sel" in lib.lcd_last_error()


def test_the_header_rule_and_a_missing_index_come_before_any_output(lcd, files, tmp_path):
    from longcalld_amd import _lib
    a, b, fa = files
    vcf, out = str(tmp_path / "o.vcf"), str(tmp_path / "o.bam")
    bo = _lib.LcdBamOut(); bo.path = out.encode()
    cases = [("len.bam", [("chr1", 100, []), ("chrM", 51, [])], "entry 1 is chrM (51)"), ("name.bam", [("chr1", 100, []), ("chrMT", 50, [])], "entry 1 is chrMT (50)"),
             ("order.bam", [("chrM", 50, []), ("chr1", 100, [])], "entry 0 is chrM (50)"), ("short.bam", [("chr1", 100, [])], "entry 1 is nothing"),
             ("long.bam", [("chr1", 100, []), ("chrM", 50, []), ("chrX", 9, [])], "entry 2 is chrX (9)")]
    for name, contigs, say in cases:
        other = str(tmp_path / name)
        fc.write_multi_bam(other, contigs)
        rc, msg = run_files(lcd, [a, b, other], fa, vcf_path=vcf.encode(), bam_out=C.pointer(bo))
        assert rc == _lib.LCD_ERR_INPUT_HEADERS == -54 and other in msg and say in msg, msg
        assert not os.path.exists(vcf) and not os.path.exists(out)
    os.rename(b + ".bai", b + ".bai.away")
    rc, msg = run_files(lcd, [a, b], fa, vcf_path=vcf.encode(), bam_out=C.pointer(bo))
    assert rc == -30 and b + ".bai" in msg and not os.path.exists(vcf) and not os.path.exists(out)
    rc, msg = run_files(lcd, [a, b], fa, idx=(0, 1, 0, None, 0), vcf_path=vcf.encode())      # an index struct without build_missing_bai
    assert rc == -30 and b + ".bai" in msg and "build_missing_bai" in msg
    elsewhere = str(tmp_path / "elsewhere.bai")
    rc, msg = run_files(lcd, [a, b], fa, bais=[None, elsewhere], vcf_path=vcf.encode())
    assert rc == -30 and elsewhere in msg and not os.path.exists(vcf)
    with pytest.raises(lcd.LcdError, match="-54"):
        lcd.call_files([a, str(tmp_path / "len.bam")], fa, vcf_path=vcf)
    with pytest.raises(lcd.LcdError, match="-2"):                                      # the refusals of the one-file run stay
        lcd.call_files([a, a], fa, vcf_path=vcf, cfg=lcd.call_cfg(0, clean=dict(out_somatic=1)))


# ---------------- the command line ----------------
def test_cli_input_order_and_options(tmp_path):
    from longcalld_amd import cli as cl
    lst = tmp_path / "list.txt"
    lst.write_text("l1.bam\n\n  \nl2.bam\n")
    o, pos = cl.parse(["ref.fa", "in.bam", "--add-bam", "x1.bam", "--bam-list", str(lst), "--add-bam=x2.bam", "--sort-merged", "chr1:1-5"])
    assert pos == ["ref.fa", "in.bam", "chr1:1-5"] and "--sort-merged" in o["flags"] and o["add_bam"] == ["x1.bam", "x2.bam"]
    assert cl.input_bams(o, pos[1]) == ["in.bam", "l1.bam", "l2.bam", "x1.bam", "x2.bam"]          # the positional BAM, the list's lines, the --add-bam files
    o, pos = cl.parse(["ref.fa", "in.bam"])
    assert cl.input_bams(o, pos[1]) == ["in.bam"] and "--sort-merged" not in o["flags"]
    assert cl.parse(["--add-bam"]) == 2                                                             # a value is needed
    for opt in ("--add-bam", "--bam-list", "--sort-merged"):
        assert opt in cl.USAGE


@pytest.mark.parametrize("args", [["-L"], ["--input-is-list"], ["-X", "extra.bam"], ["--extra-bam", "extra.bam"]], ids=lambda a: a[0])
def test_cli_still_refuses_the_reference_spellings_and_names_the_new_ones(args):
    r = cli("call", *args, "ref.fa", "in.bam")
    assert r.returncode == 2 and r.stdout == ""
    assert len(r.stderr.strip().splitlines()) == 1 and "not supported" in r.stderr
    assert ("--bam-list" if args[0] in ("-L", "--input-is-list") else "--add-bam") in r.stderr


def test_cli_reports_an_unreadable_list(tmp_path):
    r = cli("call", "ref.fa", "in.bam", "--bam-list", str(tmp_path / "absent.txt"))
    assert r.returncode == 2 and "--bam-list" in r.stderr and len(r.stderr.strip().splitlines()) == 1
