"""lcd_chunk_refine_records without a device: declared in include/lcd_hotpath.h, listed in the loader, exported; lcd_refine_stats_t's ctypes mirror against the C
compiler's layout (tests/c/refine_abi.c); argument errors raised before any device call; the entry points around it keep their answers (the rounds driver still
refuses collect_ref_read_aln_str with -2, the command line still refuses --refine-aln with one "not supported" line)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_call_file_abi import cli

NEW = ["lcd_chunk_refine_records", "lcd_refine_log_create", "lcd_refine_log_free", "lcd_refine_log_n_entries", "lcd_refine_log_row_bytes", "lcd_refine_log_append",
       "lcd_refine_log_entry", "lcd_refine_log_apply", "lcd_chunks_noisy_rounds_log", "lcd_batch_region_ref_read_rows", "lcd_chunk_set_refine", "lcd_chunk_refine_log",
       "lcd_chunks_call_refine", "lcd_write_phased", "lcd_bam_writer_open", "lcd_call_bam_regions", "lcd_call_files"]


def test_symbol_declared_listed_and_exported():
    from longcalld_amd import _lib, align
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert callable(align.DeviceChunk.refine_records) and callable(align.RefineLog)


def test_struct_mirror_has_the_compilers_layout(tmp_path):
    from longcalld_amd import _lib
    exe = str(tmp_path / "refine_abi")
    subprocess.check_call(["gcc", "-O0", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "refine_abi.c"), "-o", exe])
    want = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert C.sizeof(_lib.LcdRefineStats) == int(want["lcd_refine_stats_t"]) and C.sizeof(_lib.LcdDigar) == int(want["lcd_digar_t"]) == 24
    assert C.sizeof(_lib.LcdRefineEntry) == int(want["lcd_refine_entry_t"])
    for f, c_name in zip([f[0] for f in _lib.LcdRefineEntry._fields_], [k.split(".")[1] for k in want if k.startswith("lcd_refine_entry_t.")]):
        assert f.rstrip("_") == c_name and getattr(_lib.LcdRefineEntry, f).offset == int(want["lcd_refine_entry_t." + c_name]), f
    assert [f[0] for f in _lib.LcdRefineStats._fields_] == [k.split(".")[1] for k in want if k.startswith("lcd_refine_stats_t.")]
    for f, _t in _lib.LcdRefineStats._fields_:
        assert getattr(_lib.LcdRefineStats, f).offset == int(want[f"lcd_refine_stats_t.{f}"]), f


def test_argument_errors_need_no_device(lcd):
    from longcalld_amd import _lib
    lib = lcd.load_library()
    st = _lib.LcdRefineStats(); st.n_records = 7
    assert not lib.lcd_chunk_refine_records(None, 0, None, None, None, None, 1, 0, None, None, None, None, C.byref(st))
    assert b"lcd_chunk_refine_records" in lib.lcd_last_error() and b"not made from a BAM" in lib.lcd_last_error() and st.n_records == 0
    assert not lib.lcd_chunk_refine_records(None, 0, None, None, None, None, 1, 0, None, None, None, None, None)
    # the drivers: NULL arguments are answered as by the entry points they extend, and the stats come back zeroed
    ao = _lib.LcdAlnOpt(_lib.LCD_ALN_BAM, 1)
    ro, out = _lib.LcdRunOpt(aln=C.pointer(ao)), _lib.LcdRunOut(refine_stats=C.pointer(st))
    st.n_records = 7
    assert lib.lcd_call_files(None, None, None, C.byref(ro), None, C.byref(out)) == -4 and st.n_records == 0
    inp = _lib.LcdInputs()
    st.n_records = 7
    assert lib.lcd_call_files(C.byref(inp), None, None, C.byref(ro), None, C.byref(out)) == -4 and st.n_records == 0
    st.n_records = 7
    assert lib.lcd_call_bam_regions(None, None, None, None, 0, None, None, 30, None, None, None, None, None, None, C.byref(ro), C.byref(out)) == -4 and st.n_records == 0
    wo = _lib.LcdWriterOpt(refine_stats=C.pointer(st))
    st.n_records = 7
    assert lib.lcd_write_phased(None, 0, None, None, C.byref(wo)) == -4 and st.n_records == 0
    st.n_records = 7
    assert not lib.lcd_bam_writer_open(None, None, C.byref(wo)) and b"NULL" in lib.lcd_last_error() and st.n_records == 0
    assert lib.lcd_chunk_set_refine(None, 1) == -4 and not lib.lcd_chunk_refine_log(None)
    assert lib.lcd_chunks_call_refine(0, None, None, None, None, None, None) == -4


def test_neighbours_keep_their_answers(lcd):
    from longcalld_amd import _lib
    lib = lcd.load_library()
    opt = _lib.LcdOpt(); lib.lcd_opt_default(C.byref(opt)); opt.collect_ref_read_aln_str = 1
    po = _lib.LcdPassOpt(); lib.lcd_pass_opt_default(C.byref(po))
    ch = (_lib.LcdRoundsChunk * 1)()
    assert lib.lcd_chunks_noisy_rounds(1, ch, C.byref(opt), C.byref(po)) == -2 and b"not supported" in lib.lcd_last_error()
    r = cli("call", "ref.fa", "in.bam", "--refine-aln")
    assert r.returncode == 2 and r.stderr.count("\n") == 1 and "not supported" in r.stderr


def test_refine_log_on_the_host(lcd):
    """the log keeps entries and rows in order; an entry of a read that covers neither end leaves its list as it is (return code 2) and still names it; a read id
    outside the chunk is an error; the rounds driver without any sink is the old entry point"""
    import numpy as np
    from longcalld_amd import _lib
    log = lcd.RefineLog()
    assert len(log) == 0 and log.row_bytes() == 0 and log.apply([np.zeros((0, 5), np.int64)], [0]) == ({}, 0)
    t, q = np.array([0, 1, 2, 3, 5], np.uint8), np.array([0, 1, 5, 3, 3], np.uint8)
    log.append(1, 0, 10, 14, 1011, 1015, t, q, pass_=2)
    log.append(0, 0, 3, 3, 1004, 1004, t[:1], q[:1])
    e = log.entries()
    assert len(log) == 2 and log.row_bytes() == 12 and [x["read_id"] for x in e] == [1, 0] and e[0]["pass_"] == 2 and (e[0]["reg_beg"], e[0]["reg_end"]) == (1011, 1015)
    assert e[0]["target"].tolist() == t.tolist() and e[0]["query"].tolist() == q.tolist() and e[1]["query"].tolist() == [0]
    digs = [np.array([[1001, 7, 50, 0, 0]], np.int64), np.array([[1001, 4, 5, 0, 0], [1001, 7, 45, 5, 0]], np.int64)]
    touched, rej = log.apply(digs, [50, 50])
    assert rej == 0 and sorted(touched) == [0, 1] and touched[0].tolist() == digs[0].tolist() and touched[1].tolist() == digs[1].tolist()
    with pytest.raises(lcd.LcdError, match="outside"):
        log.apply(digs[:1], [50])
    lib = lcd.load_library()
    opt = _lib.LcdOpt(); lib.lcd_opt_default(C.byref(opt)); opt.collect_ref_read_aln_str = 1
    po = _lib.LcdPassOpt(); lib.lcd_pass_opt_default(C.byref(po))
    ch = (_lib.LcdRoundsChunk * 1)()
    assert lib.lcd_chunks_noisy_rounds_log(1, ch, C.byref(opt), C.byref(po), None) == -2 and b"lcd_chunks_noisy_rounds:" in lib.lcd_last_error()
    assert lib.lcd_chunks_noisy_rounds_log(1, ch, C.byref(opt), C.byref(po), (C.c_void_p * 1)(log.h)) == -2 and b"not supported" in lib.lcd_last_error()
    assert lib.lcd_batch_region_ref_read_rows(None, 0, 0, None, None, None) == -3
    log.close()


def test_command_line_parses_refine_bam():
    assert "--refine-bam" in cli("call", "--help").stdout
    r = cli("call", "--refine-aln", "ref.fa", "in.bam")
    assert r.returncode == 2 and len(r.stderr.strip().splitlines()) == 1 and "not supported" in r.stderr and "--refine-bam" in r.stderr
    bad = cli("call", "--no-such-option", "missing_ref.fa", "missing_in.bam")
    ok = cli("call", "--refine-bam", "-b", "out.bam", "missing_ref.fa", "missing_in.bam")
    assert "--no-such-option" in bad.stderr and bad.returncode == 2
    assert "--refine-bam" not in ok.stderr and "not supported" not in ok.stderr and ok.returncode == 1 and "missing_in.bam" in ok.stderr     # parsed; the run fails on the input
    both = cli("call", "--refine-bam", "--te-lib", "te.fa", "-b", "out.bam", "ref.fa", "in.bam")
    assert both.returncode == 2 and len(both.stderr.strip().splitlines()) == 1 and "--refine-bam" in both.stderr
    assert cli("call", "--refine-bam", "missing_ref.fa", "missing_in.bam").returncode == 1                                                   # without -b it is accepted (no effect)
