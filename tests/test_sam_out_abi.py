"""The SAM text output's entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported by the built library; their structs mirror the
header; NULL and range refusals come back before any HIP call (no GPU needed)."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ["lcd_sam_names_create", "lcd_sam_names_free", "lcd_tagged_to_sam", "lcd_records_to_sam", "lcd_sam_text_size", "lcd_sam_text_dev_ptr", "lcd_sam_text_to_host",
       "lcd_sam_text_free", "lcd_bam_writer_open", "lcd_write_phased", "lcd_call_files"]


def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert "lcd_sam_stats_t" in txt and "lcd_aln_opt_t" in txt and re.search(r"LCD_ALN_BAM\s*=\s*0\s*,\s*LCD_ALN_SAM\s*=\s*1", txt)


def test_structs_mirror_the_header():
    from longcalld_amd import _lib
    assert C.sizeof(_lib.LcdSamStats) == 7 * 8 + 3 * 8 and C.sizeof(_lib.LcdAlnOpt) == 8 and (_lib.LCD_ALN_BAM, _lib.LCD_ALN_SAM) == (0, 1)
    assert [f[0] for f in _lib.LcdSamStats._fields_] == ["n_records", "bytes_records", "bytes_text", "n_float_values", "n_cg_cigar", "n_walk_stopped", "n_bad_layout", "ms_measure",
                                                         "ms_emit", "ms_download_write"]
    txt = open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read()
    m = re.search(r"typedef struct lcd_sam_stats_t \{(.*?)\} lcd_sam_stats_t;", txt, re.S)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert names == [f[0] for f in _lib.LcdSamStats._fields_]


def test_arguments_are_checked_before_any_device_work():
    from longcalld_amd import _lib
    lib = _lib.load_library()
    err = lambda: lib.lcd_last_error()
    assert not lib.lcd_sam_names_create(-1, None) and b"n_ref" in err()
    assert not lib.lcd_sam_names_create(2, None) and b"NULL" in err()
    st = _lib.LcdSamStats(); st.n_records = 7
    assert not lib.lcd_tagged_to_sam(None, None, C.byref(st)) and b"NULL" in err() and st.n_records == 0
    rec = (C.c_uint8 * 40)()
    st.n_records = 7
    assert not lib.lcd_records_to_sam(rec, 40, None, C.byref(st)) and b"NULL" in err() and st.n_records == 0
    assert lib.lcd_sam_text_size(None) == 0 and lib.lcd_sam_text_dev_ptr(None) == 0 and lib.lcd_sam_text_to_host(None, 0, 0, None) == -41
    lib.lcd_sam_text_free(None); lib.lcd_sam_names_free(None)
    sam = _lib.LcdWriterOpt(format=_lib.LCD_ALN_SAM)
    assert not lib.lcd_bam_writer_open(None, None, C.byref(sam)) and b"NULL" in err()
    bo = _lib.LcdBamOut(); bo.path = None
    assert not lib.lcd_bam_writer_open(b"x.bam", C.byref(bo), C.byref(sam)) and b"NULL" in err()
    sam_st = _lib.LcdWriterOpt(format=_lib.LCD_ALN_SAM, sam_stats=C.pointer(st))
    st.n_records = 7
    assert not lib.lcd_bam_writer_open(None, None, C.byref(sam_st)) and st.n_records == 0
    assert lib.lcd_write_phased(None, 0, None, None, C.byref(sam)) == -4
    assert lib.lcd_write_phased(b"x.bam", 0, None, C.byref(bo), C.byref(sam)) == -4 and b"NULL" in err()
    bo.path = b"o.sam"
    assert lib.lcd_write_phased(b"x.bam", -1, None, C.byref(bo), C.byref(sam)) == -4
    assert lib.lcd_write_phased(b"x.bam", 1, None, C.byref(bo), C.byref(sam_st)) == -4
    assert not os.path.exists("o.sam")


def test_the_file_driver_s_refusals(tmp_path):
    """format outside the enum: -4; refine with fields: -2; SAM with write_out_bai: -4; SAM and VCF both on stdout: -4 -- all before a file is created; a NULL
    option is the feature off"""
    from longcalld_amd import _lib, align
    lib = _lib.load_library()
    cfg = align.call_cfg()
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    out = str(tmp_path / "o.sam")
    bo = _lib.LcdBamOut(); bo.path = out.encode()
    job.bam_path, job.fasta_path, job.vcf_path, job.bam_out = b"missing_in.bam", b"missing_ref.fa", str(tmp_path / "o.vcf").encode(), C.pointer(bo)
    st, sst, rst = _lib.LcdFileStats(), _lib.LcdSamStats(), _lib.LcdRefineStats()
    ptr = lambda x: C.pointer(x) if x is not None else None
    ro_out = []

    def call(ao, idx=None, vf=None):
        ro_out[:] = [_lib.LcdRunOpt(idx=ptr(idx), fields=ptr(vf), aln=ptr(ao)), _lib.LcdRunOut(refine_stats=C.pointer(rst), sam_stats=C.pointer(sst))]
        return lib.lcd_call_files(None, C.byref(job), C.byref(cfg), C.byref(ro_out[0]), C.byref(st), C.byref(ro_out[1]))
    assert call(None) == -30 and b"missing_in.bam" in lib.lcd_last_error()      # no lcd_aln_opt_t: a BAM output without refinement, refused for its input only
    assert call(_lib.LcdAlnOpt(2, 0)) == -4 and call(_lib.LcdAlnOpt(-1, 0)) == -4
    vf = _lib.LcdVcfFields(); vf.rnames_mode = _lib.LCD_RNAMES_ALL
    assert call(_lib.LcdAlnOpt(_lib.LCD_ALN_SAM, 1), vf=vf) == -2 and call(_lib.LcdAlnOpt(_lib.LCD_ALN_BAM, 1), vf=vf) == -2
    idx = _lib.LcdIndexOpt(1, 1, 1, None, 0)
    assert call(_lib.LcdAlnOpt(_lib.LCD_ALN_SAM, 0), idx=idx) == -4 and b"index" in lib.lcd_last_error()
    bo.path = b"-"; job.vcf_path = None
    assert call(_lib.LcdAlnOpt(_lib.LCD_ALN_SAM, 0)) == -4 and b"stdout" in lib.lcd_last_error()
    job.vcf_path = b"-"
    assert call(_lib.LcdAlnOpt(_lib.LCD_ALN_SAM, 0)) == -4 and b"stdout" in lib.lcd_last_error()
    # accepted as far as the arguments go: the run then fails on the missing input, and nothing was created
    bo.path = out.encode(); job.vcf_path = str(tmp_path / "o.vcf").encode()
    assert call(_lib.LcdAlnOpt(_lib.LCD_ALN_SAM, 1)) == -30 and b"missing_in.bam" in lib.lcd_last_error()
    assert os.listdir(str(tmp_path)) == []
