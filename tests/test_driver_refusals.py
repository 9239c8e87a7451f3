"""Every refusal of the four drivers (lcd_call_files, lcd_call_bam_regions, lcd_bam_writer_open, lcd_write_phased) as one table of (options, expected code, message
fragment), without a device.  Each row fails before an index is built or an output file is created: the directory the outputs would go to stays empty.  The
inputs named here do not exist, so a row that were accepted would fail with -30 on its input instead of the code the table expects."""
import ctypes as C
import os

import pytest

W_FILES, W_REGIONS, W_OPEN, W_WRITE = "lcd_call_files: ", "lcd_call_bam_regions: ", "lcd_bam_writer_open: ", "lcd_write_phased: "
ptr = lambda x: C.pointer(x) if x is not None else None


def _files(lib, _lib, align, d, job_kw=None, bam_out="o.bam", vcf="o.vcf", inputs=None, n=None, idx=None, fields=None, aln=None, cfg_kw=None, null=()):
    """one lcd_call_files call; the keywords are what the row changes"""
    cfg = align.call_cfg(0, **(cfg_kw or {}))
    job = _lib.LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    job.bam_path, job.fasta_path = (None if inputs is not None else b"absent_in.bam"), b"absent_ref.fa"
    job.vcf_path = os.path.join(d, vcf).encode() if vcf not in (None, "-") else (b"-" if vcf == "-" else None)
    bo = _lib.LcdBamOut()
    if bam_out is not None:
        bo.path = None if bam_out == "nopath" else b"-" if bam_out == "-" else os.path.join(d, bam_out).encode()
        job.bam_out = C.pointer(bo)
    for k, v in (job_kw or {}).items():
        setattr(job, k, v)
    inp = None
    if inputs is not None:
        inp = _lib.LcdInputs()
        arr = (C.c_char_p * max(1, len(inputs)))(*inputs)
        inp.n, inp.bam_paths = (len(inputs) if n is None else n), arr
    io = _lib.LcdIndexOpt(*idx) if idx is not None else None
    if io is not None and io.out_bai_path is None and io.write_out_bai:
        io.out_bai_path = os.path.join(d, "o.bai").encode()
    ao = _lib.LcdAlnOpt(*aln) if aln is not None else None
    st, ist, fo, rst, sst = _lib.LcdFileStats(), _lib.LcdIndexStats(), _lib.LcdVcfFieldsOut(), _lib.LcdRefineStats(), _lib.LcdSamStats()
    ist.built_bai = fo.n_te_seqs = 7; rst.n_records = sst.n_records = 7
    ro = _lib.LcdRunOpt(idx=ptr(io), fields=ptr(fields), aln=ptr(ao))
    out = _lib.LcdRunOut(idx_stats=C.pointer(ist), fields_out=C.pointer(fo), refine_stats=C.pointer(rst), sam_stats=C.pointer(sst))
    rc = lib.lcd_call_files(ptr(inp), None if "job" in null else C.byref(job), None if "cfg" in null else C.byref(cfg), C.byref(ro), None if "stats" in null else C.byref(st),
                            C.byref(out))
    assert (ist.built_bai, fo.n_te_seqs, rst.n_records, sst.n_records) == (0, 0, 0, 0)      # every named output is zeroed on a refusal path too
    return rc


def _regions(lib, _lib, align, d, bam_out="o.bam", idx=None, fields=None, aln=None, cfg_kw=None, null=()):
    cfg = align.call_cfg(0, **(cfg_kw or {}))
    bo = _lib.LcdBamOut()
    if bam_out is not None:
        bo.path = None if bam_out == "nopath" else os.path.join(d, bam_out).encode()
    rb, re_ = (C.c_int64 * 1)(1), (C.c_int64 * 1)(100)
    arr = (_lib.LcdCallChunk * 1)()
    recs, n_recs, text = C.POINTER(_lib.LcdVar1)(), C.c_int(0), C.c_void_p()
    io = _lib.LcdIndexOpt(*idx) if idx is not None else None
    ao = _lib.LcdAlnOpt(*aln) if aln is not None else None
    fo, rst = _lib.LcdVcfFieldsOut(), _lib.LcdRefineStats()
    fo.n_te_seqs = 7; rst.n_records = 7
    ro, out = _lib.LcdRunOpt(idx=ptr(io), fields=ptr(fields), aln=ptr(ao)), _lib.LcdRunOut(fields_out=C.pointer(fo), refine_stats=C.pointer(rst))
    rc = lib.lcd_call_bam_regions(None if "bam" in null else b"absent_in.bam", b"absent_in.bam.bai", b"absent_ref.fa", b"chr1", 1, rb, re_, 30,
                                  None if "cfg" in null else C.byref(cfg), arr, None if "records" in null else C.byref(recs), C.byref(n_recs), C.byref(text),
                                  C.byref(bo) if bam_out is not None else None, C.byref(ro), C.byref(out))
    assert (fo.n_te_seqs, rst.n_records) == (0, 0) and not text and not recs
    return rc


def _writer(lib, _lib, align, d, one_shot, path="o.bam", in_bam=b"absent_in.bam", block_payload=0, wopt=None, n=0, null_out=False):
    bo = _lib.LcdBamOut(); bo.path = os.path.join(d, path).encode() if path is not None else None; bo.block_payload = block_payload
    rst, sst = _lib.LcdRefineStats(), _lib.LcdSamStats()
    rst.n_records = sst.n_records = 7
    wo = _lib.LcdWriterOpt(refine_stats=C.pointer(rst), sam_stats=C.pointer(sst), **(wopt or {}))
    if wo.write_index:
        wo.index_path = os.path.join(d, "o.bai").encode()
    bop = None if null_out else C.byref(bo)
    # (an open answers with NULL and the message; the table's -4 for its rows is the code lcd_write_phased gives for the same refusal)
    rc = lib.lcd_write_phased(in_bam, n, None, bop, C.byref(wo)) if one_shot else (-4 if not lib.lcd_bam_writer_open(in_bam, bop, C.byref(wo)) else 0)
    assert (rst.n_records, sst.n_records) == (0, 0)
    return rc


BAM, SAM = 0, 1
VF_ALL = lambda _lib: _lib.LcdVcfFields(None, 0, 2)
ROWS = [
    # ---- the whole-file run ----
    ("files: NULL job", _files, dict(null=("job",)), -4, W_FILES + "NULL argument"),
    ("files: NULL cfg", _files, dict(null=("cfg",)), -4, W_FILES + "NULL argument"),
    ("files: NULL stats", _files, dict(null=("stats",)), -4, W_FILES + "NULL argument"),
    ("files: neither in nor job->bam_path", _files, dict(job_kw=dict(bam_path=None)), -4, W_FILES + "NULL argument"),
    ("files: no FASTA", _files, dict(job_kw=dict(fasta_path=None)), -4, W_FILES + "NULL argument"),
    ("files: write_out_bai without bam_out", _files, dict(bam_out=None, idx=(0, 0, 1, None, 0)), -4, W_FILES + "write_out_bai needs bam_out"),
    ("files: write_out_bai without a job", _files, dict(null=("job",), idx=(0, 0, 1, None, 0)), -4, W_FILES + "write_out_bai needs bam_out"),
    ("files: negative slab_members", _files, dict(idx=(1, 1, 1, None, -1)), -4, W_FILES + "negative slab_members"),
    ("files: bam_out without a path", _files, dict(bam_out="nopath"), -4, W_FILES + "bam_out without a path"),
    ("files: format 2", _files, dict(aln=(2, 0)), -4, W_FILES + "format must be LCD_ALN_BAM or LCD_ALN_SAM"),
    ("files: format -1", _files, dict(aln=(-1, 0)), -4, W_FILES + "format must be LCD_ALN_BAM or LCD_ALN_SAM"),
    ("files: SAM with write_out_bai", _files, dict(bam_out="o.sam", aln=(SAM, 0), idx=(1, 1, 1, None, 0)), -4, W_FILES + "a SAM output has no index"),
    ("files: SAM on - and VCF on -", _files, dict(bam_out="-", vcf="-", aln=(SAM, 0)), -4, W_FILES + "the SAM output and the VCF cannot both go to stdout"),
    ("files: SAM on - and VCF path NULL", _files, dict(bam_out="-", vcf=None, aln=(SAM, 0)), -4, W_FILES + "the SAM output and the VCF cannot both go to stdout"),
    ("files: refine with fields, BAM", _files, dict(aln=(BAM, 1), fields=VF_ALL), -2, W_FILES + "refined alignments together with the VCF fields"),
    ("files: refine with fields, SAM", _files, dict(bam_out="o.sam", aln=(SAM, 1), fields=VF_ALL), -2, W_FILES + "refined alignments together with the VCF fields"),
    ("files: somatic", _files, dict(cfg_kw=dict(clean=dict(out_somatic=1))), -2, W_FILES + "somatic / refine mode is not supported"),
    ("files: collect_ref_read_aln_str", _files, dict(cfg_kw=dict(opt=dict(collect_ref_read_aln_str=1))), -2, W_FILES + "somatic / refine mode is not supported"),
    ("files: negative window_chunks", _files, dict(job_kw=dict(window_chunks=-1)), -4, W_FILES + "negative window_chunks"),
    ("files: overlap 2", _files, dict(job_kw=dict(overlap=2)), -4, W_FILES + "negative window_chunks / loader_threads / chunk_len, or overlap outside -1 ... 1"),
    ("files: rnames_mode 3", _files, dict(fields=lambda _lib: _lib.LcdVcfFields(None, 0, 3)), -4, W_FILES + "rnames_mode"),
    ("files: te_kmer_len 16", _files, dict(fields=lambda _lib: _lib.LcdVcfFields(None, 16, 0)), -4, W_FILES + "te_kmer_len"),
    ("files: an unreadable TE file", _files, dict(fields=lambda _lib: _lib.LcdVcfFields(b"absent_te.fa", 0, 0)), -30, "absent_te.fa"),
    ("files: 0 inputs", _files, dict(inputs=[]), -4, W_FILES + "the number of inputs must be 1 ... LCD_MAX_INPUTS"),
    ("files: 65 inputs", _files, dict(inputs=[b"absent_in.bam"] * 65), -4, W_FILES + "the number of inputs must be 1 ... LCD_MAX_INPUTS"),
    ("files: a NULL input path", _files, dict(inputs=[b"absent_in.bam", None]), -4, W_FILES + "NULL input path"),
    ("files: job->bam_path is not the first input", _files, dict(inputs=[b"absent_in.bam", b"b.bam"], job_kw=dict(bam_path=b"b.bam")), -4,
     W_FILES + "job->bam_path must be NULL or the first input"),
    ("files: a missing index without lcd_index_opt_t", _files, dict(), -30, W_FILES + "cannot open the index absent_in.bam.bai"),
    ("files: a missing index without build_missing_bai", _files, dict(idx=(0, 1, 0, None, 0)), -30, "build_missing_bai would build it"),
    # ---- the regions driver ----
    ("regions: NULL bam_path", _regions, dict(null=("bam",)), -4, W_REGIONS + "NULL argument"),
    ("regions: NULL cfg", _regions, dict(null=("cfg",)), -4, W_REGIONS + "NULL argument"),
    ("regions: NULL records", _regions, dict(null=("records",)), -4, W_REGIONS + "NULL argument"),
    ("regions: bam_out without a path", _regions, dict(bam_out="nopath"), -4, W_REGIONS + "bam_out without a path"),
    ("regions: SAM", _regions, dict(aln=(SAM, 0)), -2, W_REGIONS + "SAM text is not supported by this driver"),
    ("regions: idx", _regions, dict(idx=(1, 1, 1, None, 0)), -4, W_REGIONS + "index options are not supported by this driver"),
    ("regions: format 2", _regions, dict(aln=(2, 0)), -4, W_REGIONS + "format must be LCD_ALN_BAM or LCD_ALN_SAM"),
    ("regions: refine with fields", _regions, dict(aln=(BAM, 1), fields=VF_ALL), -2, W_REGIONS + "refined alignments together with the VCF fields"),
    ("regions: somatic", _regions, dict(cfg_kw=dict(clean=dict(out_somatic=1))), -2, W_REGIONS + "somatic / refine mode is not supported"),
    ("regions: rnames_mode -1", _regions, dict(fields=lambda _lib: _lib.LcdVcfFields(None, 0, -1)), -4, W_REGIONS + "rnames_mode"),
    # ---- the writer ----
    ("open: NULL input", _writer, dict(one_shot=False, in_bam=None), -4, W_OPEN + "NULL argument"),
    ("open: NULL out", _writer, dict(one_shot=False, null_out=True), -4, W_OPEN + "NULL argument"),
    ("open: out without a path", _writer, dict(one_shot=False, path=None), -4, W_OPEN + "NULL argument"),
    ("open: format 2", _writer, dict(one_shot=False, wopt=dict(format=2)), -4, W_OPEN + "format must be LCD_ALN_BAM or LCD_ALN_SAM"),
    ("open: SAM with write_index", _writer, dict(one_shot=False, path="o.sam", wopt=dict(format=SAM, write_index=1)), -4, W_OPEN + "a SAM output has no index"),
    ("open: block_payload -1", _writer, dict(one_shot=False, block_payload=-1), -4, W_OPEN + "block_payload must be 0 or 1 ... 0xff00"),
    ("open: block_payload 0xff01", _writer, dict(one_shot=False, block_payload=0xff01), -4, W_OPEN + "block_payload must be 0 or 1 ... 0xff00"),
    ("open: block_payload 0xff01, indexed", _writer, dict(one_shot=False, block_payload=0xff01, wopt=dict(write_index=1)), -4, W_OPEN + "block_payload must be 0 or 1 ... 0xff00"),
    ("write: NULL input", _writer, dict(one_shot=True, in_bam=None), -4, W_WRITE + "NULL argument"),
    ("write: NULL out", _writer, dict(one_shot=True, null_out=True), -4, W_WRITE + "NULL argument"),
    ("write: out without a path", _writer, dict(one_shot=True, path=None), -4, W_WRITE + "NULL argument"),
    ("write: n < 0", _writer, dict(one_shot=True, n=-1), -4, W_WRITE + "NULL argument"),
    ("write: chunks NULL with n 1", _writer, dict(one_shot=True, n=1), -4, W_WRITE + "NULL argument"),
    ("write: SAM, chunks NULL with n 1", _writer, dict(one_shot=True, path="o.sam", n=1, wopt=dict(format=SAM)), -4, W_WRITE + "NULL argument"),
    ("write: format -1", _writer, dict(one_shot=True, wopt=dict(format=-1)), -4, W_WRITE + "format must be LCD_ALN_BAM or LCD_ALN_SAM"),
    ("write: SAM with write_index", _writer, dict(one_shot=True, path="o.sam", wopt=dict(format=SAM, write_index=1)), -4, W_WRITE + "a SAM output has no index"),
    ("write: block_payload 0xff01", _writer, dict(one_shot=True, block_payload=0xff01), -4, W_WRITE + "block_payload must be 0 or 1 ... 0xff00"),
]


@pytest.mark.parametrize("name,driver,kw,code,fragment", ROWS, ids=[r[0] for r in ROWS])
def test_refused_before_any_output_exists(lcd, tmp_path, monkeypatch, name, driver, kw, code, fragment):
    from longcalld_amd import _lib, align
    lib = lcd.load_library()
    d = str(tmp_path / "out")
    os.mkdir(d)
    monkeypatch.chdir(tmp_path)                       # the inputs' relative names: nothing of that name exists, nothing may appear
    kw = dict(kw)
    if callable(kw.get("fields")):
        kw["fields"] = kw["fields"](_lib)
    rc = driver(lib, _lib, align, d, **kw)
    msg = lib.lcd_last_error().decode()
    assert rc == code and fragment in msg, (name, rc, msg)
    assert os.listdir(d) == [] and os.listdir(str(tmp_path)) == ["out"]


def test_the_writer_does_not_refuse_what_the_sam_path_ignores(lcd, tmp_path, monkeypatch):
    """block_payload is the BAM writer's: the SAM writer accepts any value and fails on its input only"""
    from longcalld_amd import _lib, align
    lib = lcd.load_library()
    monkeypatch.chdir(tmp_path)
    assert _writer(lib, _lib, align, str(tmp_path), one_shot=True, path="o.sam", block_payload=-1, wopt=dict(format=SAM)) == -30
    assert b"absent_in.bam" in lib.lcd_last_error() and os.listdir(str(tmp_path)) == []
