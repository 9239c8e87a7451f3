"""The phased alignment output's entry points are declared in include/lcd_hotpath.h, listed in the Python loader and exported by the built library."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ["lcd_bgzf_deflate_dev", "lcd_bgzf_deflate_dev_ptr", "lcd_deflated_size", "lcd_deflated_n_blocks", "lcd_deflated_kernel_ms", "lcd_deflated_block_info",
       "lcd_deflated_to_host", "lcd_deflated_free", "lcd_chunk_tag_records", "lcd_tagged_dev_ptr", "lcd_tagged_size", "lcd_tagged_n_records", "lcd_tagged_to_host",
       "lcd_tagged_free", "lcd_write_phased", "lcd_call_bam_regions"]


def test_new_symbols_declared_listed_and_exported():
    from longcalld_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcd_hotpath.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/lcd_hotpath.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert "lcd_bam_out_t" in txt and "lcd_deflated_t" in txt and "lcd_tagged_t" in txt


def test_bam_out_struct_mirrors_the_header():
    """lcd_bam_out_t: two pointers, an int (padded), four int64, three doubles"""
    from longcalld_amd import _lib
    assert ctypes.sizeof(_lib.LcdBamOut) == 8 + 8 + 8 + 4 * 8 + 3 * 8
    assert [f[0] for f in _lib.LcdBamOut._fields_] == ["path", "pg_line", "block_payload", "n_records_out", "n_filtered_out", "bytes_inflated", "bytes_file", "ms_tag",
                                                       "ms_deflate", "ms_download_write"]


def test_arguments_are_checked_before_any_device_work():
    """no GPU needed: a bad block_payload, a NULL chunk and a writer without chunks fail with a message"""
    from longcalld_amd import _lib
    lib = _lib.load_library()
    assert lib.lcd_deflated_size(None) == 0 and lib.lcd_tagged_size(None) == 0 and lib.lcd_tagged_n_records(None) == 0
    assert not lib.lcd_chunk_tag_records(None, None, None, 0, 0) and b"not made from a BAM" in lib.lcd_last_error()
    bo = _lib.LcdBamOut(); bo.path = None
    assert lib.lcd_write_phased(b"x.bam", 0, None, ctypes.byref(bo), None) < 0 and b"NULL" in lib.lcd_last_error()
