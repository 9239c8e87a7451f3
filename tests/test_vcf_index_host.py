"""lcd_tbx_from_records (longcalld_amd/csrc/lcd_index_host.cpp, pure host code: the library is loaded, no device is needed) against the Python oracle, byte for
byte, for both formats."""
import numpy as np
import pytest

import vcf_index_common as vc
from longcalld_amd import align


def _table(scan):
    ls = scan["lines"]
    return ([x["tid"] for x in ls], [x["beg"] for x in ls], [x["end"] for x in ls], np.array([x["vbeg"] for x in ls], np.uint64), np.array([x["vend"] for x in ls], np.uint64))


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_finisher_equals_oracle_on_named_cases(name):
    gz, fmt, _pred, refusal = vc.CASES[name]()
    if refusal is not None:
        if refusal[0] == vc.ERR_LINE:
            return                                      # (a malformed line never becomes a table row)
        # the table of the file as a CSI scan accepts it, except that the order cases stop the scan itself: build their rows by hand
        rows = {"refused_pos_decreasing": ([b"c1"], [0, 0, 0], [499, 699, 698]), "refused_contig_reappears": ([b"c1", b"c2"], [0, 1, 0], [499, 4, 899]),
                "refused_end_over_2_29_tbi": ([b"c1"], [0, 0], [99, (1 << 29) + 4])}[name]
        n = len(rows[1])
        with pytest.raises(align.LcdError) as e:
            align.tbx_from_records(fmt, rows[0], rows[1], rows[2], [b + 1 for b in rows[2]], np.arange(n, dtype=np.uint64) << 16, (np.arange(n, dtype=np.uint64) + 1) << 16)
        assert f"error {refusal[0]}:" in str(e.value) and f"data line {refusal[1]}" in str(e.value)
        return
    scan = vc.scan_vcf(gz, fmt)
    assert align.tbx_from_records(fmt, scan["names"], *_table(scan), max_contig_len=scan["max_clen"]) == vc.oracle_index(scan, fmt)


@pytest.mark.parametrize("seed", vc.SEEDS[:4])
@pytest.mark.parametrize("fmt", [vc.TBI, vc.CSI])
def test_finisher_equals_oracle_on_seeded_files(seed, fmt):
    scan = vc.scan_vcf(vc.seeded_gz(seed, 400, seed % 2 == 0), fmt)
    assert align.tbx_from_records(fmt, scan["names"], *_table(scan), max_contig_len=scan["max_clen"]) == vc.oracle_index(scan, fmt)


def test_depth_from_header_that_does_not_hold_the_file():
    with pytest.raises(align.LcdError) as e:
        align.tbx_from_records("csi", [b"c"], [0], [5], [(1 << 29) + 9], [0], [1 << 16], max_contig_len=1000)
    assert "error -56:" in str(e.value)
    assert vc.parse_csi(align.tbx_from_records("csi", [b"c"], [0], [5], [(1 << 29) + 9], [0], [1 << 16]))["depth"] == 6


def test_bad_arguments():
    for args in (("tbi", [b"c"], [1], [5], [9], [0], [1]), ("tbi", [b"c"], [0], [5], [5], [0], [1]), ("tbi", [b"c"], [0], [-1], [5], [0], [1])):
        with pytest.raises(align.LcdError) as e:
            align.tbx_from_records(*args)
        assert "error -4:" in str(e.value)
