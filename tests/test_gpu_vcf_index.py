"""lcd_vcf_index_build on the device (vcf_index_kernel.hip behind the inflate kernel) against the pure-Python oracle of tests/vcf_index_common.py: every named case
byte for byte on the DECOMPRESSED index at slab_members 0 and 1 with the device ledger unchanged, the file on disk a valid BGZF file that ends in the EOF member,
the independence of the bytes from the slab size, the refusals, and the region reader's property on a device-built index."""
import gzip
import os

import numpy as np
import pytest

import vcf_index_common as vc

pytestmark = pytest.mark.gpu


def ledger(lcd):
    return lcd.load_library().lcd_device_bytes(0)


def build(lcd, tmp_path, gz, tag, fmt, slab_members=0):
    path = str(tmp_path / f"{tag}.vcf.gz")
    if not os.path.exists(path):
        open(path, "wb").write(gz)
    out = str(tmp_path / f"{tag}.{slab_members}.{fmt}")
    st = lcd.vcf_index_build(path, out, fmt=fmt, slab_members=slab_members)
    image = open(out, "rb").read()
    assert vc.ends_with_eof_member(image) and st["bytes_file"] == len(image) and st["wrote"] == 1
    return vc.inflate(image), st


@pytest.mark.parametrize("name", [n for n in vc.CASES if not n.startswith("refused_")])
def test_named_cases_equal_the_oracle(lcd, tmp_path, name):
    gz, fmt, pred, _ = vc.CASES[name]()
    s = vc.scan_vcf(gz, fmt)
    want = vc.oracle_index(s, fmt)
    assert pred(s, vc.parse_index(want))
    before = ledger(lcd)
    for sm in (0, 1):
        got, st = build(lcd, tmp_path, gz, name, fmt, sm)
        assert got == want, (name, sm)
        assert (st["n_data_lines"], st["n_meta_lines"], st["n_contigs"], st["bytes_index"]) == (len(s["lines"]), s["n_meta"], len(s["names"]), len(want))
    assert ledger(lcd) == before


def test_default_output_path_and_both_formats_of_one_file(lcd, tmp_path):
    gz = vc.seeded_gz(vc.SEEDS[1], 200)
    path = str(tmp_path / "d.vcf.gz")
    open(path, "wb").write(gz)
    for fmt in (vc.TBI, vc.CSI):
        lcd.vcf_index_build(path, fmt=fmt)
        assert vc.inflate(open(f"{path}.{fmt}", "rb").read()) == vc.oracle_index(vc.scan_vcf(gz, fmt), fmt)


@pytest.mark.parametrize("seed", vc.SEEDS[:3])
def test_the_index_does_not_depend_on_the_slabs(lcd, tmp_path, seed):
    gz = vc.seeded_gz(seed, 300, seed % 2 == 1)
    for fmt in (vc.TBI, vc.CSI):
        s = vc.scan_vcf(gz, fmt)
        assert {n for _c, _u, n in s["tab"]} & {1, 300, 2000}                            # members smaller than a line: lines straddle members
        want = vc.oracle_index(s, fmt)
        slabs = {}
        for sm in (1, 2, 3, 7, 0):
            got, st = build(lcd, tmp_path, gz, f"s{seed}", fmt, sm)
            assert got == want, (seed, fmt, sm)
            slabs[sm] = st["n_slabs"]
        assert slabs[0] == 1 and slabs[1] > slabs[7] >= 1 and slabs[1] > 8


@pytest.mark.parametrize("name", [n for n in vc.CASES if n.startswith("refused_")])
def test_refusals_leave_nothing_behind(lcd, tmp_path, name):
    gz, fmt, _, (code, no) = vc.CASES[name]()
    path, out = str(tmp_path / "r.vcf.gz"), str(tmp_path / "r.idx")
    open(path, "wb").write(gz)
    before = ledger(lcd)
    for sm in (0, 1):
        with pytest.raises(lcd.LcdError) as e:
            lcd.vcf_index_build(path, out, fmt=fmt, slab_members=sm)
        assert f"error {code}:" in str(e.value) and f"data line {no}" in str(e.value), str(e.value)
        if code == vc.ERR_CSI:
            assert "ask for CSI" in str(e.value)
        assert not os.path.exists(out) and ledger(lcd) == before
    if code == vc.ERR_CSI:                                                               # the same file is a CSI file of depth 6
        got, st = build(lcd, tmp_path, gz, "as_csi", vc.CSI)
        assert got == vc.oracle_csi(vc.scan_vcf(gz, vc.CSI)) and st["depth"] == 6 and vc.parse_csi(got)["depth"] == 6


def test_depth_from_the_header_that_does_not_hold_a_line(lcd, tmp_path):
    gz = vc.build_gz(vc.header([(b"c1", 1000000)]) + vc.line(b"c1", 5) + vc.line(b"c1", (1 << 29) + 77))
    path, out = str(tmp_path / "h.vcf.gz"), str(tmp_path / "h.csi")
    open(path, "wb").write(gz)
    before = ledger(lcd)
    with pytest.raises(lcd.LcdError) as e:
        lcd.vcf_index_build(path, out, fmt="csi")
    assert "error -56:" in str(e.value) and not os.path.exists(out) and ledger(lcd) == before


def test_files_that_are_not_bgzf(lcd, tmp_path):
    text = vc.seeded_text(5, 20)
    plain, gz, out = str(tmp_path / "p.vcf"), str(tmp_path / "g.vcf.gz"), str(tmp_path / "o.tbi")
    open(plain, "wb").write(text)
    open(gz, "wb").write(gzip.compress(text))
    for path, word in ((plain, "plain text"), (gz, "plain gzip")):
        with pytest.raises(lcd.LcdError) as e:
            lcd.vcf_index_build(path, out)
        assert "error -33:" in str(e.value) and word in str(e.value) and not os.path.exists(out)


def test_region_reader_on_a_device_built_index(lcd, tmp_path):
    seed = vc.SEEDS[2]
    gz = vc.seeded_gz(seed, 300)
    scan = vc.scan_vcf(gz, vc.CSI)
    rng = np.random.default_rng(seed)
    idxs = [vc.parse_index(build(lcd, tmp_path, gz, "rr", fmt, 2)[0]) for fmt in (vc.TBI, vc.CSI)]
    n = 0
    for tid in range(len(scan["names"])):
        for beg, end in vc.regions_for(rng, scan, tid, 40):
            want = vc.lines_by_scan(scan, tid, beg, end)
            for idx in idxs:
                assert vc.lines_through_index(scan, idx, tid, beg, end) == want, (idx["fmt"], tid, beg, end)
            n += bool(want)
    assert n >= 50
