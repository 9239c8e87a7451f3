"""lcd_vcf_writer_open_idx: the VCF writer that indexes what it compresses.  The index equals the oracle's index of the finished file, the .vcf.gz bytes equal those
of lcd_vcf_writer_open on the same appends, an out-of-order append completes the VCF without an index and says so, abort leaves no index."""
import os

import pytest

import vcf_index_common as vc

pytestmark = pytest.mark.gpu


def appends():
    """empty; one line; several that end without filling a member; one larger than three members (with lines that straddle its members)"""
    big = b"".join(vc.line(b"c2", 100 + 13 * i, b"A", b"A" + b"ACGT" * (i % 50), info=b"SVTYPE=INS;END=%d" % (101 + 13 * i)) for i in range(3200))
    assert len(big) > 3 * 65280
    return ["", vc.line(b"c1", 7).decode(), "".join(vc.line(b"c1", 100 + i).decode() for i in range(40)), vc.line(b"c1", 9000, b"N", b"<DEL>", info=b"END=120000").decode(),
            "", big.decode(), vc.line(b"c3", 1).decode()]


HEADER = vc.header([(b"c1", 200000), (b"c2", 100000), (b"c3", 5)]).decode()


@pytest.mark.parametrize("fmt", [vc.TBI, vc.CSI])
def test_index_equals_oracle_and_the_file_is_unchanged(lcd, tmp_path, fmt):
    plain, idxd = str(tmp_path / "plain.vcf.gz"), str(tmp_path / "idx.vcf.gz")
    before = lcd.load_library().lcd_device_bytes(0)
    assert lcd.vcf_write(plain, appends(), bgzf=1, header_text=HEADER) is None
    st = lcd.vcf_write(idxd, appends(), bgzf=1, header_text=HEADER, index=fmt)
    assert lcd.load_library().lcd_device_bytes(0) == before
    gz = open(idxd, "rb").read()
    assert gz == open(plain, "rb").read() and vc.ends_with_eof_member(gz)              # the index does not change the file
    scan = vc.scan_vcf(gz, fmt)
    assert any(n == 65280 for _c, _u, n in scan["tab"]) and sum(1 for x in scan["lines"] if sum(1 for _c, u, n in scan["tab"] if n and u < x["u1"] and u + n > x["u0"]) == 2) >= 3
    assert any(x["vend"] & 0xffff == 0 for x in scan["lines"][:-1])                     # an append's last line ends exactly at a member's end
    image = open(f"{idxd}.{fmt}", "rb").read()
    assert vc.ends_with_eof_member(image) and vc.inflate(image) == vc.oracle_index(scan, fmt)
    assert (st["wrote"], st["skipped"], st["n_data_lines"], st["n_contigs"]) == (1, 0, len(scan["lines"]), 3) and not os.path.exists(plain + "." + fmt)


def test_index_path_and_header_only(lcd, tmp_path):
    p, ip = str(tmp_path / "h.vcf.gz"), str(tmp_path / "elsewhere.tbi")
    st = lcd.vcf_write(p, [], bgzf=1, header_text=HEADER, index="tbi", index_path=ip)
    assert st["wrote"] == 1 and not os.path.exists(p + ".tbi")
    assert vc.inflate(open(ip, "rb").read()) == vc.oracle_tbi(vc.scan_vcf(open(p, "rb").read()))


def test_out_of_order_append_completes_the_vcf_without_an_index(lcd, tmp_path):
    p = str(tmp_path / "o.vcf.gz")
    texts = [vc.line(b"c1", 500).decode(), vc.line(b"c1", 400).decode(), vc.line(b"c1", 600).decode()]
    st = lcd.vcf_write(p, texts, bgzf=1, header_text=HEADER, index="tbi")
    assert vc.inflate(open(p, "rb").read()).decode() == HEADER + "".join(texts) and vc.ends_with_eof_member(open(p, "rb").read())
    assert st["skipped"] == -55 and st["wrote"] == 0 and "data line 1 " in st["skip_reason"] and not os.path.exists(p + ".tbi")
    # an interval TBI cannot hold: -56, and the same appends index as CSI
    far = [vc.line(b"c1", 5).decode(), vc.line(b"c1", (1 << 29) + 9).decode()]
    st = lcd.vcf_write(p, far, bgzf=1, header_text=vc.header().decode(), index="tbi")
    assert st["skipped"] == -56 and "ask for CSI" in st["skip_reason"] and not os.path.exists(p + ".tbi")
    assert lcd.vcf_write(p, far, bgzf=1, header_text=vc.header().decode(), index="csi")["depth"] == 6


def test_a_malformed_line_fails_the_append_and_abort_leaves_no_index(lcd, tmp_path):
    p = str(tmp_path / "a.vcf.gz")
    with pytest.raises(lcd.LcdError) as e:
        lcd.vcf_write(p, [vc.line(b"c1", 5).decode(), "c1\tx\t.\tA\tC\t.\t.\t.\n"], bgzf=1, header_text=HEADER, index="tbi")
    assert "error -57:" in str(e.value) and "data line 1 " in str(e.value) and not os.path.exists(p + ".tbi")
    assert lcd.vcf_write(p, [vc.line(b"c1", 5).decode()], bgzf=1, header_text=HEADER, index="csi", abort=True)["wrote"] == 0
    assert not os.path.exists(p + ".csi") and not vc.ends_with_eof_member(open(p, "rb").read())
