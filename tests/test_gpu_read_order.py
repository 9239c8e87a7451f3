"""lcd_chunk_read_nm on the MI355X: bam_get_NM (src/bam_utils.c:1632-1639) of a BAM chunk's records, read where the inflate left them in HBM, and the read order
sort_chunk_reads (:1641) makes of it.  The 16 records of tests/call_chunks_common.py::nm_records carry all six integer types, a negative c, a Z- / A- / f-typed NM,
no NM, an NM behind a 4.9 kb cs:Z field, behind a valid B array, behind a B array and a Z value that run past the record (0: the field does not exist), two NM
fields, and sit at every byte offset modulo 4."""
import numpy as np
import pytest

import call_chunks_common as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nm_chunk(lcd, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("nm") / "n.bam")
    recs = kc.write_aux_bam(path, kc.nm_records())
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", 1, 5000, min_mapq=30)
    yield dev, recs
    dev.close()


def test_read_nm_equals_the_written_values(lcd, nm_chunk):
    dev, recs = nm_chunk
    assert dev.n == 16 and dev.meta["names"] == [r["name"] for r in recs]
    assert (dev.read_info()["status"] == 0).all()
    before = lcd.copy_counters()
    nm = lcd.chunk_read_nm(dev)
    assert nm.tolist() == [r["nm"] for r in recs]
    assert lcd.copy_counters() == before                       # no digar and no base crossed PCIe
    assert lcd.chunk_read_nm(dev).tolist() == nm.tolist()


def test_order_from_the_device_nm_equals_the_python_sort(lcd, nm_chunk):
    dev, recs = nm_chunk
    m = dev.meta
    assert m["pos0"].tolist() == [r["pos0"] for r in recs] and m["end_pos"].tolist() == [r["pos0"] + r["qlen"] for r in recs]
    got = lcd.sort_chunk_reads(m["pos0"], m["end_pos"], lcd.chunk_read_nm(dev), m["names"])
    want = kc.python_order([r["pos0"] for r in recs], [r["pos0"] + r["qlen"] for r in recs], [r["nm"] for r in recs], [r["name"] for r in recs])
    assert got.tolist() == want.tolist()
    assert got.tolist() != list(range(16))


def test_chunk_with_a_source_choice_reads_the_same_nm(lcd, tmp_path):
    """lcd_chunk_create_from_bam_src runs lcd_bam_aux_kernel over the same fields; the NM walk is its own kernel and gives the same values"""
    path = str(tmp_path / "s.bam")
    recs = kc.write_aux_bam(path, kc.nm_records())
    ref = np.zeros(6000, np.uint8)
    dev = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", 1, 5000, min_mapq=30, src=(ref, 1, 6000, 1))
    assert lcd.chunk_read_nm(dev).tolist() == [r["nm"] for r in recs]
    dev.close()


def test_region_without_reads_and_host_array_chunk(lcd, tmp_path):
    path = str(tmp_path / "e.bam")
    kc.write_aux_bam(path, kc.nm_records())
    empty = lcd.DeviceChunk.from_bam(path, path + ".bai", "chr11", 50000, 60000, min_mapq=30)
    assert empty.n == 0 and lcd.chunk_read_nm(empty).tolist() == []
    empty.close()
    qlen = 40
    host = lcd.DeviceChunk([100], [np.array([(qlen << 4) | 7], np.uint32)], [np.full(qlen, 30, np.uint8)], [np.full(qlen // 2, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="-4"):
        lcd.chunk_read_nm(host)
    host.close()


def test_first_round_with_null_order_sorts_the_reads_and_host_chunk_is_refused(lcd, nm_chunk):
    """lcd_chunks_first_round without ordered_read_ids: the order comes from the chunk's meta and lcd_chunk_read_nm; is_rev from the flags"""
    dev, recs = nm_chunk
    item = dict(ref=np.zeros(6000, np.uint8), ref_beg=1, reg_beg=1, reg_end=5000)
    got = lcd.chunks_first_round([dev], [item])[0]
    want = kc.python_order([r["pos0"] for r in recs], [r["pos0"] + r["qlen"] for r in recs], [r["nm"] for r in recs], [r["name"] for r in recs])
    assert got["ordered_read_ids"].tolist() == want.tolist() and got["ordered_read_ids"].tolist() != list(range(16))
    assert got["is_skipped"].tolist() == [0] * 16 and got["cv"]["n_vars"] == 0 and got["cv"]["n_reads"] == 16
    given = lcd.chunks_first_round([dev], [dict(item, ordered_read_ids=np.arange(16), meta=False)])[0]
    assert given["ordered_read_ids"].tolist() == list(range(16))
    with pytest.raises(lcd.LcdError, match="-4"):
        lcd.chunks_first_round([dev], [dict(item, meta=False)])                   # a BAM chunk, but no meta to sort by
    qlen = 40
    host = lcd.DeviceChunk([100], [np.array([(qlen << 4) | 7], np.uint32)], [np.full(qlen, 30, np.uint8)], [np.full(qlen // 2, 0x11, np.uint8)], 1, 1000, 100000)
    with pytest.raises(lcd.LcdError, match="-4"):
        lcd.chunks_first_round([host], [dict(ref=np.zeros(2000, np.uint8), ref_beg=1, reg_beg=1, reg_end=1000)])
    host.close()
