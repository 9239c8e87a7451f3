"""inflate_kernel.hip on deflate streams that no zlib writer produces: the case tables of tests/inflate_streams.py, written token by token and bit by bit, through
lcd_bgzf_inflate_dev.  tests/test_inflate_streams_oracle.py proves on the CPU that zlib accepts every valid case with exactly the expected bytes, refuses every
refusal, and that each table covers what it says: match geometry against the 2 KB ring (A), code shapes on both sides of the 10- / 9-bit primary tables and the
run-length tokens of a dynamic header (B), every alignment of a stream in the 256-byte input windows (C), refusals (D), the container's limits (E) and one BAM
re-packed by this writer (F)."""
import ctypes as C
import gzip

import numpy as np
import pytest

import inflate_streams as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from longcalld_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.lcd_bgzf_inflate_dev.restype = C.c_void_p
    L.lcd_bgzf_inflate_dev.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    L.lcd_inflated_size.restype = C.c_size_t
    L.lcd_inflated_size.argtypes = [C.c_void_p]
    L.lcd_inflated_n_blocks.restype = C.c_size_t
    L.lcd_inflated_n_blocks.argtypes = [C.c_void_p]
    L.lcd_inflated_to_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_char_p]
    L.lcd_inflated_free.argtypes = [C.c_void_p]
    L.lcd_inflated_free.restype = None
    L.lcd_io_last_error.restype = C.c_char_p
    return L


def _inflate(lib, image, verify):
    """-> (the inflated stream | None, non-empty blocks)"""
    h = lib.lcd_bgzf_inflate_dev(image, len(image), verify)
    if not h:
        return None, 0
    n, nb = lib.lcd_inflated_size(h), lib.lcd_inflated_n_blocks(h)
    out = C.create_string_buffer(max(n, 1))
    assert lib.lcd_inflated_to_host(h, 0, n, out) == 0
    lib.lcd_inflated_free(h)
    return out.raw[:n], nb


def _same(lib, case, verify=1):
    got, nb = _inflate(lib, case.image, verify)
    assert got is not None, (case.name, lib.lcd_io_last_error())
    if got != case.expected:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(case.expected, np.uint8)
        n = min(len(a), len(b))
        bad = np.flatnonzero(a[:n] != b[:n])
        at = int(bad[0]) if len(bad) else n
        m = next((m for m in case.members if m.uoff <= at < m.uoff + m.ulen), case.members[-1])
        pytest.fail("%s: %d bytes for %d; the first wrong byte is byte %d of member %s (%d wrong bytes in all)" % (case.name, len(a), len(b), at - m.uoff, m.name, len(bad)))
    assert nb == sum(1 for m in case.members if m.ulen)


def test_a_match_geometry_against_the_ring(lib):
    """every distance x length x start phase of the table, each match at its planned output position; sources at byte 0 of the block and 32 768 back.  (The switch
    between ring and HBM may sit anywhere up to the ring's size: a lane reads its source byte strides before the same copy overwrites that slot.  What this table
    catches is a switch beyond the ring, a copy path that takes the wrong bytes, or a half that is flushed late.)"""
    for case in S.group_a():
        _same(lib, case)


def test_b_code_shapes(lib):
    """codes on both sides of the primary tables, the all-ones 15-bit code, HLIT / HDIST / HCLEN at their ends, run-length tokens at the edges of the 64-entry
    window that collects code lengths, block sequences that leave stale tables behind, stored headers at every bit offset"""
    for case in S.group_b():
        _same(lib, case)


def test_c_input_windows(lib):
    """every residue modulo 256 of a stream's first byte and of its end, the final bit at every position, LEN / NLEN across a window's edge, the reader restarted
    behind stored bytes at the edge: all valid, none may be refused"""
    for case in S.group_c():
        for verify in (0, 1):
            _same(lib, case, verify)


def test_d_refusals(lib):
    """Every stream is refused by zlib and sits between two valid members; the handle is NULL with and without the CRC check, the message names the member and
    carries the text of its class.  These are refusals of bad input, read off the kernel before they were run:
      * every store to the output goes through flush_half from ring bytes [flushed, pos), and pos <= ISIZE is checked before each literal (pos >= ulen), match
        (pos + len > ulen) and stored copy (pos + len > ulen): stores stay inside [dst, dst + ISIZE) for every class, the three `one over ISIZE` ones included;
      * every load of compressed bytes is a window load below lim + 256, lim <= stream end + 8 + 255, or a stored byte checked against the stream's end: inside the
        image's 1 024 spare bytes;
      * a distance before the block's start is refused (dist > pos) before `from` is used, so the HBM path never reads in front of dst;
      * bad symbols (286, 287, distance 30, 31) are refused before they index the lane tables; HLIT / HDIST above their limits before a length is stored;
      * over-subscribed sets leave build_table before any sorted-symbol or table store; a leading repeat, a run past HLIT + HDIST and a missing end-of-block code
        are refused before or right after the lengths are stored (n + rep <= 316 entries of lens[336]);
      * the unused pattern of a 1-bit code finds an empty table entry, then walks counts that sum to one symbol: no index beyond symt[0];
      * one byte short of ISIZE ends with pos < ulen: nothing is stored behind pos."""
    for case in S.group_d():
        why = dict(case.members[case.refused].claims)["why"]
        for verify in (0, 1):
            got, _ = _inflate(lib, case.image, verify)
            assert got is None, (case.name, verify)
            err = lib.lcd_io_last_error()
            assert why in err and b"BGZF block %d:" % case.refused in err, (case.name, verify, err)


def test_lenient_classes_are_pinned(lib):
    """Two classes that zlib refuses or cuts off.  The decoder builds its tables from any set of lengths that is not over-subscribed and checks only that the stream
    ends inside the member, so on paper it accepts an incomplete code whose missing patterns never occur, and bytes behind the final block inside BSIZE.  Accepted
    is pinned here, with exactly expand()'s bytes around and inside the member"""
    for case in S.group_lenient():
        for verify in (0, 1):
            _same(lib, case, verify)


def test_e_container_limits(lib):
    """ISIZE 65 536 from a few hundred bytes of stream; members of ISIZE 0 in the middle leave the stream unchanged and are not counted"""
    case, = S.group_e()
    _same(lib, case)
    assert sum(1 for m in case.members if m.ulen) == 3 and len(case.members) == 6


def test_f_a_bam_repacked_by_the_writer_loads_like_the_host_loader(lcd, lib, tmp_path):
    """the BAM of tests/test_io.py re-packed into members of this writer (stored / fixed / dynamic / two blocks, odd sizes so that records straddle members, empty
    members and extra subfields in between) and indexed: the device path (inflate_kernel.hip -> record walk -> chunk) == the host loader, which inflates the same
    file with zlib"""
    from test_gpu_bamdev import _host_reads, _same_chunk
    from test_io import BamReads, _make_bam, _write_bai
    lib.lcd_bam_load_region_indexed.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(BamReads)]
    rng = np.random.default_rng(21)
    src = str(tmp_path / "t.bam")
    recs = _make_bam(rng, src, n=200)
    data = gzip.open(src, "rb").read()
    image, blocks = S.repack(data)
    got, nb = _inflate(lib, image, 1)
    assert got == data and nb == len(blocks)
    path = str(tmp_path / "repacked.bam")
    open(path, "wb").write(image)
    for x in recs:
        x["vbeg"], x["vend"] = S.virtual_offset(blocks, x["u0"]), S.virtual_offset(blocks, x["u1"], end=True)
    _write_bai(path + ".bai", 2, recs)
    n_reads = 0
    for chrom, beg, end, mq, tlen in (("chr11", 1, 2000000, 0, 2000000), ("chr11", 300000, 420000, 30, 2000000), ("chr11", 900000, 1300000, 10, 2000000), ("chrA", 1, 50000, 0, 50000)):
        h = _host_reads(lib, path, chrom, beg, end, mq)
        dev = lcd.DeviceChunk.from_bam(path, path + ".bai", chrom, beg, end, min_mapq=mq)
        ref = _same_chunk(lcd, dev, h, beg, end, tlen)
        n_reads += h["n"]
        if ref is not None:
            ref.close()
        dev.close()
    assert n_reads > 150
