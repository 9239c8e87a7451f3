"""BGZF blocks compressed on the device (deflate_kernel.hip, lcd_bgzf_deflate_dev): the checker is Python's zlib -- every member's container fields, its raw deflate
stream inflated to exactly its payload with no bits to spare -- and the project's own device inflate with the CRC check on.  The payload classes are those of
tests/test_gpu_inflate.py (rebuilt here); conditions on the sizes keep a compressor that finds no matches, or writes no dynamic codes, from passing."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import bam_out_common as bo

pytestmark = pytest.mark.gpu
LENGTHS = (0, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65280)
EOF_MEMBER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _payloads(rng):
    text = (b"ACGTTGCAAGGCTTAACCGGTTAACC" * 40 + bytes(rng.integers(33, 74, 600).astype(np.uint8))) * 30
    bam_like = b"".join(struct.pack("<iiBBHHHiiii", 1, int(p), 12, 60, 4680, 3, 0, 150, -1, -1, 0) + b"read/%07d\0" % i + bytes(rng.integers(0, 256, 75).astype(np.uint8))
                        + bytes(rng.integers(20, 45, 150).astype(np.uint8)) for i, p in enumerate(np.sort(rng.integers(0, 1 << 28, 200))))
    skew = bytes(np.minimum(rng.geometric(0.03, 60000), 255).astype(np.uint8))
    far = bytes(rng.integers(0, 256, 400).astype(np.uint8))
    far = far + bytes(rng.integers(0, 4, 32300).astype(np.uint8)) + far
    return dict(text=text[:65280], bam=bam_like[:65280], skew=skew, run=b"\x07" * 65280, one=b"Z", random=bytes(rng.integers(0, 256, 50000).astype(np.uint8)), far=far,
                zeros_then_text=b"\0" * 20000 + text[:30000])


@pytest.fixture(scope="module")
def P():
    return _payloads(np.random.default_rng(5))


@pytest.fixture(scope="module")
def inflate_dev():
    from longcalld_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.lcd_bgzf_inflate_dev.restype = C.c_void_p
    L.lcd_bgzf_inflate_dev.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    L.lcd_inflated_size.restype = C.c_size_t
    L.lcd_inflated_size.argtypes = [C.c_void_p]
    L.lcd_inflated_to_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_char_p]
    L.lcd_inflated_free.argtypes = [C.c_void_p]
    L.lcd_inflated_free.restype = None
    L.lcd_io_last_error.restype = C.c_char_p

    def run(image):
        h = L.lcd_bgzf_inflate_dev(image, len(image), 1)
        assert h, L.lcd_io_last_error()
        n = L.lcd_inflated_size(h)
        out = C.create_string_buffer(max(n, 1))
        assert L.lcd_inflated_to_host(h, 0, n, out) == 0
        L.lcd_inflated_free(h)
        return out.raw[:n]
    return run


def check_image(lcd, inflate_dev, data, block_payload, add_eof=1):
    """every check of one image -> the result dict of lcd.bgzf_deflate"""
    r = lcd.bgzf_deflate(data, block_payload, add_eof)
    bp = block_payload or 0xff00
    image, blocks = r["image"], r["blocks"]
    members = bo.bgzf_members(image)                                   # BSIZE chain, ISIZE, CRC-32 == zlib.crc32, exact end of every stream, <= 64 KB
    if add_eof:
        assert image.endswith(EOF_MEMBER) and members[-1]["isize"] == 0
        members = members[:-1]
    assert len(members) == len(blocks) == (len(data) + bp - 1) // bp
    for i, (m, (pl, bs, kind)) in enumerate(zip(members, blocks)):
        assert m["payload"] == data[i * bp:(i + 1) * bp] and pl == len(m["payload"]) and bs == m["bsize"] and kind in (0, 1, 2)
        assert m["bsize"] <= pl + 5 + 26
        assert (m["comp"][0] >> 1) & 3 == kind                         # BTYPE of the member's (single) deflate block
    assert inflate_dev(image) == data                                  # the project's own decoder, CRC check on
    return r


@pytest.mark.parametrize("name", ["text", "bam", "skew", "run", "one", "random", "far", "zeros_then_text"])
def test_every_payload_class_round_trips_at_every_block_size(lcd, inflate_dev, P, name):
    data = P[name]
    check_image(lcd, inflate_dev, data, 0)
    check_image(lcd, inflate_dev, data, 4000)
    check_image(lcd, inflate_dev, data[:5000], 17)                     # hundreds of tiny members
    check_image(lcd, inflate_dev, data[:300], 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_around_the_format_limits(lcd, inflate_dev, P, n):
    for name in ("text", "run", "random"):
        d = (P[name] * 2)[:n]
        for bp in (0, 4000):
            check_image(lcd, inflate_dev, d, bp)
    for bp in (1, 17):
        check_image(lcd, inflate_dev, (P["text"] * 2)[:min(n, 700)], bp)
    if n == 0:
        assert lcd.bgzf_deflate(b"", 0, 1)["image"] == EOF_MEMBER and lcd.bgzf_deflate(b"", 0, 0)["image"] == b""


def test_conditions_that_a_lazy_compressor_misses(lcd, inflate_dev, P):
    size = lambda r: sum(b[1] for b in r["blocks"])
    run = check_image(lcd, inflate_dev, P["run"], 0)
    print("run: member bytes", size(run), "of", len(P["run"]))
    assert size(run) < 0.02 * len(P["run"])                            # matches are used (codes alone: 12.5 %)
    text = check_image(lcd, inflate_dev, P["text"], 0)
    print("text: member bytes", size(text), "of", len(P["text"]))
    assert size(text) < 0.30 * len(P["text"])                          # matches are used (codes alone: 51 %)
    skew = check_image(lcd, inflate_dev, P["skew"], 0)
    print("skew: member bytes", size(skew), "of", len(P["skew"]), "kind", skew["blocks"][0][2])
    assert size(skew) < 0.90 * len(P["skew"]) and skew["blocks"][0][2] == 2   # dynamic codes (fixed codes: 99.5 %)
    rnd = check_image(lcd, inflate_dev, P["random"], 0)
    print("random: member bytes", size(rnd), "of", len(P["random"]), "kind", rnd["blocks"][0][2])
    assert rnd["blocks"][0][1] <= len(P["random"]) + 5 + 26 and rnd["blocks"][0][2] == 0   # stored fallback


def test_many_blocks_of_mixed_classes_in_one_launch(lcd, inflate_dev, P):
    rng = np.random.default_rng(11)
    data = b"".join(P[k][:int(rng.integers(1000, 20000))] for k in ("bam", "random", "run", "text", "skew", "one", "far", "zeros_then_text", "random", "bam", "run")) * 3
    r = check_image(lcd, inflate_dev, data, 1501)
    kinds = {b[2] for b in r["blocks"]}
    assert len(r["blocks"]) > 100 and {0, 2} <= kinds and r["kernel_ms"] > 0
    with pytest.raises(lcd.LcdError):
        lcd.bgzf_deflate(b"abc", 0xff01)
