"""lcd_sort_chunk_reads (host code, no device): sort_chunk_reads' order (src/bam_utils.c:1616-1656) -- position, end DESCENDING, the NM tag, strcmp of the read
names, and file order where all four are equal -- against the comparator restated in Python (tests/call_chunks_common.py) on hand-made keys with every tie level."""
import numpy as np
import pytest

import call_chunks_common as kc


def hand_keys():
    """(pos, end, nm, name) in file order = by position only, as a coordinate-sorted BAM gives them"""
    k = []
    k += [(100, 900, 3, "a"), (100, 1500, 9, "b"), (100, 1200, 0, "c")]                       # same pos, different end: the longer read first, whatever its NM
    k += [(200, 800, 7, "a"), (200, 800, 2, "b"), (200, 800, 5, "c"), (200, 800, -1, "d")]     # same pos and end: NM ascending (a negative one first)
    k += [(300, 700, 4, "r10"), (300, 700, 4, "r9"), (300, 700, 4, "r1"), (300, 700, 4, "r100")]   # same three: byte order of the names, not numeric
    k += [(400, 600, 1, "twin"), (400, 600, 1, "twin"), (400, 600, 1, "twin")]                 # fully equal: file order
    k += [(500, 900, 0, "Z"), (500, 900, 0, "a"), (500, 900, 0, "B"), (500, 900, 0, "_")]      # upper case before '_' before lower case
    k += [(600, 650, 2, "p"), (600, 651, 2, "p"), (600, 650, 1, "q"), (600, 651, 3, "o")]      # the keys in their order of precedence
    k += [(700, 710, 0, "x"), (700, 710, 0, "x/1"), (700, 710, 0, "x/"), (700, 710, 0, "")]    # a prefix sorts first, the empty name before all
    k += [(800, 1 << 40, 5, "big"), (800, (1 << 40) + 1, 5, "big"), (800, 1 << 33, 5, "big")]  # 64-bit ends
    k += [(900, 950, 2147483647, "m"), (900, 950, -2147483648, "m"), (900, 950, 0, "m")]       # the int range of NM
    k += [(1000, 2000, 0, "\xc3\xa9"), (1000, 2000, 0, "z"), (1000, 2000, 0, "\x7f")]          # bytes above 127 compare as unsigned chars
    k += [(1100 + i, 1200, 0, "s") for i in range(4)]                                         # nothing to reorder
    return k


def run(lcd, keys):
    pos, end, nm, names = ([x[i] for x in keys] for i in range(4))
    names = [s.encode("latin-1") for s in names]
    return lcd.sort_chunk_reads(pos, end, nm, names), kc.python_order(pos, end, nm, names)


def test_hand_made_keys_with_every_tie_level(lcd):
    keys = hand_keys()
    assert 36 <= len(keys) <= 44
    got, want = run(lcd, keys)
    assert got.tolist() == want.tolist()
    assert got.tolist() != list(range(len(keys)))
    o = got.tolist()
    assert o[:3] == [1, 2, 0]                       # the longer read first
    assert o[3:7] == [6, 4, 5, 3]                   # NM ascending
    assert o[7:11] == [9, 7, 10, 8]                 # r1 < r10 < r100 < r9
    assert o[11:14] == [11, 12, 13]                 # equal entries keep file order


def test_permuted_input_sorts_to_the_same_keys(lcd):
    keys = hand_keys()
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(keys))
    shuffled = [keys[i] for i in perm]
    got, want = run(lcd, shuffled)
    assert got.tolist() == want.tolist()
    distinct = lambda o, ks: [ks[i] for i in o]
    assert distinct(got, shuffled) == distinct(run(lcd, keys)[0], keys)     # the same sequence of keys (equal entries are interchangeable)


def test_sorted_input_and_tiny_inputs(lcd):
    keys = hand_keys()
    got, _ = run(lcd, keys)
    srt = [keys[i] for i in got]
    again, want = run(lcd, srt)
    assert again.tolist() == want.tolist() == list(range(len(srt)))
    assert lcd.sort_chunk_reads([], [], [], []).tolist() == []
    assert lcd.sort_chunk_reads([7], [9], [1], ["only"]).tolist() == [0]


def test_comparator_restated_in_python_on_hand_cases():
    key = kc.read_sort_key
    assert key(5, 10, 0, "a") < key(6, 1, 0, "a")           # position first
    assert key(5, 20, 9, "z") < key(5, 10, 0, "a")          # then the later end
    assert key(5, 10, -2, "z") < key(5, 10, 0, "a")         # then NM
    assert key(5, 10, 0, "r10") < key(5, 10, 0, "r9")       # then the bytes of the name
    assert key(5, 10, 0, "r") < key(5, 10, 0, "r0")
    assert kc.python_order([1, 1], [2, 2], [0, 0], ["s", "s"]).tolist() == [0, 1]


def test_nm_records_of_the_device_test_cover_every_alignment():
    """the BAM the GPU test reads: its auxiliary fields start at every byte offset modulo 4, records at odd offsets included"""
    import os
    import tempfile
    recs = kc.nm_records()
    with tempfile.TemporaryDirectory() as d:
        kc.write_aux_bam(os.path.join(d, "n.bam"), recs)
    assert len(recs) == 16
    assert {r["aux0"] % 4 for r in recs} == {0, 1, 2, 3} and any(r["u0"] % 2 for r in recs)
    pos, end = [r["pos0"] for r in recs], [r["pos0"] + r["qlen"] for r in recs]
    order = kc.python_order(pos, end, [r["nm"] for r in recs], [r["name"] for r in recs])
    assert order.tolist() != list(range(16))
    assert order.tolist() != kc.python_order(pos, end, [0] * 16, [r["name"] for r in recs]).tolist()      # NM matters
    assert order.tolist() != kc.python_order(pos, end, [r["nm"] for r in recs], ["x"] * 16).tolist()      # the names matter
