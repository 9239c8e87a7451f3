"""lcd_bai_build on the device (bai_kernel.hip behind the inflate, the record walk and the CIGAR statistics) against the pure-Python oracle of tests/bai_common.py:
every named case byte for byte, the independence of the index from the slab size, slabs smaller than a record and a record larger than a slab, record counts at
the compaction's wavefront and workgroup borders, a 1 Mb read's linear windows, and the refusals."""
import os
import struct

import numpy as np
import pytest

import bai_common as bc

pytestmark = pytest.mark.gpu


def build(lcd, tmp_path, bam, tag, slab_members=0, verify_crc=0):
    path = str(tmp_path / f"{tag}.bam")
    if not os.path.exists(path):
        open(path, "wb").write(bam)
    out = str(tmp_path / f"{tag}.{slab_members}.bai")
    st = lcd.bai_build(path, out, slab_members=slab_members, verify_crc=verify_crc)
    return open(out, "rb").read(), st


def ledger(lcd):
    return lcd.load_library().lcd_device_bytes(0)


@pytest.mark.parametrize("name", [n for n in bc.CASES if not n.startswith("refused_")])
def test_named_cases_equal_the_oracle(lcd, tmp_path, name):
    bam, pred, _ = bc.CASES[name]()
    s = bc.scan_bam(bam)
    want = bc.oracle_bai(len(s["refs"]), s["recs"])
    assert pred(s, bc.parse_bai(want))
    before = ledger(lcd)
    for sm in (0, 1):
        got, st = build(lcd, tmp_path, bam, name, sm, verify_crc=1)
        assert got == want, (name, sm)
        assert st["n_records"] == len(s["recs"]) and st["n_no_coor"] == sum(1 for x in s["recs"] if x["tid"] < 0 or x["pos"] < 0) and st["bytes_index"] == len(want)
    assert ledger(lcd) == before


@pytest.mark.parametrize("name", [n for n in bc.CASES if n.startswith("refused_")])
def test_refusals_leave_nothing_behind(lcd, tmp_path, name):
    bam, _, (code, recno) = bc.CASES[name]()
    path, out = str(tmp_path / "r.bam"), str(tmp_path / "r.bai")
    open(path, "wb").write(bam)
    before = ledger(lcd)
    for sm in (0, 1):
        with pytest.raises(lcd.LcdError) as e:
            lcd.bai_build(path, out, slab_members=sm)
        assert f"error {code}:" in str(e.value) and f"record {recno} " in str(e.value), str(e.value)
        if code == bc.ERR_CSI:
            assert "only BAI is supported, not CSI" in str(e.value)
        assert not os.path.exists(out) and ledger(lcd) == before


@pytest.mark.parametrize("seed", bc.SEEDS)
def test_the_index_does_not_depend_on_the_slabs(lcd, tmp_path, seed):
    bam = bc.seeded_bam(seed)
    s = bc.scan_bam(bam)
    assert {n for _c, _u, n in s["tab"]} & {1, 700, 4000}                                # members smaller than a record: records straddle members
    want = bc.oracle_bai(len(s["refs"]), s["recs"])
    slabs = {}
    for sm in (1, 2, 3, 7, 0):
        got, st = build(lcd, tmp_path, bam, f"s{seed}", sm)
        assert got == want, (seed, sm)
        slabs[sm] = st["n_slabs"]
        assert (st["n_records"], st["n_no_coor"], st["n_indexed"]) == (305, 5, 300)
    assert slabs[0] == 1 and slabs[1] >= slabs[2] >= slabs[7] >= 1 and slabs[1] > 3 and slabs[1] > slabs[7]


def test_slabs_that_hold_less_than_one_record(lcd, tmp_path):
    """every member of the record part is smaller than the smallest record: with slab_members = 1 no slab holds a whole record and every step has to grow"""
    recs = [bc.record(1, 100 + 10 * i, [(7, 800)], name=f"small{i}", aux=b"csZ" + b":9" * (300 + 7 * i) + b"\0") for i in range(20)]
    bam = bc.build_bam([("c0", 1000), ("c1", 300000)], recs, payloads=[700])
    s = bc.scan_bam(bam)
    first_rec = s["recs"][0]["u0"]
    assert max(n for _c, u, n in s["tab"] if u >= first_rec) == 700 < min(x["u1"] - x["u0"] for x in s["recs"])
    want = bc.oracle_bai(2, s["recs"])
    for sm in (1, 2, 3, 0):
        got, st = build(lcd, tmp_path, bam, "lessthanone", sm)
        assert got == want, sm
        assert st["n_records"] == 20
    _, st1 = build(lcd, tmp_path, bam, "lessthanone", 1)
    assert st1["n_slabs"] >= 2 * 20 and st1["bytes_inflated"] > len(s["stream"])               # every record needed at least one grown slab


def test_a_record_larger_than_the_default_slab(lcd, tmp_path):
    """a 200 kb read with a long cs-like Z tag, cut into members of 100 bytes: it spans more members than the default slab's 4096, so the default has to grow too"""
    cs = b"csZ" + b":25*ct" * 60000 + b"\0"                                             # 360 kb
    recs = [bc.record(1, 100 + 10 * i, [(7, 800)], name=f"small{i}") for i in range(3)]
    recs.append(bc.record(1, 400, [(7, 200000)], name="giant", aux=cs))                   # 300 kb of bases and qualities + the tag
    recs += [bc.record(1, 500 + i, [(7, 30)], name=f"tail{i}") for i in range(3)]
    bam = bc.build_bam([("c0", 1000), ("c1", 300000)], recs, payloads=[100])
    s = bc.scan_bam(bam)
    giant = s["recs"][3]
    assert sum(1 for _c, u, n in s["tab"] if n and u < giant["u1"] and u + n > giant["u0"]) > 4096 + 100
    want = bc.oracle_bai(2, s["recs"])
    for sm in (0, 5):
        got, st = build(lcd, tmp_path, bam, "giant", sm)
        assert got == want, sm
        assert st["n_records"] == 7
        assert st["n_slabs"] >= 2 and st["bytes_inflated"] > len(s["stream"]), (sm, st)   # the slab that ended inside the giant record was read again, larger


def test_a_block_size_no_record_can_have_and_a_record_outside_its_contig(lcd, tmp_path):
    import struct
    good = [bc.record(1, 100 + 10 * i, [(7, 50)], name=f"g{i}") for i in range(3)]
    bad = bc.build_bam([("c0", 1000), ("c1", 300000)], good + [struct.pack("<i", 5) + bytes(200)])
    path, out = str(tmp_path / "bs.bam"), str(tmp_path / "bs.bai")
    open(path, "wb").write(bad)
    before = ledger(lcd)
    for sm in (0, 1):
        with pytest.raises(lcd.LcdError, match="error -33:.*record 3 .*block_size 5"):     # at once: no slab is grown to the end of the file first
            lcd.bai_build(path, out, slab_members=sm)
        assert not os.path.exists(out) and ledger(lcd) == before
    far = bc.build_bam([("c0", 1000), ("c1", 20000)], good + [bc.record(1, 40000, [(7, 50)], name="outside")])
    open(path, "wb").write(far)
    with pytest.raises(lcd.LcdError, match="error -53:.*record 3 "):
        lcd.bai_build(path, out)
    assert not os.path.exists(out) and ledger(lcd) == before


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_runs_across_wavefront_and_workgroup_borders(lcd, tmp_path, n):
    recs, k, leaf = [], 0, True
    while len(recs) < n:                                                                 # runs of 1, 2, 3, 4, 5, 1, ... records, alternating between a leaf bin and bin 585
        for _ in range(k % 5 + 1):
            if len(recs) < n:
                recs.append(bc.record(0, 10 * len(recs), [(7, 5)] if leaf else [(7, 5), (3, 20000), (7, 5)], name=f"w{len(recs)}"))
        k += 1; leaf = not leaf
    bam = bc.build_bam([("c0", 200000)], recs, payloads=[4000, 700, 65280])
    s = bc.scan_bam(bam)
    want = bc.oracle_bai(1, s["recs"])
    runs = 1 + sum(1 for a, b in zip(s["recs"], s["recs"][1:]) if bc.reg2bin(a["pos"], a["end"]) != bc.reg2bin(b["pos"], b["end"]))
    got, st = build(lcd, tmp_path, bam, f"w{n}")
    assert got == want and st["n_chunks"] == runs and (n < 65 or runs > n // 4)           # n_chunks: the runs the compaction found, before the finisher merges them


def test_a_1_mb_read_sets_its_windows(lcd, tmp_path):
    recs = [bc.record(0, 3 << 14, [(7, 10), (3, 1000000), (7, 10)], name="mb"), bc.record(0, (3 << 14) + 5, [(7, 10)], name="next"), bc.record(0, 80 << 14, [(7, 10)], name="far")]
    bam = bc.build_bam([("c0", 5000000)], recs)
    s = bc.scan_bam(bam)
    got, _ = build(lcd, tmp_path, bam, "mb")
    assert got == bc.oracle_bai(1, s["recs"])
    lin = bc.parse_bai(got)["refs"][0]["lin"]
    assert sum(1 for v in lin[3:] if v == s["recs"][0]["vbeg"]) >= 62 and lin[:3] == [0, 0, 0] and lin[80] == s["recs"][2]["vbeg"]


def test_a_file_that_does_not_exist_and_an_unwritable_output(lcd, tmp_path):
    with pytest.raises(lcd.LcdError, match="error -30:"):
        lcd.bai_build(str(tmp_path / "absent.bam"), str(tmp_path / "x.bai"))
    bam = bc.seeded_bam(bc.SEEDS[0])
    path = str(tmp_path / "ok.bam")
    open(path, "wb").write(bam)
    before = ledger(lcd)
    with pytest.raises(lcd.LcdError, match="error -30:.*no_such_dir"):
        lcd.bai_build(path, str(tmp_path / "no_such_dir" / "x.bai"))
    assert ledger(lcd) == before
