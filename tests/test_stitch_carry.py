"""lcd_stitch_chunks_carry: a chain of chunks stitched window by window, with the last chunk of a window remembered in an lcd_stitch_carry_t, leaves every array
and every flip field as lcd_stitch_chunks over each contig's chunks leaves them.  Seeded synthetic phase views, built as tests/test_emit.py builds those of its
flip test.  Host code: no device is needed."""
import copy
import ctypes as C

import numpy as np
import pytest

i32p, i64p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
KEYS = ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle")
N_OV = 12


def make_chain(seed=11):
    """six chunks, three on contig 0 and three on contig 1.  Overlap reads of neighbours (N_OV each): chunk 1 disagrees with chunk 0 on every shared read (swap);
    chunk 2 agrees with chunk 1's ORIGINAL haplotypes, i.e. disagrees with its final ones (a swap after a swapped chunk); chunk 4 agrees with chunk 3 (joined as it
    is); chunk 5 agrees on half and disagrees on half (score 0: left alone).  Chunks 2 and 3 hold lists of equal length that disagree everywhere: a stitch that
    joined across the contig change would swap chunk 3."""
    rng = np.random.default_rng(seed)
    chs = []
    for c in range(6):
        nr, nv = int(rng.integers(60, 90)), int(rng.integers(20, 40))
        main, other = 1000 * (c + 1), 1000 * (c + 1) + 500
        haps = rng.integers(1, 3, nr).astype(np.int32)
        ps = np.full(nr, main, np.int64)
        far = rng.choice(nr, nr // 5, replace=False)                  # reads of another phase set, and unphased ones
        ps[far[: len(far) // 2]] = other
        haps[far[len(far) // 2:]] = 0; ps[far[len(far) // 2:]] = -1
        free = np.setdiff1d(np.arange(nr), far)
        pick = rng.choice(free, 2 * N_OV, replace=False).astype(np.int32)
        chs.append(dict(tid=c // 3, ordered_read_ids=rng.permutation(nr).astype(np.int32), is_skipped=np.zeros(nr, np.uint8), haps=haps, phase_sets=ps,
                        var_phase_set=rng.choice([-1, main, other], nv).astype(np.int64), hap_to_cons_alle=rng.integers(-1, 2, nv * 3).astype(np.int32),
                        up_ovlp=pick[:N_OV].copy(), down_ovlp=pick[N_OV:].copy()))
    chs[0]["up_ovlp"] = np.zeros(0, np.int32); chs[5]["down_ovlp"] = np.zeros(0, np.int32)
    skip = int(chs[0]["down_ovlp"][0]); chs[0]["is_skipped"][skip] = 1                     # a skipped read does not vote
    chs[1]["haps"][chs[1]["up_ovlp"]] = 3 - chs[0]["haps"][chs[0]["down_ovlp"]]
    chs[2]["haps"][chs[2]["up_ovlp"]] = chs[1]["haps"][chs[1]["down_ovlp"]]
    chs[3]["haps"][chs[3]["up_ovlp"]] = 3 - chs[2]["haps"][chs[2]["down_ovlp"]]
    chs[4]["haps"][chs[4]["up_ovlp"]] = chs[3]["haps"][chs[3]["down_ovlp"]]
    chs[5]["haps"][chs[5]["up_ovlp"]] = chs[4]["haps"][chs[4]["down_ovlp"]]
    chs[5]["haps"][chs[5]["up_ovlp"][: N_OV // 2]] = 3 - chs[5]["haps"][chs[5]["up_ovlp"][: N_OV // 2]]
    return chs


def phase_array(chs):
    from longcalld_amd._lib import LcdChunkPhase
    arr = (LcdChunkPhase * max(1, len(chs)))()
    for s, d in zip(arr, chs):
        s.tid, s.n_reads, s.n_vars = d["tid"], len(d["haps"]), len(d["var_phase_set"])
        s.ordered_read_ids = d["ordered_read_ids"].ctypes.data_as(i32p); s.is_skipped = d["is_skipped"].ctypes.data_as(u8p)
        s.haps = d["haps"].ctypes.data_as(i32p); s.phase_sets = d["phase_sets"].ctypes.data_as(i64p)
        s.var_phase_set = d["var_phase_set"].ctypes.data_as(i64p); s.hap_to_cons_alle = d["hap_to_cons_alle"].ctypes.data_as(i32p)
        s.n_up_ovlp, s.n_down_ovlp = len(d["up_ovlp"]), len(d["down_ovlp"])
        s.up_ovlp_read_i = d["up_ovlp"].ctypes.data_as(i32p); s.down_ovlp_read_i = d["down_ovlp"].ctypes.data_as(i32p)
        s.flip_hap, s.flip_pre_PS, s.flip_cur_PS = 0, -1, -1
    return arr


def flips_of(arr, n):
    return [(arr[i].flip_hap, arr[i].flip_pre_PS, arr[i].flip_cur_PS) for i in range(n)]


def yardstick(lcd, chs, update_reads):
    """lcd_stitch_chunks over each contig's chunks"""
    lib = lcd.load_library()
    lib.lcd_stitch_chunks.argtypes = [C.c_void_p, C.c_int, C.c_int]
    chs = copy.deepcopy(chs)
    flips = []
    for lo in (0, 3):
        arr = phase_array(chs[lo:lo + 3])
        assert lib.lcd_stitch_chunks(arr, 3, update_reads) == 0
        flips += flips_of(arr, 3)
    return chs, flips


def carried(lcd, chs, window, update_reads, same_object=True):
    from longcalld_amd._lib import LcdStitchCarry
    lib = lcd.load_library()
    chs = copy.deepcopy(chs)
    carry, nxt = LcdStitchCarry(), LcdStitchCarry()
    flips, rcs = [], []
    for lo in range(0, len(chs), window):
        part = chs[lo:lo + window]
        arr = phase_array(part)
        out = carry if same_object else nxt
        rc = lcd.stitch_chunks_carry(arr, update_reads, carry if lo else None, out)
        rcs.append(rc)
        if rc:
            break
        if not same_object:
            lib.lcd_stitch_carry_free(C.byref(carry))
            carry, nxt = nxt, LcdStitchCarry()
        assert carry.valid == 1 and carry.tid == part[-1]["tid"] and carry.n_reads == len(part[-1]["haps"]) and carry.n_down_ovlp == len(part[-1]["down_ovlp"])
        assert [carry.haps[i] for i in range(carry.n_reads)] == part[-1]["haps"].tolist()                  # the FINAL state of the window's last chunk
        flips += flips_of(arr, len(part))
    lib.lcd_stitch_carry_free(C.byref(carry)); lib.lcd_stitch_carry_free(C.byref(nxt))
    assert carry.valid == 0 and not carry.haps
    return chs, flips, rcs


def test_the_yardstick_takes_every_branch(lcd):
    chs = make_chain()
    got, flips = yardstick(lcd, chs, 1)
    assert flips[0] == (0, -1, -1) and flips[3] == (0, -1, -1)                       # the first chunk of a contig is never joined
    assert flips[1][0] == 1 and flips[1][1:] == (1000, 2000)                          # swapped
    assert flips[2][0] == 1 and flips[2][1:] == (1000, 3000)                          # swapped against a chunk that was itself swapped: its final state is read
    assert flips[4][0] == 0 and flips[4][1:] == (4000, 5000)                          # joined as it is
    assert flips[5] == (0, -1, -1)                                                    # a tied vote (flip_hap_score == 0): left alone
    assert (got[1]["haps"] != chs[1]["haps"]).any() and (got[5]["haps"] == chs[5]["haps"]).all()
    # against chunk 1's ORIGINAL state chunk 2 would not have been swapped
    alone = copy.deepcopy(chs[1:3])
    lib = lcd.load_library()
    lib.lcd_stitch_chunks.argtypes = [C.c_void_p, C.c_int, C.c_int]
    arr = phase_array(alone)
    assert lib.lcd_stitch_chunks(arr, 2, 1) == 0 and arr[1].flip_hap == 0 and arr[1].flip_pre_PS == 2000


@pytest.mark.parametrize("update_reads", [1, 0])
@pytest.mark.parametrize("same_object", [True, False])
@pytest.mark.parametrize("window", [1, 2, 4, 6])
def test_windows_leave_what_the_whole_chain_leaves(lcd, window, same_object, update_reads):
    chs = make_chain()
    want, want_flips = yardstick(lcd, chs, update_reads)
    got, flips, rcs = carried(lcd, chs, window, update_reads, same_object)
    assert rcs == [0] * len(rcs) and flips == want_flips
    for g, w in zip(got, want):
        for k in KEYS + ("is_skipped", "ordered_read_ids", "up_ovlp", "down_ovlp"):
            assert (g[k] == w[k]).all(), k
    assert flips[3] == (0, -1, -1)                                                    # never joined across the contig change, whatever the lists hold


def test_without_a_carry_it_is_lcd_stitch_chunks(lcd):
    chs = make_chain()
    want, want_flips = yardstick(lcd, chs, 1)
    a = copy.deepcopy(chs)
    arr = phase_array(a)
    assert lcd.stitch_chunks_carry(arr, 1, None, None) == 0 and flips_of(arr, 6) == want_flips
    for g, w in zip(a, want):
        assert all((g[k] == w[k]).all() for k in KEYS)


def test_an_empty_window_keeps_the_carry(lcd):
    from longcalld_amd._lib import LcdStitchCarry
    lib = lcd.load_library()
    chs = copy.deepcopy(make_chain()[:1])
    c1, c2 = LcdStitchCarry(), LcdStitchCarry()
    assert lcd.stitch_chunks_carry(phase_array(chs), 1, None, c1) == 0 and c1.valid == 1
    c1.reg_beg, c1.reg_end = 7, 9
    assert lcd.stitch_chunks_carry(phase_array([]), 1, c1, c2, n=0) == 0
    assert (c2.valid, c2.tid, c2.reg_beg, c2.reg_end, c2.n_reads, c2.n_down_ovlp) == (1, 0, 7, 9, c1.n_reads, c1.n_down_ovlp)
    assert [c2.down_ovlp_read_i[i] for i in range(c2.n_down_ovlp)] == chs[0]["down_ovlp"].tolist()
    assert lcd.stitch_chunks_carry(phase_array([]), 1, c1, c1, n=0) == 0 and c1.valid == 1
    lib.lcd_stitch_carry_free(C.byref(c1)); lib.lcd_stitch_carry_free(C.byref(c2))


def test_differing_overlap_counts_are_the_same_error_across_a_border(lcd):
    chs = make_chain()
    chs[1]["up_ovlp"] = chs[1]["up_ovlp"][:-1].copy()
    arr = phase_array(copy.deepcopy(chs))
    assert lcd.stitch_chunks_carry(arr, 1, None, None) == -6                         # inside a window
    for window in (1, 2, 4):
        _, _, rcs = carried(lcd, chs, window, 1)
        assert rcs[-1] == -6 and all(r == 0 for r in rcs[:-1]) and len(rcs) == (2 if window == 1 else 1)
