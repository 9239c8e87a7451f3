"""Symmetric DUST inputs in which runs of N are DENSE, and what each of them is meant to reach (the census of tests/sdust_model.py).

The reference's automaton (src/sdust.c:129-163) resets l and t at an N but keeps the window and its counters, and computes the window start from l: the
first words behind an N see words from before it, and the perfect intervals found then carry coordinates that do not belong to the words they were found in --
their start can lie behind the current position and at or past the end of the sequence.  The device cuts the sequence into segments, one automaton per
segment, so everything here aims at the seams, at the order of the saves and at the end of the sequence.

CASES is a list of dicts(name, seq, T, W, reach, kind):
  seq    raw codes 0..4 (np.uint8) or letters (bytes)
  reach  {census key: minimum}: what sdust_full's census (max_back: sdust_segmented's) has to show for this case
  kind   None, or which failure of the ownership-by-start rule (sdust_model's rule="start", what the library did before) the case reproduces:
         "past_end"  an interval that starts at or past len, or is extended by one, is lost
         "order"     two intervals the reference keeps apart are joined, because the order of the starts is not the order of the saves
         "start"     an interval's start differs in the interior (the lead-in of 2W + 4 words does not make the lane's list P exact where N are dense)
         "cap"       one lane reports more intervals than its cap = seg + 8 slots hold: the library answered a valid sequence with error -24
tests/test_sdust_cases_oracle.py proves on the CPU that every case reaches what it names and that the suite as a whole reaches every key;
tests/test_gpu_sdust_seams.py runs the same cases through the kernel.  Everything is seeded, pure numpy, at most 3000 bases (1000 at W = 64)."""
import functools

import numpy as np

from sdust_model import seg_of

N = 4
PARAMS = ((5, 20), (10, 33), (20, 64), (1, 4))      # (5, 20) is the caller's only setting (lcd_first_round.cpp); the others get a reduced set


def periodic(unit, piece, n_run, length, phase=0):
    """a tandem repeat of `unit` cut into pieces of `piece` bases by `n_run` N (piece == 3: one triplet word per piece)"""
    u = np.asarray(unit, np.uint8)
    s = np.resize(u, length + phase)[phase:].copy()
    k = np.arange(length) % (piece + n_run)
    s[k >= piece] = N
    return s


def two_letter(seed, n, p_n):
    """iid bases over two letters, each position N with probability p_n"""
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, 2, n) * int(rng.integers(1, 4))).astype(np.uint8)
    s[rng.random(n) < p_n] = N
    return s


def seam(W, unit, off, gap=0, k_seam=1, tail=1):
    """a tandem repeat over [0, (k_seam + tail) seg) with an N at k_seam seg + off and, gap > 0, a second one `gap` bases behind it"""
    seg = seg_of(W)
    s = np.resize(np.asarray(unit, np.uint8), (k_seam + tail) * seg).copy()
    s[k_seam * seg + off] = N
    if gap:
        s[k_seam * seg + off + gap] = N
    return s


def dense_tail(seed, length, W, p_n=0.3):
    """random four-letter bases whose last 2W are two-letter with N at rate p_n (N-dense low complexity up to the end)"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, length).astype(np.uint8)
    s[length - 2 * W:] = two_letter(seed + 1000, 2 * W, p_n)
    return s


def letters(codes, style):
    """the codes as letters: style 0 'ACGTN', 1 'acgtn', 2 mixed case with N written as N, n, R, Y, - in turn (seq_nt4_table maps all of them to 4)"""
    c = np.asarray(codes, np.uint8)
    if style == 0:
        return np.frombuffer(b"ACGTN", np.uint8)[c].tobytes()
    if style == 1:
        return np.frombuffer(b"acgtn", np.uint8)[c].tobytes()
    out = np.where(np.arange(len(c)) % 3 == 0, np.frombuffer(b"acgtn", np.uint8)[c], np.frombuffer(b"ACGTN", np.uint8)[c])
    n_at = np.flatnonzero(c == N)
    out[n_at] = np.frombuffer(b"NnRY-", np.uint8)[np.arange(len(n_at)) % 5]
    return out.astype(np.uint8).tobytes()


UNITS = {1: [0], 2: [0, 1], 3: [0, 1, 2], 4: [3, 3, 0, 1], 5: [0, 0, 1, 2, 3], 6: [2, 0, 2, 1, 1, 3], 7: [0, 1, 2, 3, 3, 1, 0]}

# two-letter random sequences that the ownership-by-start rule gets wrong at (5, 20), found with the model: (seed, length, N rate, kind)
KINDS = ((7, 700, 0.4, "past_end"), (21, 2500, 0.25, "past_end"), (21, 700, 0.4, "order"), (9, 2500, 0.25, "order"), (9, 1500, 0.4, "start"),
         (39, 1500, 0.4, "start"), (31, 2500, 0.25, "start"))
# seeds of dense_tail per (T, W) whose census shows past_end > 0 at every one of the lengths used below (searched with the model)
TAIL_SEEDS = {(5, 20): (1, 2), (10, 33): (0,), (20, 64): (0,), (1, 4): (0,)}


def _case(name, seq, T, W, reach=None, kind=None):
    return dict(name=name, seq=seq, T=T, W=W, reach=dict(reach or {}), kind=kind)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for T, W in PARAMS:
        main, big, seg = (T, W) == (5, 20), W == 64, seg_of(W)
        tag = f"T{T}W{W}"
        # ---- periodic units with N between pieces
        pieces, runs = (3, 4, 5, 6, 9, 15, 21, 40), (1, 2, 5)
        n = 0
        for u in range(1, 8):
            for piece in pieces:
                for run in runs:
                    n += 1
                    if not main and n % (56 if big else 8) != 1:        # reduced set: every 8th (56th at W = 64) combination
                        continue
                    length = 520 if big else 900
                    reach = {"displaced": 1} if piece <= 6 and W > 4 else {}
                    out.append(_case(f"{tag}:periodic:u{u}p{piece}n{run}", periodic(UNITS[u], piece, run, length, phase=n % u), T, W, reach,
                                     "cap" if n == 1 and W > 4 else None))
        # one word per piece, ten N between: the W + 4 words of a lane's lead-in are 13 bases apart
        if W > 4:
            out.append(_case(f"{tag}:periodic:far", periodic(UNITS[5], 3, 10, 1000 if big else 1200), T, W, {"max_back": 2 * seg + 1}))
        # ---- two-letter random
        for p_n in (0.02, 0.10, 0.25, 0.40) if not big else (0.10, 0.40):
            for seed, length in (((0, 300), (1, 700), (2, 1300), (3, 2500)) if main else ((0, 300), (1, 700)) if big else ((0, 300), (1, 700), (2, 1300))):
                reach = {"displaced": 1} if p_n >= 0.25 and W > 4 else {}
                out.append(_case(f"{tag}:random:n{int(p_n * 100)}s{seed}l{length}", two_letter(seed, length, p_n), T, W, reach))
        if main:
            for seed, length, p_n, kind in KINDS:
                reach = {"past_end": 1} if kind == "past_end" else {"order_inversions": 1} if kind == "order" else {"displaced": 1}
                out.append(_case(f"{tag}:random:{kind}:n{int(p_n * 100)}s{seed}l{length}", two_letter(seed, length, p_n), T, W, reach, kind))
        # ---- N at the seams: one N, and a pair 3 - 30 bases apart, at every offset (every 6th at W = 33, every 64th at W = 64) in [seg - W - 4, seg + W + 4];
        # the 7-base unit: a lane inside a repeat of a shorter unit keeps three to five times as many perfect intervals and is that much slower (the
        # periodic and the spill cases have the short units)
        unit = UNITS[1] if W == 4 else UNITS[7]
        for off in range(-W - 4, W + 5, 1 if main or W == 4 else 64 if big else 6):
            gap = 3 + (off + W + 4) % 28
            out.append(_case(f"{tag}:seam:one:{off:+d}", seam(W, unit, off), T, W, {"seam_crossers": 1} if W > 4 and abs(off) > 2 else {}))
            out.append(_case(f"{tag}:seam:pair:{off:+d}g{gap}", seam(W, unit, off, gap), T, W))
        # ---- sequence ends: len = seg k - 1 .. seg k + 2, the last 2W bases N-dense; then a trailing N, and 1 - 2 bases behind an N (no word forms)
        for seed in TAIL_SEEDS[(T, W)]:
            for k in (1, 3) if not big else (2,):
                for d in (-1, 0, 1, 2):
                    s = dense_tail(seed, seg * k + d, W)
                    name = f"{tag}:end:s{seed}k{k}{d:+d}"
                    out.append(_case(name, s, T, W, {"past_end": 1} if W > 4 else {}))
                    if main or d == 0:
                        out.append(_case(name + ":N", np.concatenate([s[:-1], [N]]).astype(np.uint8), T, W))
                        out.append(_case(name + ":N1", np.concatenate([s[:-2], [N, 1]]).astype(np.uint8), T, W))
                        out.append(_case(name + ":N2", np.concatenate([s[:-3], [N, 1, 1]]).astype(np.uint8), T, W))
        # ---- long lists P: tandem repeats and homopolymers of 600+ bases with and without N (the first 32 entries of a lane's list are in LDS, the rest in HBM)
        if (T, W) in ((5, 20), (10, 33)):
            for u in (1, 2, 3, 5) if main else (2,):
                s = np.resize(np.asarray(UNITS[u], np.uint8), 640 + u).copy()
                out.append(_case(f"{tag}:spill:u{u}", s, T, W, {"max_pn": 33}))
                s = s.copy(); s[[200, 201, 330, 517]] = N
                out.append(_case(f"{tag}:spill:u{u}:N", s, T, W, {"max_pn": 33}))
            s = np.zeros(700, np.uint8); s[[250, 251, 400, 580]] = N           # a homopolymer cut by N: the longest list the model sees at this (T, W)
            out.append(_case(f"{tag}:spill:peak", s, T, W, {"max_pn": 33}))
    # ---- letters: every 9th case of (5, 20) and the KINDS as 'ACGTN', 'acgtn' and mixed case with R, Y, - for N
    for i, c in enumerate([c for c in out if c["T"] == 5 and (c["kind"] or hash_of(c["name"]) % 9 == 0)]):
        out.append(_case(c["name"] + f":letters{i % 3}", letters(c["seq"], i % 3), c["T"], c["W"], c["reach"], c["kind"]))
    names = [c["name"] for c in out]
    assert len(names) == len(set(names))
    assert all(len(c["seq"]) <= (1000 if c["W"] == 64 else 3000) for c in out)
    return out


def hash_of(name):
    """a hash that does not change between runs (str hashes are salted)"""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def full_runs():
    """{case name: (sdust_full's intervals, its census)}: the sequential model over every case, computed once for all the tests of a session"""
    import sdust_model as M
    out = {}
    for c in cases():
        cen = {}
        out[c["name"]] = (M.sdust_full(c["seq"], c["T"], c["W"], cen), cen)
    return out


def by_params():
    """{(T, W): [case]} in CASES order"""
    out = {}
    for c in cases():
        out.setdefault((c["T"], c["W"]), []).append(c)
    return out


def pack_order(cs, past_end_names):
    """the order of one launch: a case whose census shows past_end directly in front of every other case where possible (an interval past one
    sequence's end must not be taken for the next sequence's), the rest in CASES order"""
    pe = [c for c in cs if c["name"] in past_end_names]
    rest = [c for c in cs if c["name"] not in past_end_names]
    out = []
    while pe or rest:
        if pe:
            out.append(pe.pop(0))
        if rest:
            out.append(rest.pop(0))
    return out


def first_round_chunk():
    """a chunk whose reference has an N-dense two-letter stretch straddling reg_end: the region's sequence (what lcd_first_round.cpp hands to lcd_sdust_batch)
    ends inside the stretch -> dict(ref, ref_beg, reg_beg, reg_end) for call_chunks_common.low_comp_of"""
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 4, 3000).astype(np.uint8)
    for p in (300, 1100, 1900):
        ref[p:p + 90] = np.resize(np.asarray(UNITS[2], np.uint8), 90)
    ref[2400:2600] = two_letter(7, 200, 0.4)
    return dict(ref=ref, ref_beg=5001, reg_beg=5201, reg_end=5001 + 2500)
