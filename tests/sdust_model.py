"""Symmetric DUST (src/sdust.c:65-163) in plain Python, twice: the sequential automaton, and the decomposition into segments that lcd_sdust_batch
(lcd_calls.cpp) and lcd_sdust_kernel (sdust_kernel.hip) run on the device.  No GPU and no oracle/_ref needed; tests/test_sdust_cases_oracle.py proves the
first equal to the reference's own sdust() where that is built, and the second equal to the first on every case of tests/sdust_cases.py.

  sdust_full(seq, T, W, census=None)                    one automaton over the whole sequence -> [(start, finish)]
  sdust_segmented(seq, T, W, census=None, rule="step")  one automaton per segment, the host's chain of their reports -> [(start, finish)]

The two rules of sdust_segmented:

  "step"   what the library does.  Lane k owns the STEPS i in [a, b) = [k seg, min(len, a + seg)); the last lane owns the end-of-sequence flush i == len as well.
           It reports, folded with save_masked_regions' own merge, every interval that the automaton saves at one of its steps, whatever the interval's
           coordinates, and the host folds the lanes' lists in lane order: that is the order in which the sequential automaton saves them.  For that the lane's
           state has to be exact from step a on.  An interval in the list P at step i was inserted at i - 2W + 5 or later (an entry's start is at most W - 5
           past the step it was inserted at, and it leaves P once the window start, at least i + 1 - W in a piece free of N, has passed it; an N empties P), and
           so was every entry its insertion looked at (those start at or behind it, so they are still in P).  So window, counters, L and l have to be exact at
           a - 2W: the lane starts W + 4 triplet words before that position (W - 2 fill the window; l is exact after the first N and, past W, cancels from the
           window start).  What it inserts before its state is exact is gone from P before step a for the same reason.
  "start"  what the library did before: lane k starts 2W + 4 words before a - W, runs 2W + 8 bases past b and owns the intervals whose START lies in [a, b);
           the host chains the reports in (lane, order within the lane) order.  Wrong where an N displaces coordinates (the words in the window stay across an
           N, the window start is computed from l): an interval whose start is at or past len belongs to no lane, and the order of the starts is not the
           order of the saves, so the host's chain joins intervals the reference keeps apart.  Kept as the record of that design: the cases named in
           sdust_cases.KINDS tell the two rules apart, which the oracle test asserts.

census (a dict, updated in place; counters add up over calls, maxima are kept):
  max_pn            the longest list P
  displaced         intervals inserted into P with start > i
  past_end          saved (segmented: reported) intervals with start >= len
  max_back          the largest a - from over the segments (segmented only)
  max_lane          the longest folded list of one lane (segmented, rule "step"): the device holds cap = seg + 8 per lane
  order_inversions  pairs of consecutive saves, in the order in which the result is chained, whose owning segments by start (start // seg) decrease
  seam_crossers     result intervals that hold bases of two segments"""
import numpy as np

_CODE = np.full(256, 4, np.uint8)
_CODE[:4] = np.arange(4)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k


def codes_of(seq):
    """seq_nt4_table (src/sdust.c:22-39) over raw codes, a letter array, bytes or a str -> list of 0..4"""
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(bytes(seq), np.uint8)
    return _CODE[np.asarray(seq, np.uint8)].tolist()


def seg_of(W):
    return 128 if W <= 32 else 256


def _bump(census, key, v=1):
    if census is not None:
        census[key] = census.get(key, 0) + v


def _peak(census, key, v):
    if census is not None:
        census[key] = max(census.get(key, 0), v)


def _automaton(code, n, T, W, steps, save, census=None, count_from=0):
    """sdust_core over the steps `steps` (a range; step n is the end-of-sequence flush) from an empty state; save(i, start, finish) for every interval
    save_masked_regions would write, in its order.  Insertions at steps >= count_from go into census['displaced']."""
    w = []                       # the window's words, oldest first (at most W - 2)
    cv, cw = [0] * 64, [0] * 64
    P = []                       # [start, finish, r, l], descending start
    rv = rw = L = l = t = 0
    max_pn = 0
    T2 = T << 1

    def flush(i, start):
        if not P or P[-1][0] >= start:
            return
        save(i, P[-1][0], P[-1][1])
        while P and P[-1][0] < start:
            P.pop()

    for i in steps:
        b = code[i] if i < n else 4
        if b < 4:
            l += 1
            t = (t << 2 | b) & 63
            if l < 3:
                continue
            start = (l - W if l > W else 0) + (i + 1 - l)
            flush(i, start)
            if len(w) >= W - 2:                                   # shift_window
                s = w.pop(0)
                cw[s] -= 1; rw -= cw[s]
                if L > len(w):
                    L -= 1; cv[s] -= 1; rv -= cv[s]
            w.append(t)
            L += 1
            rw += cw[t]; cw[t] += 1
            rv += cv[t]; cv[t] += 1
            if cv[t] * 10 > T2:
                while True:
                    s = w[len(w) - L]
                    cv[s] -= 1; rv -= cv[s]; L -= 1
                    if s == t:
                        break
            if rw * 10 > L * T:                                   # find_perfect
                c = cv[:]
                r, max_r, max_l, nw = rv, 0, 0, len(w)
                j = 0
                for x in range(nw - L - 1, -1, -1):
                    tt = w[x]
                    r += c[tt]; c[tt] += 1
                    new_l = nw - x - 1
                    if r * 10 > T * new_l:
                        # (the reference scans P from its head for every x; the scan goes on from where the last one stopped here, which finds the same j and
                        # the same maximum: x + start only falls, and an entry the scan has passed, or the one just inserted, cannot raise max_r / max_l again)
                        while j < len(P) and P[j][0] >= x + start:
                            p = P[j]
                            if max_r == 0 or p[2] * max_l > max_r * p[3]:
                                max_r, max_l = p[2], p[3]
                            j += 1
                        if max_r == 0 or r * max_l >= max_r * new_l:
                            max_r, max_l = r, new_l
                            P.insert(j, [x + start, nw + 2 + start, r, new_l])
                            if x + start > i and i >= count_from:
                                _bump(census, "displaced")
                if len(P) > max_pn:
                    max_pn = len(P)
        else:
            start = (l - W + 1 if l - W + 1 > 0 else 0) + (i + 1 - l)
            while P:
                flush(i, start)
                start += 1
            l = t = 0
    _peak(census, "max_pn", max_pn)


def _chain(res, ps, pf):
    """save_masked_regions' merge into the previous result (src/sdust.c:93-98)"""
    if res and ps <= res[-1][1]:
        if pf > res[-1][1]:
            res[-1][1] = pf
    else:
        res.append([ps, pf])


def _close(res, saves, n, seg, census):
    if census is not None:
        _bump(census, "past_end", sum(1 for s, _ in saves if s >= n))
        _bump(census, "order_inversions", sum(1 for x, y in zip(saves, saves[1:]) if y[0] // seg < x[0] // seg))
        _bump(census, "seam_crossers", sum(1 for s, f in res if s // seg != (f - 1) // seg))
    return [(s, f) for s, f in res]


def sdust_full(seq, T, W, census=None):
    code = codes_of(seq); n = len(code)
    res, saves = [], []

    def save(i, ps, pf):
        saves.append((ps, pf)); _chain(res, ps, pf)
    _automaton(code, n, T, W, range(n + 1), save, census)
    return _close(res, saves, n, seg_of(W), census)


def lane_starts(code, n, W, seg, words, back):
    """lcd_sdust_batch's ring of word ends: per segment the first base of the `words`-th last triplet word that ends before max(0, a - back), 0 where there
    are fewer (a word ends at i when i - 2 .. i are all A/C/G/T)"""
    n_seg = (n + seg - 1) // seg
    ring, rn, l, nxt = [-1] * words, 0, 0, 0
    frm = [0] * n_seg
    for i in range(n):
        if nxt >= n_seg:
            break
        while nxt < n_seg and max(0, nxt * seg - back) == i:
            frm[nxt] = max(0, ring[rn % words] - 2) if rn >= words else 0
            nxt += 1
        if code[i] < 4:
            l += 1
            if l >= 3:
                ring[rn % words] = i; rn += 1
        else:
            l = 0
    return frm


def sdust_segmented(seq, T, W, census=None, rule="step"):
    assert rule in ("step", "start")
    code = codes_of(seq); n = len(code)
    seg = seg_of(W)
    n_seg = (n + seg - 1) // seg
    frm = lane_starts(code, n, W, seg, W + 4, 2 * W) if rule == "step" else lane_starts(code, n, W, seg, 2 * W + 4, W)
    res, saves = [], []
    for k in range(n_seg):
        a = k * seg; b = min(n, a + seg)
        _peak(census, "max_back", a - frm[k])
        mine = []
        if rule == "step":
            last = k == n_seg - 1
            lane = []                                             # the lane folds its own saves; the host folds the lanes' lists

            def save(i, ps, pf):
                if i >= a:
                    mine.append((ps, pf)); _chain(lane, ps, pf)
            _automaton(code, n, T, W, range(frm[k], n + 1 if last else b), save, census, count_from=a)
            _peak(census, "max_lane", len(lane))
            for ps, pf in lane:
                _chain(res, ps, pf)
        else:
            to = min(n, b + 2 * W + 8)

            def save(i, ps, pf):
                if a <= ps < b:
                    mine.append((ps, pf))
            _automaton(code, n, T, W, range(frm[k], to + 1 if to == n else to), save, census, count_from=a)
            _peak(census, "max_lane", len(mine))                   # (unfolded: more than cap on pieces of one word, error -24 on valid input)
            for ps, pf in mine:
                _chain(res, ps, pf)
        saves += mine
    return _close(res, saves, n, seg, census)
