"""A plain reference for raw deflate streams (RFC 1951), pure Python: what zlib's inflate cannot tell a test about the stream deflate_kernel.hip wrote.
  * decode(comp): a bit-level reader of one raw stream -> every block's header fields, code lengths, run-length tokens and LZ77 tokens with their bit positions;
    it raises DeflateError on anything RFC 1951 forbids;
  * huffman_cost(freqs): the optimal unrestricted cost sum f * len (the cost is unique, the lengths are not: tests compare costs);
  * package_merge(freqs, limit): optimal length-limited code lengths (Larmore & Hirschberg 1990);
  * mk_lengths(freqs, limit): the construction that the kernel's header NAMES -- Moffat & Katajainen's minimum-redundancy lengths on the (frequency, symbol)
    order, clamped to the limit, repaired down the Kraft sum (the code-length alphabet: replaced by the package-merge lengths when they are too deep), the most
    frequent symbols taking the shortest lengths -- rebuilt here from that description; it is
    used only where a stream cannot show the kernel's own choice (the dynamic size of a block that was written with the fixed code);
  * rle_tokens(lens): the greedy run-length coding of a code-length sequence; sizes(...): the bit counts of the stored / fixed / dynamic forms;
  * the payload builders of tests/test_gpu_deflate_stream.py, so that tests/test_deflate_stream_oracle.py checks their preconditions without a GPU.
Written from RFC 1951 only."""
import heapq

import numpy as np

CLORD = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
RLE_EXTRA = {16: 2, 17: 3, 18: 7}


class DeflateError(ValueError):
    pass


def len_symbol(length):
    """3 ... 258 -> (literal/length symbol, extra bits)"""
    for s in range(28, -1, -1):
        if length >= LEN_BASE[s]:
            return 257 + s, LEN_EXTRA[s]
    raise ValueError(length)


def dist_symbol(dist):
    """1 ... 32 768 -> (distance symbol, extra bits)"""
    for s in range(29, -1, -1):
        if dist >= DIST_BASE[s]:
            return s, DIST_EXTRA[s]
    raise ValueError(dist)


def kraft(lens, limit=15):
    """the Kraft sum of the non-zero lengths in units of 2 ** -limit (a complete code gives 1 << limit)"""
    return sum(1 << (limit - l) for l in lens if l)


def _table(lens, what, one_code_ok):
    """code lengths -> ({(length, bit-reversed code): symbol}, sorted lengths in use); RFC 1951 3.2.2.  Raises on an over-subscribed code and on an incomplete one,
    except (one_code_ok) a lone code of one bit, which zlib accepts as well"""
    used = [l for l in lens if l]
    if not used:
        return {}, []
    k = kraft(used)
    if k > 1 << 15:
        raise DeflateError("over-subscribed %s code" % what)
    if k < 1 << 15 and not (one_code_ok and used == [1]):
        raise DeflateError("incomplete %s code" % what)
    count = [0] * 16
    for l in used:
        count[l] += 1
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    tab = {}
    for s, l in enumerate(lens):
        if l:
            c = nxt[l]; nxt[l] += 1
            tab[(l, int(format(c, "0%db" % l)[::-1], 2))] = s
    return tab, sorted(set(used))


def decode(comp):
    """one raw deflate stream -> dict(blocks, data, bits).  blocks: one dict per deflate block with bfinal, btype, bit_start, bit_end, data_start, data_end and
      stored:  len, nlen
      coded:   tokens = [(bit position, bits, literal byte | (length, distance))] (the end-of-block symbol is not a token: eob_bits is its length),
               lit_lens (288 for the fixed code, HLIT for a dynamic one), dist_lens
      dynamic: hlit, hdist, hclen (the COUNTS: 257 ..., 1 ..., 4 ...), cl_lens (19, by symbol), rle = [(code-length symbol, extra value)]
    bits: the bits consumed up to the end of the final block; data: the reconstructed bytes."""
    comp = bytes(comp)
    nb_total = len(comp)
    acc = cnt = bp = pos = 0
    out = bytearray()
    blocks = []
    mask = [(1 << i) - 1 for i in range(64)]

    def take(n):
        nonlocal acc, cnt, bp, pos
        while cnt < n:
            if bp >= nb_total:
                raise DeflateError("the stream ends inside a block")
            acc |= comp[bp] << cnt; cnt += 8; bp += 1
        v = acc & mask[n]
        acc >>= n; cnt -= n; pos += n
        return v

    def sym_of(tab, lengths, what):
        nonlocal acc, cnt, bp, pos
        while cnt < 15 and bp < nb_total:
            acc |= comp[bp] << cnt; cnt += 8; bp += 1
        for l in lengths:
            s = tab.get((l, acc & mask[l]))
            if s is not None:
                if l > cnt:
                    raise DeflateError("the stream ends inside a block")
                acc >>= l; cnt -= l; pos += l
                return s, l
        raise DeflateError("no %s code matches" % what)

    while True:
        b = dict(bit_start=pos, data_start=len(out))
        b["bfinal"] = take(1); b["btype"] = bt = take(2)
        if bt == 3:
            raise DeflateError("reserved block type")
        if bt == 0:
            take(cnt & 7)                                              # to the byte boundary
            b["len"] = n = take(16); b["nlen"] = take(16)
            if b["len"] ^ b["nlen"] != 0xffff:
                raise DeflateError("stored LEN / NLEN mismatch")
            start = bp - (cnt >> 3)
            if start + n > nb_total:
                raise DeflateError("the stream ends inside a stored block")
            out += comp[start:start + n]
            acc = cnt = 0; bp = start + n; pos += 8 * n
        else:
            if bt == 1:
                lit_lens, dist_lens = list(FIXED_LIT), list(FIXED_DIST)
            else:
                b["hlit"] = hlit = take(5) + 257; b["hdist"] = hdist = take(5) + 1; b["hclen"] = hclen = take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise DeflateError("too many length or distance symbols")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORD[i]] = take(3)
                b["cl_lens"] = cl
                ctab, clen = _table(cl, "code-length", False)
                lens, rle = [], []
                while len(lens) < hlit + hdist:
                    s, _ = sym_of(ctab, clen, "code-length")
                    if s < 16:
                        rle.append((s, 0)); lens.append(s)
                    else:
                        e = take(RLE_EXTRA[s])
                        rle.append((s, e))
                        if s == 16:
                            if not lens:
                                raise DeflateError("a repeat with nothing before it")
                            lens += [lens[-1]] * (3 + e)
                        else:
                            lens += [0] * ((3 if s == 17 else 11) + e)
                if len(lens) > hlit + hdist:
                    raise DeflateError("a run passes the end of the code lengths")
                b["rle"] = rle
                b["header_bits"] = pos - b["bit_start"]
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
                if lit_lens[256] == 0:
                    raise DeflateError("no end-of-block code")
            b["lit_lens"], b["dist_lens"] = lit_lens, dist_lens
            ltab, llen = _table(lit_lens, "literal/length", False)
            dtab, dlen = _table(dist_lens, "distance", True)
            toks = []
            lget, dget = ltab.get, dtab.get
            while True:
                while cnt < 48 and bp < nb_total:                      # a token has at most 15 + 5 + 15 + 13 bits
                    acc |= int.from_bytes(comp[bp:bp + 6], "little") << cnt
                    got = min(6, nb_total - bp); cnt += 8 * got; bp += got
                s = None
                for l in llen:
                    s = lget((l, acc & mask[l]))
                    if s is not None:
                        break
                if s is None:
                    raise DeflateError("no literal/length code matches")
                if s < 256:
                    acc >>= l; cnt -= l
                    if cnt < 0:
                        raise DeflateError("the stream ends inside a block")
                    toks.append((pos, l, s)); pos += l
                    out.append(s)
                    continue
                if s == 256:
                    acc >>= l; cnt -= l
                    if cnt < 0:
                        raise DeflateError("the stream ends inside a block")
                    b["eob_bits"] = l; pos += l
                    break
                if s > 285:
                    raise DeflateError("length symbol above 285")
                nb = l
                acc >>= l
                e = LEN_EXTRA[s - 257]
                length = LEN_BASE[s - 257] + (acc & mask[e])
                acc >>= e; nb += e
                d = None
                for l in dlen:
                    d = dget((l, acc & mask[l]))
                    if d is not None:
                        break
                if d is None:
                    raise DeflateError("no distance code matches")
                if d > 29:
                    raise DeflateError("distance symbol above 29")
                acc >>= l; nb += l
                e = DIST_EXTRA[d]
                dist = DIST_BASE[d] + (acc & mask[e])
                acc >>= e; nb += e
                cnt -= nb
                if cnt < 0:
                    raise DeflateError("the stream ends inside a block")
                if dist > len(out):
                    raise DeflateError("a distance before the start of the data")
                toks.append((pos, nb, (length, dist))); pos += nb
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
            b["tokens"] = toks
        b["bit_end"] = pos; b["data_end"] = len(out)
        blocks.append(b)
        if b["bfinal"]:
            break
    return dict(blocks=blocks, data=bytes(out), bits=pos)


# ---------------- optimal codes ----------------
def huffman_cost(freqs):
    """sum f * len of an optimal prefix code of the non-zero frequencies, no length limit: the sum of the merged weights.  One symbol alone costs one bit each"""
    h = [int(f) for f in freqs if f > 0]
    if len(h) < 2:
        return sum(h)
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        cost += a
        heapq.heappush(h, a)
    return cost


def package_merge(freqs, limit):
    """optimal code lengths of at most `limit` bits (0 for a zero frequency): package-merge.  An item is (weight, how often each symbol is in it); `limit` lists of
    the sorted leaves, each merged with the packages (pairs) of the list before it; the first 2n - 2 items of the last list say how long each code is"""
    syms = [s for s, f in enumerate(freqs) if f > 0]
    n = len(syms)
    lens = [0] * len(freqs)
    if n == 0:
        return lens
    if n == 1:
        lens[syms[0]] = 1
        return lens
    if n > 1 << limit:
        raise ValueError("%d symbols have no code of %d bits" % (n, limit))
    order = sorted(syms, key=lambda s: (int(freqs[s]), s))
    idx = {s: i for i, s in enumerate(order)}
    leaves = []
    for s in order:
        v = np.zeros(n, dtype=np.int64); v[idx[s]] = 1
        leaves.append((int(freqs[s]), v))
    cur = list(leaves)
    for _ in range(limit - 1):
        packs = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        merged, i, j = [], 0, 0
        while i < n or j < len(packs):
            if j >= len(packs) or (i < n and leaves[i][0] <= packs[j][0]):
                merged.append(leaves[i]); i += 1
            else:
                merged.append(packs[j]); j += 1
        cur = merged
    tot = np.zeros(n, dtype=np.int64)
    for w, v in cur[:2 * n - 2]:
        tot += v
    for s in order:
        lens[s] = int(tot[idx[s]])
    return lens


def cost(freqs, lens):
    return sum(int(f) * int(l) for f, l in zip(freqs, lens))


def mk_depths(sorted_freqs):
    """Moffat & Katajainen's in-place minimum-redundancy code lengths of frequencies in ascending order (>= 2 of them) -> the depths, deepest first.  A tie between a
    leaf and an internal node takes the leaf (the rule the kernel's construction uses)"""
    a = [int(f) for f in sorted_freqs]
    n = len(a)
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            v = a[root]; a[root] = nxt; root += 1
        else:
            v = a[leaf]; leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            v += a[root]; a[root] = nxt; root += 1
        else:
            v += a[leaf]; leaf += 1
        a[nxt] = v
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            used += 1; root -= 1
        while avbl > used:
            a[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl = 2 * used; dpth += 1; used = 0
    return a


def mk_lengths(freqs, limit, info=None):
    """the kernel header's construction (see the module text) -> lengths by symbol.  At least two symbols get a code: the first free symbols are given frequency 1.
    info (a dict) receives depth = the deepest code before limiting, clamped = the symbols beyond the limit, steps = the repair steps"""
    f = [int(x) for x in freqs]
    need = 2 - sum(1 for x in f if x)
    for s in range(min(3, len(f))):
        if need > 0 and not f[s]:
            f[s] = 1; need -= 1
    order = sorted((s for s in range(len(f)) if f[s]), key=lambda s: (f[s], s))
    depths = mk_depths([f[s] for s in order])
    cnt = [0] * (limit + 1)
    for d in depths:
        cnt[min(d, limit)] += 1
    total = sum(cnt[i] << (limit - i) for i in range(1, limit + 1))
    steps = 0
    if total != 1 << limit and limit <= 7 and len(order) <= 21:        # a small alphabet (the code-length one) is limited by package-merge
        pm = package_merge(f, limit)
        cnt = [sum(1 for l in pm if l == i) for i in range(limit + 1)]
        cnt[0], total = 0, 1 << limit
    while total != 1 << limit:
        cnt[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if cnt[i]:
                cnt[i] -= 1; cnt[i + 1] += 2
                break
        total -= 1; steps += 1
    if info is not None:
        info.update(depth=max(depths), clamped=sum(1 for d in depths if d > limit), steps=steps)
    lens = [0] * len(f)
    q = 0
    for l in range(1, limit + 1):                                      # the most frequent symbols take the shortest lengths
        for _ in range(cnt[l]):
            lens[order[len(order) - 1 - q]] = l; q += 1
    return lens


# ---------------- header coding and the three sizes ----------------
def rle_tokens(lens):
    """the greedy run-length coding of a code-length sequence -> [(symbol, extra value)]: a run of zeros (<= 138) becomes 17 / 18 from 3 on, a run of a length that
    repeats the one in front of it (<= 6) becomes 16 from 3 on, everything else is written plainly"""
    out, i, prev = [], 0, -1
    while i < len(lens):
        v, cap, run = lens[i], 138 if lens[i] == 0 else 6, 1
        while run < cap and i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            out.append((18, run - 11))
        elif v == 0 and run >= 3:
            out.append((17, run - 3))
        elif v == prev and run >= 3:
            out.append((16, run - 3))
        else:
            out.append((v, 0)); run = 1
        i += run; prev = v
    return out


def histograms(tokens):
    """decode()'s tokens -> (literal/length histogram of 286 with the end-of-block symbol counted once, distance histogram of 30)"""
    hl, hd = [0] * 286, [0] * 30
    for _, _, t in tokens:
        if isinstance(t, tuple):
            hl[len_symbol(t[0])[0]] += 1; hd[dist_symbol(t[1])[0]] += 1
        else:
            hl[t] += 1
    hl[256] += 1
    return hl, hd


def rle_histogram(rle):
    h = [0] * 19
    for s, _ in rle:
        h[s] += 1
    return h


def body_bits(tokens, lit_lens, dist_lens):
    """the bits of the tokens and the end-of-block symbol under the given code lengths, extra bits included"""
    bits = lit_lens[256]
    for _, _, t in tokens:
        if isinstance(t, tuple):
            ls, le = len_symbol(t[0]); ds, de = dist_symbol(t[1])
            bits += lit_lens[ls] + le + dist_lens[ds] + de
        else:
            bits += lit_lens[t]
    return bits


def sizes(tokens, n, lit_lens=None, dist_lens=None, cl_lens=None, rle=None, hclen=None):
    """the bit counts of one block's three forms -> dict(stored, fixed, dynamic): stored = 8 (n + 5); fixed = 3 + the tokens under the fixed code; dynamic = 3 + 14 +
    3 HCLEN + the run-length tokens under cl_lens with their 2 / 3 / 7 extra bits + the tokens under lit_lens / dist_lens (None without a dynamic code)"""
    r = dict(stored=8 * (n + 5), fixed=3 + body_bits(tokens, FIXED_LIT, FIXED_DIST), dynamic=None)
    if lit_lens is not None:
        r["dynamic"] = 3 + 14 + 3 * hclen + sum(cl_lens[s] + RLE_EXTRA.get(s, 0) for s, _ in rle) + body_bits(tokens, lit_lens, dist_lens)
    return r


def dynamic_form(tokens):
    """the dynamic form that the kernel header's construction gives these tokens -> the keyword arguments of sizes()"""
    hl, hd = histograms(tokens)
    lit, dist = mk_lengths(hl, 15), mk_lengths(hd, 15)
    hlit = max(257, max(s for s in range(286) if lit[s]) + 1)
    hdist = max([s + 1 for s in range(30) if dist[s]] or [1])
    rle = rle_tokens(lit[:hlit] + dist[:hdist])
    cl = mk_lengths(rle_histogram(rle), 7)
    hclen = max(4, max(i + 1 for i in range(19) if cl[CLORD[i]]))
    return dict(lit_lens=lit, dist_lens=dist, cl_lens=cl, rle=rle, hclen=hclen)


# ---------------- payloads ----------------
def existing_payloads():
    """the payload classes of tests/test_gpu_deflate.py, byte for byte"""
    from test_gpu_deflate import _payloads
    return _payloads(np.random.default_rng(5))


def from_counts(counts, seed):
    """{byte value: count} -> the bytes in a seeded random order"""
    a = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in sorted(counts.items())])
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


TAIL_RARE = (1, 2, 4, 7, 12, 20, 33, 54, 88, 143, 232, 376)
SINGLES_CHAIN = (65, 130, 196, 330, 530)
CLSKEW_L = {3: 1, 7: 54, 8: 88, 9: 33, 10: 20, 11: 12, 12: 7, 13: 4, 14: 2, 15: 1}


def tail_counts():
    """128 bulk values with 438 + i (450 + i trimmed by 12 each, to fit 65 280 bytes) and 12 rare values with tie-free counts"""
    c = {i: 438 + i for i in range(128)}
    c.update({128 + k: v for k, v in enumerate(TAIL_RARE)})
    return c


def singles_counts():
    """110 bulk values near 520, 64 values that occur once, and the chain 65, 130, 196, 330, 530"""
    c = {i: 517 + i % 7 for i in range(110)}
    c.update({110 + k: 1 for k in range(64)})
    c.update({174 + k: v for k, v in enumerate(SINGLES_CHAIN)})
    return c


def singles_long_counts():
    """singles with the chain 90, 180, 270, 450: the few length symbols that the matcher adds to the histogram (some hundred 3-byte matches) take singles off its
    edge -- 4 symbols beyond the limit instead of 65 -- and leave this one on it"""
    c = {i: 517 + i % 7 for i in range(110)}
    c.update({110 + k: 1 for k in range(64)})
    c.update({174 + k: v for k, v in enumerate((90, 180, 270, 450))})
    return c


def clskew_counts():
    """byte value i occurs round(65 000 * 2 ** -L_i) times; the multiset of L is CLSKEW_L, dealt to the byte values 0 ... 221 in a seeded random order"""
    L = np.array([l for l, k in sorted(CLSKEW_L.items()) for _ in range(k)])
    np.random.default_rng(77).shuffle(L)
    return {i: int(round(65000 * 2.0 ** -int(l))) for i, l in enumerate(L)}


def limit_payloads():
    """the payloads whose literal/length code (clskew: whose code-length code as well) is deeper than its limit"""
    return dict(skew=existing_payloads()["skew"], tail=from_counts(tail_counts(), 21), singles=from_counts(singles_counts(), 22),
                singles_long=from_counts(singles_long_counts(), 22), clskew=from_counts(clskew_counts(), 23))


def byte_histogram(data):
    """the literal/length histogram of a payload coded without a single match: its bytes and one end-of-block symbol"""
    h = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=286).tolist()
    h[256] = 1
    return h


def far_payload(dist, seed=31):
    """400 random bytes, a filler over 4 symbols, the same 400 bytes `dist` behind their first copy"""
    rng = np.random.default_rng(seed)
    head = bytes(rng.integers(0, 256, 400).astype(np.uint8))
    return head + bytes(rng.integers(0, 4, dist - 400).astype(np.uint8)) + head


def len3_payload(dist, n_plants=40, seed=32):
    """random bytes over 64 values (so that the block is coded, not stored, and its tokens can be seen) with n_plants repeats of exactly three bytes `dist` behind
    their first copy (the bytes on either side of the copy differ from the original's) -> (bytes, [position of each copy])"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 64, dist + 64 * n_plants + 64).astype(np.uint8)
    at = []
    for k in range(n_plants):
        p = dist + 32 + 64 * k
        a[p:p + 3] = a[p - dist:p - dist + 3]
        a[p + 3] = a[p - dist + 3] ^ 0x15
        a[p - 1] = a[p - dist - 1] ^ 0x15
        at.append(p)
    return a.tobytes(), at


def zero_run_payload(seed=33):
    """20 000 bytes over the values 0 ... 9 and 200 ... 255 with a skewed distribution: 190 unused literal symbols in a row, more than one symbol 18 can cover"""
    rng = np.random.default_rng(seed)
    vals = np.array(list(range(10)) + list(range(200, 256)), dtype=np.uint8)
    return vals[np.minimum(rng.geometric(0.08, 20000) - 1, len(vals) - 1)].tobytes()


def longtok_payload(n_short=5000, n_far=60, n_rare=6, seed=35):
    """40 000 random bytes with n_short short repeats (4 - 6 bytes, 10 - 500 back), n_far long ones (150 - 250 bytes, 16 385 - 24 000 back) and n_rare more at
    24 577 - 32 000 back.  A far token carries up to 5 + 13 extra bits behind a rare length code and a distance code that is rare among the short repeats': the
    n_far ones are about 37 bits each and many enough for some to start late in a dword, the n_rare ones use a distance symbol of their own and pass 40 bits"""
    rng = np.random.default_rng(seed)
    n = 40000
    a = rng.integers(0, 256, n).astype(np.uint8)

    def plant(lo, count, len_lo, len_hi, d_lo, d_hi):
        for p in np.sort(rng.choice(np.arange(lo, n - 300 if len_hi > 10 else n - 10), count, replace=False)):
            l, d = int(rng.integers(len_lo, len_hi + 1)), int(rng.integers(d_lo, d_hi + 1))
            a[p:p + l] = a[p - d:p - d + l]
    plant(600, n_short, 4, 6, 10, 500)
    plant(24100, n_far, 150, 250, 16385, 24000)
    plant(32100, n_rare, 150, 250, 24577, 32000)
    return a.tobytes()


def hash3(data):
    """the match pass's bucket of the three bytes at every position of a payload that has three bytes left (numpy array)"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    if len(a) < 3:
        return np.zeros(0, dtype=np.uint64)
    w = a[:-2] | (a[1:-1] << np.uint64(8)) | (a[2:] << np.uint64(16))
    return ((w * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)) >> np.uint64(20)


def pass_collision_free(data):
    """True when the match pass cannot meet a hash collision whose winner matters: the payload fits one pass of 64 positions (the table is written after the pass
    and never read again), or no two positions less than 64 apart share a bucket"""
    if len(data) <= 64:
        return True
    h = hash3(data)
    for d in range(1, min(64, len(h))):
        if (h[d:] == h[:-d]).any():
            return False
    return True
