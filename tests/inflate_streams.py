"""A raw-deflate WRITER driven by tokens (RFC 1951), pure Python: the mirror image of tests/deflate_stream.py's reader.  A zlib writer can only be steered through
level, strategy and flush points; here a test decides every bit -- each token, each code length, each run-length token of a dynamic header, each padding bit -- and
zlib's inflate is the judge of whether the stream is valid.
  * BitWriter, canonical(lens): bits LSB first, canonical codes from code lengths (no validation: an over-subscribed set can be written too);
  * stored_block / fixed_block / dynamic_block: the three block kinds; a token is a literal byte or (length, distance);
  * expand(tokens, prefix): the bytes the tokens stand for, in plain Python (independent of zlib);
  * member(raw, data, ...): one BGZF block around a raw stream, with other gzip extra subfields before / after 'BC';
  * group_a() ... group_e(), repack(): the case tables of tests/test_inflate_streams_oracle.py (CPU: zlib judges them, the coverage claims are proved) and
    tests/test_gpu_inflate_streams.py (the device's decoder, inflate_kernel.hip).  Each table is a list of Case(name, image, expected bytes | None,
    index of the member expected to be refused | None, members).
Numbers that come from the kernel are written as literals next to the constant's name."""
import struct
import zlib
from collections import namedtuple

import numpy as np

from deflate_stream import CLORD, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA, dist_symbol, kraft, len_symbol, package_merge, rle_tokens

# members: [Member] in file order (the EOF block is not listed)
Case = namedtuple("Case", "name image expected refused members")
# off: file offset of the member; src: file offset of its raw stream; clen: the stream's bytes; uoff / ulen: its place in the inflated stream; claims: what the
# CPU test proves about the stream [(kind, value ...)]
Member = namedtuple("Member", "name off src clen uoff ulen claims raw")


# ---------------- bits, codes, blocks ----------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, c):
        """a Huffman code from canonical(): (bit-reversed code, length)"""
        self.bits(c[0], c[1])

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self, fill=0):
        """to the next byte boundary; the skipped bits take the low bits of `fill`"""
        if self.n:
            self.bits(fill, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self, fill=0):
        """the bytes; the unused high bits of the last byte take the low bits of `fill`"""
        out = bytes(self.out)
        if self.n:
            out += bytes([(self.acc | ((fill << self.n) & 255)) & 255])
        return out


def canonical(lens):
    """code lengths -> [(bit-reversed code, length) | None] by symbol, RFC 1951 3.2.2.  Nothing is validated: for an over-subscribed set the codes wrap"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l:
            c = nxt[l] & ((1 << l) - 1); nxt[l] += 1
            out.append((int(format(c, "0%db" % l)[::-1], 2), l))
        else:
            out.append(None)
    return out


def put_tokens(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, tuple):
            ls, le = len_symbol(t[0]); w.code(lit[ls]); w.bits(t[0] - LEN_BASE[ls - 257], le)
            ds, de = dist_symbol(t[1]); w.code(dist[ds]); w.bits(t[1] - DIST_BASE[ds], de)
        else:
            w.code(lit[t])


def stored_block(w, data, final=0, len_=None, nlen=None, pad=0):
    """header, the padding bits (low bits of `pad`), LEN / NLEN (explicit ones may lie), the bytes"""
    w.bits(final, 1); w.bits(0, 2); w.align(pad)
    n = len(data) if len_ is None else len_
    w.bits(n, 16); w.bits(n ^ 0xffff if nlen is None else nlen, 16)
    w.raw(data)


FIXED_LIT_CODES, FIXED_DIST_CODES = canonical(FIXED_LIT), canonical(FIXED_DIST)


def fixed_block(w, tokens, final=0, eob=True):
    w.bits(final, 1); w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LIT_CODES, FIXED_DIST_CODES)
    if eob:
        w.code(FIXED_LIT_CODES[256])


def default_cl_lens(rle):
    """a complete code-length code (<= 7 bits) for these run-length tokens; a lone symbol gets a partner so that the code is complete"""
    h = [0] * 19
    for s, _ in rle:
        h[s] += 1
    if sum(1 for x in h if x) < 2:
        h[0 if not h[0] else 1] += 1
    return package_merge(h, 7)


def dynamic_block(w, tokens, lit_lens, dist_lens, final=0, cl_lens=None, hclen=None, rle=None, hlit=None, hdist=None, eob=True):
    """lit_lens: HLIT entries (257 ... 286), dist_lens: HDIST entries (1 ... 30); rle: the caller's own [(code-length symbol, extra value)] for lit_lens + dist_lens
    (default: the greedy coding); cl_lens: 19 lengths by symbol; hclen: the COUNT (4 ... 19); hlit / hdist: raw 5-bit FIELD values that override the lists' sizes"""
    rle = rle_tokens(list(lit_lens) + list(dist_lens)) if rle is None else rle
    cl_lens = default_cl_lens(rle) if cl_lens is None else cl_lens
    hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CLORD[i]])) if hclen is None else hclen
    w.bits(final, 1); w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5); w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5); w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CLORD[i]], 3)
    cl = canonical(cl_lens)
    for s, e in rle:
        w.code(cl[s])
        if s >= 16:
            w.bits(e, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    put_tokens(w, tokens, lit, dist)
    if eob:
        w.code(lit[256])


def expand(tokens, prefix=b""):
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, tuple):
            length, d = t
            assert 1 <= d <= len(out)
            for _ in range(length):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)


# ---------------- the container ----------------
def subfield(n, si=b"XY"):
    """a gzip extra subfield of n >= 4 bytes in all that is not BGZF's"""
    assert n >= 4
    return si + struct.pack("<H", n - 4) + bytes((7 * k + n) & 255 for k in range(n - 4))


def member(raw, data, extra_before=b"", extra_after=b"", crc=None, isize=None):
    """one BGZF block (SAM specification 4.1): a gzip member whose extra field holds 'B' 'C' 2 BSIZE, here between the caller's other subfields"""
    xlen = 6 + len(extra_before) + len(extra_after)
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536, total
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + extra_before + struct.pack("<BBHH", 66, 67, 2, total - 1) + extra_after + raw
            + struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xffffffff, len(data) if isize is None else isize))


def fixed_empty():
    w = BitWriter(); fixed_block(w, [], final=1)
    return w.getvalue()


EOF_BLOCK = member(fixed_empty(), b"")


class Image:
    """members in file order with their offsets"""

    def __init__(self):
        self.image, self.expected, self.members = bytearray(), bytearray(), []

    def add(self, name, raw, data, claims=(), extra_before=b"", extra_after=b"", crc=None, isize=None):
        off = len(self.image)
        src = off + 18 + len(extra_before) + len(extra_after)
        self.image += member(raw, data, extra_before, extra_after, crc, isize)
        self.members.append(Member(name, off, src, len(raw), len(self.expected), len(data), tuple(claims), raw))
        self.expected += data

    def add_at(self, name, raw, data, claims=(), src_mod=None, end_mod=None, bc_first=True):
        """the member shifted by one extra subfield so that (file offset of the stream) % 256 == src_mod, or (stream's end) % 256 == end_mod"""
        base = len(self.image) + 18 + 4
        want = src_mod if src_mod is not None else end_mod - len(raw)
        sf = subfield(4 + (want - base) % 256)
        self.add(name, raw, data, claims, extra_before=b"" if bc_first else sf, extra_after=sf if bc_first else b"")

    def case(self, name, expected=True, refused=None):
        return Case(name, bytes(self.image) + EOF_BLOCK, bytes(self.expected) if expected else None, refused, list(self.members))


def rbytes(rng, n, lo=0, hi=256):
    return bytes(rng.integers(lo, hi, n).astype(np.uint8))


def prefixed_fixed(prefix, tokens):
    """a stored block of `prefix` (if any), then the tokens in one final fixed-code block"""
    w = BitWriter()
    if prefix:
        stored_block(w, prefix)
    fixed_block(w, tokens, final=1)
    return w.getvalue()


# ---------------- A: match geometry against the ring ----------------
# inflate_kernel.hip: WINB = 2048 (ring bytes), HALF = 1024 (a half goes to HBM when pos - flushed reaches it), NEAR = 1536 (a match further back reads HBM);
# a match copy runs in strides of 64 lanes with three overlap paths (distance >= length, distance 1, distance < length)
A_DISTANCES = (1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 1023, 1024, 1025, 1535, 1536, 1537, 1538, 1793, 2047, 2048, 2049, 4095, 4096,
               4097, 16384, 32767, 32768)
A_LENGTHS = (3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 192, 193, 257, 258)
A_NEAR_PREFIX, A_FAR_PREFIX = 2560, 32768      # stored bytes in front of the coded block: more than the largest distance of the class


def a_phases(length):
    """pos mod 1024 (HALF) at the start of the match: 766 + 258 ends exactly on a half, 1023 is the largest unflushed backlog, 1024 - length ends on a half"""
    return sorted({0, 1, 766, 767, 1023, 1024 - length})


def a_plan():
    return [(d, l, p) for d in A_DISTANCES for l in A_LENGTHS for p in a_phases(l)]


def _a_members(img, plan, prefix_len, rng, tag):
    by_phase = {}
    for k in rng.permutation(len(plan)):
        by_phase.setdefault(plan[k][2], []).append(plan[k])
    i = 0
    while by_phase:
        prefix = rbytes(rng, prefix_len)
        toks, pos, planned = [], prefix_len, []
        while by_phase:
            ph = min(by_phase, key=lambda p: (p - pos) % 1024)       # the phase is set with literals: the nearest one ahead costs the fewest
            pad = (ph - pos) % 1024
            d, l, _ = by_phase[ph][-1]
            if pos + pad + l > 65536:
                break
            by_phase[ph].pop()
            if not by_phase[ph]:
                del by_phase[ph]
            toks += list(rbytes(rng, pad)); pos += pad
            toks.append((l, d)); planned.append((pos, l, d)); pos += l
        img.add("%s%d" % (tag, i), prefixed_fixed(prefix, toks), expand(toks, prefix), [("matches", tuple(planned))])
        i += 1


def group_a():
    rng = np.random.default_rng(101)
    img = Image()
    plan = a_plan()
    _a_members(img, [m for m in plan if m[0] < A_NEAR_PREFIX], A_NEAR_PREFIX, rng, "near")
    _a_members(img, [m for m in plan if m[0] >= A_NEAR_PREFIX], A_FAR_PREFIX, rng, "far")
    for d in A_DISTANCES:              # distance == pos: the source starts at byte 0 of the block (d = 32768: the window's far end at pos 32768)
        prefix = rbytes(rng, d)
        toks, planned = [(258, d)], [(d, 258, d)]
        if d + 259 <= 32768:           # and once more, one literal later: again from byte 0
            toks += [7, (3, d + 259)]; planned.append((d + 259, 3, d + 259))
        img.add("dist_eq_pos_%d" % d, prefixed_fixed(prefix, toks), expand(toks, prefix), [("matches", tuple(planned))])
    for d in (1, 2, 3, 4):             # the same with the source bytes coded as literals (no stored block in front)
        lits = list(rbytes(rng, d))
        toks = lits + [(258, d)]
        img.add("lit_dist_eq_pos_%d" % d, prefixed_fixed(b"", toks), expand(toks), [("matches", ((d, 258, d),))])
    return [img.case("A")]


# ---------------- B: code shapes ----------------
def complete(fixed, n_free):
    """n_free further lengths that complete the code begun by the lengths `fixed` (zeros ignored): the rest of the Kraft sum in binary, the shortest split until
    there are enough"""
    rest = (1 << 15) - kraft(fixed)
    parts = [1, 1] if rest == 1 << 15 else [l for l in range(1, 16) if rest >> (15 - l) & 1]
    assert 0 < len(parts) <= n_free, (rest, n_free)
    while len(parts) < n_free:
        l = min(parts)
        assert l < 15
        parts.remove(l); parts += [l + 1, l + 1]
    return sorted(parts)


def all_symbol_tokens(lit_lens, dist_lens, rng):
    """every literal, every length symbol and every distance symbol that has a code, at least once -> (tokens, bytes needed in front for the distances)"""
    lits = [s for s in range(256) if lit_lens[s]]
    toks = [lits[k] for k in rng.permutation(len(lits))]
    ls = [s for s in range(257, min(len(lit_lens), 286)) if lit_lens[s]]
    ds = [s for s in range(min(len(dist_lens), 30)) if dist_lens[s]]
    need = 0
    if ls and ds:
        for i in range(max(len(ls), len(ds))):
            a, b = ls[i % len(ls)] - 257, ds[i % len(ds)]
            length = LEN_BASE[a] + (int(rng.integers(0, 1 << LEN_EXTRA[a])) if a != 27 else int(rng.integers(0, 31)))
            dist = DIST_BASE[b] + int(rng.integers(0, 1 << DIST_EXTRA[b]))
            toks.append((length, dist)); need = max(need, dist)
            if lits:
                toks.append(lits[int(rng.integers(0, len(lits)))])
    return toks, need


def _prefix_for(need):
    return 0 if need == 0 else 2048 if need <= 2048 else 32768


def _dyn_member(img, name, rng, lit_lens, dist_lens, claims, **kw):
    toks, need = all_symbol_tokens(lit_lens, dist_lens, rng)
    prefix = rbytes(rng, _prefix_for(need))
    w = BitWriter()
    if prefix:
        stored_block(w, prefix)
    dynamic_block(w, toks, lit_lens, dist_lens, final=1, **kw)
    img.add(name, w.getvalue(), expand(toks, prefix), claims)


def shaped_lit_lens(rng):
    """286 literal/length lengths: the chain 1, 2, ... 14, 15, 15 with one code each of 10, 11 and two of 15 bits kept (both sides of the 10-bit primary table, LBITS;
    the bit-serial walk to its end) and the other leaves split until there are 286.  Literal 65 takes 10 bits, length symbol 285 takes 11, literal 0 the first and
    the end-of-block symbol the last code of 15 bits: all ones"""
    free = [l for l in range(1, 15) if l not in (10, 11)]
    while len(free) + 4 < 286:
        l = min(free); free.remove(l); free += [l + 1, l + 1]
    lens = [0] * 286
    lens[65], lens[285], lens[0], lens[256] = 10, 11, 15, 15
    rest = [s for s in range(286) if not lens[s]]
    for s, l in zip((rest[k] for k in rng.permutation(len(rest))), sorted(free)):
        lens[s] = l
    return lens


def shaped_dist_lens(rng):
    """30 distance lengths with codes of 9, 10 and 15 bits (both sides of the 9-bit primary table, DBITS): 1 ... 8, 9, 10, 13 x 2, 14 x 6, 15 x 12"""
    lens = list(range(1, 11)) + [13] * 2 + [14] * 6 + [15] * 12
    return [lens[k] for k in rng.permutation(30)]


def skewed_cl_lens(rle):
    """a complete code-length code that reaches 7 bits: the symbols in use ranked by frequency, weights 3 ** rank (the limit of 7 bits binds)"""
    h = [0] * 19
    for s, _ in rle:
        h[s] += 1
    used = sorted((s for s in range(19) if h[s]), key=lambda s: (h[s], s))
    fake = [0] * 19
    for r, s in enumerate(used):
        fake[s] = 3 ** r
    return package_merge(fake, 7)


def rle_layout(hlit, hdist, runs, rng):
    """code lengths with run-length tokens exactly where the caller wants them.  runs: [(kind 16 | 17 | 18, first entry, count, repeated length for 16)], in order,
    not overlapping, none of the zero runs over entry 256.  The entry in front of a 16 holds its length; every other entry gets a non-zero length of its own, chosen
    so that both codes are complete, and is written as a plain token -> (lit_lens, dist_lens, rle tokens)"""
    total = hlit + hdist
    lens = [None] * total
    for kind, s, n, L in runs:
        assert 0 <= s and s + n <= total and n >= (11 if kind == 18 else 3) and n <= {16: 6, 17: 10, 18: 138}[kind]
        if kind == 16:
            assert lens[s - 1] in (None, L)
            lens[s - 1] = L
        for k in range(s, s + n):
            assert lens[k] is None
            lens[k] = L if kind == 16 else 0
    assert lens[256] != 0
    for lo, hi in ((0, hlit), (hlit, total)):
        free = [k for k in range(lo, hi) if lens[k] is None]
        if free:
            vals = complete([l for l in lens[lo:hi] if l], len(free))
            for k, v in zip(free, (vals[q] for q in rng.permutation(len(vals)))):
                lens[k] = v
    rle, k, runs_at = [], 0, {s: (kind, n) for kind, s, n, _ in runs}
    while k < total:
        if k in runs_at:
            kind, n = runs_at[k]
            rle.append((kind, n - (11 if kind == 18 else 3))); k += n
        else:
            rle.append((lens[k], 0)); k += 1
    return lens[:hlit], lens[hlit:], rle


# the decoder collects code lengths in a 64-entry lane window (pend / pbase) that it writes out at entries 64, 128, 192 and 256; entry 256 is the end-of-block symbol
B_RLE_ENTRIES = (63, 64, 65, 127, 128, 129, 255, 256, 257)
B_RUN_COUNT = {16: 4, 17: 5, 18: 20}


def b_rle_runs():
    """(kind, first entry, count, mode, entry): a run of each kind that begins at / ends at each entry of B_RLE_ENTRIES.  Entry 256 must keep a non-zero length, so the
    zero runs (17, 18) take only the cases that stay clear of it"""
    out = []
    for kind in (16, 17, 18):
        n = B_RUN_COUNT[kind]
        for e in B_RLE_ENTRIES:
            for mode, s in (("begin", e), ("end", e - n + 1)):
                if kind != 16 and s <= 256 < s + n:
                    continue
                out.append((kind, s, n, mode, e))
    return out


def group_b():
    rng = np.random.default_rng(202)
    img = Image()
    lit, dist = shaped_lit_lens(rng), shaped_dist_lens(rng)
    _dyn_member(img, "long_codes", rng, lit, dist, [("lit_bits", 10), ("lit_bits", 11), ("lit_bits", 15), ("dist_bits", 9), ("dist_bits", 10), ("dist_bits", 15),
                                                    ("first_last_longest", "lit"), ("first_last_longest", "dist"), ("eob_bits", 15), ("hlit", 286), ("hdist", 30)])
    # the same lengths under a code-length code with 7-bit codes; length 15 is in use, so HCLEN is 19 (symbol 15 is the last of the transmission order)
    rle = rle_tokens(lit + dist)
    _dyn_member(img, "hclen19_cl7", rng, lit, dist, [("hclen", 19), ("cl_bits", 7)], rle=rle, cl_lens=skewed_cl_lens(rle))
    # HLIT 257, HDIST 1 with length 0, and the smallest HCLEN that can spell a block: with 4 only the symbols 16, 17, 18 and 0 have codes, every length would be
    # 0 and there would be no end-of-block code; the fifth symbol of the order is 8, and 256 literal/length codes of 8 bits are a complete code
    lens8 = [0] + [8] * 256
    _dyn_member(img, "hclen5_hlit257_hdist1_zero", rng, lens8, [0], [("hclen", 5), ("hlit", 257), ("hdist", 1), ("dist_lens", (0,))],
                rle=[(l, 0) for l in lens8 + [0]], cl_lens=[1 if s in (0, 8) else 0 for s in range(19)])
    # HDIST 1 with one 1-bit code: the only incomplete code that zlib takes
    few = [0] * 286
    for s, l in zip((3, 77, 200, 256, 257, 270, 285), (2, 2, 3, 3, 3, 4, 4)):
        few[s] = l
    assert kraft(few) == 1 << 15
    _dyn_member(img, "hdist1_one_bit", rng, few, [1], [("hdist", 1), ("dist_lens", (1,)), ("has_match", 1)])
    # run-length tokens at the lane window's edges
    for kind, s, n, mode, e in b_rle_runs():
        l, d, rle = rle_layout(286, 2, [(kind, s, n, 9)], rng)
        _dyn_member(img, "rle%d_%s_%d" % (kind, mode, e), rng, l, d, [("rle_" + mode, kind, e)], rle=rle)
    for s in (64, 118):                # a run of 138 zeros from entry 64 (ends at 201) and one that ends at entry 255
        l, d, rle = rle_layout(286, 2, [(18, s, 138, 0)], rng)
        _dyn_member(img, "rle18_138_from_%d" % s, rng, l, d, [("rle_run", 18, 138), ("rle_begin", 18, s), ("rle_end", 18, s + 137)], rle=rle)
    for kind, n in ((16, 6), (17, 10), (18, 30)):
        hlit = 280
        # over the border between the two alphabets
        l, d, rle = rle_layout(hlit, 30, [(kind, hlit - 2 if kind != 18 else hlit - 15, n, 5)], rng)
        _dyn_member(img, "rle%d_crosses" % kind, rng, l, d, [("rle_cross", kind)], rle=rle)
        # up to the last entry, HLIT + HDIST
        l, d, rle = rle_layout(hlit, 30, [(kind, hlit + 30 - n, n, 5)], rng)
        _dyn_member(img, "rle%d_ends_at_total" % kind, rng, l, d, [("rle_ends_total", kind)], rle=rle)
    l, d, rle = rle_layout(286, 2, [(18, 70, 40, 0), (16, 110, 5, 0)], rng)                  # a 16 directly after an 18 repeats the zero
    _dyn_member(img, "rle16_after_18", rng, l, d, [("rle_16_after_18",)], rle=rle)
    # two dynamic blocks in one member, the second with a smaller alphabet and shorter codes: whatever the first left in the tables must be gone
    toks1, need = all_symbol_tokens(lit, dist, rng)
    small = [0] * 257
    for s, l in zip((9, 120, 255, 256), (2, 2, 2, 2)):
        small[s] = l
    toks2 = [9, 120, 255, 255, 9, 120] * 5
    prefix = rbytes(rng, _prefix_for(need))
    w = BitWriter()
    stored_block(w, prefix); dynamic_block(w, toks1, lit, dist); dynamic_block(w, toks2, small, [0], final=1)
    img.add("two_dynamic_second_smaller", w.getvalue(), expand(toks1 + toks2, prefix), [("blocks", (0, 2, 2)), ("second_smaller",)])
    small2 = small + [3]; small2[256] = 3         # 2, 2, 2, 3, 3: complete; one length symbol, two 1-bit distance codes
    toks3 = [9, 120, 255, (3, 1), (3, 2), 9]
    w = BitWriter()
    stored_block(w, prefix); dynamic_block(w, toks1, lit, dist); dynamic_block(w, toks3, small2, [1, 1], final=1)
    img.add("two_dynamic_second_smaller_with_matches", w.getvalue(), expand(toks1 + toks3, prefix), [("blocks", (0, 2, 2)), ("second_smaller",)])
    # fifty non-final blocks that hold only the end-of-block code, fixed and dynamic in turn
    two = [0] * 257; two[0] = two[256] = 1
    w = BitWriter()
    for k in range(50):
        if k % 2:
            dynamic_block(w, [], two, [0])
        else:
            fixed_block(w, [])
    tail = list(rbytes(rng, 40))
    fixed_block(w, tail, final=1)
    img.add("fifty_empty_blocks", w.getvalue(), bytes(tail), [("n_empty_blocks", 50)])
    # fixed -> empty stored -> dynamic -> stored -> fixed
    t1, t2, t3 = list(rbytes(rng, 300)) + [(40, 7)], [3, 77, 200, (3, 1), (24, 1), (258, 1), 3], [(258, 300), 1, 2, (9, 2)]
    s4 = rbytes(rng, 777)
    w = BitWriter()
    fixed_block(w, t1); stored_block(w, b""); dynamic_block(w, t2, few, [1]); stored_block(w, s4, pad=0x7f); fixed_block(w, t3, final=1)
    data = expand(t3, expand(t2, expand(t1)) + s4)
    img.add("fixed_stored0_dynamic_stored_fixed", w.getvalue(), data, [("blocks", (1, 0, 2, 0, 1))])
    # stored blocks whose header begins at each bit offset: a fixed block of k 9-bit literals is 3 + 9 k + 7 bits long
    for o in range(8):
        k = next(k for k in range(8) if (10 + 9 * k) % 8 == o)
        lits = list(rbytes(rng, k, 144, 256))
        body = rbytes(rng, 100 + o)
        w = BitWriter()
        fixed_block(w, lits); stored_block(w, body, pad=0xff if o % 2 else 0x55); fixed_block(w, [(20, 50)], final=1)
        img.add("stored_at_bit_%d" % o, w.getvalue(), expand([(20, 50)], bytes(lits) + body), [("stored_bit_offset", o)])
    return [img.case("B")]


# ---------------- C: input windows ----------------
def _c_stream(rng, k, j):
    """a final fixed block of j 8-bit and k 9-bit literals: 3 + 8 j + 9 k + 7 bits, so its last bit sits at position (9 + 9 k) % 8 of the last byte"""
    lits = list(rbytes(rng, j, 0, 144)) + list(rbytes(rng, k, 144, 256))
    w = BitWriter(); fixed_block(w, lits, final=1)
    return w.getvalue(int(rng.integers(0, 256))), bytes(lits)


def group_c():
    """the decoder reads its input through 256-byte windows (BitIn); lcd_bgzf_inflate_dev puts the image at the start of an allocation, so a stream's address modulo
    256 is its file offset modulo 256"""
    rng = np.random.default_rng(303)
    img = Image()
    two = [0] * 257; two[97] = two[256] = 1
    for r in range(256):               # every residue of the stream's first byte, the block kinds in turn
        w = BitWriter()
        if r % 3 == 0:
            toks = list(rbytes(rng, 5 + r % 7)) + [(4 + r % 50, 3)]
            fixed_block(w, toks, final=1); data = expand(toks)
        elif r % 3 == 1:
            toks = [97] * (1 + r % 40)
            dynamic_block(w, toks, two, [0], final=1); data = expand(toks)
        else:
            data = rbytes(rng, 1 + r % 9)
            stored_block(w, data, final=1)
        img.add_at("src_%d" % r, w.getvalue(), data, [("src_mod", r)], src_mod=r, bc_first=bool(r & 1))
    for r in range(256):               # every residue of the stream's end with the final bit at each position of the last byte
        for k in range(8):
            raw, data = _c_stream(rng, k, int(rng.integers(0, 4)))
            img.add_at("end_%d_bit_%d" % (r, (9 + 9 * k) % 8), raw, data, [("end_mod", r), ("final_bit", (9 + 9 * k) % 8)], end_mod=r, bc_first=bool(k & 1))
    for r in (252, 253, 254):          # LEN / NLEN over a window's edge: the stored header is the stream's first byte, LEN starts at 253, 254, 255
        for final_stored in (1, 0):
            data = rbytes(rng, 300)
            w = BitWriter()
            stored_block(w, data, final=final_stored)
            toks = [] if final_stored else [(30, 300), 5]
            if not final_stored:
                fixed_block(w, toks, final=1)
            img.add_at("len_field_at_%d_%s" % (r + 1, "final" if final_stored else "then_fixed"), w.getvalue(), expand(toks, data), [("len_field_mod", r + 1)], src_mod=r)
    for r in (252, 253, 254, 255, 0, 1, 2, 3):   # stored data that ends there, and the stream goes on: the reader restarts in that window
        for follow in ("fixed", "dynamic", "stored"):
            n = 40 + int(rng.integers(0, 300))
            data = rbytes(rng, n)
            w = BitWriter()
            stored_block(w, data)
            if follow == "fixed":
                toks = [(258, n), 1, 2, 3]; fixed_block(w, toks, final=1)
            elif follow == "dynamic":
                toks = [97] * 9; dynamic_block(w, toks, two, [0], final=1)
            else:
                toks = list(rbytes(rng, 7)); stored_block(w, bytes(toks), final=1)
            img.add_at("stored_ends_at_%d_then_%s" % (r, follow), w.getvalue(), expand(toks, data), [("stored_end_mod", r)], src_mod=(r - 5 - n) % 256)
    return [img.case("C")]


# ---------------- D: refusals ----------------
# lcd_io.cpp's why[] texts
T_DIST, T_SYMBOL, T_OVERSUB, T_LENGTHS, T_NO_EOB, T_TOO_MANY, T_TYPE, T_CODE, T_MORE, T_FEWER = (
    b"distance before the start of the block", b"invalid symbol", b"over-subscribed code", b"bad code lengths", b"no end-of-block code", b"too many codes",
    b"reserved block type", b"invalid code", b"more output than ISIZE", b"fewer bytes than ISIZE")


def _d_streams():
    """(name, raw stream, the ISIZE the member claims, the CRC's data, why[] text).  Every one is refused by zlib: by raw inflate, or (the last four) by the gzip
    trailer's length check"""
    rng = np.random.default_rng(404)
    out = []
    few = [0] * 286
    for s, l in zip((3, 77, 200, 256, 257, 270, 285), (2, 2, 3, 3, 3, 4, 4)):
        few[s] = l

    def fx(tokens, prefix=b"", claim=None):
        return prefixed_fixed(prefix, tokens), (len(expand([t for t in tokens if not isinstance(t, tuple)], prefix)) + 300 if claim is None else claim)

    out.append(("dist_first_symbol",) + fx([(3, 1), 1, 2]) + (b"", T_DIST))
    out.append(("dist_6_at_pos_5",) + fx([1, 2, 3, 4, 5, (4, 6), 9]) + (b"", T_DIST))
    p = rbytes(rng, 700)
    out.append(("dist_past_stored_prefix",) + fx([(10, 701)], p) + (b"", T_DIST))
    for sym in (286, 287):
        w = BitWriter(); w.bits(1, 1); w.bits(1, 2); w.code(FIXED_LIT_CODES[65]); w.code(FIXED_LIT_CODES[sym]); w.bits(0, 16); w.code(FIXED_LIT_CODES[256])
        out.append(("fixed_symbol_%d" % sym, w.getvalue(), 300, b"", T_SYMBOL))
    for sym in (30, 31):
        w = BitWriter(); w.bits(1, 1); w.bits(1, 2); w.code(FIXED_LIT_CODES[65]); w.code(FIXED_LIT_CODES[257]); w.code(FIXED_DIST_CODES[sym]); w.bits(0, 16)
        w.code(FIXED_LIT_CODES[256])
        out.append(("fixed_distance_symbol_%d" % sym, w.getvalue(), 300, b"", T_SYMBOL))
    toks = [3, 77, 200, (3, 1), (24, 1), (258, 1), 3]

    def dyn(name, why, lit=few, dist=(1,), tokens=toks, **kw):
        w = BitWriter(); dynamic_block(w, tokens, list(lit), list(dist), final=1, **kw)
        out.append((name, w.getvalue(), 300, b"", why))
    over = list(few); over[4] = 2                                     # five codes of 2 bits
    dyn("oversubscribed_litlen", T_OVERSUB, lit=over)
    dyn("oversubscribed_distance", T_OVERSUB, dist=(1, 1, 1))
    rle = rle_tokens(few + [1])
    cl = default_cl_lens(rle)
    bad_cl, spare = list(cl), [x for x in range(19) if not cl[x]][:2]
    for x in spare:
        bad_cl[x] = 1                                                 # a complete code and two more codes of 1 bit
    assert kraft(bad_cl) > 1 << 15
    dyn("oversubscribed_code_lengths", T_LENGTHS, rle=rle, cl_lens=bad_cl)
    lead = [(16, 0)] + rle_tokens(few[3:] + [1])                       # a repeat with nothing before it
    cl16 = default_cl_lens(lead)
    dyn("leading_repeat", T_LENGTHS, rle=lead, cl_lens=cl16)
    past = rle_tokens(few + [1])[:-1] + [(18, 100)]                    # the last token runs 110 entries past HLIT + HDIST
    dyn("run_past_the_lengths", T_LENGTHS, rle=past, cl_lens=default_cl_lens(past))
    no_eob = list(few); no_eob[256], no_eob[255] = 0, 3
    dyn("no_end_of_block_code", T_NO_EOB, lit=no_eob, tokens=[3, 77], eob=False)
    dyn("hlit_287", T_TOO_MANY, hlit=30)
    dyn("hlit_288", T_TOO_MANY, hlit=31)
    dyn("hdist_31", T_TOO_MANY, hdist=30)
    dyn("hdist_32", T_TOO_MANY, hdist=31)
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 29)
    out.append(("block_type_3", w.getvalue(), 300, b"", T_TYPE))
    # a lone 1-bit distance code is the pattern 0; a match that sends 1
    lit = canonical(few)
    w = BitWriter(); dynamic_block(w, [3, 77], few, [1], final=1, eob=False)
    w.code(lit[257]); w.bits(1, 1); w.code(lit[3]); w.code(lit[256])
    out.append(("unused_pattern_of_a_one_bit_distance_code", w.getvalue(), 300, b"", T_CODE))
    # the trailer's ISIZE is one byte off (the CRC is that of the bytes the stream really holds)
    lits = list(rbytes(rng, 200))
    raw, _ = fx(lits)
    out.append(("one_over_isize_by_a_literal", raw, 199, bytes(lits), T_MORE))
    t = lits + [(50, 30)]
    out.append(("one_over_isize_by_a_match", fx(t)[0], 249, expand(t), T_MORE))
    w = BitWriter(); fixed_block(w, lits); stored_block(w, bytes(lits), final=1)
    out.append(("one_over_isize_by_a_stored_block", w.getvalue(), 399, bytes(lits) * 2, T_MORE))
    out.append(("one_short_of_isize", raw, 201, bytes(lits), T_FEWER))
    return out


def group_d():
    """one image per refused stream: valid member, the refused one, valid member, EOF"""
    rng = np.random.default_rng(405)
    good1, good2 = list(rbytes(rng, 900)) + [(100, 900)], list(rbytes(rng, 50))
    cases = []
    for name, raw, isize, crc_data, why in _d_streams():
        img = Image()
        img.add("good_before", prefixed_fixed(b"", good1), expand(good1))
        img.add(name, raw, b"\0" * isize, [("why", why)], crc=zlib.crc32(crc_data), isize=isize)
        img.add("good_after", prefixed_fixed(b"", good2), expand(good2))
        cases.append(img.case(name, expected=False, refused=1))
    return cases


def group_lenient():
    """streams that zlib refuses and the kernel, on paper, accepts: incomplete codes whose missing patterns never occur, and bytes behind the final block inside
    BSIZE.  expected holds expand()'s bytes: a decoder that accepts them must give exactly those"""
    rng = np.random.default_rng(406)
    good = list(rbytes(rng, 500))
    cases = []

    def one(name, raw, data):
        img = Image()
        img.add("good_before", prefixed_fixed(b"", good), bytes(good))
        img.add(name, raw, data)
        img.add("good_after", prefixed_fixed(b"", good[:77]), bytes(good[:77]))
        cases.append(img.case(name))
    inc = [0] * 257
    for s in (65, 66, 256):
        inc[s] = 2                                                     # three codes of 2 bits: the pattern 11 is nobody's
    toks = [65, 66, 66, 65] * 10
    w = BitWriter(); dynamic_block(w, toks, inc, [0], final=1)
    one("incomplete_litlen", w.getvalue(), expand(toks))
    few = [0] * 286
    for s, l in zip((3, 77, 200, 256, 257, 270, 285), (2, 2, 3, 3, 3, 4, 4)):
        few[s] = l
    toks = [3, 77, 200, (3, 1), (24, 2), 3]
    w = BitWriter(); dynamic_block(w, toks, few, [2, 2], final=1)      # two distance codes of 2 bits
    one("incomplete_distance", w.getvalue(), expand(toks))
    rle = rle_tokens(few + [1])
    cl = [l + 1 if l else 0 for l in default_cl_lens(rle)]              # every code-length code one bit longer: half the patterns are nobody's
    if max(cl) <= 7:
        w = BitWriter(); dynamic_block(w, [3, 77, (3, 1)], few, [1], final=1, rle=rle, cl_lens=cl)
        one("incomplete_code_lengths", w.getvalue(), expand([3, 77, (3, 1)]))
    raw = prefixed_fixed(b"", good[:300])
    one("bytes_behind_the_final_block", raw + rbytes(rng, 37), bytes(good[:300]))
    return cases


# ---------------- E: container ----------------
def group_e():
    rng = np.random.default_rng(505)
    img = Image()
    toks = [0x41] + [(258, 1)] * 254 + [0x42, 0x43, 0x44]             # 1 + 254 * 258 + 3 = 65 536
    img.add("isize_65536_fixed", prefixed_fixed(b"", toks), expand(toks))
    img.add("empty_fixed", fixed_empty(), b"")
    seed = list(rbytes(rng, 1031))
    toks = seed + [(258, 1031)] * 250 + [(5, 4096)]                    # 1 031 + 250 * 258 + 5 = 65 536
    assert len(expand(toks)) == 65536
    img.add("isize_65536_period_1031", prefixed_fixed(b"", toks), expand(toks))
    w = BitWriter(); stored_block(w, b"", final=1)
    img.add("empty_stored", w.getvalue(), b"", extra_before=subfield(9))
    img.add("empty_fixed_again", fixed_empty(), b"")
    tail = rbytes(rng, 333)
    w = BitWriter(); stored_block(w, tail, final=1)
    img.add("after_the_empty_ones", w.getvalue(), tail)
    return [img.case("E")]


# ---------------- F: a file re-packed by this writer ----------------
def lz_tokens(data, max_dist=32768):
    """a plain greedy LZ77 pass (3-byte hash, last occurrence only): enough to give real data real matches"""
    toks, last, i, n = [], {}, 0, len(data)
    while i < n:
        key = data[i:i + 3]
        j = last.get(key) if len(key) == 3 else None
        if len(key) == 3:
            last[key] = i
        if j is not None and i - j <= max_dist:
            l = 3
            while l < 258 and i + l < n and data[j + l] == data[i + l]:
                l += 1
            toks.append((l, i - j)); i += l
        else:
            toks.append(data[i]); i += 1
    return toks


def dynamic_lens(tokens):
    """code lengths of at most 15 bits for these tokens (package-merge on their histogram) -> (literal/length lengths, distance lengths)"""
    hl, hd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            hl[len_symbol(t[0])[0]] += 1; hd[dist_symbol(t[1])[0]] += 1
        else:
            hl[t] += 1
    hl[256] += 1
    if sum(1 for x in hl if x) < 2:
        hl[0 if not hl[0] else 1] += 1
    lit, dist = package_merge(hl, 15), package_merge(hd, 15)
    hlit = max(257, max(s for s in range(286) if lit[s]) + 1)
    hdist = max([s + 1 for s in range(30) if dist[s]] or [1])
    return lit[:hlit], dist[:hdist]


F_SIZES = (1, 2, 3, 255, 1021, 4093, 16385, 30011, 50021, 60013)


def repack(data, seed=606):
    """the bytes of a BGZF file's inflated stream in members of this writer: odd sizes, the block kinds in turn, empty members in the middle, extra subfields
    -> (image with the EOF block, [(uncompressed offset, uncompressed length, file offset)] of the non-empty members)"""
    rng = np.random.default_rng(seed)
    img = Image()
    o, i = 0, 0
    while o < len(data):
        n = int(rng.choice(F_SIZES))
        chunk = data[o:o + n]
        kind = i % 4
        w = BitWriter()
        if kind == 0:
            stored_block(w, chunk, final=1)
        elif kind == 1:
            fixed_block(w, lz_tokens(chunk), final=1)
        elif kind == 2:
            toks = lz_tokens(chunk)
            lit, dist = dynamic_lens(toks)
            dynamic_block(w, toks, lit, dist, final=1)
        else:                                                         # two blocks in one member
            h = len(chunk) // 2
            toks = lz_tokens(chunk)
            a, acc = [], 0
            while toks and acc < h:
                t = toks.pop(0); a.append(t); acc += t[0] if isinstance(t, tuple) else 1
            lit, dist = dynamic_lens(a)
            dynamic_block(w, a, lit, dist)
            fixed_block(w, toks, final=1)
        img.add("m%d" % i, w.getvalue(), chunk, extra_before=subfield(4 + i % 5) if i % 3 == 0 else b"", extra_after=subfield(4 + i % 7) if i % 3 == 1 else b"")
        if i % 5 == 2:
            img.add("empty%d" % i, fixed_empty(), b"")
        o += len(chunk); i += 1
    return bytes(img.image) + EOF_BLOCK, [(m.uoff, m.ulen, m.off) for m in img.members if m.ulen]


def virtual_offset(blocks, u, end=False):
    """the BGZF virtual offset of uncompressed position u; a position at a member's end is the next member's start, except (end) at the end of the data"""
    for uoff, ulen, off in blocks:
        if uoff <= u < uoff + ulen:
            return (off << 16) | (u - uoff)
    uoff, ulen, off = blocks[-1]
    assert end and u == uoff + ulen
    return (off << 16) | ulen
