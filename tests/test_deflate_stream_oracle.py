"""The reference of tests/deflate_stream.py checked on its own, without a GPU: decode() against zlib's raw streams of every payload class, level and strategy and
against hand-made streams that RFC 1951 forbids; package_merge() against brute force and against the unrestricted Huffman cost; and the preconditions of the
"limit binds" payloads of tests/test_gpu_deflate_stream.py -- on the plain byte histogram, which is what the kernel codes when its matcher takes nothing (the GPU
test repeats the check on the histogram it decodes)."""
import itertools
import zlib

import numpy as np
import pytest

import deflate_stream as ds


@pytest.fixture(scope="module")
def P():
    p = ds.existing_payloads()
    p.update(ds.limit_payloads())
    p.update(zero_run=ds.zero_run_payload(), longtok=ds.longtok_payload(), far4097=ds.far_payload(4097), len3=ds.len3_payload(4096)[0], empty=b"")
    return p


def _raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for o in range(0, len(data), flush_every):
        out += c.compress(data[o:o + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def _check(comp, data):
    r = ds.decode(comp)
    assert r["data"] == data
    assert (r["bits"] + 7) // 8 == len(comp)
    assert r["blocks"][-1]["bfinal"] == 1 and all(b["bfinal"] == 0 for b in r["blocks"][:-1])
    pos = 0
    for b in r["blocks"]:
        assert b["bit_start"] == pos
        pos = b["bit_end"]
        if b["btype"] == 0:
            assert b["len"] == b["data_end"] - b["data_start"]
            continue
        # the tokens tile the block's bits and bytes, and sizes() counts what the stream used
        at, n = b["tokens"][0][0] if b["tokens"] else b["bit_end"] - b["eob_bits"], 0
        for p, nb, t in b["tokens"]:
            assert p == at
            at += nb; n += t[0] if isinstance(t, tuple) else 1
        assert at + b["eob_bits"] == b["bit_end"] and n == b["data_end"] - b["data_start"]
        if b["btype"] == 1:
            assert ds.sizes(b["tokens"], n)["fixed"] == b["bit_end"] - b["bit_start"]
        else:
            assert ds.sizes(b["tokens"], n, b["lit_lens"], b["dist_lens"], b["cl_lens"], b["rle"], b["hclen"])["dynamic"] == b["bit_end"] - b["bit_start"]
            lens = b["lit_lens"] + b["dist_lens"]
            assert len(lens) == b["hlit"] + b["hdist"] and len(b["cl_lens"]) == 19
    return r


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_decode_reproduces_zlib_streams_of_every_level(P, level):
    for name, data in P.items():
        r = _check(_raw(data, level), data)
        if level == 0 and data:
            assert {b["btype"] for b in r["blocks"]} == {0}


@pytest.mark.parametrize("strategy", [zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE])
def test_decode_reproduces_zlib_streams_of_every_strategy(P, strategy):
    for name, data in P.items():
        r = _check(_raw(data, 6, strategy), data)
        if strategy == zlib.Z_FIXED:
            assert {b["btype"] for b in r["blocks"]} <= {0, 1}
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert not any(isinstance(t[2], tuple) for b in r["blocks"] if b["btype"] for t in b["tokens"])


def test_decode_reads_several_blocks_per_stream(P):
    for name in ("text", "bam", "random", "run"):
        r = _check(_raw(P[name], 6, flush_every=7000), P[name])
        assert len(r["blocks"]) >= len(P[name]) // 7000               # every full flush ends a block (and adds an empty stored one)
        assert any(b["btype"] == 0 and b["len"] == 0 for b in r["blocks"])


def test_a_full_size_block_decodes_in_about_a_second(P):
    import time
    comp = _raw(P["skew"] + P["skew"][:5280], 6, zlib.Z_HUFFMAN_ONLY)
    t = time.perf_counter()
    ds.decode(comp)
    dt = time.perf_counter() - t
    print("decode of 65 280 literals: %.2f s" % dt)
    assert dt < 5.0


# ---------------- hand-made streams ----------------
class Bits:
    def __init__(self):
        self.v = self.n = 0

    def put(self, value, nbits):                                      # LSB first: header fields and extra bits
        self.v |= value << self.n; self.n += nbits
        return self

    def code(self, code, nbits):                                      # a Huffman code: most significant bit first
        return self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _fixed_lit(b, s):
    if s < 144:
        return b.code(0x30 + s, 8)
    if s < 256:
        return b.code(0x190 + s - 144, 9)
    if s < 280:
        return b.code(s - 256, 7)
    return b.code(0xc0 + s - 280, 8)


def _dynamic_header(cl_lens, hlit=257, hdist=1):
    b = Bits().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in ds.CLORD:
        b.put(cl_lens[s], 3)
    return b


def test_decode_accepts_the_hand_made_good_streams():
    # the builders below are right: a fixed block "ab" + (3, 2) + end, and zlib agrees
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(_fixed_lit(b, 97), 98)
    _fixed_lit(b, 257).code(1, 5)                                     # length 3, distance 2
    _fixed_lit(b, 256)
    assert ds.decode(b.bytes())["data"] == b"ababa" == zlib.decompress(b.bytes(), -15)
    assert ds.decode(b.bytes())["blocks"][0]["tokens"][2] == (3 + 16, 12, (3, 2))


def test_decode_rejects_an_over_subscribed_code():
    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = 1                                         # three codes of one bit
    comp = _dynamic_header(cl).put(0, 64).bytes()
    with pytest.raises(ds.DeflateError, match="over-subscribed"):
        ds.decode(comp)
    with pytest.raises(zlib.error):
        zlib.decompress(comp, -15)


def test_decode_rejects_an_incomplete_literal_code():
    # code-length code: symbols 0, 1, 2 and 18 with lengths 1, 2, 3, 3 (complete): 0 -> "0", 1 -> "10", 2 -> "110", 18 -> "111".  Literal lengths: 'a' has one bit
    # and 256 has two: the Kraft sum is 3/4 (a LONE one-bit code is what zlib lets pass, for either alphabet; this is not it)
    cl = [0] * 19
    cl[0], cl[1], cl[2], cl[18] = 1, 2, 3, 3
    zeros = lambda b, n: b.code(7, 3).put(n - 11, 7)

    def stream(len_256):
        b = _dynamic_header(cl)
        zeros(b, 97).code(2, 2)                                       # zeros, then 'a': length 1
        zeros(zeros(b, 138), 256 - 98 - 138)                          # zeros up to 255
        b.code(2, 2) if len_256 == 1 else b.code(6, 3)                # 256
        b.code(2, 2)                                                  # the one distance code: length 1
        return b
    comp = stream(2).put(0, 32).bytes()
    with pytest.raises(ds.DeflateError, match="incomplete literal"):
        ds.decode(comp)
    with pytest.raises(zlib.error):
        zlib.decompress(comp, -15)
    # with both literal codes of one bit the header is accepted: its single distance code of one bit is the incomplete code that zlib accepts too
    b = stream(1).code(0, 1).code(0, 1).code(1, 1)                    # "aa", end
    assert ds.decode(b.bytes())["data"] == b"aa" == zlib.decompress(b.bytes(), -15)
    assert ds.decode(b.bytes())["blocks"][0]["dist_lens"] == [1]


def test_decode_rejects_distance_32769():
    # 32 768 is the last distance with a symbol (29, extra 8191); one more would need symbol 30, which the fixed code can spell and RFC 1951 forbids
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(b, 97)
    _fixed_lit(b, 257).code(30, 5).put(0, 13)
    comp = _fixed_lit(b, 256).bytes()
    with pytest.raises(ds.DeflateError, match="distance symbol above 29"):
        ds.decode(comp)
    with pytest.raises(zlib.error):
        zlib.decompress(comp, -15)
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(_fixed_lit(b, 97), 286)                                # and a length symbol above 285
    with pytest.raises(ds.DeflateError, match="length symbol above 285"):
        ds.decode(_fixed_lit(b, 256).bytes())


def test_decode_rejects_a_distance_before_the_start():
    b = Bits().put(1, 1).put(1, 2)
    _fixed_lit(_fixed_lit(b, 97), 98)
    _fixed_lit(b, 257).code(2, 5)                                     # distance 3 after two bytes
    comp = _fixed_lit(b, 256).bytes()
    with pytest.raises(ds.DeflateError, match="before the start"):
        ds.decode(comp)
    with pytest.raises(zlib.error):
        zlib.decompress(comp, -15)


def test_decode_rejects_a_stored_length_mismatch_and_a_cut_stream(P):
    good = _raw(b"hello", 0)
    assert ds.decode(good)["data"] == b"hello"
    bad = bytearray(good); bad[3] ^= 1
    with pytest.raises(ds.DeflateError, match="LEN / NLEN"):
        ds.decode(bytes(bad))
    comp = _raw(P["text"][:3000])
    for cut in (1, 2, len(comp) // 2, len(comp) - 1):
        with pytest.raises(ds.DeflateError, match="ends inside"):
            ds.decode(comp[:cut])


# ---------------- optimal codes ----------------
def _brute(freqs, limit):
    n, best = len(freqs), None
    for lens in itertools.product(range(1, limit + 1), repeat=n):
        if sum(1 << (limit - l) for l in lens) <= 1 << limit:
            c = sum(f * l for f, l in zip(freqs, lens))
            best = c if best is None or c < best else best
    return best


def test_package_merge_equals_brute_force():
    rng = np.random.default_rng(41)
    n_bound = 0
    for trial in range(120):
        limit = 3 + trial % 2
        n = int(rng.integers(2, 8))
        f = [int(x) for x in (rng.integers(1, 30, n) if trial % 3 else np.minimum(rng.geometric(0.15, n) ** 2, 500))]
        lens = ds.package_merge(f, limit)
        assert all(1 <= l <= limit for l in lens) and ds.kraft(lens, limit) <= 1 << limit
        assert ds.cost(f, lens) == _brute(f, limit), (f, limit, lens)
        n_bound += ds.cost(f, lens) > ds.huffman_cost(f)
    assert n_bound >= 10                                               # the limit did bind in a fair share of the trials


def test_package_merge_equals_huffman_when_the_limit_does_not_bind():
    rng = np.random.default_rng(42)
    for trial in range(40):
        n = int(rng.integers(1, 287))
        f = np.zeros(286, dtype=np.int64)
        f[rng.choice(286, n, replace=False)] = rng.integers(1, 1000, n) if trial % 2 else np.minimum(rng.geometric(0.01, n), 5000)
        f = f.tolist()
        depth = max(ds.mk_depths(sorted(x for x in f if x))) if n >= 2 else 1
        for limit in (15, 20, 32):
            if depth <= limit:
                lens = ds.package_merge(f, limit)
                assert ds.cost(f, lens) == ds.huffman_cost(f) and (n < 2 or ds.kraft(lens, limit) == 1 << limit)
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]    # depth 17
    assert ds.cost(fib, ds.package_merge(fib, 17)) == ds.huffman_cost(fib) < ds.cost(fib, ds.package_merge(fib, 15)) < ds.cost(fib, ds.package_merge(fib, 5))
    assert ds.package_merge([0, 7, 0], 15) == [0, 1, 0] and ds.package_merge([0, 0], 15) == [0, 0] and ds.huffman_cost([0, 7]) == 7


def test_the_named_construction_is_a_code_and_never_beats_the_optimum():
    # mk_lengths: complete, within the limit, monotone, at the Huffman cost when the limit does not bind, never below package-merge when it does
    rng = np.random.default_rng(43)
    for trial in range(40):
        n = int(rng.integers(2, 287))
        f = np.zeros(286, dtype=np.int64)
        f[rng.choice(286, n, replace=False)] = np.minimum(rng.geometric(0.002, n) ** (1 + trial % 3), 60000)
        f = f.tolist()
        for limit in (15, 9):
            info = {}
            lens = ds.mk_lengths(f, limit, info)
            assert max(lens) <= limit and ds.kraft(lens, limit) == 1 << limit and all((l > 0) == (x > 0) for l, x in zip(lens, f))
            opt = ds.cost(f, ds.package_merge(f, limit))
            assert ds.cost(f, lens) >= opt >= ds.huffman_cost(f)
            if info["depth"] <= limit:
                assert ds.cost(f, lens) == ds.huffman_cost(f) and info["steps"] == 0
    assert ds.mk_lengths([0, 0, 5, 0], 15) == [1, 0, 1, 0] and ds.mk_lengths([0] * 30, 15)[:3] == [1, 1, 0]


def test_rle_tokens_follow_the_greedy_rule():
    lens = [0] * 150 + [5] * 8 + [0, 0] + [3, 3, 3] + [0] * 4 + [7] * 4
    t = ds.rle_tokens(lens)
    assert t == [(18, 127), (18, 1), (5, 0), (16, 3), (5, 0), (0, 0), (0, 0), (3, 0), (3, 0), (3, 0), (17, 1), (7, 0), (16, 0)]


# ---------------- the payloads' preconditions ----------------
@pytest.mark.parametrize("name", ["skew", "tail", "singles", "singles_long", "clskew"])
def test_limit_payloads_make_the_limit_bind(P, name):
    data = P[name]
    assert len(data) <= 65280
    h = ds.byte_histogram(data)
    info = {}
    ds.mk_lengths(h, 15, info)
    pm = ds.package_merge(h, 15)
    print(name, "bytes", len(data), "depth", info["depth"], "clamped", info["clamped"], "repair steps", info["steps"],
          "package-merge / huffman %.6f" % (ds.cost(h, pm) / ds.huffman_cost(h)), "named construction / package-merge %.6f" % (ds.cost(h, ds.mk_lengths(h, 15)) / ds.cost(h, pm)))
    if name != "clskew":
        assert ds.cost(h, pm) > ds.huffman_cost(h)
    else:                                                              # its lengths are 3 ... 15 by construction: the alphabet that must overflow is the code-length one
        hlit = max(s for s in range(286) if pm[s]) + 1
        hc = ds.rle_histogram(ds.rle_tokens(pm[:hlit] + [1, 1]))
        ci = {}
        ds.mk_lengths(hc, 7, ci)
        print(name, "code-length histogram", hc, "depth", ci["depth"], "repair steps", ci["steps"])
        assert ds.cost(hc, ds.package_merge(hc, 7)) > ds.huffman_cost(hc)


def test_edge_payloads_are_what_they_say(P):
    for d in (4096, 4097, 32767, 32768, 32769):
        f = ds.far_payload(d)
        assert len(f) == d + 400 and f[:400] == f[d:] and max(f[400:d]) < 4
    for d in (4096, 4097):
        data, at = ds.len3_payload(d)
        assert len(at) == 40 and len(data) <= 65280
        for p in at:
            assert data[p:p + 3] == data[p - d:p - d + 3] and data[p + 3] != data[p - d + 3] and data[p - 1] != data[p - d - 1]
    z = np.bincount(np.frombuffer(P["zero_run"], dtype=np.uint8), minlength=256)
    assert (z[10:200] == 0).all() and (z[:10] > 0).all() and (z[200:] > 0).all()
    assert ds.pass_collision_free(b"abcabcabc" * 7) and not ds.pass_collision_free(b"abcabcabc" * 8) and ds.pass_collision_free(bytes(range(200)))
