"""What zlib cannot see of the streams deflate_kernel.hip writes: every member is DECODED by the plain reference of tests/deflate_stream.py, and the test asserts
what the kernel decided -- code lengths against the package-merge optimum, the stored / fixed / dynamic choice against the three forms' sizes, the matcher's
window edges and the run-length coding of the header on the decoded tokens, the bit packer's three-dword path on the tokens' bit positions -- and that a block
compressed on a later trip of its workgroup's grid-stride loop is the block it would have been alone.  tests/test_gpu_deflate.py keeps checking the container and
the round trip; its checker is reused here.  At most about a dozen full-size blocks are decoded per test; the decoded streams are shared."""
import pytest

import bam_out_common as bo
import deflate_stream as ds
from test_gpu_deflate import check_image, inflate_dev  # noqa: F401  (the device inflate fixture)

pytestmark = pytest.mark.gpu
GRID = 2048                                                            # lcd_bgzf_deflate_dev launches min(n_blocks, 2048) workgroups
LIMIT_NAMES = ("skew", "tail", "singles", "singles_long", "clskew")
EXISTING = ("text", "bam", "skew", "run", "one", "random", "far", "zeros_then_text")
NAMES = EXISTING + ("tail", "singles", "singles_long", "clskew", "zero_run", "longtok", "text4000")
MARGIN = 0.001                                                         # cost over the package-merge optimum that a limited code may have (0.1 %)


@pytest.fixture(scope="module")
def P():
    p = ds.existing_payloads()
    p.update(ds.limit_payloads())
    p.update(zero_run=ds.zero_run_payload(), longtok=ds.longtok_payload(), text4000=p["text"][:4000])
    return p


def decode_member(m):
    """one member of bam_out_common.bgzf_members -> its single deflate block, decoded; the bytes and the bit count are the member's"""
    r = ds.decode(m["comp"])
    assert r["data"] == m["payload"] and (r["bits"] + 7) // 8 == len(m["comp"]) and len(r["blocks"]) == 1
    b = r["blocks"][0]
    b["n"] = len(m["payload"])
    return b


@pytest.fixture(scope="module")
def streams(lcd, inflate_dev, P):
    """name -> the decoded block of that payload compressed as ONE member (checked once by test_gpu_deflate's checker, decoded once)"""
    cache = {}

    def get(name):
        if name not in cache:
            r = check_image(lcd, inflate_dev, P[name], 0)
            b = decode_member(bo.bgzf_members(r["image"])[0])
            assert b["btype"] == r["blocks"][0][2]
            cache[name] = b
        return cache[name]
    return get


def token_rules(b):
    """what holds for the tokens of every coded block: 3 <= length <= 258, 1 <= distance <= 32 768, no 3-byte match further back than TOO_FAR = 4 096"""
    for _, nb, t in b["tokens"]:
        if isinstance(t, tuple):
            assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768 and not (t[0] == 3 and t[1] > 4096), t
            assert nb <= 48


# ---------------- a. the grid stride ----------------
def _lone(lcd, data, bp):
    """every block of the image compressed on the FIRST trip of its workgroup: calls of at most GRID blocks, so that no workgroup has compressed anything before"""
    members, blocks = [], []
    for o in range(0, len(data), GRID * bp):
        r = lcd.bgzf_deflate(data[o:o + GRID * bp], bp, 0)
        assert len(r["blocks"]) <= GRID
        members += bo.bgzf_members(r["image"]); blocks += r["blocks"]
    return members, blocks


def _stale_pair():
    """two 17-byte blocks for the same workgroup, j and j + GRID.  The first leaves the bucket of b"ABC" pointing at position 0.  The second has b"ABCD" at 0 and at 8:
    alone it is one pass of literals (a pass never looks at its own positions), while a hash table that kept the first block's entry gives position 8 a match"""
    a, b = b"ABCDefghijklmnopq", b"ABCDwxyzABCDrstuv"
    h = ds.hash3(a).tolist()
    assert len(a) == len(b) == 17 and h.count(h[0]) == 1
    return a, b


def test_blocks_on_later_trips_of_the_grid_stride_loop(lcd, inflate_dev, P, streams):
    bp, n_blocks = 1501, 4200
    # derived from the existing classes: 187 random bytes nine times over have few literals and many matches, which the fixed code wins
    rep = lambda k: (P["random"][187 * k:187 * k + 187] * 9)[:bp]
    cyc = ("text", "bam", "rep", "skew", "run", "random", "far", "zeros_then_text", "rep")    # 9 classes: GRID % 9 = 5, a workgroup meets another class on every trip
    parts, cls = [], []
    for j in range(n_blocks - 1):
        c = cyc[j % len(cyc)]
        if c == "rep":
            parts.append(rep(j % 200))
        else:
            src = P[c]
            o = (j // len(cyc) * 1009) % (len(src) - bp)
            parts.append(src[o:o + bp])
        cls.append(c)
    parts.append(P["one"]); cls.append("one")                          # the last block: one byte
    data = b"".join(parts)
    r = check_image(lcd, inflate_dev, data, bp)                        # every member through zlib, the whole image through the device inflate with the CRC check
    members = bo.bgzf_members(r["image"])[:-1]
    kinds = [b[2] for b in r["blocks"]]
    assert len(kinds) == n_blocks > 2 * GRID
    assert {0, 1, 2} <= set(kinds[GRID:2 * GRID]) and {0, 1, 2} <= set(kinds[2 * GRID:])
    after_fixed = [j for j in range(n_blocks - GRID) if kinds[j] == 1 and kinds[j + GRID] == 2]
    assert after_fixed, "no workgroup writes a dynamic block on the trip after a fixed one"
    # A block's bytes and kind do not depend on what its workgroup compressed before.  The kernel lets a hash collision inside one pass keep either position, so
    # the stream of a block with such a collision is not pinned down by its bytes alone: kind and payload are compared for every block, the member's size and
    # bytes for the classes where no collision can change the tokens' cost (run, one, random) and for the blocks that cannot meet a collision at all
    lone_m, lone_b = _lone(lcd, data, bp)
    n_exact = 0
    for j in range(n_blocks):
        assert r["blocks"][j][0] == lone_b[j][0] and kinds[j] == lone_b[j][2], (j, cls[j], r["blocks"][j], lone_b[j])
        assert members[j]["payload"] == lone_m[j]["payload"] == parts[j]
        if cls[j] in ("run", "one", "random") or ds.pass_collision_free(parts[j]):
            assert r["blocks"][j][1] == lone_b[j][1] and members[j]["comp"] == lone_m[j]["comp"], (j, cls[j])
            n_exact += 1
    same = sum(a["comp"] == b["comp"] for a, b in zip(members, lone_m))
    print("grid stride, payload 1501: %d blocks, %d fixed-then-dynamic workgroups, %d compared byte for byte, %d of all members identical to the lone block's" %
          (n_blocks, len(after_fixed), n_exact, same))
    assert n_exact >= n_blocks // 5
    # a dozen blocks of the later trips, decoded: the dynamic one after a fixed one first
    for j in [after_fixed[0] + GRID, after_fixed[-1] + GRID] + list(range(2 * GRID, 2 * GRID + 9)) + [n_blocks - 1]:
        b = decode_member(members[j])
        assert b["btype"] == kinds[j]
        if b["btype"]:
            token_rules(b); code_rules(b); form_rules(b)


def test_tiny_blocks_on_later_trips_of_the_grid_stride_loop(lcd, inflate_dev, P):
    bp, n_blocks = 17, 5000
    cyc = ("text", "bam", "skew", "run", "random", "far", "zeros_then_text")          # 7 classes: GRID % 7 = 4
    parts = []
    for j in range(n_blocks):
        src = P[cyc[j % len(cyc)]]
        o = (j // len(cyc) * 1009) % (len(src) - bp)
        parts.append(src[o:o + bp])
    a, b = _stale_pair()
    for j in (5, GRID + 9):
        parts[j], parts[j + GRID] = a, b
    data = b"".join(parts)
    r = check_image(lcd, inflate_dev, data, bp)
    members = bo.bgzf_members(r["image"])[:-1]
    lone_m, lone_b = _lone(lcd, data, bp)
    # a payload of 17 bytes is one pass: its hash table is written after the pass and never read, so no collision can matter and every member is compared exactly
    assert all(ds.pass_collision_free(p) for p in parts[:50])
    for j in range(n_blocks):
        assert r["blocks"][j] == lone_b[j] and members[j]["comp"] == lone_m[j]["comp"], (j, r["blocks"][j], lone_b[j])
    assert {1} <= {k for _, _, k in r["blocks"][GRID:]}
    for j in (5 + GRID, 2 * GRID + 9):                                 # the block that a stale hash table would give a match
        d = decode_member(members[j])
        assert d["btype"] == 1 and [t for _, _, t in d["tokens"]] == list(b), d["tokens"]


# ---------------- b. the code lengths ----------------
def effective_histograms(b):
    """the histograms that the block's codes were built for: the decoded tokens', with the kernel's fill-in (an alphabet with fewer than two symbols in use gets
    frequency 1 on the first free symbols, so that every code is complete)"""
    hl, hd = ds.histograms(b["tokens"])
    assert not any(hl[b["hlit"]:]) and not any(hd[b["hdist"]:]), "a symbol in use beyond HLIT / HDIST"
    hl, hd = hl[:b["hlit"]], hd[:b["hdist"]]
    hc = ds.rle_histogram(b["rle"])
    for h, lens in ((hl, b["lit_lens"]), (hd, b["dist_lens"]), (hc, b["cl_lens"])):
        used = sum(1 for f in h if f)
        for s, l in enumerate(lens):
            if l and not h[s]:
                assert used < 2 and s < 3, "a code for a symbol that does not occur"
                h[s] = 1; used += 1
    return hl, hd, hc


def code_rules(b, figures=None):
    """one dynamic block: each of its three codes is complete, monotone in the frequencies, and optimal -- or, where the limit binds, within MARGIN of the
    package-merge optimum.  -> {alphabet: dict(bound, excess, depth)}"""
    if b["btype"] != 2:
        return {}
    out = {}
    for what, h, lens, limit in zip(("literal/length", "distance", "code-length"), effective_histograms(b), (b["lit_lens"], b["dist_lens"], b["cl_lens"]), (15, 15, 7)):
        assert all((l > 0) == (f > 0) for l, f in zip(lens, h)), what
        assert max(lens) <= limit and ds.kraft(lens, limit) == 1 << limit, (what, "Kraft sum", ds.kraft(lens, limit), 1 << limit)
        # f_a > f_b => len_a <= len_b: the longest length of every frequency class is no longer than the shortest of the next rarer one
        by_f = {}
        for f, l in zip(h, lens):
            if f:
                lo, hi = by_f.get(f, (99, 0))
                by_f[f] = (min(lo, l), max(hi, l))
        fs = sorted(by_f, reverse=True)
        for fa, fb in zip(fs, fs[1:]):
            assert by_f[fa][1] <= by_f[fb][0], (what, "not monotone", fa, by_f[fa], fb, by_f[fb])
        c, huff, opt = ds.cost(h, lens), ds.huffman_cost(h), ds.cost(h, ds.package_merge(h, limit))
        info = {}
        ds.mk_lengths(h, limit, info)
        if opt == huff:
            assert c == huff, (what, "cost", c, "optimum", huff)
        else:
            assert max(lens) == limit, what
            assert opt <= c <= opt * (1 + MARGIN), (what, "cost", c, "package-merge", opt, "excess %.6f %%" % (100.0 * (c - opt) / opt))
        out[what] = dict(bound=opt > huff, excess=100.0 * (c - opt) / opt, depth=info["depth"], steps=info["steps"], clamped=info["clamped"])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_dynamic_codes_are_optimal_or_correctly_limited(streams, name):
    b = streams(name)
    fig = code_rules(b)
    for what, f in fig.items():
        print("%s %s: limit %s, depth before limiting %d, clamped %d, repair steps %d, excess over package-merge %.5f %%" %
              (name, what, "binds" if f["bound"] else "does not bind", f["depth"], f["clamped"], f["steps"], f["excess"]))   # (depth, clamped, steps: the reference
                                                                                                                          # construction on the decoded histogram)
    if name in LIMIT_NAMES:
        # the payload is here to reach the limiter: a matcher that moves it off that edge fails this test instead of passing on nothing
        assert b["btype"] == 2
        assert fig["code-length" if name == "clskew" else "literal/length"]["bound"], "the limit does not bind"
    if name == "singles_long":
        # the repair loop's long case: every once-only symbol is beyond the limit, and the loop runs several times as often as for any other payload here
        assert fig["literal/length"]["clamped"] > 60 and fig["literal/length"]["steps"] >= 30
    if name in ("text", "bam", "far", "zeros_then_text", "zero_run", "longtok", "text4000") + LIMIT_NAMES:
        assert b["btype"] == 2
    if name == "run":
        assert b["btype"] and not any(not isinstance(t, tuple) and t != 7 for _, _, t in b["tokens"])


# ---------------- c. the form ----------------
def form_rules(b):
    """one decoded block: sizes() of its tokens reproduces the bits it used, its form is the cheaper of fixed and dynamic (dynamic only when strictly smaller) and
    smaller than the stored form.  The dynamic size of a block written with the fixed code is that of the construction the kernel's header describes"""
    n, used = b["n"], b["bit_end"] - b["bit_start"]
    if b["btype"] == 0:
        assert b["len"] == n and used == 8 * (n + 5)
        return
    if b["btype"] == 2:
        s = ds.sizes(b["tokens"], n, b["lit_lens"], b["dist_lens"], b["cl_lens"], b["rle"], b["hclen"])
        assert s["dynamic"] == used and s["dynamic"] < s["fixed"], s
        assert b["hlit"] == max(257, max(i for i, l in enumerate(b["lit_lens"]) if l) + 1) and b["hdist"] == max(i for i, l in enumerate(b["dist_lens"]) if l) + 1
        assert b["hclen"] == max(4, max(i + 1 for i in range(19) if b["cl_lens"][ds.CLORD[i]]))
    else:
        s = ds.sizes(b["tokens"], n, **ds.dynamic_form(b["tokens"]))
        assert s["fixed"] == used and s["fixed"] <= s["dynamic"], s
    assert (used + 7) // 8 < n + 5


@pytest.mark.parametrize("name", NAMES)
def test_the_form_written_is_the_cheapest(streams, name):
    b = streams(name)
    form_rules(b)
    token_rules(b) if b["btype"] else None
    if name == "random":
        assert b["btype"] == 0                                         # (LEN / NLEN and the bytes were checked by decode)


def test_small_blocks_take_the_fixed_code_and_larger_ones_the_dynamic(lcd, inflate_dev, P):
    kinds = {}
    # 1, 17, 64, 200 and 4 000, and the sizes between 17 and 64 where the two forms cross: a hundred small blocks each, so that some lie within a few bits of the
    # crossing, where a size that is counted wrongly picks the wrong form
    for bp in (1, 17, 24, 32, 40, 48, 64, 200, 4000):
        data = P["text"][:100 * bp] if bp <= 64 else P["text"][:min(12 * bp, 24000)]
        r = check_image(lcd, inflate_dev, data, bp)
        members = bo.bgzf_members(r["image"])[:-1]
        for j in range(len(members) if bp <= 64 else min(12, len(members))):
            b = decode_member(members[j])
            assert b["btype"] == r["blocks"][j][2]
            form_rules(b); code_rules(b)
            token_rules(b) if b["btype"] else None
            kinds.setdefault(bp, set()).add(b["btype"])
            if b["btype"] == 2:
                rle_rules(b)
            if bp == 1:                                                # 3 + 8 or 9 + 7 bits against 6 bytes
                assert b["btype"] == 1 and b["bit_end"] in (18, 19)
        assert all(k == 1 for _, _, k in r["blocks"]) or bp > 1
    print("kinds by block payload:", kinds)
    assert 1 in set.union(*kinds.values()) and 2 in set.union(*kinds.values()) and kinds[4000] == {2}


# ---------------- d. the window's edges ----------------
@pytest.mark.parametrize("dist", [4096, 4097, 32767, 32768, 32769])
def test_a_match_at_the_far_end_of_the_window(lcd, inflate_dev, dist):
    data = ds.far_payload(dist)
    r = check_image(lcd, inflate_dev, data, 0)
    b = decode_member(bo.bgzf_members(r["image"])[0])
    assert b["btype"] == 2
    token_rules(b); form_rules(b); code_rules(b)
    covered, at = 0, 0
    for _, _, t in b["tokens"]:
        if isinstance(t, tuple):
            if t[1] == dist and at >= dist:
                covered += t[0]
            at += t[0]
        else:
            at += 1
    print("far match at distance %d: %d of 400 bytes covered by tokens of that distance" % (dist, covered))
    if dist <= 32768:
        assert covered >= 300
    else:
        assert covered == 0 and max(t[1] for _, _, t in b["tokens"] if isinstance(t, tuple)) <= 32768


def test_three_byte_matches_up_to_too_far_and_no_further(lcd, inflate_dev):
    for dist in (4096, 4097):
        data, at = ds.len3_payload(dist)
        r = check_image(lcd, inflate_dev, data, 0)
        b = decode_member(bo.bgzf_members(r["image"])[0])
        # (the payload is random bytes: it is stored unless the planted repeats pay for a code, so the tokens may not exist)
        assert b["btype"] != 0, "the planted payload was stored: its tokens cannot be seen"
        token_rules(b)                                                 # no (3, d > 4 096) among them
        hits, p = 0, 0
        for _, _, t in b["tokens"]:
            if isinstance(t, tuple):
                hits += t == (3, dist) and p in at
                p += t[0]
            else:
                p += 1
        print("three-byte repeats at distance %d: %d of %d planted ones are tokens" % (dist, hits, len(at)))
        assert (hits >= 1) if dist == 4096 else (hits == 0)


@pytest.mark.parametrize("n", [257, 258, 259, 260, 261, 65280])
def test_run_tokens_end_with_the_payload(lcd, inflate_dev, P, n):
    r = check_image(lcd, inflate_dev, P["run"][:n], 0)
    b = decode_member(bo.bgzf_members(r["image"])[0])
    assert b["btype"] != 0
    token_rules(b); form_rules(b); code_rules(b)
    ms = [t for _, _, t in b["tokens"] if isinstance(t, tuple)]
    # the first pass has nothing behind it: 64 literals; then matches only, the last one ending with the payload (decode_member compared the bytes: the lengths add
    # up to n).  A match reaches back to a position of the pass before it -- any of its 64, all in one bucket -- so its distance is at most its own pass's advance
    assert sum(1 for _, _, t in b["tokens"] if not isinstance(t, tuple)) == 64 and isinstance(b["tokens"][-1][2], tuple)
    assert 64 + sum(l for l, _ in ms) == n and all(1 <= d <= 258 for _, d in ms)
    assert [l for l, _ in ms] == [258] * ((n - 64) // 258) + ([(n - 64) % 258] if (n - 64) % 258 else [])
    print("run of %d: matches %s" % (n, sorted(set(ms))))


# ---------------- e. the run-length coding of the code lengths ----------------
def rle_rules(b):
    lens, rle = b["lit_lens"] + b["dist_lens"], b["rle"]
    seq = []
    for i, (s, e) in enumerate(rle):
        if s == 18:
            assert 0 <= e <= 127                                       # a run of 11 ... 138
            seq += [0] * (11 + e)
        elif s == 17:
            assert 0 <= e <= 7
            seq += [0] * (3 + e)
        elif s == 16:
            assert 0 <= e <= 3 and seq and seq[-1] != 0 and rle[i - 1][0] in (16, seq[-1])     # repeats the length in front of it, never a zero
            seq += [seq[-1]] * (3 + e)
        else:
            seq.append(s)
    assert seq == lens
    plain = [s if s < 16 else -1 for s, _ in rle]
    for i in range(len(plain)):
        assert plain[i:i + 3] != [0, 0, 0], "three plain zeros in a row"
        assert not (plain[i] > 0 and plain[i:i + 4] == [plain[i]] * 4), "four equal plain lengths in a row"
    assert rle == ds.rle_tokens(lens)                                  # the greedy rule, token for token


@pytest.mark.parametrize("name", NAMES)
def test_code_lengths_are_run_length_coded_by_the_greedy_rule(streams, name):
    b = streams(name)
    if b["btype"] == 2:
        rle_rules(b)
    else:
        assert name in ("one", "random", "run")
    if name == "zero_run":
        # literal symbols 10 ... 199 are unused: 190 zeros, one symbol 18 covers 138 of them and a second one the rest
        assert b["btype"] == 2 and b["lit_lens"][10:200] == [0] * 190 and b["lit_lens"][9] and b["lit_lens"][200]
        i = b["rle"].index((18, 127))
        assert b["rle"][i + 1] == (18, 190 - 138 - 11), b["rle"][i:i + 3]


# ---------------- f. the bit packer's third dword ----------------
def test_long_tokens_reach_the_third_dword(streams):
    b = streams("longtok")                                             # (round trip: the fixture's check_image)
    assert b["btype"] == 2
    longest = max(nb for _, nb, _ in b["tokens"])
    third = [(p, nb, t) for p, nb, t in b["tokens"] if (p & 31) + nb > 64]
    print("longtok: longest token %d bits, %d tokens of 40 bits or more, %d tokens whose bits reach a third dword" %
          (longest, sum(nb >= 40 for _, nb, _ in b["tokens"]), len(third)))
    assert longest >= 40
    assert third, "no token of this stream crosses two dword boundaries"
