"""The case tables of tests/inflate_streams.py checked without a GPU: zlib's inflate is the judge of every stream (valid ones give exactly expand()'s bytes and reach
the end of the stream, the refusals raise), and what each table claims to cover is proved on the streams themselves -- with the bit-level reader of
tests/deflate_stream.py for token positions and code lengths, and with plain arithmetic on the file offsets for the input windows."""
import zlib

import pytest

import deflate_stream as ds
import inflate_streams as S


@pytest.fixture(scope="module")
def tables():
    return dict(A=S.group_a(), B=S.group_b(), C=S.group_c(), D=S.group_d(), L=S.group_lenient(), E=S.group_e())


def _zlib_raw(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    return out, d.eof, d.unused_data


def _valid(case):
    for m in case.members:
        out, eof, unused = _zlib_raw(m.raw)
        assert eof and unused == b"", (case.name, m.name)
        assert out == case.expected[m.uoff:m.uoff + m.ulen], (case.name, m.name)
        # the container: gzip's own reader takes the member, extra subfields included
        assert zlib.decompress(case.image[m.off:m.src + m.clen + 8], 31) == out, (case.name, m.name)


@pytest.mark.parametrize("group", ["A", "B", "C", "E"])
def test_zlib_accepts_every_valid_case_and_gives_expands_bytes(tables, group):
    for case in tables[group]:
        assert case.refused is None
        _valid(case)


def test_writer_and_reader_agree_bit_for_bit():
    """a stream of this writer read back by deflate_stream.decode: the same header fields, code lengths, run-length tokens and tokens"""
    import numpy as np
    rng = np.random.default_rng(1)
    lit, dist = S.shaped_lit_lens(rng), S.shaped_dist_lens(rng)
    toks, need = S.all_symbol_tokens(lit, dist, rng)
    prefix = S.rbytes(rng, 32768)
    rle = ds.rle_tokens(lit + dist)
    w = S.BitWriter()
    S.stored_block(w, prefix); S.dynamic_block(w, toks, lit, dist, rle=rle); S.fixed_block(w, toks[:50], final=1)
    d = ds.decode(w.getvalue())
    b0, b1, b2 = d["blocks"]
    assert (b0["btype"], b0["len"], b1["btype"], b2["btype"], b2["bfinal"]) == (0, 32768, 2, 1, 1)
    assert b1["lit_lens"] == lit and b1["dist_lens"] == dist and b1["rle"] == rle and (b1["hlit"], b1["hdist"]) == (286, 30)
    assert [t for _, _, t in b1["tokens"]] == toks and [t for _, _, t in b2["tokens"]] == toks[:50]
    assert d["data"] == S.expand(toks + toks[:50], prefix) and d["bits"] == w.bitpos()


def test_every_refusal_is_refused_by_zlib(tables):
    whys = set()
    for case in tables["D"]:
        assert case.refused == 1 and case.expected is None and [m.name for m in case.members][::2] == ["good_before", "good_after"]
        for k, m in enumerate(case.members):
            blob = case.image[m.off:m.src + m.clen + 8]
            if k != case.refused:
                zlib.decompress(blob, 31)
                continue
            with pytest.raises(zlib.error):                            # the gzip reader: the deflate stream itself, or the trailer's length check
                zlib.decompress(blob, 31)
            why = dict(m.claims)["why"]
            whys.add(why)
            if why not in (S.T_MORE, S.T_FEWER):
                with pytest.raises(zlib.error):
                    _zlib_raw(m.raw)
            else:                                                      # a good stream whose length is one byte off the trailer's ISIZE, in the right direction
                out, eof, _ = _zlib_raw(m.raw)
                assert eof and len(out) - m.ulen == (1 if why == S.T_MORE else -1)
    assert whys == {S.T_DIST, S.T_SYMBOL, S.T_OVERSUB, S.T_LENGTHS, S.T_NO_EOB, S.T_TOO_MANY, S.T_TYPE, S.T_CODE, S.T_MORE, S.T_FEWER}
    assert len(tables["D"]) == 23


def test_lenient_classes_are_what_they_say(tables):
    """zlib refuses the incomplete codes; the bytes they stand for are still well defined (no token uses a missing pattern): the reader below takes the codes as they
    are.  Bytes behind the final block: zlib stops at the end of the stream and leaves them unused"""
    names = [c.name for c in tables["L"]]
    assert names == ["incomplete_litlen", "incomplete_distance", "incomplete_code_lengths", "bytes_behind_the_final_block"]
    for case in tables["L"]:
        m = case.members[1]
        if case.name.startswith("incomplete"):
            with pytest.raises(zlib.error, match="set"):
                _zlib_raw(m.raw)
            with pytest.raises(ds.DeflateError, match="incomplete"):
                ds.decode(m.raw)
        else:
            out, eof, unused = _zlib_raw(m.raw)
            assert eof and len(unused) == 37 and out == case.expected[m.uoff:m.uoff + m.ulen]


# ---------------- the coverage claims ----------------
def _tokens_at(dec):
    """[(output position, length, distance)] of every match of a decoded stream"""
    out = []
    for b in dec["blocks"]:
        pos = b["data_start"]
        for _, _, t in b.get("tokens", ()):
            if isinstance(t, tuple):
                out.append((pos, t[0], t[1])); pos += t[0]
            else:
                pos += 1
    return out


def test_group_a_holds_the_whole_product_at_the_planned_positions(tables):
    case, = tables["A"]
    seen = set()
    for m in case.members:
        dec = ds.decode(m.raw)
        at = set(_tokens_at(dec))
        planned = dict(m.claims)["matches"]
        assert planned and set(planned) <= at, m.name
        seen |= {(d, l, pos % 1024) for pos, l, d in planned}
        if m.name.startswith("dist_eq_pos"):
            assert planned[0][0] == planned[0][2] and dec["blocks"][0]["btype"] == 0
    plan = set(S.a_plan())
    assert len(plan) == 35 * (14 * 5 + 12) and plan <= seen          # (lengths 257 and 258 have 1024 - length among the five fixed phases)
    assert all((32768, l, p) in seen for l in S.A_LENGTHS for p in S.a_phases(l))
    assert any(pos == 32768 and d == 32768 for mm in case.members for pos, l, d in dict(mm.claims)["matches"])
    assert max(mm.ulen for mm in case.members) <= 65536


def _rle_spans(b):
    """[(symbol, first entry, last entry)] of a dynamic block's run-length tokens"""
    out, k = [], 0
    for s, e in b["rle"]:
        n = 1 if s < 16 else e + (11 if s == 18 else 3)
        out.append((s, k, k + n - 1)); k += n
    return out


def _code_bits_in_use(b):
    """(literal/length code lengths, distance code lengths, symbols) that the block's tokens and its end-of-block code use"""
    lb, db, lsym, dsym = {b["eob_bits"]}, set(), {256}, set()
    for _, _, t in b["tokens"]:
        if isinstance(t, tuple):
            ls, d = ds.len_symbol(t[0])[0], ds.dist_symbol(t[1])[0]
            lb.add(b["lit_lens"][ls]); db.add(b["dist_lens"][d]); lsym.add(ls); dsym.add(d)
        else:
            lb.add(b["lit_lens"][t]); lsym.add(t)
    return lb, db, lsym, dsym


def _check_claim(dec, claim):
    kind, args = claim[0], claim[1:]
    blocks = dec["blocks"]
    dyn = [b for b in blocks if b["btype"] == 2]
    if kind in ("lit_bits", "dist_bits"):
        return any(args[0] in _code_bits_in_use(b)[0 if kind == "lit_bits" else 1] for b in dyn)
    if kind == "eob_bits":
        return any(b["eob_bits"] == args[0] for b in dyn)
    if kind == "first_last_longest":
        b = dyn[0]
        lens, used = (b["lit_lens"], _code_bits_in_use(b)[2]) if args[0] == "lit" else (b["dist_lens"], _code_bits_in_use(b)[3])
        longest = [s for s, l in enumerate(lens) if l == max(lens)]
        codes = S.canonical(lens)
        all_ones = codes[longest[-1]] == ((1 << 15) - 1, 15)         # (all ones reads the same in both bit orders)
        return max(lens) == 15 and len(longest) > 1 and longest[0] in used and longest[-1] in used and all_ones
    if kind in ("hlit", "hdist", "hclen"):
        return any(b[kind] == args[0] for b in dyn)
    if kind == "cl_bits":
        return any(b["cl_lens"][s] == args[0] for b in dyn for s, _ in b["rle"])
    if kind == "dist_lens":
        return any(tuple(b["dist_lens"]) == args[0] for b in dyn)
    if kind == "has_match":
        return any(isinstance(t, tuple) for b in dyn for _, _, t in b["tokens"])
    if kind in ("rle_begin", "rle_end"):
        return any(s == args[0] and (lo if kind == "rle_begin" else hi) == args[1] for b in dyn for s, lo, hi in _rle_spans(b))
    if kind == "rle_run":
        return any(s == args[0] and hi - lo + 1 == args[1] for b in dyn for s, lo, hi in _rle_spans(b))
    if kind == "rle_cross":
        return any(s == args[0] and lo < b["hlit"] <= hi for b in dyn for s, lo, hi in _rle_spans(b))
    if kind == "rle_ends_total":
        return any(_rle_spans(b)[-1][0] == args[0] and _rle_spans(b)[-1][2] == b["hlit"] + b["hdist"] - 1 for b in dyn)
    if kind == "rle_16_after_18":
        return any(a[0] == 18 and c[0] == 16 for b in dyn for a, c in zip(_rle_spans(b), _rle_spans(b)[1:]))
    if kind == "blocks":
        return tuple(b["btype"] for b in blocks) == args[0]
    if kind == "second_smaller":
        a, c = dyn
        return c["hlit"] < a["hlit"] and c["hdist"] < a["hdist"] and max(c["lit_lens"]) < min(l for l in a["lit_lens"] if l) and \
            sum(1 for l in c["lit_lens"] if l) < sum(1 for l in a["lit_lens"] if l) and len(c["tokens"]) > 0
    if kind == "n_empty_blocks":
        head = blocks[:args[0]]
        return all(not b["bfinal"] and b["btype"] in (1, 2) and not b["tokens"] for b in head) and {b["btype"] for b in head} == {1, 2} and len(blocks) == args[0] + 1
    if kind == "stored_bit_offset":
        return any(b["btype"] == 0 and b["bit_start"] % 8 == args[0] and b["bit_start"] > 0 for b in blocks)
    raise AssertionError(kind)


def test_group_b_streams_use_the_features_they_name(tables):
    case, = tables["B"]
    kinds = {}
    for m in case.members:
        dec = ds.decode(m.raw)
        assert m.claims, m.name
        for claim in m.claims:
            assert _check_claim(dec, claim), (m.name, claim)
            kinds.setdefault(claim[0], set()).add(claim[1:])
    assert {a[0] for a in kinds["lit_bits"]} == {10, 11, 15} and {a[0] for a in kinds["dist_bits"]} == {9, 10, 15}
    assert {a[0] for a in kinds["hlit"]} == {257, 286} and {a[0] for a in kinds["hdist"]} == {1, 30} and {a[0] for a in kinds["hclen"]} == {5, 19}
    assert kinds["dist_lens"] == {((0,),), ((1,),)} and kinds["first_last_longest"] == {("lit",), ("dist",)} and (7,) in kinds["cl_bits"]
    # run-length tokens: every kind begins at and ends at every entry of the list, except where a zero run would cover entry 256 (the end-of-block symbol)
    for kind in (16, 17, 18):
        for e in S.B_RLE_ENTRIES:
            n = S.B_RUN_COUNT[kind]
            for mode, first in (("rle_begin", e), ("rle_end", e - n + 1)):
                assert ((kind, e) in kinds[mode]) == (kind == 16 or not first <= 256 < first + n), (kind, e, mode)
        assert (kind,) in kinds["rle_cross"] and (kind,) in kinds["rle_ends_total"]
    assert (18, 138) in kinds["rle_run"] and () in kinds["rle_16_after_18"] and (50,) in kinds["n_empty_blocks"]
    assert ((1, 0, 2, 0, 1),) in kinds["blocks"] and {a[0] for a in kinds["stored_bit_offset"]} == set(range(8)) and () in kinds["second_smaller"]


def test_the_smallest_hclen_is_five():
    """HCLEN 4 gives codes to the symbols 16, 17, 18 and 0 only: every length is 0 or a repeat of 0, so there is no end-of-block code and zlib refuses the block"""
    lens = [0] * 258
    w = S.BitWriter()
    S.dynamic_block(w, [], lens[:257], [0], final=1, rle=[(18, 127), (17, 7), (18, 99)], cl_lens=[1 if s in (17, 18) else 0 for s in range(19)], hclen=4, eob=False)
    with pytest.raises(zlib.error, match="end-of-block"):
        _zlib_raw(w.getvalue() + b"\0\0")


def test_group_c_covers_every_residue_of_the_input_windows(tables):
    case, = tables["C"]
    claims = {}
    for m in case.members:
        for claim in m.claims:
            claims.setdefault(claim[0], []).append((m, claim[1]))
    # a stream's first byte and the byte behind its last one: every residue modulo 256 (the window size), the claim checked against the member's real offsets
    assert {m.src % 256 for m, r in claims["src_mod"] if m.src % 256 == r} == set(range(256))
    assert {case.image[m.off + 12] == 66 for m, _ in claims["src_mod"]} == {True, False}           # 'BC' first and not first
    ends = set()
    for m, r in claims["end_mod"]:
        assert (m.src + m.clen) % 256 == r
        bit = (ds.decode(m.raw)["bits"] - 1) % 8
        assert ("final_bit", bit) in m.claims and 8 * (m.clen - 1) < ds.decode(m.raw)["bits"] <= 8 * m.clen
        ends.add((r, bit))
    assert ends == {(r, b) for r in range(256) for b in range(8)}
    # LEN / NLEN: four bytes that begin at 253, 254, 255 lie across the edge
    got = set()
    for m, r in claims["len_field_mod"]:
        b = ds.decode(m.raw)["blocks"][0]
        assert b["btype"] == 0 and b["bit_start"] == 0 and (m.src + 1) % 256 == r
        got.add((r, b["bfinal"]))
    assert got == {(r, f) for r in (253, 254, 255) for f in (0, 1)}
    got = set()
    for m, r in claims["stored_end_mod"]:
        b0, b1 = ds.decode(m.raw)["blocks"]
        assert b0["btype"] == 0 and not b0["bfinal"] and (m.src + 5 + b0["len"]) % 256 == r
        got.add((r, b1["btype"]))
    assert got == {(r, t) for r in (252, 253, 254, 255, 0, 1, 2, 3) for t in (0, 1, 2)}
    assert max(m.src - m.off for m in case.members) > 18 + 200                                      # XLEN well above 6


def test_group_e_and_the_repacked_file(tables):
    case, = tables["E"]
    sizes = [m.ulen for m in case.members]
    assert sizes == [65536, 0, 65536, 0, 0, 333] and max(m.clen for m in case.members[:3]) < 2000   # ISIZE at its limit, highly compressible
    import numpy as np
    data = S.rbytes(np.random.default_rng(3), 30000, 0, 7) + bytes(range(256)) * 40 + S.rbytes(np.random.default_rng(4), 20000)
    image, blocks = S.repack(data)
    out, o, n_empty = b"", 0, 0
    while o < len(image):
        d = zlib.decompressobj(31)
        part = d.decompress(image[o:])
        assert d.eof
        n_empty += not part
        out += part; o = len(image) - len(d.unused_data)
    assert out == data and n_empty > 1
    assert [b[0] for b in blocks] == sorted(b[0] for b in blocks) and sum(b[1] for b in blocks) == len(data)
    assert S.virtual_offset(blocks, blocks[1][0]) == blocks[1][2] << 16 and S.virtual_offset(blocks, len(data), end=True) == (blocks[-1][2] << 16) | blocks[-1][1]
    assert S.expand(S.lz_tokens(data[:40000])) == data[:40000] and any(isinstance(t, tuple) for t in S.lz_tokens(data[:40000]))
