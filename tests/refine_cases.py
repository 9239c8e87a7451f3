"""The case table of the refined alignment output: hand-built records and digar lists, one named case per condition of rules R1-R5 and of the project rules
(include/lcd_hotpath.h, lcd_chunk_refine_records).  Every read is a truthful alignment on one seeded reference (bam_src_common.build_on_ref), so its digars, its
CIGAR spellings and its bases describe the same thing; `digars` says where a read's final digars come from:
  'ops'    one digar per operation of the case's list, handed over as a TOUCHED read (what a noisy region's rewrite leaves);
  'chunk'  the chunk's own digars (in HBM on the device; on the CPU the digar oracle of the record's source);
  a list   explicit rows.
The window of the rewrite is [REF_BEG, REF_END] (inclusive), narrower than the reads' span: the first and the last cases put events on its first / last base and
one past it.  `want` lists trace entries of refine_common.refine_record that the case must reach, `state` its outcome.
Used by tests/test_refine_oracle.py (CPU) and tests/test_gpu_refine_records.py."""
import numpy as np

import bam_src_common as bs
import refine_common as rc
from digar_inputs import BASES

TLEN = 120000
REF_BEG, REF_END = 1003, 40000
MIN_MAPQ = 30
FILTER_FLAGS = 0x4 | 0x100 | 0x800
_rng = np.random.default_rng(41)
REF = _rng.integers(0, 4, TLEN).astype(np.uint8)          # codes; REF[p - 1] = position p
WIN = REF[REF_BEG - 1:REF_END]                            # ref[0] = position REF_BEG


def letters():
    return bytes(BASES[b] for b in REF)


def ops_digars(pos0, ops):
    """one digar per operation: [pos (1-based), type, len, qi, 0]; a hard clip here stands for a palindromic soft clip: it counts bases"""
    out, p, q = [], pos0 + 1, 0
    for o, l, _ in ops:
        out.append([p, o, l, q, 0])
        if o in (7, 8):
            p += l; q += l
        elif o == 2:
            p += l
        elif o in (1, 4, 5):
            q += l
    return out


def alternating(n, first_eq=True, end="X", ev=(8, 1, 2)):
    """n operations, '=' runs of 1-3 bases alternating with events of length 1 cycling through `ev`; the last event is `end` (a CIGAR does not end in D / I here)"""
    ops, k = [], 0
    for i in range(n):
        if (i % 2 == 0) == first_eq:
            ops.append((7, 1 + i % 3, None))
        else:
            ops.append((ev[k % len(ev)], 1, None)); k += 1
    if ops[-1][0] != 7:
        ops[-1] = (8 if end == "X" else ops[-1][0], 1, None)
    return ops


def _wrong3(a, d):
    return [("NM", "i", 77), ("MD", "Z", b"5A5"), ("cs", "Z", b":5*ac:5")]


def _right3(a, d):
    return [("NM", "i", rc.digars_nm(d)), ("MD", "Z", rc.digars_md(d, WIN, REF_BEG, REF_END)), ("cs", "Z", rc.digars_cs(d, rc.read_codes(bs.record(a, a["eqx"], [])["body"]), WIN, REF_BEG, REF_END))]


def table():
    """[dict(name, ops, kind 'eqx' | 'm' | 'cg' | 'one_eq', fields(a, digars) -> list, digars, flag, mapq, hap, ps, want, state, pos (0-based, or None: next slot))]"""
    E = REF_END
    none = lambda a, d: []
    body = [(7, 30, None), (8, 1, None), (7, 25, None), (1, 2, None), (7, 20, None), (2, 3, None), (7, 30, None)]
    split63 = alternating(64, first_eq=False)[:63] + [(7, 2, None), (7, 3, None), (8, 1, None), (7, 4, None)]                      # digars 63 and 64 are both '='
    ins63 = alternating(63, ev=(8,)) + [(1, 2, None), (7, 3, None), (8, 1, None), (7, 4, None)]                                     # 62 '=', 63 I, 64 '=', 65 X
    assert split63[63][0] == split63[64][0] == 7 and ins63[62][0] == 7 and ins63[63][0] == 1 and ins63[64][0] == 7 and ins63[65][0] == 8
    c = [
        dict(name="window_first_base_D", pos=999, ops=[(7, 2, None), (2, 2, None), (7, 50, None)], kind="m", fields=_wrong3, want=["changed", "MD:replaced", "cs:replaced"]),
        dict(name="window_first_base_X", pos=1000, ops=[(7, 1, None), (8, 2, None), (7, 50, None)], kind="m", fields=_wrong3, want=["changed", "MD:replaced", "cs:replaced", "M_input"]),
        dict(name="identical_eqx_chunk_digars", ops=[(4, 5, None)] + body, kind="eqx", fields=lambda a, d: [("HP", "C", 1), ("NM", "i", 99)], digars="chunk", hap=2, ps=0,
             want=["identical", "HP:replaced:C"], state="identical"),
        dict(name="m_input_chunk_digars_no_tags", ops=body + [(4, 6, None)], kind="m", fields=none, digars="chunk", want=["changed", "M_input", "NM:absent", "MD:absent", "cs:absent"]),
        dict(name="hard_to_soft_both_ends", ops=[(5, 7, None)] + body + [(5, 9, None)], kind="m", fields=_wrong3, want=["changed", "hard_to_soft"]),
        dict(name="pos_moved_by_a_front_soft_clip", ops=[(7, 100, None)], kind="eqx", fields=_wrong3, digars="front_clip", want=["changed", "pos_moved"]),
        dict(name="pos_moved_identical_cigar", ops=[(7, 90, None)], kind="eqx", fields=none, digars="shifted", want=["identical", "pos_moved"], state="identical"),
        dict(name="digars_1", ops=[(7, 80, None)], kind="eqx", fields=_wrong3, want=["identical"], state="identical"),
        dict(name="digars_63", ops=alternating(63), kind="m", fields=_wrong3, want=["changed", "NM:replaced:i", "MD:replaced", "cs:replaced"]),
        dict(name="digars_64", ops=alternating(64), kind="m", fields=_wrong3, want=["changed"]),
        dict(name="digars_65", ops=alternating(65), kind="m", fields=_wrong3, want=["changed"]),
        dict(name="digars_130", ops=alternating(130), kind="m", fields=_wrong3, want=["changed"]),
        dict(name="eq_run_merged_across_64", ops=split63, kind="m", fields=_wrong3, want=["changed"]),
        dict(name="md_eq_len_over_insertion_and_64", ops=ins63, kind="m", fields=_wrong3, want=["changed"]),
        dict(name="decimal_widths", ops=[(7, 9, None), (8, 1, None), (7, 10, None), (8, 1, None), (7, 99, None), (2, 1, None), (7, 100, None), (8, 1, None), (7, 5, None)],
             kind="m", fields=_wrong3, want=["changed"]),
        dict(name="adjacent_eq_all_three_equal", ops=[(7, 12, None), (7, 8, None), (8, 1, None), (7, 10, None)], kind="m", fields=_right3, want=["changed", "NM:kept:i", "MD:kept", "cs:kept"]),
        dict(name="nm_typed_C", ops=body, kind="m", fields=lambda a, d: [("NM", "C", 200)], want=["changed", "NM:replaced:C", "MD:absent"]),
        dict(name="nm_typed_C_equal", ops=body, kind="m", fields=lambda a, d: [("NM", "C", rc.digars_nm(d))], want=["changed", "NM:kept:C"]),
        dict(name="md_typed_i_cs_typed_A", ops=[(7, 100, None)], kind="eqx", digars="front_clip", fields=lambda a, d: [("MD", "i", 5), ("cs", "A", b"x")],
             want=["changed", "MD:not_Z:i", "cs:not_Z:A"]),                # (an EQX record: with an 'M' CIGAR these tags would be the read's digar source)
        dict(name="second_md_field", ops=[(7, 100, None)], kind="eqx", digars="front_clip", fields=lambda a, d: [("MD", "Z", b"7"), ("XA", "A", b"q"), ("MD", "Z", b"second")], want=["changed", "MD:replaced"]),
        dict(name="tags_around_a_B_array", ops=[(7, 100, None)], kind="eqx", digars="front_clip", hap=1, ps=4000,
             fields=lambda a, d: [("HP", "C", 1), ("NM", "i", 500), ("XB", "B", ("I", [1, 2, 3])), ("cs", "Z", b":1"), ("PS", "i", 7), ("Xb", "B", ("c", [-1])), ("MD", "Z", b"1")],
             want=["changed", "NM:replaced:i", "cs:replaced", "MD:replaced", "HP:kept_in_place:C", "PS:replaced:i"]),
        dict(name="field_past_the_record", ops=body, kind="m", fields=lambda a, d: [("NM", "i", 500), (None, None, b"XBBi\xe8\x03\0\0\x01\0\0\0"), ("MD", "Z", b"1")],
             want=["changed", "NM:replaced:i", "MD:absent"]),
        dict(name="filtered_between_kept", ops=body, kind="eqx", flag=256, fields=lambda a, d: [("HP", "C", 1), ("NM", "i", 500), ("PS", "i", 7)], want=["filtered"], state="filtered"),
        dict(name="unrefined_no_digars_skipped_read", ops=body, kind="m", fields=lambda a, d: [("cs", "i", 5), ("HP", "C", 2)], digars="chunk", hap=1, want=["unrefined:no_digars"], state="no_digars"),
        dict(name="unrefined_no_digars_empty_list", ops=body, kind="eqx", fields=none, digars=[], want=["unrefined:no_digars"], state="no_digars"),
        dict(name="unrefined_qlen_hard_clipped_primary", ops=[(5, 7, None)] + body + [(5, 9, None)], kind="eqx", fields=_wrong3, digars="chunk", want=["unrefined:qlen_mismatch"],
             state="qlen_mismatch"),
        dict(name="unrefined_bad_pos", ops=[(7, 60, None)], kind="eqx", fields=_wrong3, digars=[[0, 7, 60, 0, 0]], want=["unrefined:bad_pos"], state="bad_pos"),
        dict(name="unrefined_cg_cigar", ops=body, kind="cg", fields=_wrong3, want=["unrefined:cg_cigar"], state="cg_cigar"),
        dict(name="window_last_base_X", pos=E - 12, ops=[(7, 10, None), (8, 3, None), (7, 30, None)], kind="m", fields=_wrong3, want=["changed", "MD:replaced"]),
        dict(name="window_last_base_D", pos=E - 11, ops=[(7, 9, None), (2, 3, None), (7, 30, None)], kind="m", fields=_wrong3, want=["changed", "MD:replaced"]),
        dict(name="unrefined_too_many_ops", pos=E + 1000, ops=[(7, 65536, None)], kind="one_eq", fields=none, digars="alternating_65536", want=["unrefined:too_many_ops"],
             state="too_many_ops"),
    ]
    return c


def build():
    """-> [case dicts with rec (bam_src_common.record), digars (rows | 'chunk'), hap, ps] in file order"""
    rng = np.random.default_rng(43)
    out, at = [], 1400
    for i, c in enumerate(table()):
        c = dict(c)
        pos = c.pop("pos", None)
        if pos is None:
            pos, at = at, at + 300
        ops = c["ops"]
        a = bs.build_on_ref(rng, REF, pos, [(4 if o == 5 else o, l, p) for o, l, p in ops])    # (the clipped bases exist: a hard-clip digar is a palindromic soft clip)
        if c["name"] == "unrefined_qlen_hard_clipped_primary":
            a = bs.build_on_ref(rng, REF, pos, ops)                                             # ... except for the true hard clip
        a["qual"] = np.full(a["qlen"], 35, np.uint8); a["flag"] = c.get("flag", 0); a["name"] = (b"c%d" % i) + b"x" * (i % 5)
        src = c.get("digars", "ops")
        if src == "ops":
            d = ops_digars(pos, ops)
        elif src == "front_clip":
            d = [[pos + 11, 4, 10, 0, 0], [pos + 11, 7, 90, 10, 0]]
        elif src == "shifted":
            d = [[pos + 3, 7, 90, 0, 0]]                                                        # (not a truthful alignment: R1 alone)
        elif src == "alternating_65536":
            d = [[pos + 1 + k // 2, 7 if k % 2 == 0 else 1, 1, k, 0] for k in range(65536)]
        else:
            d = src
        fields = c["fields"](a, d if not isinstance(d, str) else ops_digars(pos, ops))
        if c["kind"] == "cg":
            cig = [(a["qlen"] << 4) | 4, (a["rlen"] << 4) | 3]
            fields = fields + [("CG", "B", ("I", [int(w) for w in a["eqx"]]))]
            c["cg_words"] = a["eqx"]
        else:
            cig = a["eqx"] if c["kind"] in ("eqx", "one_eq") else a["mcig"]
        c.update(rec=bs.record(a, cig, fields, mapq=c.get("mapq", 60)), digars=d, hap=c.get("hap", i % 3), ps=c.get("ps", 4000 if i & 1 else 0), state=c.get("state", "changed"))
        out.append(c)
    assert all(x["rec"]["pos0"] < y["rec"]["pos0"] for x, y in zip(out[:-1], out[1:]))
    return out


def resolve(cases, orc):
    """the 'chunk' digars from the digar oracle of each record's source -> (digars per KEPT read, skipped per kept read, touched {read id: rows}, kept case indices)"""
    let = letters()
    digars_of, skipped, touched, kept = [], [], {}, []
    for i, c in enumerate(cases):
        if c["rec"]["flag"] & FILTER_FLAGS or c.get("mapq", 60) < MIN_MAPQ:
            continue
        r = len(kept); kept.append(i)
        # (a read the loader skips stays skipped, whatever a rewrite hands over; the loader reads a CG record's operations from its tag)
        _, _, e = bs.expected(orc, dict(c["rec"], cig=c["cg_words"]) if c["kind"] == "cg" else c["rec"], let, 1, TLEN, 1, TLEN, 0)
        skipped.append(e["rc"] != 0)
        if isinstance(c["digars"], str):
            digars_of.append(e["digars"].tolist() if e["rc"] == 0 else [])
        else:
            digars_of.append(c["digars"]); touched[r] = c["digars"]
    return digars_of, skipped, touched, kept

