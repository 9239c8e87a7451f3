"""S6 test inputs (vars_kernel.hip vs oracle/cand_vars.c): hand-built noisy regions with planted variants, in the dict layout of jobs.make_region, and the
conditions each of them is meant to reach.  A condition is a predicate over what the oracle returns for the case (collect_noisy_reg_aln_strs and
make_vars_from_msa_cons_aln) and over the compacted ref<->cons columns recomputed here from the strings.  tests/test_vars_cases_oracle.py proves on the
CPU that every case reaches the conditions it names and that every condition is reached; tests/test_gpu_vars.py runs the same cases through the kernels.

Reads are error-free copies of their haplotype unless a case says otherwise, so a cluster's consensus is the planted haplotype; reads carry a haplotype
tag and a common phase set (the K1 branch, one cluster per tag) except in the untagged cases, which go through K2.  Pure numpy: no GPU, no reference."""
import functools

import numpy as np

BOTH, LEFT, RIGHT = 12, 8, 4
SNP, INS, DEL = 8, 1, 2        # var_type: BAM_CDIFF, BAM_CINS, BAM_CDEL
GAP = 5
A, C, G, T = 0, 1, 2, 3


def seq(s):
    return np.array(["ACGT".index(c) for c in s], np.uint8)


def plain_ref(seed, n):
    """n random bases in which no two neighbours are equal: no homopolymer, so a planted gap between distinct flanks has one placement"""
    rng = np.random.default_rng(seed)
    out = [int(rng.integers(0, 4))]
    while len(out) < n:
        out.append(int((out[-1] + 1 + rng.integers(0, 3)) % 4))
    return np.array(out, np.uint8)


def edit(ref, edits):
    """a haplotype: ref with edits applied.  ("X", p, base) substitutes ref[p]; ("I", p, bases) inserts in front of ref[p] (p == len(ref): at the end);
    ("D", p, n) deletes ref[p:p + n].  Edits must not overlap; an insertion at p goes in front of a substitution or deletion at p."""
    out, last = [], 0
    for kind, p, x in sorted(edits, key=lambda e: (e[1], e[0] != "I")):
        assert p >= last, (kind, p)
        out.append(ref[last:p]); last = p
        if kind == "X":
            assert int(x) != int(ref[p])
            out.append(np.array([x], np.uint8)); last = p + 1
        elif kind == "I":
            out.append(np.asarray(x, np.uint8))
        else:
            last = p + int(x)
    out.append(ref[last:])
    return np.concatenate(out).astype(np.uint8)


def region(ref, reads, tagged=True, ps=4242):
    """reads: (hap 1 | 2, bases, cover).  tagged: every read carries its haplotype and the phase set; otherwise none does (K2 decides)"""
    n = len(reads)
    return dict(reg_len=len(ref), read_ids=np.arange(n, dtype=np.int32) + 100, seqs=[np.asarray(s, np.uint8) for _, s, _ in reads],
                quals=[np.full(len(s), 30, np.uint8) for _, s, _ in reads], covers=np.array([c for _, _, c in reads], np.int32),
                haps=np.array([h if tagged else 0 for h, _, _ in reads], np.int32), phase_sets=np.array([ps if tagged else -1] * n, np.int64), ref=ref)


def full_reads(h1, h2, n1, n2):
    return [(1, h1, BOTH)] * n1 + [(2, h2, BOTH)] * n2


# ---------------------------------------------------------------- what a case's oracle output shows ----------------------------------------------------------------
def columns(rc):
    """the ref<->cons string without its gap/gap columns (src/collect_var.c:1863-1868) -> R, C"""
    keep = (rc["target"] != GAP) | (rc["query"] != GAP)
    return rc["target"][keep], rc["query"][keep]


def col_class(R, Cc):
    return np.where(R == Cc, 0, np.where(R == GAP, 2, np.where(Cc == GAP, 3, 1)))     # 0 equal, 1 mismatch, 2 insertion column, 3 deletion column


def runs(R, Cc):
    """every mismatch column and every maximal insertion / deletion run: dict(col, end, cls, ref_off, is_var)"""
    cls = col_class(R, Cc)
    L = len(cls)
    ref_off = np.concatenate([[0], np.cumsum(R != GAP)])
    out, i = [], 0
    while i < L:
        if cls[i] == 0:
            i += 1
        elif cls[i] == 1:
            out.append(dict(col=i, end=i, cls=1, ref_off=int(ref_off[i]), is_var=i + 1 == L or cls[i + 1] < 2)); i += 1
        else:
            j = i
            while j + 1 < L and cls[j + 1] == cls[i]:
                j += 1
            out.append(dict(col=i, end=j, cls=int(cls[i]), ref_off=int(ref_off[i]), is_var=True)); i = j + 1
    return out


def window(s):
    return max(s["query_beg"], s["target_beg"]), min(s["query_end"], s["target_end"])


def count_eq(s, tp, n):
    """is_match_aln_str's n_eq (src/collect_var.c:1960-1985) of a cons<->read string for the consensus bases [tp, tp + n)"""
    lo, hi = window(s)
    cur, n_eq = -1, 0
    for i in range(s["aln_len"]):
        cur += s["target"][i] != GAP
        if cur == tp + n:
            break
        if i < lo:
            continue
        if i > hi:
            break
        if cur >= tp:
            n_eq += int(s["query"][i] == s["target"][i])
    return n_eq


def cons_span_of_ref(rc, beg_ref, end_ref):
    """get_full_cover_from_ref_cons_aln_str's (beg_in_cons, end_in_cons), src/collect_var.c:2107-2126"""
    cr = cc = -1
    bc = ec = -1
    reach = False
    for i in range(rc["aln_len"]):
        cr += rc["target"][i] != GAP; cc += rc["query"][i] != GAP
        if cr == beg_ref and bc == -1:
            bc = cc
        reach |= cr == end_ref
        if reach and rc["query"][i] != GAP:
            ec = cc
            break
    return bc, ec


def last_cons_pos(s):
    """consensus base index under the last column of a cons<->read string's window"""
    lo, hi = window(s)
    return int((s["target"][:hi + 1] != GAP).sum()) - 1


def first_cons_pos(s):
    lo, hi = window(s)
    return int((s["target"][:lo + 1] != GAP).sum()) - 1


class Seen:
    """one case through the oracle: res, exp, the column runs per consensus and the (row, variant) cells"""
    def __init__(self, case, res, exp):
        self.case, self.res, self.exp = case, res, exp
        self.n_cons, self.n = res["n_cons"], exp["n_vars"]
        self.beg = case["beg"]
        self.cols = [columns(res["aln_strs"][c][0]) for c in range(self.n_cons)]
        self.runs = [runs(*rc) for rc in self.cols]
        self.starts = [[r for r in rr if r["is_var"]] for rr in self.runs]
        self.v = [dict(i=i, off=int(exp["pos"][i] - self.beg), type=int(exp["var_type"][i]), ref_len=int(exp["ref_len"][i]), alt_len=int(exp["alt_len"][i]),
                       cate=int(exp["cate"][i]), src=int(exp["from_cons"][i]), hp=int(exp["is_homopolymer_indel"][i]), arb=int(exp["alt_ref_base"][i]),
                       alt=exp["alt_seqs"][i].tolist()) for i in range(self.n)]
        self.cells = []
        row = 0
        for c in range(self.n_cons):
            for j in range(res["clu_n_seqs"][c]):
                s = res["aln_strs"][c][2 * j + 1]
                delta = 0
                for v in self.v:
                    mine = self.n_cons == 1 or (v["src"] & (c + 1)) != 0
                    lo, hi = window(s)
                    self.cells.append(dict(row=row, clu=c, s=s, v=v, mine=mine, tp=v["off"] - delta, al=int(exp["prof_alleles"][row, v["i"]]),
                                           partial=lo > 0 or hi < s["aln_len"] - 1, rid=int(res["clu_read_ids"][c][j])))
                    if mine:
                        delta += -v["alt_len"] if v["type"] == INS else (v["ref_len"] if v["type"] == DEL else 0)
                row += 1

    def start_at(self, col, shifted=True):
        """a variant starts at compacted column col of some consensus (with ref_off != col: an insertion lies in front of it)"""
        return any(r["col"] == col and (not shifted or r["ref_off"] != col) for st in self.starts for r in st)

    def run_over(self, cls, lo, hi):
        return any(r["cls"] == cls and r["col"] <= lo and r["end"] >= hi for rr in self.runs for r in rr)

    def var(self, **kw):
        return [v for v in self.v if all(v[k] == x for k, x in kw.items())]

    def ins_cell(self, n_eq, n, al):
        return any(x["mine"] and x["v"]["type"] == INS and x["v"]["alt_len"] == n and x["al"] == al and count_eq(x["s"], x["tp"], n) == n_eq for x in self.cells)


def _followed(seen, nxt):
    """a mismatch column directly followed by an insertion (2) / deletion (3) column, and no SNP recorded at its position"""
    for c in range(seen.n_cons):
        cls = col_class(*seen.cols[c])
        for r in seen.runs[c]:
            if r["cls"] == 1 and not r["is_var"] and cls[r["col"] + 1] == nxt:
                if not [v for v in seen.var(type=SNP, off=r["ref_off"]) if v["src"] & (c + 1)]:
                    return True
    return False


def _adjacent(seen, first, second):
    for rr in seen.runs:
        for a, b in zip(rr, rr[1:]):
            if a["cls"] == first and b["cls"] == second and b["col"] == a["end"] + 1:
                return True
    return False


def _pair(seen, first_src):
    """two consecutive merged variants, same site / type / lengths, different alt bases, from haplotype first_src and then from the other"""
    for a, b in zip(seen.v, seen.v[1:]):
        if (a["off"], a["type"], a["ref_len"], a["alt_len"]) == (b["off"], b["type"], b["ref_len"], b["alt_len"]) and a["alt"] != b["alt"]:
            if (a["src"], b["src"]) == (first_src, 3 - first_src):
                return True
    return False


def _site(v):
    return v["off"] if v["type"] == SNP else v["off"] - 1


def _partial_in_ins(seen, left):
    """a LEFT read that ends inside / a RIGHT read that starts inside an insertion of its own consensus: not fully covered, profile -1"""
    for x in seen.cells:
        if x["mine"] and x["v"]["type"] == INS and x["partial"] and x["al"] == -1:
            p = last_cons_pos(x["s"]) if left else first_cons_pos(x["s"])
            lo, hi = window(x["s"])
            if (left and hi < x["s"]["aln_len"] - 1 or not left and lo > 0) and x["tp"] <= p < x["tp"] + x["v"]["alt_len"] and (p < x["tp"] + x["v"]["alt_len"] - 1 if left else p > x["tp"]):
                return True
    return False


def _via_ref(seen, want):
    """a deletion seen by a read of the other cluster (get_full_cover_from_ref_cons_aln_str): 'full' = a read that covers it (allele 0); 'inside' = a
    partial read whose window ends inside the deleted span as its own consensus carries it (not covered, -1)"""
    for x in seen.cells:
        if x["mine"] or x["v"]["type"] != DEL:
            continue
        bc, ec = cons_span_of_ref(seen.res["aln_strs"][x["clu"]][0], x["v"]["off"] - 1, x["v"]["off"] + x["v"]["ref_len"])
        if want == "full" and x["al"] == 0 and ec - bc - 1 >= x["v"]["ref_len"]:
            return True
        if want == "inside" and x["al"] == -1 and x["partial"] and bc < last_cons_pos(x["s"]) < ec and first_cons_pos(x["s"]) <= bc:
            return True
    return False


def _deltas(seen):
    """hap 1 opens with an insertion >= 20 and hap 2 with a deletion >= 12; behind both come a private variant of each haplotype and a shared one"""
    i1 = [v for v in seen.v if v["type"] == INS and v["alt_len"] >= 20 and v["src"] == 1]
    d2 = [v for v in seen.v if v["type"] == DEL and v["ref_len"] >= 12 and v["src"] == 2]
    if not i1 or not d2:
        return False
    k = max(i1[0]["i"], d2[0]["i"])
    later = {v["src"] for v in seen.v[k + 1:]}
    return later == {1, 2, 3}


def _three_in_two_steps(seen):
    for st in seen.starts:
        per = np.bincount([r["col"] // 64 for r in st], minlength=4)
        if any(per[k] >= 3 and per[k + 1] >= 3 for k in range(len(per) - 1)):
            return True
    return False


def _end_run(seen, cls):
    return any(rr and rr[-1]["cls"] == cls and rr[-1]["end"] == len(seen.cols[c][0]) - 1 for c, rr in enumerate(seen.runs))


def _col0(seen, typ):
    return any(r["col"] == 0 and r["cls"] == (2 if typ == INS else 3) for rr in seen.runs for r in rr) and bool([v for v in seen.var(type=typ, off=0) if v["arb"] == 4])


CONDITIONS = {
    # scan kernel: lane-step boundaries (each start has an insertion in front of it: ref_off != column)
    **{f"start_at_col_{c}": (lambda s, c=c: s.start_at(c)) for c in (62, 63, 64, 65, 126, 127, 128, 129)},
    "ins_run_over_63_64": lambda s: s.run_over(2, 63, 64),
    "del_run_over_63_64": lambda s: s.run_over(3, 63, 64),
    "three_starts_in_two_steps": _three_in_two_steps,
    # scan kernel: start rule
    "mismatch_then_ins_is_no_variant": lambda s: _followed(s, 2),
    "mismatch_then_del_is_no_variant": lambda s: _followed(s, 3),
    "mismatch_in_last_column": lambda s: any(rr and rr[-1]["cls"] == 1 and rr[-1]["col"] == len(s.cols[c][0]) - 1 and s.var(type=SNP, off=rr[-1]["ref_off"])
                                             for c, rr in enumerate(s.runs)),
    "ins_at_col_0": lambda s: _col0(s, INS),
    "del_at_col_0": lambda s: _col0(s, DEL),
    "ins_at_right_end": lambda s: _end_run(s, 2),
    "del_at_right_end": lambda s: _end_run(s, 3),
    "ins_run_then_del_run": lambda s: _adjacent(s, 2, 3),
    "del_run_then_ins_run": lambda s: _adjacent(s, 3, 2),
    # profile kernel: is_match_aln_str
    **{f"ins_len_{n}": (lambda s, n=n: bool(s.var(type=INS, alt_len=n))) for n in (9, 10, 11, 20)},
    "cell_9_of_10_allele_1": lambda s: s.ins_cell(9, 10, 1),
    "cell_9_of_11_allele_0": lambda s: s.ins_cell(9, 11, 0),
    "cell_18_of_20_allele_1": lambda s: s.ins_cell(18, 20, 1),
    "cell_17_of_20_allele_0": lambda s: s.ins_cell(17, 20, 0),
    "cell_8_of_9_allele_0": lambda s: s.ins_cell(8, 9, 0),
    "left_read_ends_inside_ins": lambda s: _partial_in_ins(s, True),
    "right_read_starts_inside_ins": lambda s: _partial_in_ins(s, False),
    # profile kernel: deletions
    "del_at_ref_off_0_left_flank_negative": lambda s: any(x["mine"] and x["v"]["type"] == DEL and x["tp"] - 1 < 0 and x["al"] == 1 for x in s.cells),
    "other_cluster_read_covers_del": lambda s: _via_ref(s, "full"),
    "other_cluster_partial_read_ends_inside_del": lambda s: _via_ref(s, "inside"),
    "carrier_read_with_bases_inside_del": lambda s: any(x["mine"] and x["v"]["type"] == DEL and x["v"]["ref_len"] >= 3 and x["al"] == 0 and not x["partial"] for x in s.cells),
    # merge: exact_comp_var_site
    "identical_on_both_haps": lambda s: s.n_cons == 2 and bool(s.var(src=3, cate=0x200)),
    "same_site_snp_and_ins": lambda s: any(a["type"] == SNP and b["type"] == INS and _site(a) == _site(b) and {a["src"], b["src"]} == {1, 2} for a in s.v for b in s.v),
    "same_site_other_alt_hap1_first": lambda s: _pair(s, 1),
    "same_site_other_alt_hap2_first": lambda s: _pair(s, 2),
    "same_site_and_type_other_length": lambda s: any(a["type"] == b["type"] != SNP and _site(a) == _site(b) and (a["ref_len"], a["alt_len"]) != (b["ref_len"], b["alt_len"])
                                                     and {a["src"], b["src"]} == {1, 2} for a in s.v for b in s.v),
    "one_list_empty_other_two_or_more": lambda s: s.n_cons == 2 and s.n >= 2 and len({v["src"] for v in s.v}) == 1 and s.v[0]["src"] in (1, 2),
    # running ref/alt length differences per cluster
    "opposite_deltas_before_later_rows": _deltas,
    # exits and rows
    "one_consensus_all_hom": lambda s: s.n_cons == 1 and s.n >= 2 and all(v["cate"] == 0x200 and v["src"] == 1 for v in s.v),
    "no_variant_rows_minus1_minus2": lambda s: s.n_cons >= 1 and s.n == 0 and s.exp["n_rows"] > 0 and (s.exp["prof_start"] == -1).all() and (s.exp["prof_end"] == -2).all(),
    # host: var_is_homopolymer_indel
    "hp_ins_flag_1": lambda s: any(v["hp"] == 1 and v["alt_len"] >= 2 for v in s.var(type=INS)),
    "hp_del_flag_1": lambda s: any(v["hp"] == 1 and v["ref_len"] >= 2 for v in s.var(type=DEL)),
    "hp_ins_with_foreign_base_flag_0": lambda s: any(v["hp"] == 0 and v["alt_len"] >= 3 and len(set(v["alt"])) == 2 and sorted(v["alt"]).count(max(set(v["alt"]), key=v["alt"].count)) == v["alt_len"] - 1
                                                     and (s.case["chunk_ref"][v["off"] + s.beg - s.case["chunk_ref_beg"]:][:5] == max(set(v["alt"]), key=v["alt"].count)).all()
                                                     for v in s.var(type=INS)),
    "indel_5_before_chunk_ref_end": lambda s: any(v["type"] != SNP and v["off"] + s.beg - s.case["chunk_ref_beg"] + 5 == len(s.case["chunk_ref"]) and v["hp"] == 1 for v in s.v),
}


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
def _others(ref, b):
    """the three bases other than b, in ascending order (the order memcmp puts two alt bases in)"""
    return sorted(x for x in range(4) if x != int(b))


def _foreign(ref, p, n, seed):
    """n bases to insert in front of ref[p]: no equal neighbours inside, first and last differ from the reference bases on both sides of the gap"""
    rng = np.random.default_rng(seed)
    left, right = (int(ref[p - 1]) if p > 0 else -1), (int(ref[p]) if p < len(ref) else -1)
    out = []
    for k in range(n):
        bad = {out[-1] if out else left, left if k == 0 else -1, right if k in (0, n - 1) else -1, left if k == n - 1 else -1}
        out.append(int(rng.choice([x for x in range(4) if x not in bad])))
    return np.array(out, np.uint8)


def _case(ref, reads, want, tagged=True, beg=20000, chunk_ref=None, chunk_ref_beg=None, gap_aln=1):
    return dict(region=region(ref, reads, tagged), beg=beg, chunk_ref=ref if chunk_ref is None else chunk_ref, chunk_ref_beg=beg if chunk_ref_beg is None else chunk_ref_beg,
                gap_aln=gap_aln, want=tuple(want))


def lane_steps():
    """200 bp.  Both haplotypes open with a short insertion (2 and 3 bases), so columns run ahead of reference offsets by different amounts; SNPs then sit at
    columns 40, 62, 64, 100, 126, 128 of consensus 1 and 63, 65, 127, 129 of consensus 2.  The SNPs of the two haplotypes share reference positions 60, 62,
    124 and 126: other alt base with hap 1 first (60) and hap 2 first (62), the same alt base (124), other alt base again (126)."""
    ref = plain_ref(11, 200)
    lo = {p: _others(ref, ref[p]) for p in (38, 60, 62, 98, 124, 126)}
    h1 = edit(ref, [("I", 20, _foreign(ref, 20, 2, 1)), ("X", 38, lo[38][0]), ("X", 60, lo[60][0]), ("X", 62, lo[62][2]), ("X", 98, lo[98][1]), ("X", 124, lo[124][1]),
                    ("X", 126, lo[126][0])])
    h2 = edit(ref, [("I", 30, _foreign(ref, 30, 3, 2)), ("X", 60, lo[60][1]), ("X", 62, lo[62][0]), ("X", 124, lo[124][1]), ("X", 126, lo[126][2])])
    return _case(ref, full_reads(h1, h2, 6, 6), [f"start_at_col_{c}" for c in (62, 63, 64, 65, 126, 127, 128, 129)] +
                 ["three_starts_in_two_steps", "same_site_other_alt_hap1_first", "same_site_other_alt_hap2_first", "identical_on_both_haps"])


def runs_over_step():
    """160 bp.  Both haplotypes insert the same 2 bases at 10.  Hap 1 inserts 12 bases at 56 (columns 58..69), hap 2 deletes 11 bases from 58 (columns 60..70).
    Hap 1 has a LEFT read that ends 6 bases into the insertion, a RIGHT read that starts 6 bases into it and a LEFT read that ends at reference 63, inside
    the span hap 2 deletes; every full hap 1 read covers that span.  One hap 2 read keeps 4 of the 11 deleted bases."""
    ref = plain_ref(12, 160)
    i2 = _foreign(ref, 10, 2, 3)
    big = _foreign(ref, 56, 12, 4)
    h1 = edit(ref, [("I", 10, i2), ("I", 56, big)])
    h2 = edit(ref, [("I", 10, i2), ("D", 58, 11)])
    keeps = edit(ref, [("I", 10, i2), ("D", 58, 2), ("D", 64, 5)])           # reference 60..63 stay
    cut = 58 + 6                                                             # hap 1 coordinates: 2 + 56 bases, then the insertion
    reads = full_reads(h1, h2, 7, 7) + [(2, keeps, BOTH), (1, h1[:cut], LEFT), (1, h1[cut:], RIGHT), (1, h1[:2 + 12 + 64], LEFT)]
    return _case(ref, reads, ["ins_run_over_63_64", "del_run_over_63_64"] +
                 ["left_read_ends_inside_ins", "right_read_starts_inside_ins", "other_cluster_read_covers_del", "other_cluster_partial_read_ends_inside_del",
                  "carrier_read_with_bases_inside_del", "identical_on_both_haps"])


def start_rule():
    """120 bp.  Hap 1: two foreign bases in front of the reference (insertion at column 0), four reference bases near 40 replaced by one foreign base (a mismatch column
    directly followed by a deletion run), the last base substituted.  Hap 2: reference 0..2 missing (deletion at column 0), one reference base near 70 replaced by three
    foreign bases (a mismatch column directly followed by an insertion run), two foreign bases behind the reference (insertion in the last columns)."""
    ref = plain_ref(13, 120)
    L = len(ref)
    f = lambda p, ban: next(x for x in range(4) if x not in {int(b) for b in ban})
    q = next(p for p in range(40, 60) if len(set(ref[p - 1:p + 5].tolist())) < 4)      # reference q..q+3 -> one base that occurs nowhere in q-1..q+4
    h1 = edit(ref, [("I", 0, _foreign(ref, 0, 2, 5)), ("D", q, 3), ("X", q + 3, f(q + 3, ref[q - 1:q + 5])), ("X", L - 1, f(L - 1, ref[L - 3:]))])
    p = next(p for p in range(65, 100) if ref[p - 1] == ref[p + 1])                    # two letters occur nowhere in p-1..p+1: y, z -> y z y for reference p
    y, z = (x for x in range(4) if x not in (int(ref[p - 1]), int(ref[p])))
    h2 = edit(ref, [("D", 0, 3), ("X", p, y), ("I", p + 1, [z, y]), ("I", L, _foreign(ref, L, 2, 7))])
    return _case(ref, full_reads(h1, h2, 5, 5), ["ins_at_col_0", "del_at_col_0", "mismatch_then_del_is_no_variant", "mismatch_then_ins_is_no_variant", "mismatch_in_last_column",
                                                  "ins_at_right_end", "del_at_ref_off_0_left_flank_negative"])


AC_BLOCK, GT_BLOCK = seq("ACACCACAACCACAC"), seq("GTGTTGTGGTTGTGTGGT")


def _replaced_block(gap_aln, want):
    """110 bp, hap 2 is the reference.  Hap 1 replaces 12 bases over {A, C} by 8 bases over {G, T} (a deletion run and an insertion run side by side: the
    aligner's gap side decides which comes first) and loses the last 3 reference bases (a deletion run in the last columns)."""
    ref = plain_ref(14, 110)
    ref[40:52] = AC_BLOCK[:12]
    ref[-1] = next(x for x in range(4) if x not in (int(ref[-4]), int(ref[-2])))        # the deletion of the last 3 bases cannot move left
    h1 = edit(ref, [("D", 40, 12), ("I", 40, GT_BLOCK[:8]), ("D", len(ref) - 3, 3)])
    return _case(ref, full_reads(h1, ref, 5, 5), want, gap_aln=gap_aln)


def match_thresholds():
    """230 bp.  Hap 1 inserts 10 bases at 30, 20 at 90 and 9 at 150; hap 2 inserts 11 bases at 60.  Ten reads per haplotype; single reads carry substitutions
    inside an insertion (each column keeps its majority, so the consensus is the planted haplotype): 1 of 10, 2 of 20, 3 of 20, 1 of 9 on hap 1 and 2 of 11
    on hap 2 -- 9/10 and 18/20 reach 0.9, 17/20 and 9/11 do not, and below 10 bases only an exact match counts."""
    ref = plain_ref(15, 230)
    ins = {p: _foreign(ref, p, n, 20 + n) for p, n in ((30, 10), (90, 20), (150, 9), (60, 11))}
    h1 = edit(ref, [("I", p, ins[p]) for p in (30, 90, 150)])
    h2 = edit(ref, [("I", 60, ins[60])])

    def sub(h, at):
        out = h.copy()
        for k in at:
            out[k] = (out[k] + 2) % 4
        return out
    o90, o150 = 90 + 10, 150 + 30            # hap 1 coordinates of the later insertions
    reads = full_reads(h1, h2, 6, 9) + [(1, sub(h1, [30 + 4]), BOTH), (1, sub(h1, [o90 + 3, o90 + 12]), BOTH), (1, sub(h1, [o90 + 6, o90 + 9, o90 + 16]), BOTH),
                                        (1, sub(h1, [o150 + 5]), BOTH), (2, sub(h2, [60 + 2, 60 + 7]), BOTH)]
    return _case(ref, reads, ["ins_len_9", "ins_len_10", "ins_len_11", "ins_len_20", "cell_9_of_10_allele_1", "cell_18_of_20_allele_1", "cell_17_of_20_allele_0",
                              "cell_8_of_9_allele_0", "cell_9_of_11_allele_0"])


def site_ties():
    """130 bp.  Reference 30: SNP on hap 1, a 3-base insertion anchored there (in front of 31) on hap 2.  In front of 60: 4 inserted bases on hap 1, 6 on hap 2.
    From 90: 3 bases deleted on hap 1, 5 on hap 2."""
    ref = plain_ref(16, 130)
    h1 = edit(ref, [("X", 30, _others(ref, ref[30])[0]), ("I", 60, _foreign(ref, 60, 4, 8)), ("D", 90, 3)])
    h2 = edit(ref, [("I", 31, _foreign(ref, 31, 3, 9)), ("I", 60, _foreign(ref, 60, 6, 10)), ("D", 90, 5)])
    return _case(ref, full_reads(h1, h2, 5, 5), ["same_site_snp_and_ins", "same_site_and_type_other_length"])


def deltas():
    """260 bp.  Hap 1 opens with a 22-base insertion (running difference -22), hap 2 with a 14-base deletion (+14); behind them private SNPs and indels of each
    haplotype and shared ones, all classified with both differences in force."""
    ref = plain_ref(17, 260)
    sh_x, sh_i = _others(ref, ref[180])[1], _foreign(ref, 240, 3, 11)
    h1 = edit(ref, [("I", 30, _foreign(ref, 30, 22, 12)), ("X", 120, _others(ref, ref[120])[0]), ("X", 180, sh_x), ("D", 200, 4), ("I", 240, sh_i)])
    h2 = edit(ref, [("D", 50, 14), ("X", 150, _others(ref, ref[150])[2]), ("X", 180, sh_x), ("I", 220, _foreign(ref, 220, 5, 13)), ("I", 240, sh_i)])
    reads = full_reads(h1, h2, 6, 6) + [(1, h1[:22 + 210], LEFT), (2, h2[100:], RIGHT)]
    return _case(ref, reads, ["opposite_deltas_before_later_rows", "identical_on_both_haps", "other_cluster_read_covers_del"])


def one_consensus():
    """100 bp, ten identical untagged reads with a SNP, an insertion and a deletion: K2 finds one consensus, every variant is homozygous"""
    ref = plain_ref(18, 100)
    h = edit(ref, [("X", 20, _others(ref, ref[20])[1]), ("I", 40, _foreign(ref, 40, 3, 14)), ("D", 60, 4)])
    return _case(ref, [(1, h, BOTH)] * 10, ["one_consensus_all_hom"], tagged=False)


def no_variant():
    """67 bp, both haplotypes are the reference: two consensus sequences and no variant"""
    ref = plain_ref(19, 67)
    return _case(ref, full_reads(ref, ref, 4, 4), ["no_variant_rows_minus1_minus2"])


def homopolymer_flags():
    """120 bp inside a chunk reference that starts 7 bases earlier and ends with the region.  G x 6 at 30 gains GG on hap 1; A x 7 at 60 loses AA on hap 2;
    C x 6 at 85 gains CCA on hap 1 (left-aligned: CCA in front of the run -- one foreign base); the reference ends in T GGGGG and hap 2 loses one G, which
    left-aligned is the deletion of the base 5 in front of the end of the chunk reference."""
    ref = plain_ref(20, 120)
    ref[29:37] = [T, G, G, G, G, G, G, C]
    ref[59:68] = [C, A, A, A, A, A, A, A, G]
    ref[84:92] = [T, C, C, C, C, C, C, G]
    ref[-7:] = [C, T, G, G, G, G, G]
    h1 = edit(ref, [("I", 32, [G, G]), ("I", 87, [A, C, C])])
    h2 = edit(ref, [("D", 62, 2), ("D", len(ref) - 2, 1)])
    beg = 31000
    return _case(ref, full_reads(h1, h2, 5, 5), ["hp_ins_flag_1", "hp_del_flag_1", "hp_ins_with_foreign_base_flag_0", "indel_5_before_chunk_ref_end"], beg=beg,
                 chunk_ref=np.concatenate([plain_ref(21, 7), ref]).astype(np.uint8), chunk_ref_beg=beg - 7)


CASE_NAMES = ("lane_steps", "runs_over_step", "start_rule", "replaced_block_left", "replaced_block_right", "match_thresholds", "site_ties", "deltas", "one_consensus",
              "no_variant", "homopolymer_flags")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case; built once per process, never modified by a test"""
    out = dict(lane_steps=lane_steps(), runs_over_step=runs_over_step(), start_rule=start_rule(),
               replaced_block_left=_replaced_block(1, ["del_run_then_ins_run", "del_at_right_end", "one_list_empty_other_two_or_more"]),
               replaced_block_right=_replaced_block(2, ["ins_run_then_del_run", "del_at_right_end", "one_list_empty_other_two_or_more"]),
               match_thresholds=match_thresholds(), site_ties=site_ties(), deltas=deltas(), one_consensus=one_consensus(), no_variant=no_variant(),
               homopolymer_flags=homopolymer_flags())
    assert tuple(out) == CASE_NAMES
    for c in out.values():
        assert 67 <= c["region"]["reg_len"] <= 400 and 8 <= len(c["region"]["seqs"]) <= 20 and set(c["want"]) <= set(CONDITIONS)
    return out


def oracle_opt(oracle, gap_aln):
    o = oracle.default_opt()
    o.gap_aln = gap_aln
    return o


def through_oracle(oracle, case, gap_aln=None):
    """(res, exp) of a case: the oracle's strings and its variants / profile"""
    res = oracle.collect_noisy_reg_aln_strs(case["region"], oracle_opt(oracle, case["gap_aln"] if gap_aln is None else gap_aln))
    return res, oracle.make_vars_from_msa_cons_aln(res, case["beg"], case["chunk_ref"], case["chunk_ref_beg"])
