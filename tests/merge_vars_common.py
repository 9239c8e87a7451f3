"""Shared by tests/test_merge_vars_oracle.py, tests/test_gpu_merge_vars.py, tests/test_gpu_chunk_noisy_pass.py and tools/bench_merge_vars.py:
an independent pure-Python oracle of lcd_merge_region_vars (a pass's noisy-region variants folded into the chunk's variant table and read x variant
profile, one merge per region), a seeded generator of chunk states and region outputs, hand-built cases with their results written out, and a
field-for-field comparer.  States are clean_vars_dict layouts, regions are RegionBatch.region_vars layouts (longcalld_amd/align.py)."""
import numpy as np

CDIFF, CINS, CDEL = 8, 1, 2
FIELDS = ("pos", "var_type", "ref_len", "alt_len", "cate", "total_cov", "low_qual_cov", "alle_covs", "strand_alle_covs", "alt_off", "alt_pool",
          "is_homopolymer_indel", "regs", "start_var_idx", "end_var_idx", "allele_off", "alleles", "alt_qi", "cr_read")


# ---------------- the oracle ----------------
def var_key(pos, var_type, ref_len, alt_len, alt):
    """the comparator as a tuple: position key, type, ref_len, alt_len, alt bases of X / INS"""
    return (int(pos) if var_type == CDIFF else int(pos) - 1, int(var_type), int(ref_len), int(alt_len),
            bytes(bytearray(int(x) for x in alt)) if var_type in (CDIFF, CINS) else b"")


def _rs_sort(a, lo, hi, s):
    """in-place most-significant-byte radix sort of a[lo:hi] ((key, label) pairs) on bits s..s+7, cycle by cycle from the first bucket; buckets of more than
    64 entries recurse on the next byte, smaller ones are insertion-sorted: the order of equal keys is the algorithm's, not the input's"""
    cnt = [0] * 256
    for i in range(lo, hi):
        cnt[(a[i][0] >> s) & 255] += 1
    b, e, at = [0] * 256, [0] * 256, lo
    for k in range(256):
        b[k] = at; at += cnt[k]; e[k] = at
    first = list(b)
    k = 0
    while k < 256:
        if b[k] == e[k]:
            k += 1
            continue
        dst = (a[b[k]][0] >> s) & 255
        if dst == k:
            b[k] += 1
            continue
        tmp = a[b[k]]
        while dst != k:
            tmp, a[b[dst]] = a[b[dst]], tmp
            b[dst] += 1
            dst = (tmp[0] >> s) & 255
        a[b[k]] = tmp
        b[k] += 1
    if s:
        s = s - 8 if s > 8 else 0
        for k in range(256):
            n = e[k] - first[k]
            if n > 64:
                _rs_sort(a, first[k], e[k], s)
            elif n > 1:
                a[first[k]:e[k]] = sorted(a[first[k]:e[k]], key=lambda x: x[0])


def cr_labels(intervals):
    """labels of (start, label) intervals in interval-index order: kept as added when the starts never decrease, else sorted by start (up to 64 entries: a stable
    insertion sort; more: the radix sort above)"""
    a = [(max(int(s), 0), int(l)) for s, l in intervals]
    if all(a[i - 1][0] <= a[i][0] for i in range(1, len(a))):
        return np.array([l for _, l in a], np.int32)
    if len(a) <= 64:
        a.sort(key=lambda x: x[0])
    else:
        _rs_sort(a, 0, len(a), 56)
    return np.array([l for _, l in a], np.int32)


def read_cr(start, end, ordered, skipped):
    return cr_labels([(start[r], r) for r in ordered if not skipped[r] and start[r] >= 0 and end[r] >= 0])


def _alts(cv):
    return [cv["alt_pool"][int(cv["alt_off"][i]):int(cv["alt_off"][i + 1])] for i in range(cv["n_vars"])]


def merge_one(cv, reg, ordered, skipped):
    """one merge: state x one region -> (new state, a_to_merged, b_to_merged)"""
    nb = int(reg["n_vars"])
    if nb <= 0:
        return cv, np.arange(cv["n_vars"], dtype=np.int32), np.zeros(0, np.int32)
    V, R = cv["n_vars"], cv["n_reads"]
    alts = _alts(cv)
    ka = [var_key(cv["pos"][i], cv["var_type"][i], cv["ref_len"][i], cv["alt_len"][i], alts[i]) for i in range(V)]
    kb = [var_key(reg["pos"][j], reg["var_type"][j], reg["ref_len"][j], reg["alt_len"][j], reg["alt_seqs"][j]) for j in range(nb)]
    a2m, b2m, src = np.full(V, -1, np.int32), np.full(nb, -1, np.int32), []
    i = j = 0
    while i < V and j < nb:
        if ka[i] < kb[j]:
            a2m[i] = len(src); src.append(("a", i)); i += 1
        elif ka[i] > kb[j]:
            b2m[j] = len(src); src.append(("b", j)); j += 1
        else:
            a2m[i] = len(src); src.append(("a", i)); i += 1; j += 1
    while i < V:
        a2m[i] = len(src); src.append(("a", i)); i += 1
    while j < nb:
        b2m[j] = len(src); src.append(("b", j)); j += 1
    M = len(src)
    out = dict(n_vars=M, n_reads=R, regs=np.array(cv["regs"], np.int64).reshape(-1, 3), qual_upload_bytes=0)
    cols = {k: [] for k in ("pos", "var_type", "ref_len", "alt_len", "cate", "total_cov", "low_qual_cov", "is_homopolymer_indel")}
    alle, strand, pool, aoff = [], [], [], [0]
    for side, q in src:
        if side == "a":
            for k in cols:
                cols[k].append(int(cv[k][q]))
            alle += [int(x) for x in cv["alle_covs"][2 * q:2 * q + 2]]; strand += [int(x) for x in cv["strand_alle_covs"][4 * q:4 * q + 4]]
            pool += [int(x) for x in alts[q]]
        else:
            for k in ("pos", "var_type", "ref_len", "alt_len", "cate", "total_cov", "is_homopolymer_indel"):
                cols[k].append(int(reg[k][q]))
            cols["low_qual_cov"].append(0)
            alle += [int(reg["alle_covs"][q][0]), int(reg["alle_covs"][q][1])]; strand += [0, 0, 0, 0]
            if int(reg["var_type"][q]) in (CDIFF, CINS):
                pool += [int(x) for x in reg["alt_seqs"][q]]
        aoff.append(len(pool))
    for k, v in cols.items():
        out[k] = np.array(v, np.int64 if k == "pos" else np.int32)
    out["alle_covs"] = np.array(alle, np.int32); out["strand_alle_covs"] = np.array(strand, np.int32)
    out["alt_pool"] = np.array(pool, np.uint8); out["alt_off"] = np.array(aoff, np.uint64)
    row_of = {int(r): q for q, r in enumerate(reg["row_read_ids"])}
    pa = np.asarray(reg["prof_alleles"]).reshape(len(reg["row_read_ids"]), nb)
    live = np.zeros(R, bool)
    for r in ordered:
        live[r] = not skipped[r]
    start, end, off, al, qi = np.full(R, -1, np.int32), np.full(R, -2, np.int32), [0], [], []
    for r in range(R):
        cells = {}
        if live[r]:
            s, e = int(cv["start_var_idx"][r]), int(cv["end_var_idx"][r])
            if s >= 0 and e >= s:
                o = int(cv["allele_off"][r])
                for v in range(s, e + 1):
                    cells[int(a2m[v])] = (int(cv["alleles"][o + v - s]), int(cv["alt_qi"][o + v - s]))
            if r in row_of:
                q = row_of[r]
                s, e = int(reg["prof_start"][q]), int(reg["prof_end"][q])
                if s >= 0 and e >= s:
                    for v in range(s, e + 1):
                        if b2m[v] >= 0:
                            cells[int(b2m[v])] = (int(pa[q, v]), -1)
        if cells:
            start[r], end[r] = min(cells), max(cells)
            for m in range(start[r], end[r] + 1):
                a_, q_ = cells.get(m, (-1, -1))
                al.append(a_); qi.append(q_)
        off.append(len(al))
    out.update(start_var_idx=start, end_var_idx=end, allele_off=np.array(off, np.uint64), alleles=np.array(al, np.int32), alt_qi=np.array(qi, np.int32),
               cr_read=read_cr(start, end, ordered, skipped))
    return out, a2m, b2m


def oracle_merge(cv, regions, ordered, skipped):
    """the left fold over the regions in the order given -> (state, cur_to_merged, [region_to_merged]) with the maps composed through the whole fold"""
    ordered = [int(x) for x in ordered]
    state = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in cv.items()}
    state["qual_upload_bytes"] = 0
    c2m, r2m = np.arange(cv["n_vars"], dtype=np.int32), []
    for reg in regions:
        state, a2m, b2m = merge_one(state, reg, ordered, skipped)
        c2m = a2m[c2m] if len(c2m) else c2m
        r2m = [np.where(m >= 0, a2m[np.maximum(m, 0)], -1).astype(np.int32) if len(m) else m for m in r2m]
        r2m.append(b2m)
    return state, c2m.astype(np.int32), r2m


def same_merge(got, want):
    """(state, cur_to_merged, [region_to_merged]) equal in every field of the state and in both maps"""
    (a, ac, ar), (b, bc, br) = got, want
    assert a["n_vars"] == b["n_vars"] and a["n_reads"] == b["n_reads"], (a["n_vars"], b["n_vars"], a["n_reads"], b["n_reads"])
    assert int(a["qual_upload_bytes"]) == 0
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "regs":
            x, y = x.reshape(-1, 3), y.reshape(-1, 3)
        assert x.shape == y.shape and (x.astype(np.int64) == y.astype(np.int64)).all(), (k, x.shape, y.shape, x.reshape(-1)[:20], y.reshape(-1)[:20])
    assert np.array_equal(np.asarray(ac), np.asarray(bc)), ("cur_to_merged", ac, bc)
    assert len(ar) == len(br)
    for k, (x, y) in enumerate(zip(ar, br)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), ("region_to_merged", k, x, y)


# ---------------- building states and regions ----------------
def make_cv(variants, reads, skipped=(), regs=((10, 20, 3),), ordered=None):
    """variants: (pos, type, ref_len, alt_len, alt codes); reads: None | (start, [alleles]) per read.  Per-variant numbers: cate 4, total_cov 20 + i,
    low_qual_cov 1 + i, alle_covs (10 + i, 5 + i), strand counts i + (1, 2, 3, 4); alt_qi of the k-th cell of the chunk: 100 + k"""
    V, R = len(variants), len(reads)
    pool, aoff = [], [0]
    for v in variants:
        pool += list(v[4]) if v[1] in (CDIFF, CINS) else []
        aoff.append(len(pool))
    start, end, off, al = np.full(R, -1, np.int32), np.full(R, -2, np.int32), [0], []
    for r, p in enumerate(reads):
        if p is not None:
            start[r], end[r] = p[0], p[0] + len(p[1]) - 1
            al += list(p[1])
        off.append(len(al))
    sk = np.zeros(R, np.uint8)
    sk[list(skipped)] = 1
    ordered = list(range(R)) if ordered is None else list(ordered)
    iv = np.arange(V)
    return dict(n_vars=V, n_reads=R, pos=np.array([v[0] for v in variants], np.int64), var_type=np.array([v[1] for v in variants], np.int32),
                ref_len=np.array([v[2] for v in variants], np.int32), alt_len=np.array([v[3] for v in variants], np.int32), cate=np.full(V, 4, np.int32),
                total_cov=(20 + iv).astype(np.int32), low_qual_cov=(1 + iv).astype(np.int32), alle_covs=np.stack([10 + iv, 5 + iv], 1).reshape(-1).astype(np.int32),
                strand_alle_covs=(iv[:, None] + np.array([1, 2, 3, 4])).reshape(-1).astype(np.int32), alt_off=np.array(aoff, np.uint64),
                alt_pool=np.array(pool, np.uint8), is_homopolymer_indel=np.zeros(V, np.int32), regs=np.array(regs, np.int64).reshape(-1, 3),
                start_var_idx=start, end_var_idx=end, allele_off=np.array(off, np.uint64), alleles=np.array(al, np.int32),
                alt_qi=(100 + np.arange(len(al))).astype(np.int32), cr_read=read_cr(start, end, ordered, sk), qual_upload_bytes=0), np.array(ordered, np.int32), sk


def make_reg(variants, rows, cate=0x100):
    """variants as in make_cv; rows: (read, prof_start, prof_end, [allele per region variant]).  Per-variant numbers: total_cov 30 + j, alle_covs (7 + j, 8 + j),
    is_homopolymer_indel j % 2"""
    n = len(variants)
    jv = np.arange(n)
    return dict(n_vars=n, n_rows=len(rows), pos=np.array([v[0] for v in variants], np.int64), var_type=np.array([v[1] for v in variants], np.int64),
                ref_len=np.array([v[2] for v in variants], np.int64), alt_len=np.array([v[3] for v in variants], np.int64), cate=np.full(n, cate, np.int64),
                total_cov=30 + jv, is_homopolymer_indel=jv % 2, alle_covs=np.stack([7 + jv, 8 + jv], 1).astype(np.int32).reshape(n, 2),
                alt_seqs=[np.array(v[4], np.uint8) for v in variants], row_read_ids=np.array([r[0] for r in rows], np.int32),
                prof_start=np.array([r[1] for r in rows], np.int32), prof_end=np.array([r[2] for r in rows], np.int32),
                prof_alleles=np.array([r[3] for r in rows], np.int32).reshape(len(rows), n))


def X(pos, base):
    return (pos, CDIFF, 1, 1, [base])


def INS(pos, bases):
    return (pos, CINS, 0, len(bases), list(bases))


def DEL(pos, n):
    return (pos, CDEL, n, 0, [])


def hand_cases():
    """name -> (cv, regions, ordered, skipped, expected): expected holds the result's fields written out by hand"""
    cases = {}
    # X at p followed by INS at p + 1 share the position key 105 and INS < X by type: the region list is out of comparator order and is walked as given.
    # read 1 has no profile and gains one.
    cv, o, s = make_cv([X(100, 0), X(110, 1)], [(0, [1, 0]), None])
    reg = make_reg([X(105, 1), INS(106, [2, 2])], [(0, 0, 1, [0, 1]), (1, 1, 1, [-1, 1])])
    cases["out_of_comparator_order"] = (cv, [reg], o, s, dict(
        pos=[100, 105, 106, 110], var_type=[8, 8, 1, 8], ref_len=[1, 1, 0, 1], alt_len=[1, 1, 2, 1], cate=[4, 0x100, 0x100, 4], total_cov=[20, 30, 31, 21],
        low_qual_cov=[1, 0, 0, 2], alle_covs=[10, 5, 7, 8, 8, 9, 11, 6], strand_alle_covs=[1, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 4, 5],
        alt_off=[0, 1, 2, 4, 5], alt_pool=[0, 1, 2, 2, 1], is_homopolymer_indel=[0, 0, 1, 0], start_var_idx=[0, 2], end_var_idx=[3, 2], allele_off=[0, 4, 5],
        alleles=[1, 0, 1, 0, 1], alt_qi=[100, -1, -1, 101, -1], cr_read=[0, 1], cur_to_merged=[0, 3], region_to_merged=[[1, 2]]))
    # the region's first variant equals a current one: dropped, map -1, the old allele stays.  read 1's only cell is lost; read 2's span starts at the
    # dropped variant, so its start moves to the next one.
    cv, o, s = make_cv([X(100, 0), DEL(120, 3)], [(0, [0]), None, None])
    reg = make_reg([X(100, 0), X(101, 1)], [(0, 0, 1, [1, 1]), (1, 0, 0, [1, -1]), (2, 0, 1, [1, 1])])
    cases["equal_variant_dropped"] = (cv, [reg], o, s, dict(
        pos=[100, 101, 120], var_type=[8, 8, 2], ref_len=[1, 1, 3], alt_len=[1, 1, 0], cate=[4, 0x100, 4], total_cov=[20, 31, 21], low_qual_cov=[1, 0, 2],
        alle_covs=[10, 5, 8, 9, 11, 6], alt_off=[0, 1, 2, 2], alt_pool=[0, 1], is_homopolymer_indel=[0, 1, 0], start_var_idx=[0, -1, 1], end_var_idx=[1, -2, 1],
        allele_off=[0, 2, 2, 3], alleles=[0, 1, 1], alt_qi=[100, -1, -1], cr_read=[0, 2], cur_to_merged=[0, 2], region_to_merged=[[-1, 1]]))
    # a region with n_vars = 0; a row with prof_start = -1; holes filled with -1; a skipped read; an allele -1 inside a row's span still stretches the span
    cv, o, s = make_cv([X(100, 0), X(200, 1), X(300, 2)], [(0, [1, -1, 0]), None, (0, [1]), None], skipped=[1], ordered=[3, 2, 1, 0])
    empty = make_reg([], [])
    reg = make_reg([X(150, 3), X(250, 3)], [(0, -1, -2, [-1, -1]), (1, 0, 1, [1, 1]), (2, 1, 1, [-1, 0]), (3, 0, 1, [-1, 1])])
    cases["holes_skipped_empty_region"] = (cv, [empty, reg], o, s, dict(
        pos=[100, 150, 200, 250, 300], cate=[4, 0x100, 4, 0x100, 4], start_var_idx=[0, -1, 0, 1], end_var_idx=[4, -2, 3, 3], allele_off=[0, 5, 5, 9, 12],
        alleles=[1, -1, -1, -1, 0, 1, -1, -1, 0, -1, -1, 1], alt_qi=[100, -1, 101, -1, 102, 103, -1, -1, -1, -1, -1, -1], cr_read=[2, 0, 3],
        cur_to_merged=[0, 2, 4], region_to_merged=[[], [1, 3]]))
    # the chunk has no variant yet and every profile is empty
    cv, o, s = make_cv([], [None, None])
    reg = make_reg([INS(50, [0, 1]), DEL(60, 2)], [(0, 0, 1, [1, 0])])
    cases["empty_current_table"] = (cv, [reg], o, s, dict(
        pos=[50, 60], var_type=[1, 2], ref_len=[0, 2], alt_len=[2, 0], cate=[0x100, 0x100], total_cov=[30, 31], low_qual_cov=[0, 0], alle_covs=[7, 8, 8, 9],
        strand_alle_covs=[0] * 8, alt_off=[0, 2, 2], alt_pool=[0, 1], is_homopolymer_indel=[0, 1], start_var_idx=[0, -1], end_var_idx=[1, -2],
        allele_off=[0, 2, 2], alleles=[1, 0], alt_qi=[-1, -1], cr_read=[0], cur_to_merged=[], region_to_merged=[[0, 1]]))
    # the second region ties with a variant the first one added: the first wins (its category and coverage stay, its allele stays)
    cv, o, s = make_cv([X(100, 0)], [(0, [0])])
    r0 = make_reg([X(200, 3)], [(0, 0, 0, [1])], cate=0x100)
    r1 = make_reg([X(200, 3), X(210, 0)], [(0, 0, 1, [0, 1])], cate=0x200)
    cases["second_region_ties_with_first"] = (cv, [r0, r1], o, s, dict(
        pos=[100, 200, 210], cate=[4, 0x100, 0x200], total_cov=[20, 30, 31], alle_covs=[10, 5, 7, 8, 8, 9], start_var_idx=[0], end_var_idx=[2], allele_off=[0, 3],
        alleles=[0, 1, 1], alt_qi=[100, -1, -1], cr_read=[0], cur_to_merged=[0], region_to_merged=[[1], [-1, 2]]))
    return cases


def check_expected(got, exp):
    st, c2m, r2m = got
    for k, v in exp.items():
        if k == "cur_to_merged":
            assert list(c2m) == v, (k, list(c2m), v)
        elif k == "region_to_merged":
            assert [list(m) for m in r2m] == v, (k, [list(m) for m in r2m], v)
        else:
            assert [int(x) for x in np.asarray(st[k]).reshape(-1)] == v, (k, [int(x) for x in np.asarray(st[k]).reshape(-1)], v)
    assert st["n_vars"] == len(exp["pos"])


# ---------------- seeded shapes ----------------
def _rand_var(rng, pos):
    t = int(rng.integers(0, 3))
    if t == 0:
        return X(pos, int(rng.integers(0, 4)))
    if t == 1:
        return INS(pos, [int(x) for x in rng.integers(0, 4, int(rng.integers(1, 4)))])
    return DEL(pos, int(rng.integers(1, 4)))


def make_case(seed, n_reads, n_vars, n_regions, span=8, p_profile=0.9, p_skip=0.05, p_tie=0.25, n_all_ties=0, sorted_regions=False, max_reg_vars=5):
    """a seeded chunk state (comparator-sorted, distinct variants; random read spans of about `span` variants; a shuffled ordered_read_ids; a few skipped
    reads) and n_regions region outputs of 1..max_reg_vars variants around a locus in position order (NOT comparator order unless sorted_regions), some equal
    to a current variant or to one of an earlier region, the last n_all_ties regions made of current variants only; rows over a random subset of the reads
    with random sub-spans, some without a span"""
    rng = np.random.default_rng(seed)
    keyed = {}
    for p in sorted(rng.choice(np.arange(1000, 1000 + 40 * max(n_vars, 1)), n_vars, replace=False)):
        v = _rand_var(rng, int(p))
        keyed[var_key(*v)] = v
    variants = [keyed[k] for k in sorted(keyed)]
    V = len(variants)
    reads = []
    for r in range(n_reads):
        if V == 0 or rng.random() >= p_profile:
            reads.append(None)
            continue
        s = int(rng.integers(0, V)); n = int(min(V - s, max(1, rng.integers(span // 2, span + span // 2 + 1))))
        reads.append((s, [int(x) for x in rng.integers(-1, 2, n)]))
    skipped = [r for r in range(n_reads) if rng.random() < p_skip]
    for r in skipped:
        reads[r] = None
    cv, ordered, sk = make_cv(variants, reads, skipped=skipped, regs=[(100 * i, 100 * i + 50, 5 + i % 3) for i in range(4)], ordered=rng.permutation(n_reads))
    cv["cate"] = rng.choice([4, 8, 0x10, 0x80], V).astype(np.int32)
    regions, added = [], []
    for k in range(n_regions):
        nv = int(rng.integers(1, max_reg_vars + 1))
        locus = int(rng.integers(1000, 1000 + 40 * max(n_vars, 1)))
        vs = []
        for _ in range(nv):
            u = rng.random()
            if V and (k >= n_regions - n_all_ties or u < p_tie / 2):
                vs.append(variants[int(rng.integers(0, V))])
            elif added and u < p_tie:
                vs.append(added[int(rng.integers(0, len(added)))])
            else:
                vs.append(_rand_var(rng, locus + int(rng.integers(0, 12))))
        uniq = {var_key(*v): v for v in vs}
        vs = [uniq[k_] for k_ in sorted(uniq)] if sorted_regions else sorted(uniq.values(), key=lambda v: v[0])
        added += vs
        nv = len(vs)
        rows = []
        for r in rng.choice(n_reads, int(rng.integers(0, min(n_reads, 40) + 1)), replace=False):
            if rng.random() < 0.15:
                rows.append((int(r), -1, -2, [-1] * nv))
                continue
            s = int(rng.integers(0, nv)); e = int(rng.integers(s, nv))
            al = [-1] * nv
            al[s:e + 1] = [int(x) for x in rng.integers(-1, 2, e - s + 1)]
            rows.append((int(r), s, e, al))
        regions.append(make_reg(vs, rows, cate=int(rng.choice([0x100, 0x200]))))
    return cv, regions, ordered, sk


SHAPES = {
    # just over one wavefront of reads
    "A": dict(seed=11, n_reads=70, n_vars=40, n_regions=6, span=8),
    # read spans of about 30 variants: about 9 000 cells, two workgroups of reads, so the offset scan crosses workgroups
    "B": dict(seed=12, n_reads=300, n_vars=120, n_regions=20, span=30),
    # half the reads without a profile; the last three regions hold current variants only, so every cell of their rows is dropped
    "C": dict(seed=13, n_reads=130, n_vars=30, n_regions=8, span=6, p_profile=0.5, n_all_ties=3),
}
