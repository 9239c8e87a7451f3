"""Tie-dense inputs for the POA / WFA / edlib parity tests: reads on which the oracle's backtrack has to DECIDE between alternatives of equal score.

The kernels are correct in the sense that their tie-breaks follow oracle/poa.c and oracle/wfa2p.c.  Reads of iid bases hardly ever produce a tie (the census of
oracle/poa.c, pyoracle.poa_tie_census, counts them by kind), so the generators below construct them:

  bubble_chain  SNP bubbles whose two branches carry EQUAL weight, third-allele and N reads at the bubble sites, indels of exactly the length at which the two gap
                pieces cost the same (o1 + e1 * L == o2 + e2 * L: 18 bases at the default scoring), deletions that span bubbles, short tandem-repeat blocks
  str_chain     reads that are tandem repeats from end to end, with the indel errors of homopolymer / STR sequencing
  tie_pairs     (pattern, text) pairs from the same material for WFA and edlib

Everything is seeded, pure numpy, and returns reads only.  POA_CASES is the table the CPU test (tests/test_tie_cases_oracle.py: census minimums, planned class)
and the GPU test (tests/test_gpu_poa_ties.py: parity with the oracle) share; oracle results are computed once per (reads, mode, scoring) and cached here."""
import numpy as np

DEFAULT_SCORING = dict(match=2, mismatch=6, gap_open1=6, gap_ext1=2, gap_open2=24, gap_ext2=1)
ALT_SCORING = dict(match=2, mismatch=6, gap_open1=8, gap_ext1=3, gap_open2=30, gap_ext2=2)     # crossover 22
WIDE_SCORING = dict(match=1, mismatch=33, gap_open1=6, gap_ext1=2, gap_open2=24, gap_ext2=1)   # outside the lean rows' 6-bit score field


def crossover(scoring=None):
    """the gap length at which both gap pieces cost the same, (o2 - o1) / (e1 - e2); must be an integer"""
    s = dict(DEFAULT_SCORING, **(scoring or {}))
    num, den = s["gap_open2"] - s["gap_open1"], s["gap_ext1"] - s["gap_ext2"]
    assert den > 0 and num % den == 0, s
    return num // den


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def _tandem(rng, length, units=(1, 4)):
    """a tandem repeat of `length` bases whose unit has units[0]..units[1] bases and is not itself a repeat of a single base (unless it has one base)"""
    u = int(rng.integers(units[0], units[1] + 1))
    unit = rng.integers(0, 4, u)
    if u > 1 and (unit == unit[0]).all():
        unit[-1] = (unit[0] + 1) % 4
    return np.tile(unit, length // u + 1)[:length]


def _edit(h, dels=(), ins=()):
    """h with `dels` [(pos, n)]: n bases removed from pos on, and `ins` [(pos, bases)]: bases inserted before pos"""
    dels, ins = dict(dels), dict(ins)
    out, i = [], 0
    while i < len(h):
        if i in ins:
            out.extend(ins[i])
        if i in dels:
            i += dels[i]
            continue
        out.append(h[i]); i += 1
    return _u8(out)


def bubble_sites(L):
    return list(range(12, L - 12, 25))


def bubble_chain(rng, L, scoring=None, indel_len=None, n_plain=4):
    """17 reads (at n_plain = 4) over an L-base backbone, see the module docstring.  indel_len replaces the crossover-length indels by indels of that length (at
    sites far enough apart for them)"""
    X = crossover(scoring)
    h1 = rng.integers(0, 4, L).astype(np.uint8)
    for p in range(30, L - 45, 90):                       # tandem-repeat blocks of unit 1 - 4 and length 40, one every ~90 bases
        h1[p:p + 40] = _tandem(rng, 40)
    sites = bubble_sites(L)
    h2 = h1.copy()
    h2[sites] = (h1[sites] + 1) % 4                       # a SNP every 25 bases
    third, withn = h1.copy(), h2.copy()
    third[sites] = (h1[sites] + 2) % 4
    withn[sites] = 4
    third_sites = lambda k0: sites[k0::3]
    if indel_len is None:
        plan = lambda k0, d: [(s, d) for s in third_sites(k0)]
    else:   # the long indels at sites far enough apart for them, crossover-length ones at the third sites that stay clear of those
        def plan(k0, d):
            far = [s for s in sites[k0::3 * (1 + (indel_len + 60) // 75)] if s - indel_len // 2 - 30 >= 0 and s + indel_len // 2 + 30 < L]
            return sorted([(s, indel_len + d - X) for s in far] + [(s, d) for s in third_sites(k0) if all(abs(s - f) > indel_len // 2 + 60 for f in far)])
    reads = [(h1 if i % 2 == 0 else h2).copy() for i in range(2 * n_plain)]     # 4 + 4 exact copies, alternating: both branches of every bubble weigh the same
    reads += [third, withn]
    for k, h in enumerate((h1, h2)):                      # deletions of exactly the crossover length centred on every third site
        reads.append(_edit(h, dels=[(s - d // 2, d) for s, d in plan(k, X)]))
    for k, (h, n) in enumerate(((h1, X), (h2, X + 1), (h1, X - 1))):     # insertions of crossover, crossover + 1 and crossover - 1 bases at every third site
        reads.append(_edit(h, ins=[(s, rng.integers(0, 4, d)) for s, d in plan(k, n)]))
    reads.append(_edit(h1, dels=[(s - 1, 3) for s in third_sites(1)]))     # 3-base deletions that span every third site: the site in the middle of the gap ...
    reads.append(_edit(h2, dels=[(s - 2, 3) for s in third_sites(2)]))     # ... and the site as the gap's last base
    return reads


def _str_hap(rng, L):
    parts, n = [rng.integers(0, 4, 12)], 12
    while n < L - 12:
        run = _tandem(rng, int(rng.integers(12, 71)), (1, 6))
        sp = rng.integers(0, 4, int(rng.integers(0, 7)))
        parts += [run, sp]; n += len(run) + len(sp)
    h = np.concatenate(parts)[:L - 12]
    return _u8(np.concatenate([h, rng.integers(0, 4, 12)]))


def _str_errors(rng, h, rate):
    """`rate` errors per base: 45 % a deleted base, 45 % a doubled base, 10 % a substitution"""
    x = rng.random(len(h))
    sub = rng.integers(1, 4, len(h))
    out = []
    for i, b in enumerate(h):
        if x[i] < 0.45 * rate:
            continue
        if x[i] < 0.9 * rate:
            out += [b, b]
        elif x[i] < rate:
            out.append((b + sub[i]) % 4)
        else:
            out.append(b)
    return _u8(out)


def str_haps(rng, L):
    """two haplotypes of tandem-repeat runs (unit 1 - 6, run length 12 - 70, 0 - 6 iid spacer bases) between 12-base iid flanks; h2 differs from h1 by one
    copy-number change of 1 - 12 bases per 300 bases"""
    h1 = _str_hap(rng, L)
    dels, ins = [], []
    for a in range(20, L - 40, 300):
        p, k = int(rng.integers(a, min(a + 280, L - 30))), int(rng.integers(1, 13))
        if rng.random() < 0.5:
            dels.append((p, k))
        else:
            ins.append((p, h1[p:p + k].copy()))          # (the next k bases once more: a copy gained)
    return h1, _edit(h1, dels=dels, ins=ins)


def str_chain(rng, L, n, rate):
    h1, h2 = str_haps(rng, L)
    return [_str_errors(rng, h1 if i % 2 == 0 else h2, rate) for i in range(n)]


# The seed of the iid comparison chain.  Its multi_* and open_and_ext counts are 0 - 4 whatever the seed; its cross_kind count (an inserted base that equals its
# neighbour ties a match with an insertion run) is 20 - 40 over seeds 0 - 7 at this size, around the constructed chains' minimum of 30: 2 is the smallest seed below it
IID_SEED = 2


def iid_chain(rng, L=300, n=12, rate=0.02):
    """the kind of chain the older kernel tests draw (tests/test_gpu_kernels.py _poa_chains): iid bases, two haplotypes, uniform errors"""
    from conftest import mutate
    truth = rng.integers(0, 4, L).astype(np.uint8)
    hap2 = truth.copy()
    for p in range(10, L - 10, max(20, L // 6)):
        hap2[p] = (hap2[p] + 1) % 4
    return [mutate(rng, truth if i % 2 == 0 else hap2, rate) for i in range(n)]


# ---------------------------------------------------------------- WFA / edlib pairs
WFA_PENALTIES = [(6, 6, 2, 24, 1), (4, 6, 2, 24, 1), (5, 8, 3, 30, 2)]     # (mismatch, o1, e1, o2, e2); crossover 18, 18, 22
EDLIB_LENS = (63, 64, 65, 300, 2300, 4300)


def _pen_crossover(pen):
    return crossover(dict(gap_open1=pen[1], gap_ext1=pen[2], gap_open2=pen[3], gap_ext2=pen[4]))


def tie_pairs(kind, seed=0, penalties=WFA_PENALTIES[0]):
    """(pattern, text) pairs.  kind:
      "str"        str_chain reads against their haplotype, 150 - 900 bases, both ways round
      "crossover"  one indel of exactly the crossover length of `penalties`, crossover + 1 and crossover - 1, in iid and in tandem-repeat context, both ways round
      "wide"       a tandem-repeat text of 1 000 bases with a 1 500 - 2 900 base tandem-repeat insertion (rows of >= 2 048 diagonals)
      "edlib"      homopolymer and dinucleotide pairs at 63 / 64 / 65 / 300 / 2 300 / 4 300 bases (word, tile and Hirschberg edges), (target, query)"""
    rng = np.random.default_rng([seed, {"str": 1, "crossover": 2, "wide": 3, "edlib": 4}[kind]])
    pairs = []
    if kind == "str":
        for L in (150, 400, 400, 650, 900):
            h1, h2 = str_haps(rng, L)
            r = _str_errors(rng, h2, 0.03)
            pairs += [(r, h1), (h1, r)]
    elif kind == "crossover":
        X = _pen_crossover(penalties)
        for d in (X, X + 1, X - 1):
            t = rng.integers(0, 4, 240).astype(np.uint8)
            p = _edit(t, ins=[(120, rng.integers(0, 4, d))])
            pairs += [(p, t), (t, p)]
            t = _str_hap(rng, 300)
            p = _edit(t, dels=[(140, d)])
            pairs += [(p, t), (t, p)]
            t = _u8(np.concatenate([rng.integers(0, 4, 60), _tandem(rng, 120, (2, 3)), rng.integers(0, 4, 60)]))
            p = _edit(t, ins=[(100, t[100:100 + d].copy())])     # a copy-number gain inside the repeat: the gap can sit anywhere in it
            pairs += [(p, t), (t, p)]
    elif kind == "wide":
        for i, D in enumerate((1500, 2200, 2900)):
            t = _str_hap(rng, 1000)
            at = int(rng.integers(100, 900))
            p = _u8(np.concatenate([t[:at], _str_hap(rng, D - 30), t[at - 30:at], t[at:]]))     # (ends in the 30 bases before it: the gap can sit 30 columns further left)
            pairs.append((p, t) if i % 2 == 0 else (t, p))
    elif kind == "edlib":
        for L in EDLIB_LENS:
            hom, di = np.full(L, int(rng.integers(0, 4)), np.uint8), np.tile(np.array([1, 2], np.uint8), L // 2 + 1)[:L]
            pairs.append((hom, hom[:L - 1 - L // 40].copy()))                     # a homopolymer against a shorter one: every gap placement ties
            if L <= 2300:
                q = di.copy(); q[L // 3] = 3
                pairs.append((di, _edit(q, dels=[(L // 2, 1 + L // 60)])))         # a dinucleotide run with a substitution and a deletion
                pairs.append((di, np.tile(np.array([1, 2, 2], np.uint8), L // 3 + 1)[:max(1, L - L // 8)]))     # against a trinucleotide run
    return pairs


def wfa_pairs(penalties=WFA_PENALTIES[0], seed=0):
    """the WFA set of one scoring: tandem-repeat pairs, indels of the scoring's own crossover length, and (default scoring) the long-insertion pairs"""
    return tie_pairs("str", seed, penalties) + tie_pairs("crossover", seed, penalties) + (tie_pairs("wide", seed, penalties) if tuple(penalties) == WFA_PENALTIES[0] else [])


# ---------------------------------------------------------------- the POA case table
# Read sets: name -> (generator, its arguments after rng, seed).  The seeds are the smallest for which the census minimums of tests/test_tie_cases_oracle.py hold
# under every (mode, scoring) the set is used with.  Sizes: a bubble_chain's inserted reads are 3 x crossover bases longer per 225 bases of backbone, so L is
# chosen with the LONGEST read in mind (the planner's classes go by it).
READS = {
    "b190": ("bubble", dict(L=190), 1), "b230": ("bubble", dict(L=230), 2), "b300": ("bubble", dict(L=300), 0), "b380": ("bubble", dict(L=380), 0),
    "b800": ("bubble", dict(L=800), 0), "b900": ("bubble", dict(L=900), 0), "b1200": ("bubble", dict(L=1200), 0), "b1500": ("bubble", dict(L=1500), 0),
    "b1700": ("bubble", dict(L=1700), 0), "b3800": ("bubble", dict(L=3800, n_plain=2), 0), "b7600": ("bubble", dict(L=7600, n_plain=2), 0),
    "b900_150": ("bubble", dict(L=900, indel_len=150), 0),
    "b300_alt": ("bubble", dict(L=300, scoring=ALT_SCORING), 0), "b300_wide": ("bubble", dict(L=300, scoring=WIDE_SCORING), 0),
    "s230": ("str", dict(L=230, n=10, rate=0.05), 0), "s300": ("str", dict(L=300, n=10, rate=0.05), 0), "s470": ("str", dict(L=470, n=8, rate=0.04), 0),
    "s900": ("str", dict(L=900, n=8, rate=0.02), 0), "s1200": ("str", dict(L=1200, n=8, rate=0.04), 0), "s1500": ("str", dict(L=1500, n=8, rate=0.02), 0),
    "s1500_noisy": ("str", dict(L=1500, n=8, rate=0.04), 0), "s1800": ("str", dict(L=1800, n=8, rate=0.02), 0), "s2100": ("str", dict(L=2100, n=6, rate=0.02), 0),
    "s4400": ("str", dict(L=4400, n=6, rate=0.01), 0), "s4700": ("str", dict(L=4700, n=6, rate=0.01), 0), "s9500": ("str", dict(L=9500, n=6, rate=0.01), 0),
}


def _case(name, mode, reads, planned, is_ont=0, scoring=None, env=None, also=()):
    """reads: a key of READS; planned: what chain_plan_cases.probe must report under `env` (a subset of threads / wmax / cert / ring16 / solo); also: further
    environments the GPU test runs the same reads under (each compared with the oracle)"""
    return dict(name=name, mode=mode, reads=reads, gen=READS[reads][0], args=READS[reads][1], is_ont=is_ont, scoring=scoring or {}, env=env or {}, planned=planned,
                also=list(also))


FULL = {"LCD_CERT": "0"}
CERT = {"LCD_CERT": "1"}


def _poa_cases():
    c = []
    # K2, full rows: the class by the longest read + 2 guard columns (<= 254: 64 threads, <= 510: 128, <= 1 022: 256, <= 2 046: 512, <= 4 094: 1 024)
    for b, s, thr, wmax in (("b190", "s230", 64, 256), ("b380", "s470", 128, 512), ("b800", "s900", 256, 1024), ("b1500", "s1800", 512, 2048), ("b1700", "s2100", 1024, 4096)):
        c.append(_case(f"k2_full_bubble_{thr}t", 1, b, dict(threads=thr, wmax=wmax, cert=0), env=FULL))
        c.append(_case(f"k2_full_str_{thr}t", 1, s, dict(threads=thr, wmax=wmax, cert=0), env=FULL))
    # ... and one chain of 6 reads beyond the widest window: column tiles, against the generic rows as well
    c.append(_case("k2_tiles_str_4400", 1, "s4400", dict(threads=1024, wmax=4096, cert=0), env=FULL, also=[dict(FULL, LCD_DBG="8")]))
    # K2, certified band, clean reads (the ring slots of these chains are LCD_CERT_RING = 512 columns wide)
    variants = [dict(CERT, LCD_RING16="0"), dict(CERT, LCD_RING16="2"), dict(CERT, LCD_CERT_SOLO_LEN="200"), dict(CERT, LCD_DBG="16"),
                dict(CERT, LCD_SOLO_RL="1", LCD_SOLO_CYC_MIN="0"), dict(CERT, LCD_SOLO_RL="1", LCD_SOLO_MW="1"), dict(CERT, LCD_DBG="8")]
    lean = dict(threads=64, wmax=512, cert=1, ring16=1, solo=0)
    # (190: every read's intervals fit the 256-column window, the indel reads' ties are decided in the lean rows; 300: all but three; 900: the indel reads take the generic rows)
    for L in (190, 300, 900):
        c.append(_case(f"k2_cert_bubble_{L}", 1, f"b{L}", lean, env=CERT, also=variants))
    for L in (300, 900):
        c.append(_case(f"k2_cert_str_{L}", 1, f"s{L}", lean, env=CERT, also=variants))     # (widest interval 90 and 142 columns: the 124- and the 256-column lean rows)
    c.append(_case("k2_cert_bubble_150base_indels", 1, "b900_150", lean, env=CERT))     # intervals wider than 124 and 256 columns: the wider lean rows, the generic rows
    # ... the classes of the variants that change the plan (one row each: their GPU runs are the `also` environments above)
    c.append(_case("k2_cert_bubble_300_ring32", 1, "b300", dict(threads=64, cert=1, ring16=0, solo=0), env=variants[0]))
    c.append(_case("k2_cert_bubble_300_solo_len", 1, "b300", dict(threads=256, cert=1, ring16=0, solo=3), env=variants[2]))
    c.append(_case("k2_cert_bubble_300_pipeline", 1, "b300", dict(threads=256, cert=1, solo=3), env=variants[4]))
    c.append(_case("k2_cert_bubble_300_four_wavefronts", 1, "b300", dict(threads=256, cert=1, solo=2), env=variants[5]))
    # K2, noisy reads: the band in the systolic rows of the class the reads' length asks for, and LCD_CERT=2 (the single-wavefront band)
    sys_ = {"LCD_CERT_SYS": "1"}
    c.append(_case("k2_ont_sys_bubble_300", 1, "b300", dict(threads=128, cert=2), is_ont=1, env=sys_))
    c.append(_case("k2_ont_sys_str_300", 1, "s300", dict(threads=128, cert=2), is_ont=1, env=sys_))
    c.append(_case("k2_ont_sys_bubble_1200", 1, "b1200", dict(threads=512, cert=2), is_ont=1, env=sys_))
    c.append(_case("k2_ont_sys_str_1200", 1, "s1200", dict(threads=512, cert=2), is_ont=1, env=sys_))
    c.append(_case("k2_ont_cert2_bubble_300", 1, "b300", dict(threads=64, cert=1), is_ont=1, env={"LCD_CERT": "2"}))
    c.append(_case("k2_ont_cert2_str_300", 1, "s300", dict(threads=64, cert=1), is_ont=1, env={"LCD_CERT": "2"}))
    # K1: the window by the longest read (< 1 400: 64 columns, < 4 600: 128, from 4 600: 256), the 128-thread windowed rows from 9 400 bases on
    dbg8 = [{"LCD_DBG": "8"}]
    c.append(_case("k1_bubble_230", 0, "b230", dict(threads=64, wmax=64, cert=0), also=dbg8))
    c.append(_case("k1_str_230", 0, "s230", dict(threads=64, wmax=64, cert=0), also=dbg8))
    c.append(_case("k1_bubble_1500", 0, "b1500", dict(threads=64, wmax=128, cert=0), also=dbg8))
    c.append(_case("k1_str_1500", 0, "s1500", dict(threads=64, wmax=128, cert=0), also=dbg8))
    c.append(_case("k1_bubble_4700", 0, "b3800", dict(threads=64, wmax=256, cert=0)))
    c.append(_case("k1_str_4700", 0, "s4700", dict(threads=64, wmax=256, cert=0)))
    c.append(_case("k1_bubble_9500", 0, "b7600", dict(threads=128, wmax=512, cert=0)))
    c.append(_case("k1_str_9500", 0, "s9500", dict(threads=128, wmax=512, cert=0)))
    # ... noisy reads: eight ring slots (LCD_RING_K), two, and the 256-thread workgroup whose wavefront 0 runs the rows
    ont_k1 = [{"LCD_RING_K": "2"}, {"LCD_SOLO_RL": "1"}]
    c.append(_case("k1_ont_bubble_1500", 0, "b1500", dict(threads=64, wmax=128, cert=0, solo=0), is_ont=1, also=ont_k1))
    c.append(_case("k1_ont_str_1500", 0, "s1500_noisy", dict(threads=64, wmax=128, cert=0, solo=0), is_ont=1, also=ont_k1))
    c.append(_case("k1_ont_bubble_1500_solo", 0, "b1500", dict(threads=256, wmax=128, solo=1), is_ont=1, env=ont_k1[1]))
    # scoring: crossover 22, and match / mismatch outside the lean rows' 6-bit field
    for tag, sc in (("alt", ALT_SCORING), ("wide", WIDE_SCORING)):
        c.append(_case(f"k1_bubble_300_{tag}_scoring", 0, f"b300_{tag}", dict(threads=64, wmax=64, cert=0), scoring=sc))
        c.append(_case(f"k1_str_300_{tag}_scoring", 0, "s300", dict(threads=64, wmax=64, cert=0), scoring=sc))
        c.append(_case(f"k2_bubble_300_{tag}_scoring", 1, f"b300_{tag}", dict(threads=64, wmax=512, cert=1), scoring=sc, env=CERT, also=[FULL]))
        c.append(_case(f"k2_str_300_{tag}_scoring", 1, "s300", dict(threads=64, wmax=512, cert=1), scoring=sc, env=CERT, also=[FULL]))
    return c


POA_CASES = _poa_cases()
_reads, _oracle = {}, {}


def read_set(name, seed=None):
    """the reads of READS[name] (cached)"""
    gen, args, s0 = READS[name]
    seed = s0 if seed is None else seed
    if (name, seed) not in _reads:
        rng = np.random.default_rng(seed)
        _reads[(name, seed)] = bubble_chain(rng, **args) if gen == "bubble" else str_chain(rng, **args)
    return _reads[(name, seed)]


def case_reads(case):
    return read_set(case["reads"])


def oracle_opt(case):
    from oracle import pyoracle
    o = pyoracle.default_opt()
    for k, v in case["scoring"].items():
        setattr(o, k, v)
    return o


def oracle_chain(reads, mode, opt=None):
    """-> (the oracle's K1 (mode 0, every read full-cover) or K2 (mode 1) chain, its tie census)"""
    from oracle import pyoracle
    with pyoracle.poa_tie_census() as tc:
        res = pyoracle.poa_aln_msa_cons(reads, 2, opt) if mode == 1 else pyoracle.poa_partial_aln_msa_cons(reads, [12] * len(reads), opt)
    return res, tc.counts


def case_oracle(case):
    """-> (the oracle's chain for the case, its tie census), computed once per (reads, mode, scoring) and never changed"""
    k = (case["reads"], case["mode"], tuple(sorted(case["scoring"].items())))
    if k not in _oracle:
        _oracle[k] = oracle_chain(case_reads(case), case["mode"], oracle_opt(case))
    return _oracle[k]


def plan_case(case):
    """the chain_plan_cases entry of a POA case: poa_batch plans without a submission around the chain (n_chains = 2^40)"""
    import chain_plan_cases as T
    return T.chain(case["name"], case["mode"], 0, 0, lens=[len(r) for r in case_reads(case)], ont=case["is_ont"], n_chains=1 << 40, opt=dict(case["scoring"]), env=case["env"])
