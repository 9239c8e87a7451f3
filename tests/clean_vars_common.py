"""Shared by the clean-region tests (tests/test_clean_vars_oracle.py, tests/test_gpu_clean_vars.py) and
tools/bench_clean_vars.py: the CPU oracle of lcd_chunk_clean_vars (tests/c/clean_vars_oracle.c, compiled with gcc on first use), seeded chunk generators
built on tests/digar_inputs.py, and the oracle chain from EQX records to its lcd_clean_vars_t."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from digar_inputs import pack4

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SRC = os.path.join(HERE, "c", "clean_vars_oracle.c")
CDIFF, CINS, CDEL, CEQUAL, CSOFT = 8, 1, 2, 7, 4
NON_VAR, LOW_COV, STRAND_BIAS, LOW_AF, HET_SNP, HET_INDEL, REP_HET, HOM = 0x800, 0x001, 0x002, 0x400, 0x004, 0x008, 0x010, 0x080

_lib = None


def oracle_lib():
    """the C oracle, built into a temporary directory once per process"""
    global _lib
    if _lib is None:
        from longcalld_amd._lib import LcdCleanOpt, LcdCleanVars, LcdNoisyIv
        d = tempfile.mkdtemp(prefix="cvo_")
        so = os.path.join(d, "libclean_vars_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, ORACLE_SRC, "-lm"])
        L = C.CDLL(so)
        i32p, i64p, u64p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
        L.cvo_clean_vars.argtypes = [C.POINTER(LcdCleanOpt), C.c_int, i32p, i32p, i64p, i64p, u64p, C.c_void_p, u8p, u64p, u8p, u64p, i32p, u64p,
                                     C.POINTER(LcdNoisyIv), u8p, u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(LcdNoisyIv), C.c_int, i64p, C.c_int,
                                     C.POINTER(LcdCleanVars)]
        L.cvo_clean_vars_free.argtypes = [C.POINTER(LcdCleanVars)]
        L.cvo_cr_merge2.argtypes = [C.POINTER(LcdNoisyIv), C.c_int, C.POINTER(LcdNoisyIv), C.c_int, C.c_int, C.POINTER(C.POINTER(LcdNoisyIv))]
        L.cvo_fisher_exact_test.argtypes = [C.c_int] * 4
        L.cvo_fisher_exact_test.restype = C.c_double
        _lib = L
    return _lib


def default_opt(is_ont=0, **kw):
    """lcd_clean_opt_t defaults (src/call_var_main.c), filled on the Python side: the non-GPU tests do not load the HIP library's options"""
    from longcalld_amd._lib import LcdCleanOpt
    o = LcdCleanOpt(5, 2, 10, 30, 5, 10, 500, int(is_ont), 0, 0.20, 0.80, 0.01)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ivs(rows):
    from longcalld_amd._lib import LcdNoisyIv
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    return (LcdNoisyIv * max(1, len(rows)))(*[LcdNoisyIv(int(r[0]), int(r[1]), int(r[2]), 0) for r in rows]), len(rows)


def cr_merge2(a, b, fixed_win=-1):
    """the oracle's cr_merge2 of two interval lists (k,3) in index order -> (m,3)"""
    L = oracle_lib()
    from longcalld_amd._lib import LcdNoisyIv
    pa, na = _ivs(a); pb, nb = _ivs(b)
    out = C.POINTER(LcdNoisyIv)()
    n = L.cvo_cr_merge2(pa, na, pb, nb, int(fixed_win), C.byref(out))
    res = np.array([(out[i].start, out[i].end, out[i].label) for i in range(n)], np.int64).reshape(-1, 3)
    C.CDLL(None).free(C.cast(out, C.c_void_p))
    return res


# ---------------- a chunk: records (EQX CIGARs) + the oracle's digars ----------------
def read_digars(ch, oracle, is_ont=0):
    """collect_digar_from_eqx_cigar (oracle/digar.c) for every record of the chunk -> per read dict(rc, digars, noisy, beg, end)"""
    opt = oracle.digar_opt(is_ont)
    return [oracle.collect_digar_from_eqx_cigar(r["pos0"], r["cigar"], r["qual"], ch["reg_beg"], ch["reg_end"], ch["whole_ref_len"], opt=opt) for r in ch["reads"]]


def run_oracle(ch, digs, opt, pre_regs=(), low_comp=(), ordered=None, call_only=False):
    """cvo_clean_vars on the chunk's records and their digars -> clean_vars_dict (call_only: the bare C call, f(out) -> rc, for timing)"""
    from longcalld_amd._lib import LcdCleanVars, LcdDigar
    from longcalld_amd.align import clean_vars_dict
    L = oracle_lib()
    reads = ch["reads"]; n = len(reads)
    ordered = np.ascontiguousarray(np.arange(n) if ordered is None else ordered, np.int32)
    status = np.array([d["rc"] for d in digs] + [0], np.int32)
    beg = np.array([d["beg"] for d in digs] + [0], np.int64); end = np.array([d["end"] for d in digs] + [0], np.int64)
    doff = np.concatenate([[0], np.cumsum([len(d["digars"]) for d in digs])]).astype(np.uint64)
    allg = np.concatenate([d["digars"] for d in digs] + [np.zeros((1, 5), np.int64)])
    dg = (LcdDigar * len(allg))(*[LcdDigar(int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[4])) for x in allg])
    seqs = [np.ascontiguousarray(r["bseq"], np.uint8) for r in reads]; quals = [np.ascontiguousarray(r["qual"], np.uint8) for r in reads]
    soff = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.uint64); qoff = np.concatenate([[0], np.cumsum([len(x) for x in quals])]).astype(np.uint64)
    spool = np.concatenate(seqs + [np.zeros(2, np.uint8)]); qpool = np.concatenate(quals + [np.zeros(2, np.uint8)])
    qlen = np.array([len(x) for x in quals] + [0], np.int32)
    ivoff = np.concatenate([[0], np.cumsum([len(d["noisy"]) for d in digs])]).astype(np.uint64)
    ivs, _ = _ivs(np.concatenate([d["noisy"].reshape(-1, 3) for d in digs] + [np.zeros((0, 3), np.int64)]))
    rev = np.array([r["is_rev"] for r in reads] + [0], np.uint8)
    ref = np.ascontiguousarray(ch["ref"], np.uint8)
    pre, npre = _ivs(pre_regs)
    low = np.ascontiguousarray(np.asarray(low_comp, np.int64).reshape(-1)); low = low if low.size else np.zeros(2, np.int64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    def call(out):
        return L.cvo_clean_vars(C.byref(opt), n, P(ordered, C.c_int), P(status, C.c_int), P(beg, C.c_int64), P(end, C.c_int64), P(doff, C.c_uint64), C.cast(dg, C.c_void_p),
                          P(spool, C.c_uint8), P(soff, C.c_uint64), P(qpool, C.c_uint8), P(qoff, C.c_uint64), P(qlen, C.c_int), P(ivoff, C.c_uint64), ivs,
                          P(rev, C.c_uint8), P(ref, C.c_uint8), int(ch["ref_beg"]), int(ch["ref_beg"]) + len(ref) - 1, int(ch["reg_beg"]), int(ch["reg_end"]),
                              pre, npre, P(low, C.c_int64), len(np.asarray(low_comp).reshape(-1)) // 2, C.byref(out))
    if call_only:
        return call
    out = LcdCleanVars()
    rc = call(out)
    assert rc == 0, rc
    res = clean_vars_dict(out)
    L.cvo_clean_vars_free(C.byref(out))
    return res


def same_clean_vars(a, b, fields=None):
    from longcalld_amd.align import CLEAN_VARS_FIELDS
    assert a["n_vars"] == b["n_vars"], (a["n_vars"], b["n_vars"])
    for k in fields or CLEAN_VARS_FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x == y).all(), (k, x.shape, y.shape, np.flatnonzero(x.reshape(-1) != y.reshape(-1))[:10] if x.shape == y.shape else None)


# ---------------- records ----------------
def record(pos0, ops, seq, qual, is_rev=0):
    """one read: 0-based pos0, EQX operations [(op, len)], bases (codes 0-4) and qualities"""
    seq = np.asarray(seq, np.uint8)
    assert sum(l for o, l in ops if o in (7, 8, 1, 4)) == len(seq) == len(qual)
    return dict(pos0=int(pos0), cigar=np.array([(l << 4) | o for o, l in ops], np.uint32), bseq=pack4(seq), seq=seq, qual=np.asarray(qual, np.uint8),
                is_rev=int(is_rev))


def read_from_hap(ref, pos0, length, events, rng=None, err=0.0, qual=None, lowq=0.0):
    """a read of `length` reference bases from 0-based pos0 that carries `events` {0-based ref pos: (op, payload)} -- ('X', base), ('I', codes) inserted
    before that base, ('D', n) -- plus random errors at rate err; qualities 30-40 with a fraction lowq below 10.  Leading / trailing indels are dropped."""
    ops, seq = [], []
    def push(o, l, bases=()):
        if ops and ops[-1][0] == o and o != 1:
            ops[-1] = (o, ops[-1][1] + l)
        else:
            ops.append((o, l))
        seq.extend(bases)
    p, end = pos0, min(len(ref), pos0 + length)
    while p < end:
        ev = events.get(p)
        if ev is None and rng is not None and err > 0 and rng.random() < err:
            k = rng.random()
            ev = ("X", int((ref[p] + rng.integers(1, 4)) % 4)) if k < 0.5 else ("I", [int(rng.integers(0, 4))]) if k < 0.75 else ("D", 1)
        if ev is None:
            push(7, 1, [int(ref[p])]); p += 1
        elif ev[0] == "X":
            push(8, 1, [ev[1]]); p += 1
        elif ev[0] == "I":
            push(1, len(ev[1]), list(ev[1])); push(7, 1, [int(ref[p])]); p += 1
        else:
            push(2, min(ev[1], end - p)); p += ev[1]
    while ops and ops[0][0] in (1, 2):
        o, l = ops.pop(0)
        if o == 1:
            del seq[:l]
        else:
            pos0 += l
    while ops and ops[-1][0] in (1, 2):
        o, l = ops.pop()
        if o == 1:
            del seq[len(seq) - l:]
    if rng is not None:
        q = rng.integers(30, 41, len(seq)).astype(np.uint8)
        if lowq > 0:
            q[rng.random(len(seq)) < lowq] = rng.integers(2, 10)
    else:
        q = np.full(len(seq), 30 if qual is None else qual, np.uint8)
    return record(pos0, ops, seq, q)


def make_diploid_chunk(seed, ref_len=30000, depth=16, read_len=(2000, 6000), is_ont=0, err=0.001, lowq=0.003, n_bias=0, reg_pad=200):
    """seeded diploid chunk: het / hom SNPs and indels, homopolymer and tandem-repeat blocks with indels in them, SV-size insertions (a family of similar lengths),
    both strands, random errors and low-quality bases; ONT: n_bias SNPs carried by every reverse-strand read and no forward one"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, ref_len).astype(np.uint8)
    for b in rng.integers(500, ref_len - 500, ref_len // 1500):         # homopolymers
        ref[b:b + int(rng.integers(6, 14))] = rng.integers(0, 4)
    for b in rng.integers(500, ref_len - 500, ref_len // 2000):         # tandem repeats
        unit = rng.integers(0, 4, int(rng.integers(2, 4)))
        k = int(rng.integers(4, 8))
        ref[b:b + k * len(unit)] = np.tile(unit, k)
    haps = [dict(), dict()]
    for p in np.sort(rng.choice(np.arange(300, ref_len - 300), ref_len // 400, replace=False)):
        p = int(p)
        k = rng.random()
        ev = ("X", int((ref[p] + rng.integers(1, 4)) % 4)) if k < 0.6 else ("I", rng.integers(0, 4, int(rng.integers(1, 4))).tolist()) if k < 0.75 else \
            ("D", int(rng.integers(1, 4))) if k < 0.92 else ("I", rng.integers(0, 4, int(rng.integers(30, 60))).tolist())
        z = rng.random()
        for h in ((0,) if z < 0.4 else (1,) if z < 0.8 else (0, 1)):
            haps[h][p] = ev
    bias = {}
    for p in rng.choice(np.arange(300, ref_len - 300), n_bias, replace=False):
        if int(p) not in haps[0] and int(p) not in haps[1]:
            bias[int(p)] = ("X", int((ref[int(p)] + 1) % 4))
    reads = []
    n_reads = int(depth * ref_len / np.mean(read_len))
    for s in np.sort(rng.integers(0, ref_len - read_len[0], n_reads)):
        h = int(rng.integers(0, 2)); rev = int(rng.integers(0, 2))
        ev = dict(haps[h])
        if rev:
            ev.update(bias)
        r = read_from_hap(ref, int(s), int(rng.integers(*read_len)), ev, rng=rng, err=err, lowq=lowq)
        r["is_rev"] = rev
        r["hap"] = h + 1
        reads.append(r)
    order = np.argsort([r["pos0"] for r in reads], kind="stable")
    reads = [reads[i] for i in order]
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=reg_pad, reg_end=ref_len - reg_pad, whole_ref_len=ref_len, is_ont=is_ont)


def chunk_inputs(ch, digs):
    """pre_process_noisy_regs' inputs from the oracle's digars: the chunk-noisy windows in cr_add order, per-read beg / end / windows (skipped reads left out)"""
    keep = [i for i, d in enumerate(digs) if d["rc"] != -1]
    chunk_noisy = np.concatenate([digs[i]["chunk_noisy"].reshape(-1, 3) for i in keep] + [np.zeros((0, 3), np.int64)])
    return dict(chunk_noisy=chunk_noisy, read_beg=[digs[i]["beg"] for i in keep], read_end=[digs[i]["end"] for i in keep],
                read_ivs=[digs[i]["noisy"].reshape(-1, 3) for i in keep])


def events_chunk(path=None):
    """the real HG002 chunk of tests/golden/testdata_events.npz (tests/golden/make_events_fixture.py) rebuilt as records: '=' bases from the reference slice,
    X / I bases and the qualities the digar code reads from the fixture, soft clips N, other qualities 30.  Region = the reads' span."""
    z = np.load(path or os.path.join(HERE, "golden", "testdata_events.npz"))
    ref, rb = z["ref"], int(z["ref_beg"])
    reads = []
    for i in range(len(z["pos0"])):
        cig = z["cigar"][z["cigar_off"][i]:z["cigar_off"][i + 1]]
        es = z["ev_seq"][z["ev_off"][i]:z["ev_off"][i + 1]]; eq = z["ev_qual"][z["ev_off"][i]:z["ev_off"][i + 1]]
        dq = z["del_qual"][2 * z["del_off"][i]:2 * z["del_off"][i + 1]]
        qlen = sum(int(c >> 4) for c in cig if int(c & 0xf) in (7, 8, 1, 4))
        seq = np.full(qlen, 4, np.uint8); qual = np.full(qlen, 30, np.uint8)
        pos, qi, e, d = int(z["pos0"][i]) + 1, 0, 0, 0
        for c in cig:
            op, ln = int(c & 0xf), int(c >> 4)
            if op == 7:
                seq[qi:qi + ln] = ref[pos - rb:pos - rb + ln]
            elif op in (8, 1):
                seq[qi:qi + ln] = es[e:e + ln]; qual[qi:qi + ln] = eq[e:e + ln]; e += ln
            elif op == 2:
                if qi > 0:
                    qual[qi - 1] = dq[2 * d]
                if qi < qlen:
                    qual[qi] = dq[2 * d + 1]
                d += 1
            if op in (7, 8, 2, 3):
                pos += ln
            if op in (7, 8, 1, 4):
                qi += ln
        reads.append(dict(pos0=int(z["pos0"][i]), cigar=cig.astype(np.uint32), bseq=pack4(seq), seq=seq, qual=qual, is_rev=int(z["flag"][i] & 0x10 != 0), end=pos - 1))
    return dict(reads=reads, ref=ref, ref_beg=rb, reg_beg=min(r["pos0"] for r in reads) + 1, reg_end=max(r["end"] for r in reads),
                whole_ref_len=int(z["whole_ref_len"]), is_ont=0)
