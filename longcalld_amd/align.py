"""Host-side mirror of the reference's src/align.h surface over the C ABI (liblcd_hotpath.so).

Function names and argument meaning follow the reference (src/align.c); arrays are numpy uint8 byte codes
A0 C1 G2 T3 N4, gap 5.  Everything here calls the HIP library -- nothing is computed in Python.
"""
import ctypes as C

import numpy as np

from ._lib import (LcdAlnStr, LcdBatchStats, LcdCleanOpt, LcdCleanVars, LcdDigar, LcdDigar1, LcdDigarOpt, LcdError, LcdNoisyIv, LcdNoisyVar, LcdOpt, LcdReadView, check,
                   load_library)

_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]

u8p, i32p, u64p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

GAP_LEFT_ALN, GAP_RIGHT_ALN = 1, 2  # src/align.h:28-29
WFA_NO_HEURISTIC, WFA_AFFINE_2P = 0, 1  # src/align.h:35-40
NOISY_RIGHT_GAP, NOISY_LEFT_GAP, NOISY_RIGHT_COVER, NOISY_LEFT_COVER, NOISY_BOTH_COVER = 1, 2, 4, 8, 12  # src/align.h:6-11


def default_opt():
    lib = load_library()
    o = LcdOpt()
    lib.lcd_opt_default(C.byref(o))
    return o


def _p8(a):
    return a.ctypes.data_as(u8p)


def _pool(arrays):
    """pack byte arrays into one pool, 16-byte aligned; returns pool, offsets"""
    offs, tot = [], 0
    for a in arrays:
        offs.append(tot)
        tot += (len(a) + 15) // 16 * 16
    pool = np.full(tot + 16, 4, np.uint8)
    for a, o in zip(arrays, offs):
        pool[o:o + len(a)] = a
    return pool, np.array(offs, np.uint64)


def edlib_batch(pairs):
    """pairs: list of (target, query) uint8 arrays -> dict of int arrays dist/xgaps/n_eq/n_xid  (src/align.c:210-254)."""
    lib = load_library()
    n = len(pairs)
    arrs = [np.ascontiguousarray(x, np.uint8) for p in pairs for x in (p[1], p[0])]  # query, target
    pool, offs = _pool(arrs)
    qo, to = np.ascontiguousarray(offs[0::2]), np.ascontiguousarray(offs[1::2])
    ql = np.array([len(p[1]) for p in pairs], np.int32)
    tl = np.array([len(p[0]) for p in pairs], np.int32)
    out = {k: np.zeros(n, np.int32) for k in ("dist", "xgaps", "n_eq", "n_xid")}
    check(lib.lcd_edlib_batch(n, _p8(pool), pool.size, qo.ctypes.data_as(u64p), ql.ctypes.data_as(i32p), to.ctypes.data_as(u64p),
                              tl.ctypes.data_as(i32p), *[out[k].ctypes.data_as(i32p) for k in ("dist", "xgaps", "n_eq", "n_xid")]), lib)
    return out


def edlib_batch_hw(pairs):
    """HW (infix) mode, edlib_infix_aln (src/align.c:256): pairs of (target, query) -> dict of int arrays dist/xgaps/n_eq/n_xid/start/end"""
    lib = load_library()
    n = len(pairs)
    arrs = [np.ascontiguousarray(x, np.uint8) for p in pairs for x in (p[1], p[0])]  # query, target
    pool, offs = _pool(arrs)
    qo, to = np.ascontiguousarray(offs[0::2]), np.ascontiguousarray(offs[1::2])
    ql = np.array([len(p[1]) for p in pairs], np.int32)
    tl = np.array([len(p[0]) for p in pairs], np.int32)
    keys = ("dist", "xgaps", "n_eq", "n_xid", "start", "end")
    out = {k: np.zeros(n, np.int32) for k in keys}
    check(lib.lcd_edlib_batch_hw(n, _p8(pool), pool.size, qo.ctypes.data_as(u64p), ql.ctypes.data_as(i32p), to.ctypes.data_as(u64p),
                                 tl.ctypes.data_as(i32p), *[out[k].ctypes.data_as(i32p) for k in keys]), lib)
    return out


def edlib_infix_aln(target, query):
    """edlib_infix_aln, src/align.c:256 -> (distance, n_eq, n_xid) through the per-call export"""
    lib = load_library()
    t, q = np.ascontiguousarray(target, np.uint8), np.ascontiguousarray(query, np.uint8)
    a, b = C.c_int(), C.c_int()
    d = lib.lcd_edlib_infix_aln(_p8(t), len(t), _p8(q), len(q), C.byref(a), C.byref(b))
    return d, a.value, b.value


def edlib_xgaps(target, query):
    """edlib_xgaps, src/align.c:222"""
    return int(edlib_batch([(target, query)])["xgaps"][0])


def edlib_end2end_aln(target, query):
    """edlib_end2end_aln, src/align.c:234 -> (distance, n_eq, n_xid)"""
    r = edlib_batch([(target, query)])
    return int(r["dist"][0]), int(r["n_eq"][0]), int(r["n_xid"][0])


def wfa_batch(pairs, gap_aln=GAP_LEFT_ALN, b=6, q=6, e=2, q2=24, e2=1):
    """pairs: list of (pattern, text) -> list of dict(score, cigar[uint32], pattern_alg, text_alg)  (src/align.c:374-460)."""
    lib = load_library()
    n = len(pairs)
    arrs = [np.ascontiguousarray(x, np.uint8) for p in pairs for x in (p[0], p[1])]
    pool, offs = _pool(arrs)
    po, to = np.ascontiguousarray(offs[0::2]), np.ascontiguousarray(offs[1::2])
    pl = np.array([len(p[0]) for p in pairs], np.int32)
    tl = np.array([len(p[1]) for p in pairs], np.int32)
    ga = np.full(n, gap_aln, np.int32) if np.isscalar(gap_aln) else np.asarray(gap_aln, np.int32)
    stride = int((pl + tl).max()) + 1 if n else 1
    score, ncig, alen = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    cig = np.zeros((n, stride), np.uint32)
    rows = np.zeros((n, 2, stride), np.uint8)
    check(lib.lcd_wfa_batch(n, _p8(pool), pool.size, po.ctypes.data_as(u64p), pl.ctypes.data_as(i32p), to.ctypes.data_as(u64p),
                            tl.ctypes.data_as(i32p), ga.ctypes.data_as(i32p), b, q, e, q2, e2, 3, score.ctypes.data_as(i32p),
                            cig.ctypes.data_as(u32p), stride, ncig.ctypes.data_as(i32p), _p8(rows), stride, alen.ctypes.data_as(i32p)), lib)
    return [dict(score=int(score[i]), cigar=cig[i, :ncig[i]].copy(), pattern_alg=rows[i, 0, :alen[i]].copy(), text_alg=rows[i, 1, :alen[i]].copy())
            for i in range(n)]


def wfa_arena_bytes(plen, tlen, score_bound, b=6, q=6, e=2, q2=24, e2=1):
    """device work-arena bytes of one K3 alignment with the given score bound (lcd_wfa_arena_bytes)"""
    return int(load_library().lcd_wfa_arena_bytes(int(plen), int(tlen), int(score_bound), b, q, e, q2, e2))


def wfa_end2end_aln(pattern, text, gap_aln=GAP_LEFT_ALN, b=6, q=6, e=2, q2=24, e2=1):
    """wfa_end2end_aln through the per-call C mirror (exercises the malloc/ownership contract, src/align.c:374)."""
    lib = load_library()
    pattern = np.ascontiguousarray(pattern, np.uint8)
    text = np.ascontiguousarray(text, np.uint8)
    cb, cl, pa, ta, al = u32p(), C.c_int(), u8p(), u8p(), C.c_int()
    check(lib.lcd_wfa_end2end_aln(_p8(pattern), len(pattern), _p8(text), len(text), gap_aln, b, q, e, q2, e2, WFA_NO_HEURISTIC, WFA_AFFINE_2P,
                                  C.byref(cb), C.byref(cl), C.byref(pa), C.byref(ta), C.byref(al)), lib)
    cigar = np.ctypeslib.as_array(cb, shape=(max(cl.value, 1),))[:cl.value].copy()
    p_alg = np.ctypeslib.as_array(pa, shape=(max(al.value, 1),))[:al.value].copy()
    t_alg = np.ctypeslib.as_array(ta, shape=(max(al.value, 1),))[:al.value].copy()
    _libc.free(cb)
    _libc.free(pa)  # one block: only the first pointer is freed (src/align.c:490)
    return cigar, p_alg, t_alg


def poa_batch(chains, opt=None):
    """chains: list of dict(mode, reads=[uint8 arrays], skip=[...], anchors=[(ref_beg, ref_end, read_beg, read_end)]) -> list of dict."""
    lib = load_library()
    opt = opt or default_opt()
    reads = [np.ascontiguousarray(r, np.uint8) for ch in chains for r in ch["reads"]]
    pool, offs = _pool(reads)
    lens = np.array([len(r) for r in reads], np.int32)
    nC = len(chains)
    mode = np.array([ch["mode"] for ch in chains], np.int32)
    nr = np.array([len(ch["reads"]) for ch in chains], np.int32)
    r0 = np.concatenate([[0], np.cumsum(nr)[:-1]]).astype(np.int32)
    skip = np.array([s for ch in chains for s in ch.get("skip", [0] * len(ch["reads"]))], np.int32)
    anch = []
    for ch in chains:
        a = ch.get("anchors")
        for k, r in enumerate(ch["reads"]):
            anch.extend(a[k] if a is not None else (1, len(ch["reads"][0]), 1, len(r)))
    anch = np.array(anch, np.int32)
    max_reads = int(nr.max())
    stride = int(max(sum(len(r) for r in ch["reads"]) for ch in chains)) + 2
    status, n_cons, msa_len = np.zeros(nC, np.int32), np.zeros(nC, np.int32), np.zeros(nC, np.int32)
    cons_len, clu_n = np.zeros((nC, 2), np.int32), np.zeros((nC, 2), np.int32)
    cons = np.zeros((nC, 2, stride), np.uint8)
    msa = np.zeros((nC, max_reads + 2, stride), np.uint8)
    clu_ids = np.zeros((nC, 2, max_reads), np.int32)
    check(lib.lcd_poa_batch(C.byref(opt), nC, mode.ctypes.data_as(i32p), r0.ctypes.data_as(i32p), nr.ctypes.data_as(i32p), len(reads),
                            offs.ctypes.data_as(u64p), lens.ctypes.data_as(i32p), skip.ctypes.data_as(i32p), anch.ctypes.data_as(i32p),
                            _p8(pool), pool.size, status.ctypes.data_as(i32p), n_cons.ctypes.data_as(i32p), cons_len.ctypes.data_as(i32p),
                            msa_len.ctypes.data_as(i32p), clu_n.ctypes.data_as(i32p), _p8(cons), stride, _p8(msa), stride, max_reads,
                            clu_ids.ctypes.data_as(i32p)), lib)
    out = []
    for c in range(nC):
        nc = int(n_cons[c])
        out.append(dict(status=int(status[c]), n_cons=nc, msa_len=int(msa_len[c]),
                        cons=[cons[c, k, :cons_len[c, k]].copy() for k in range(nc)],
                        msa=[msa[c, r, :msa_len[c]].copy() for r in range(int(nr[c]) + nc)],
                        clu=[clu_ids[c, k, :clu_n[c, k]].copy() for k in range(nc)]))
    return out


DEVICE_ANY = -2  # LCD_DEVICE_ANY: a host-only job buffer, bound to a GPU at upload / dispatch time


def lpt_assign(costs, n_bins):
    """lcd_lpt_assign: longest-processing-time assignment -> (bin of every item, load per bin); pure host code (no GPU needed)"""
    lib = load_library()
    c = np.ascontiguousarray(costs, np.float64)
    out = np.zeros(max(len(c), 1), np.int32); load = np.zeros(max(n_bins, 1), np.float64)
    lib.lcd_lpt_assign(len(c), c.ctypes.data_as(C.POINTER(C.c_double)), int(n_bins), out.ctypes.data_as(i32p), load.ctypes.data_as(C.POINTER(C.c_double)))
    return out[:len(c)].copy(), load[:n_bins].copy()


class Dispatcher:
    """lcd_dispatch_*: one process driving every GPU of the node -- per-device submitter threads pulling job buffers from one cost-ordered queue
    (the GPU-side analogue of kt_for, src/kthread.c:24-64)"""

    def __init__(self, devices=None, coalesce=16):
        self.lib = load_library()
        if devices is None:
            self.h = self.lib.lcd_dispatch_create(0, None, int(coalesce))
        else:
            d = np.ascontiguousarray(devices, np.int32)
            self.h = self.lib.lcd_dispatch_create(len(d), d.ctypes.data_as(i32p), int(coalesce))
        if not self.h:
            raise RuntimeError("lcd_dispatch_create failed: " + self.lib.lcd_last_error().decode())

    @property
    def n_devices(self):
        return int(self.lib.lcd_dispatch_n_devices(self.h))

    def run(self, batches):
        """uploads, runs and downloads every batch; returns the device each batch ran on"""
        arr = (C.c_void_p * len(batches))(*[b.h for b in batches])
        dev = np.full(max(len(batches), 1), -1, np.int32)
        check(self.lib.lcd_dispatch_run(self.h, arr, len(batches), dev.ctypes.data_as(i32p)), self.lib)
        return dev[:len(batches)].copy()

    def set_flags(self, flags):
        """bit 0: leave the results on the device (no download after a submission)"""
        self.lib.lcd_dispatch_set_flags.argtypes = [C.c_void_p, C.c_int]
        self.lib.lcd_dispatch_set_flags(self.h, int(flags))

    def busy(self):
        """-> (ms inside submissions, #submissions) per device of the dispatcher, for the last run()"""
        n = self.n_devices
        ms = np.zeros(max(n, 1), np.float64); ns = np.zeros(max(n, 1), np.int32)
        self.lib.lcd_dispatch_busy.argtypes = [C.c_void_p, C.POINTER(C.c_double), i32p]
        self.lib.lcd_dispatch_busy(self.h, ms.ctypes.data_as(C.POINTER(C.c_double)), ns.ctypes.data_as(i32p))
        return ms[:n].copy(), ns[:n].copy()

    def close(self):
        if self.h:
            self.lib.lcd_dispatch_destroy(self.h)
            self.h = None


class RegionBatch:
    """Batched collect_noisy_reg_aln_strs (src/align.c:1760) over many independent regions of one pass (SURVEY CS-2)."""

    def __init__(self, opt=None, device=-1):
        """device: the GPU this batch lives on (lcd_batch_create_on); -1 = the calling thread's / process default device"""
        self.lib = load_library()
        self.opt = opt or default_opt()
        self.h = self.lib.lcd_batch_create_on(C.byref(self.opt), int(device))
        if not self.h:
            raise RuntimeError("lcd_batch_create failed: " + self.lib.lcd_last_error().decode())
        self.n_reads = []
        self._keep = []

    def close(self):
        if self.h:
            self.lib.lcd_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        self.lib.lcd_batch_clear(self.h)
        self.n_reads = []

    def add_region(self, reg):
        """reg: dict(reg_len, read_ids, seqs, quals(optional), covers, haps, phase_sets, ref) -- the outputs of collect_noisy_read_info"""
        n = len(reg["seqs"])
        seqs = [np.ascontiguousarray(s, np.uint8) for s in reg["seqs"]]
        quals = reg.get("quals")
        quals = [np.ascontiguousarray(s, np.uint8) for s in quals] if quals is not None else [np.zeros(max(len(s), 1), np.uint8) for s in seqs]
        sp = (u8p * n)(*[_p8(s) for s in seqs])
        qp = (u8p * n)(*[_p8(s) for s in quals])
        ids = np.asarray(reg["read_ids"], np.int32)
        lens = np.array([len(s) for s in seqs], np.int32)
        cov = np.asarray(reg["covers"], np.int32)
        haps = np.asarray(reg["haps"], np.int32)
        pss = np.asarray(reg["phase_sets"], np.int64)
        ref = np.ascontiguousarray(reg["ref"], np.uint8)
        idx = check(self.lib.lcd_batch_add_region(self.h, int(reg["reg_len"]), n, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sp, qp,
                                                  cov.ctypes.data_as(i32p), haps.ctypes.data_as(i32p), pss.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  _p8(ref), len(ref)), self.lib)
        self.n_reads.append(n)
        return idx

    def add_region_from_chunk(self, views, reg_beg, reg_end, noisy_reads, ref_slice, packed=False):
        """region [reg_beg, reg_end] (1-based, flanks included) of a chunk whose reads are `views` (make_read_views): the digar walk of
        collect_noisy_read_info (src/align.c:1377-1461) runs inside the library; noisy_reads = chunk read ids overlapping the region.
        packed: the reads' bases stay 4-bit packed on the host and are unpacked on the device by upload() (lcd_batch_add_region_from_chunk_packed)"""
        ids = np.ascontiguousarray(noisy_reads, np.int32)
        ref = np.ascontiguousarray(ref_slice, np.uint8)
        fn = self.lib.lcd_batch_add_region_from_chunk_packed if packed else self.lib.lcd_batch_add_region_from_chunk
        idx = check(fn(self.h, views[0], int(reg_beg), int(reg_end), len(ids), ids.ctypes.data_as(i32p), _p8(ref), len(ref)), self.lib)
        self.n_reads.append(len(ids))
        return idx

    def read_slices(self, region):
        """-> dict(read_ids, covers, read_beg, read_end) of a region's reads in sorted order (lcd_batch_region_read_slices)"""
        n = max(self.n_reads[region], 1)
        ids, cov, rb, re = (np.zeros(n, np.int32) for _ in range(4))
        k = check(self.lib.lcd_batch_region_read_slices(self.h, region, ids.ctypes.data_as(i32p), cov.ctypes.data_as(i32p), rb.ctypes.data_as(i32p), re.ctypes.data_as(i32p)), self.lib)
        return dict(read_ids=ids[:k].copy(), covers=cov[:k].copy(), read_beg=rb[:k].copy(), read_end=re[:k].copy())

    def cost(self):
        """the work estimate queues and shards are ordered by (DP cells of the batch's chains; host only)"""
        return float(self.lib.lcd_batch_cost(self.h))

    def upload(self):
        check(self.lib.lcd_batch_upload(self.h), self.lib)

    def run(self):
        check(self.lib.lcd_batch_run(self.h), self.lib)

    @staticmethod
    def run_many(batches):
        """lcd_batch_run_many: the hot path of several uploaded batches as ONE set of launches per stage (batches[0] leads)"""
        if not batches:
            return
        arr = (C.c_void_p * len(batches))(*[b.h for b in batches])
        check(batches[0].lib.lcd_batch_run_many(arr, len(batches)), batches[0].lib)

    def download(self):
        check(self.lib.lcd_batch_download(self.h), self.lib)

    def k4_pairs(self):
        """the (target, query) pairs of the batch's K4 jobs (lcd_batch_k4_jobs), copied out of the host pool"""
        n = self.lib.lcd_batch_k4_jobs(self.h, 0, None, None, None, None, None, None)
        if n <= 0:
            return []
        to, qo = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        tl, ql = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pool, plen = u8p(), C.c_uint64(0)
        self.lib.lcd_batch_k4_jobs(self.h, n, to.ctypes.data_as(u64p), tl.ctypes.data_as(i32p), qo.ctypes.data_as(u64p), ql.ctypes.data_as(i32p),
                                   C.byref(pool), C.byref(plen))
        h = np.ctypeslib.as_array(pool, shape=(plen.value,))
        return [(h[int(to[i]):int(to[i]) + int(tl[i])].copy(), h[int(qo[i]):int(qo[i]) + int(ql[i])].copy()) for i in range(n)]

    def stats(self):
        st = LcdBatchStats()
        self.lib.lcd_batch_get_stats(self.h, C.byref(st))
        return {f[0]: getattr(st, f[0]) for f in LcdBatchStats._fields_}

    def digest(self):
        return int(self.lib.lcd_batch_digest(self.h))

    def materialize(self):
        """every region's results as the per-call mirror returns them (malloc()'d), freed again -> bytes of alignment rows"""
        return int(self.lib.lcd_batch_materialize(self.h))

    def sorted_ids(self, region):
        out = np.zeros(max(self.n_reads[region], 1), np.int32)
        n = self.lib.lcd_batch_region_sorted_ids(self.h, region, out.ctypes.data_as(i32p))
        return out[:n].copy()

    def region_vars(self, region, noisy_reg_beg, chunk_ref, chunk_ref_beg):
        """make_vars_from_msa_cons_aln (src/collect_var.c:2279) of one region, computed in stage S6 (opt.collect_noisy_vars):
        -> dict(n_vars, per-variant arrays, alle_covs (n, 2), alt_seqs, row_read_ids, prof_start, prof_end, prof_alleles (rows x n))"""
        cref = np.ascontiguousarray(chunk_ref, np.uint8)
        vp = C.POINTER(LcdNoisyVar)(); nrows = C.c_int(0)
        ids, ps, pe, pa = i32p(), i32p(), i32p(), i32p()
        n = check(self.lib.lcd_batch_region_vars(self.h, region, int(noisy_reg_beg), _p8(cref), int(chunk_ref_beg), len(cref), C.byref(vp), C.byref(nrows),
                                                 C.byref(ids), C.byref(ps), C.byref(pe), C.byref(pa)), self.lib)
        rows = nrows.value
        out = dict(n_vars=n, n_rows=rows)
        for k in ("pos", "var_type", "ref_len", "alt_len", "cate", "from_cons", "is_homopolymer_indel", "ref_base", "alt_ref_base", "total_cov"):
            out[k] = np.array([getattr(vp[i], k) for i in range(n)], np.int64)
        out["alle_covs"] = np.array([[vp[i].alle_covs[0], vp[i].alle_covs[1]] for i in range(n)], np.int32).reshape(n, 2)
        out["alt_seqs"] = [np.array([vp[i].alt_seq[k] for k in range(vp[i].alt_len)], np.uint8) for i in range(n)]
        as_arr = lambda p, m: np.ctypeslib.as_array(p, shape=(max(m, 1),))[:m].copy() if p else np.zeros(0, np.int32)
        out["row_read_ids"] = as_arr(ids, rows); out["prof_start"] = as_arr(ps, rows); out["prof_end"] = as_arr(pe, rows)
        out["prof_alleles"] = as_arr(pa, rows * n).reshape(rows, n)
        for i in range(n):
            if vp[i].alt_seq:
                _libc.free(C.cast(vp[i].alt_seq, C.c_void_p))
        for p in (vp, ids, ps, pe, pa):
            if p:
                _libc.free(C.cast(p, C.c_void_p))
        return out

    def n_cons(self, region):
        """lcd_batch_region_n_cons: 0 = the region could not be resolved (works with opt.collect_noisy_vars == 2, where result() does not)"""
        return check(self.lib.lcd_batch_region_n_cons(self.h, int(region)), self.lib)

    def add_planned(self, chunk, plan, haps, phase_sets, ref, ref_beg):
        """lcd_batch_add_planned: every LCD_PLAN_SUBMIT region of a plan (plan_pass) of DeviceChunk `chunk`; haps / phase_sets per chunk read, ref = the chunk's
        reference codes starting at ref_beg -> batch index per region of the plan (-1: not submitted)"""
        keep = []
        pl = _pass_plan_struct(plan, keep)
        hp = np.ascontiguousarray(haps, np.int32); ps = np.ascontiguousarray(phase_sets, np.int64); rf = np.ascontiguousarray(ref, np.uint8)
        idx = np.full(max(1, len(plan["status"])), -1, np.int32)
        check(self.lib.lcd_batch_add_planned(self.h, chunk.h, C.byref(pl), hp.ctypes.data_as(i32p), ps.ctypes.data_as(C.POINTER(C.c_int64)), _p8(rf), int(ref_beg),
                                             idx.ctypes.data_as(i32p)), self.lib)
        idx = idx[:len(plan["status"])].copy()
        for i in np.argsort(np.where(idx >= 0, idx, 1 << 30), kind="stable"):
            if idx[i] >= 0:
                self.n_reads.append(int(plan["read_off"][i + 1] - plan["read_off"][i]))
        return idx

    def result(self, region):
        """-> dict(n_cons, clu_n_seqs, clu_read_ids, aln_strs[c][j] = None | dict(target, query, beg/end...)), freeing the C buffers"""
        n = self.n_reads[region]
        m = 1 + 2 * n
        clu_n = (C.c_int * 2)(0, 0)
        clu_ids = (i32p * 2)()
        a0, a1 = (LcdAlnStr * m)(), (LcdAlnStr * m)()
        arr = (C.POINTER(LcdAlnStr) * 2)(C.cast(a0, C.POINTER(LcdAlnStr)), C.cast(a1, C.POINTER(LcdAlnStr)))
        nc = check(self.lib.lcd_batch_region_result(self.h, region, clu_n, clu_ids, arr), self.lib)
        res = dict(n_cons=nc, clu_n_seqs=[int(clu_n[0]), int(clu_n[1])], clu_read_ids=[], aln_strs=[[], []])
        for c in range(2):
            if clu_ids[c]:
                res["clu_read_ids"].append(np.ctypeslib.as_array(clu_ids[c], shape=(max(clu_n[c], 1),))[:clu_n[c]].copy())
                _libc.free(clu_ids[c])
            else:
                res["clu_read_ids"].append(None)
            for j in range(m):
                s = (a0, a1)[c][j]
                if not s.target_aln:
                    res["aln_strs"][c].append(None)
                    continue
                L = s.aln_len
                t = np.ctypeslib.as_array(s.target_aln, shape=(max(L, 1),))[:L].copy()
                q = np.ctypeslib.as_array(s.query_aln, shape=(max(L, 1),))[:L].copy()
                res["aln_strs"][c].append(dict(target=t, query=q, aln_len=L, target_beg=s.target_beg, target_end=s.target_end,
                                               query_beg=s.query_beg, query_end=s.query_end))
                _libc.free(s.target_aln)
        return res


    def results_arena(self, parse=True):
        """lcd_batch_region_results_arena: every region's results in ONE host block (interior pointers, one free).  parse=True -> list of dicts like result();
        parse=False -> (n_regions, arena bytes) -- what bench.py times"""
        from ._lib import LcdRegionResult
        tab = C.POINTER(LcdRegionResult)(); arena = C.c_void_p(); nbytes = C.c_uint64()
        fn = self.lib.lcd_batch_region_results_arena
        fn.argtypes = [C.c_void_p, C.POINTER(C.POINTER(LcdRegionResult)), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        n = check(fn(self.h, C.byref(tab), C.byref(arena), C.byref(nbytes)), self.lib)
        if not parse:
            _libc.free(arena)
            return n, int(nbytes.value)
        out = []
        for r in range(n):
            rr = tab[r]
            res = dict(n_cons=rr.n_cons, clu_n_seqs=[int(rr.clu_n_seqs[0]), int(rr.clu_n_seqs[1])], clu_read_ids=[], aln_strs=[[], []])
            for c in range(2):
                res["clu_read_ids"].append(np.ctypeslib.as_array(rr.clu_read_ids[c], shape=(max(rr.clu_n_seqs[c], 1),))[:rr.clu_n_seqs[c]].copy() if rr.clu_read_ids[c] else None)
                for j in range(rr.n_aln_strs):
                    s = rr.aln_strs[c][j]
                    if not s.target_aln:
                        res["aln_strs"][c].append(None)
                        continue
                    L = s.aln_len
                    res["aln_strs"][c].append(dict(target=np.ctypeslib.as_array(s.target_aln, shape=(max(L, 1),))[:L].copy(), query=np.ctypeslib.as_array(s.query_aln, shape=(max(L, 1),))[:L].copy(),
                                                   aln_len=L, target_beg=s.target_beg, target_end=s.target_end, query_beg=s.query_beg, query_end=s.query_end))
            out.append(res)
        _libc.free(arena)
        return out


def make_read_views(digars, bseqs, quals, qlens, haps, phase_sets):
    """lcd_read_view_t[] over numpy storage: digars[i] = (n, 4) int64 rows (pos, type, len, qi) as digar1_t (src/bam_utils.h:27-33),
    bseqs[i] = 4-bit BAM-packed bases, quals[i] = phred bytes.  Returns (ctypes array, keep-alive list)."""
    n = len(digars)
    arr = (LcdReadView * n)()
    keep = []
    for i in range(n):
        d = np.asarray(digars[i], np.int64)
        da = (LcdDigar1 * max(len(d), 1))()
        for k in range(len(d)):
            da[k].pos, da[k].type, da[k].len, da[k].qi = int(d[k, 0]), int(d[k, 1]), int(d[k, 2]), int(d[k, 3])
        bs = np.ascontiguousarray(bseqs[i], np.uint8); ql = np.ascontiguousarray(quals[i], np.uint8)
        arr[i].digars = da; arr[i].n_digar = len(d); arr[i].qlen = int(qlens[i])
        arr[i].bseq = _p8(bs); arr[i].qual = _p8(ql); arr[i].hap = int(haps[i]); arr[i].phase_set = int(phase_sets[i])
        keep += [da, bs, ql]
    return arr, keep


def copy_counters():
    """lcd_copy_counters: bytes of [digars D2H, digars H2D, read bases H2D, read bases D2H] since process start"""
    lib = load_library()
    out = (C.c_ulonglong * 4)()
    lib.lcd_copy_counters.argtypes = [C.POINTER(C.c_ulonglong)]
    lib.lcd_copy_counters(out)
    return [int(x) for x in out]


class DeviceChunk:
    """lcd_chunk_t: a chunk's reads uploaded once; digars made and kept in HBM; region slices cut there; a batch's read bases unpacked from there"""

    def __init__(self, pos0, cigars, quals, bseqs, reg_beg, reg_end, whole_ref_len, is_ont=0, pal_flags=None):
        self.lib = lib = load_library()
        opt = LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), int(is_ont))
        n = self.n = len(cigars)
        cg = [np.ascontiguousarray(c, np.uint32) for c in cigars]; ql = [np.ascontiguousarray(q, np.uint8) for q in quals]; sq = [np.ascontiguousarray(x, np.uint8) for x in bseqs]
        off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
        coff, qoff, soff = off(cg), off(ql), off(sq)
        cpool = np.concatenate(cg + [np.zeros(1, np.uint32)]); qpool = np.concatenate(ql + [np.zeros(1, np.uint8)]); spool = np.concatenate(sq + [np.zeros(2, np.uint8)])
        ncig = np.array([len(c) for c in cg], np.int32); qlen = np.array([len(q) for q in ql], np.int32)
        p0 = np.ascontiguousarray(pos0, np.int64)
        pf = np.ascontiguousarray(pal_flags if pal_flags is not None else np.zeros(n, np.uint8), np.uint8)
        u64p_, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        lib.lcd_chunk_create.restype = C.c_void_p
        lib.lcd_chunk_create.argtypes = [C.POINTER(LcdDigarOpt), C.c_int, i64p, C.POINTER(C.c_uint32), u64p_, i32p, u8p, u64p_, i32p, u8p, u8p, u64p_, C.c_int64, C.c_int64, C.c_int64]
        self.h = lib.lcd_chunk_create(C.byref(opt), n, p0.ctypes.data_as(i64p), cpool.ctypes.data_as(C.POINTER(C.c_uint32)), coff.ctypes.data_as(u64p_), ncig.ctypes.data_as(i32p),
                                      _p8(qpool), qoff.ctypes.data_as(u64p_), qlen.ctypes.data_as(i32p), _p8(pf), _p8(spool), soff.ctypes.data_as(u64p_),
                                      int(reg_beg), int(reg_end), int(whole_ref_len))
        if not self.h:
            raise RuntimeError("lcd_chunk_create failed: " + lib.lcd_last_error().decode())
        self.packed_bytes = int(soff[-1])

    @classmethod
    def from_bam(cls, bam_path, bai_path, chrom, reg_beg, reg_end, min_mapq=30, is_ont=0, verify_crc=1, src=None):
        """lcd_chunk_create_from_bam: the region's BGZF blocks inflated on the device, records found / filtered / turned into digars there.
        src=(ref, ref_beg, ref_end, is_ont) -> lcd_chunk_create_from_bam_src: every read from the source the reference chooses for it (EQX CIGAR, cs tag, MD tag,
        comparison with `ref` = the chunk's reference window as letters or codes 0-4, bytes / uint8 array or None) and, with is_ont, the SA-tag palindrome rule;
        the digar options are those of src's is_ont.  -> the chunk; .meta = per-read scalars and names (dict of numpy arrays / list)"""
        from ._lib import LcdBamReads, LcdChunkSrc
        self = cls.__new__(cls)
        self.lib = lib = load_library()
        opt = LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), int(is_ont))
        m = LcdBamReads()
        lib.lcd_chunk_create_from_bam.restype = C.c_void_p
        lib.lcd_chunk_create_from_bam.argtypes = [C.POINTER(LcdDigarOpt), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(LcdBamReads)]
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        if src is None:
            self.h = lib.lcd_chunk_create_from_bam(C.byref(opt), enc(bam_path), enc(bai_path), enc(chrom), int(reg_beg), int(reg_end), int(min_mapq), int(verify_crc), C.byref(m))
        else:
            ref, ref_beg, ref_end, src_ont = src
            lib.lcd_digar_opt_default(C.byref(opt), int(src_ont))
            refb = None if ref is None else (bytes(ref) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8).tobytes())
            refbuf = C.create_string_buffer(refb, len(refb) + 1) if refb is not None else None   # (codes 0-4 contain NULs: not a C string; alive until the call returns)
            cs = LcdChunkSrc(); cs.ref_seq = C.cast(refbuf, C.c_char_p) if refbuf is not None else None
            cs.ref_beg, cs.ref_end, cs.is_ont = int(ref_beg), int(ref_end), int(src_ont)
            if refb is not None and len(refb) < cs.ref_end - cs.ref_beg + 1:
                raise ValueError("DeviceChunk.from_bam: ref is shorter than [ref_beg, ref_end]")
            lib.lcd_chunk_create_from_bam_src.restype = C.c_void_p
            lib.lcd_chunk_create_from_bam_src.argtypes = lib.lcd_chunk_create_from_bam.argtypes[:-1] + [C.POINTER(LcdChunkSrc), C.POINTER(LcdBamReads)]
            self.h = lib.lcd_chunk_create_from_bam_src(C.byref(opt), enc(bam_path), enc(bai_path), enc(chrom), int(reg_beg), int(reg_end), int(min_mapq), int(verify_crc),
                                                       C.byref(cs), C.byref(m))
        if not self.h:
            raise RuntimeError("lcd_chunk_create_from_bam failed: " + lib.lcd_last_error().decode())
        n = self.n = m.n_reads
        arr = lambda p, dt: np.array([p[i] for i in range(n)], dt)
        self.meta = dict(tid=m.tid, n_targets=m.n_targets, target_len=m.target_len, pos0=arr(m.pos0, np.int64), end_pos=arr(m.end_pos, np.int64), mapq=arr(m.mapq, np.int32),
                         flag=arr(m.flag, np.int32), n_cigar=arr(m.n_cigar, np.int32), qlen=arr(m.qlen, np.int32),
                         names=[C.string_at(C.addressof(m.name_pool.contents) + m.name_off[i]).decode() for i in range(n)])
        lib.lcd_bam_reads_free.argtypes = [C.POINTER(LcdBamReads)]
        lib.lcd_bam_reads_free(C.byref(m))
        self.packed_bytes = 0
        return self

    @classmethod
    def open_from_bam(cls, bam_path, bai_path, chrom, reg_beg, reg_end, min_mapq=30, is_ont=0, verify_crc=1):
        """lcd_chunk_open_from_bam: the first phase of from_bam -- region image, inflate, record walk, loader's rule; .meta is filled (the reads' span is known), the
        handle has no digars until resolve()"""
        from ._lib import LcdBamReads
        self = cls.__new__(cls)
        self.lib = lib = load_library()
        opt = LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), int(is_ont))
        m = LcdBamReads()
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        self.h = lib.lcd_chunk_open_from_bam(C.byref(opt), enc(bam_path), enc(bai_path), enc(chrom), int(reg_beg), int(reg_end), int(min_mapq), int(verify_crc), C.byref(m))
        if not self.h:
            raise RuntimeError("lcd_chunk_open_from_bam failed: " + lib.lcd_last_error().decode())
        n = self.n = m.n_reads
        arr = lambda p, dt: np.array([p[i] for i in range(n)], dt)
        self.meta = dict(tid=m.tid, n_targets=m.n_targets, target_len=m.target_len, pos0=arr(m.pos0, np.int64), end_pos=arr(m.end_pos, np.int64), mapq=arr(m.mapq, np.int32),
                         flag=arr(m.flag, np.int32), n_cigar=arr(m.n_cigar, np.int32), qlen=arr(m.qlen, np.int32),
                         names=[C.string_at(C.addressof(m.name_pool.contents) + m.name_off[i]).decode() for i in range(n)])
        lib.lcd_bam_reads_free.argtypes = [C.POINTER(LcdBamReads)]
        lib.lcd_bam_reads_free(C.byref(m))
        self.packed_bytes = 0
        return self

    @classmethod
    def open_from_bams(cls, bam_paths, bai_paths, chrom, reg_beg, reg_end, min_mapq=30, is_ont=0, verify_crc=1):
        """lcd_chunk_open_from_bams: open_from_bam over the files of one sample -- their region images appended, one inflate, the reads file-major.  bai_paths None, or
        an entry None: <bam>.bai.  .n_files and .file_of_read (per kept read its file index) are filled beside .meta"""
        from ._lib import LcdBamReads
        self = cls.__new__(cls)
        self.lib = lib = load_library()
        opt = LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), int(is_ont))
        m = LcdBamReads()
        bams, n = _str_array(bam_paths)
        bais = None
        if bai_paths is not None:
            assert len(bai_paths) == n
            bais = (C.c_char_p * max(1, n))(*[_enc(x) if x is not None else None for x in bai_paths])
        self.h = lib.lcd_chunk_open_from_bams(C.byref(opt), n, bams, bais, _enc(chrom), int(reg_beg), int(reg_end), int(min_mapq), int(verify_crc), C.byref(m))
        if not self.h:
            raise LcdError("lcd_chunk_open_from_bams failed: " + lib.lcd_last_error().decode())
        n = self.n = m.n_reads
        arr = lambda p, dt: np.array([p[i] for i in range(n)], dt)
        self.meta = dict(tid=m.tid, n_targets=m.n_targets, target_len=m.target_len, pos0=arr(m.pos0, np.int64), end_pos=arr(m.end_pos, np.int64), mapq=arr(m.mapq, np.int32),
                         flag=arr(m.flag, np.int32), n_cigar=arr(m.n_cigar, np.int32), qlen=arr(m.qlen, np.int32),
                         names=[C.string_at(C.addressof(m.name_pool.contents) + m.name_off[i]).decode() for i in range(n)])
        lib.lcd_bam_reads_free.argtypes = [C.POINTER(LcdBamReads)]
        lib.lcd_bam_reads_free(C.byref(m))
        self.packed_bytes = 0
        self.n_files = int(lib.lcd_chunk_n_files(self.h))
        fr = np.zeros(max(n, 1), np.int32)
        check(lib.lcd_chunk_read_files(self.h, fr.ctypes.data_as(i32p)), lib)
        self.file_of_read = fr[:n]
        return self

    def tag_records_sel(self, haps, phase_sets, skip=None, order=None):
        """lcd_chunk_tag_records_sel: tag_records for the records with skip[i] == 0, in the order `order` names them (merged_record_plan's outputs) -> (bytes, number)"""
        lib = self.lib
        hp = np.concatenate([np.ascontiguousarray(haps, np.int32), np.zeros(1, np.int32)]); ps = np.concatenate([np.ascontiguousarray(phase_sets, np.int64), np.zeros(1, np.int64)])
        if len(hp) <= self.n or len(ps) <= self.n:
            raise ValueError("tag_records_sel: haps / phase_sets shorter than the chunk's reads")
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        od = np.ascontiguousarray(order, np.int32) if order is not None else None
        h = lib.lcd_chunk_tag_records_sel(self.h, hp.ctypes.data_as(i32p), ps.ctypes.data_as(C.POINTER(C.c_int64)), _p8(sk) if sk is not None else None,
                                          od.ctypes.data_as(i32p) if od is not None else None)
        if not h:
            raise LcdError("lcd_chunk_tag_records_sel failed: " + lib.lcd_last_error().decode())
        try:
            n = lib.lcd_tagged_size(h)
            buf = C.create_string_buffer(max(n, 1))
            check(lib.lcd_tagged_to_host(h, 0, n, buf), lib)
            return buf.raw[:n], int(lib.lcd_tagged_n_records(h))
        finally:
            lib.lcd_tagged_free(h)

    def refine_records(self, haps, phase_sets, touched=None, ref=None, ref_beg=1, ref_end=0, skip=None, order=None):
        """lcd_chunk_refine_records: tag_records_sel where every kept record first gets the alignment of its read's final digars (CIGAR, POS, bin, NM / MD / cs).
        touched = {read id: (n, >= 4) rows [pos, type, len, qi(, is_low_qual)]} for the reads a noisy region rewrote (any other read uses the chunk's digars in HBM);
        ref = the chunk's reference window as letters or codes 0-4 (bytes / uint8 array), ref[0] = position ref_beg, ref_end inclusive.
        -> (bytes of the records back to back, their number, stats dict)"""
        from ._lib import LcdDigar, LcdRefineStats
        lib = self.lib
        hp = np.concatenate([np.ascontiguousarray(haps, np.int32), np.zeros(1, np.int32)]); ps = np.concatenate([np.ascontiguousarray(phase_sets, np.int64), np.zeros(1, np.int64)])
        if len(hp) <= self.n or len(ps) <= self.n:
            raise ValueError("refine_records: haps / phase_sets shorter than the chunk's reads")
        touched = touched or {}
        ids = np.array(sorted(touched), np.int32)
        rows = [np.asarray(touched[int(r)], np.int64) for r in ids]
        rows = [x.reshape(-1, x.shape[-1]) if x.size else np.zeros((0, 5), np.int64) for x in rows]
        off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.uint64)
        dg = (LcdDigar * max(int(off[-1]), 1))()
        k = 0
        for x in rows:
            for d in x:
                dg[k].pos, dg[k].type, dg[k].len, dg[k].qi = int(d[0]), int(d[1]), int(d[2]), int(d[3])
                dg[k].is_low_qual = int(d[4]) if len(d) > 4 else 0
                k += 1
        refb = None if ref is None else (bytes(ref) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8).tobytes())
        if refb is not None and len(refb) < int(ref_end) - int(ref_beg) + 1:
            raise ValueError("refine_records: ref is shorter than [ref_beg, ref_end]")
        refbuf = C.create_string_buffer(refb, len(refb) + 1) if refb is not None else None     # (codes contain NULs: not a C string)
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        od = np.ascontiguousarray(order, np.int32) if order is not None else None
        st = LcdRefineStats()
        h = lib.lcd_chunk_refine_records(self.h, len(ids), ids.ctypes.data_as(i32p), off.ctypes.data_as(C.POINTER(C.c_uint64)), dg,
                                         C.cast(refbuf, C.c_char_p) if refbuf is not None else None, int(ref_beg), int(ref_end), hp.ctypes.data_as(i32p),
                                         ps.ctypes.data_as(C.POINTER(C.c_int64)), _p8(sk) if sk is not None else None, od.ctypes.data_as(i32p) if od is not None else None,
                                         C.byref(st))
        if not h:
            raise LcdError("lcd_chunk_refine_records failed: " + lib.lcd_last_error().decode())
        try:
            n = lib.lcd_tagged_size(h)
            buf = C.create_string_buffer(max(n, 1))
            check(lib.lcd_tagged_to_host(h, 0, n, buf), lib)
            return buf.raw[:n], int(lib.lcd_tagged_n_records(h)), {f: getattr(st, f) for f, _ in LcdRefineStats._fields_}
        finally:
            lib.lcd_tagged_free(h)

    def resolve(self, src=None):
        """lcd_chunk_resolve: the second phase -- src = (ref, ref_beg, ref_end, is_ont) as for from_bam, or None; a second call raises (-4)"""
        from ._lib import LcdChunkSrc
        if src is None:
            return check(self.lib.lcd_chunk_resolve(self.h, None), self.lib)
        ref, ref_beg, ref_end, src_ont = src
        refb = None if ref is None else (bytes(ref) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8).tobytes())
        refbuf = C.create_string_buffer(refb, len(refb) + 1) if refb is not None else None
        cs = LcdChunkSrc(); cs.ref_seq = C.cast(refbuf, C.c_char_p) if refbuf is not None else None
        cs.ref_beg, cs.ref_end, cs.is_ont = int(ref_beg), int(ref_end), int(src_ont)
        if refb is not None and len(refb) < cs.ref_end - cs.ref_beg + 1:
            raise ValueError("DeviceChunk.resolve: ref is shorter than [ref_beg, ref_end]")
        return check(self.lib.lcd_chunk_resolve(self.h, C.byref(cs)), self.lib)

    def tag_records(self, haps, phase_sets, n_skip_kept=0, n_skip_filtered=0):
        """lcd_chunk_tag_records: the records of a chunk made from a BAM with HP:i / PS:i rewritten in HBM -> (bytes of the records back to back, their number)"""
        lib = self.lib
        hp = np.ascontiguousarray(haps, np.int32); ps = np.ascontiguousarray(phase_sets, np.int64)
        if len(hp) < self.n or len(ps) < self.n:
            raise ValueError("tag_records: haps / phase_sets shorter than the chunk's reads")
        hp = np.concatenate([hp, np.zeros(1, np.int32)]); ps = np.concatenate([ps, np.zeros(1, np.int64)])
        h = lib.lcd_chunk_tag_records(self.h, hp.ctypes.data_as(i32p), ps.ctypes.data_as(C.POINTER(C.c_int64)), int(n_skip_kept), int(n_skip_filtered))
        if not h:
            raise LcdError("lcd_chunk_tag_records failed: " + lib.lcd_last_error().decode())
        try:
            n = lib.lcd_tagged_size(h)
            buf = C.create_string_buffer(max(n, 1))
            check(lib.lcd_tagged_to_host(h, 0, n, buf), lib)
            return buf.raw[:n], int(lib.lcd_tagged_n_records(h))
        finally:
            lib.lcd_tagged_free(h)

    def mod_pileup(self, haps, ref, ref_beg, ref_end, code="m", threshold=204, combine_strands=False):
        """lcd_chunk_mod_pileup: the per-haplotype CpG methylation table of the chunk's region from the MM / ML tags of its kept records.  haps: 0 / 1 / 2 per kept
        read; ref: the window as letters or codes 0-4 (bytes / uint8 array), ref[0] = position ref_beg (1-based), ref_end inclusive.
        -> (rows [(position, strand, nine counters hap-major: mod, canon, filtered)], stats dict)"""
        from ._lib import LcdModsOpt, LcdModsStats
        lib = self.lib
        hp = np.ascontiguousarray(haps, np.int32)
        if len(hp) < self.n:
            raise ValueError("mod_pileup: haps shorter than the chunk's reads")
        hp = np.concatenate([hp, np.zeros(1, np.int32)])
        refb = bytes(ref) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8).tobytes()
        if len(refb) < int(ref_end) - int(ref_beg) + 1:
            raise ValueError("mod_pileup: ref is shorter than [ref_beg, ref_end]")
        refbuf = C.create_string_buffer(refb, len(refb) + 1)                  # (codes contain NULs: not a C string)
        o = LcdModsOpt(); lib.lcd_mods_opt_default(C.byref(o))
        o.code, o.threshold, o.combine_strands = ord(code) if isinstance(code, str) and len(code) == 1 else -1, int(threshold), int(bool(combine_strands))
        o.ref_seq = C.cast(refbuf, C.c_char_p); o.ref_beg, o.ref_end = int(ref_beg), int(ref_end)
        st = LcdModsStats()
        h = lib.lcd_chunk_mod_pileup(self.h, hp.ctypes.data_as(i32p), C.byref(o), C.byref(st))
        if not h:
            raise LcdError("lcd_chunk_mod_pileup failed: " + lib.lcd_last_error().decode())
        try:
            n = int(lib.lcd_mods_n_rows(h))
            pos = np.zeros(max(n, 1), np.int64); strand = C.create_string_buffer(max(n, 1)); cnt = np.zeros(9 * max(n, 1), np.uint32)
            check(lib.lcd_mods_rows_to_host(h, pos.ctypes.data_as(C.POINTER(C.c_int64)), strand, cnt.ctypes.data_as(C.POINTER(C.c_uint32))), lib)
            rows = [(int(pos[k]), strand.raw[k:k + 1].decode(), tuple(int(x) for x in cnt[9 * k:9 * k + 9])) for k in range(n)]
            return rows, {f: getattr(st, f) for f, _ in LcdModsStats._fields_}
        finally:
            lib.lcd_mods_free(h)

    def depth(self, haps, skip_dels=False):
        """lcd_chunk_depth: the per-haplotype depth track of the chunk's region from the CIGARs of its kept records.  haps: 0 / 1 / 2 per kept read.
        -> (rows [(beg, end, (depth of haplotype 0, 1, 2))] that tile the region in position order, stats dict; "bases" is a list of three)"""
        from ._lib import LcdDepthOpt, LcdDepthStats
        lib = self.lib
        hp = np.ascontiguousarray(haps, np.int32)
        if len(hp) < self.n:
            raise ValueError("depth: haps shorter than the chunk's reads")
        hp = np.concatenate([hp, np.zeros(1, np.int32)])
        o = LcdDepthOpt(); lib.lcd_depth_opt_default(C.byref(o))
        o.skip_dels = int(bool(skip_dels))
        st = LcdDepthStats()
        h = lib.lcd_chunk_depth(self.h, hp.ctypes.data_as(i32p), C.byref(o), C.byref(st))
        if not h:
            raise LcdError("lcd_chunk_depth failed: " + lib.lcd_last_error().decode())
        try:
            n = int(lib.lcd_depth_n_rows(h))
            beg = np.zeros(max(n, 1), np.int64); end = np.zeros(max(n, 1), np.int64); dep = np.zeros(3 * max(n, 1), np.uint32)
            check(lib.lcd_depth_rows_to_host(h, beg.ctypes.data_as(C.POINTER(C.c_int64)), end.ctypes.data_as(C.POINTER(C.c_int64)), dep.ctypes.data_as(C.POINTER(C.c_uint32))), lib)
            rows = [(int(beg[k]), int(end[k]), tuple(int(x) for x in dep[3 * k:3 * k + 3])) for k in range(n)]
            return rows, _depth_stats(st)
        finally:
            lib.lcd_depth_free(h)

    def read_info(self):
        n = self.n
        st = np.zeros(n, np.int32); beg = np.zeros(n, np.int64); end = np.zeros(n, np.int64); nc = np.zeros(n, np.int32); nd = np.zeros(n, np.int32)
        i64p = C.POINTER(C.c_int64)
        self.lib.lcd_chunk_read_info.argtypes = [C.c_void_p, i32p, i64p, i64p, i32p, i32p]
        check(self.lib.lcd_chunk_read_info(self.h, st.ctypes.data_as(i32p), beg.ctypes.data_as(i64p), end.ctypes.data_as(i64p), nc.ctypes.data_as(i32p), nd.ctypes.data_as(i32p)), self.lib)
        return dict(status=st, beg=beg, end=end, n_cand=nc, n_digars=nd)

    def sources(self):
        """lcd_chunk_read_sources -> dict(source: LCD_SRC_* per read (0 EQX, 1 cs, 2 MD, 3 reference comparison), is_ont_palindrome per read, tag_bytes_d2h)"""
        so = np.zeros(max(self.n, 1), np.uint8); pl = np.zeros(max(self.n, 1), np.uint8); tb = C.c_uint64(0)
        self.lib.lcd_chunk_read_sources.argtypes = [C.c_void_p, u8p, u8p, C.POINTER(C.c_uint64)]
        self.lib.lcd_chunk_read_sources(self.h, _p8(so), _p8(pl), C.byref(tb))
        return dict(source=so[:self.n], is_ont_palindrome=pl[:self.n], tag_bytes_d2h=int(tb.value))

    def stage_ms(self):
        """lcd_chunk_stage_ms -> [aux fields, reference comparison, tag download + host parse, digars] of from_bam(src=...), milliseconds"""
        out = (C.c_double * 4)()
        self.lib.lcd_chunk_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self.lib.lcd_chunk_stage_ms.restype = None
        self.lib.lcd_chunk_stage_ms(self.h, out)
        return [float(x) for x in out]

    def digars(self):
        """lcd_chunk_digars: the digars the chunk holds in HBM, downloaded -> per read an (n, 5) int64 array [pos, type, len, qi, is_low_qual] (digar_batch's layout)"""
        u64p_ = C.POINTER(C.c_uint64)
        doff, dg = u64p_(), C.POINTER(LcdDigar)()
        self.lib.lcd_chunk_digars.argtypes = [C.c_void_p, C.POINTER(u64p_), C.POINTER(C.POINTER(LcdDigar))]
        check(self.lib.lcd_chunk_digars(self.h, C.byref(doff), C.byref(dg)), self.lib)
        if not doff:
            return []
        tot = int(doff[self.n])
        dt = np.dtype([("pos", "<i8"), ("type", "<i4"), ("len", "<i4"), ("qi", "<i4"), ("lq", "<i4")])
        D = np.frombuffer((C.c_char * (24 * max(tot, 1))).from_address(C.addressof(dg.contents)), dtype=dt, count=tot).copy() if tot else np.zeros(0, dt)
        out = []
        for r in range(self.n):
            d = D[int(doff[r]):int(doff[r + 1])]
            out.append(np.stack([d["pos"], d["type"].astype(np.int64), d["len"].astype(np.int64), d["qi"].astype(np.int64), d["lq"].astype(np.int64)], 1).reshape(-1, 5))
        for p_ in (doff, dg):
            _libc.free(C.cast(p_, C.c_void_p))
        return out

    def intervals(self):
        """-> per read (noisy (m, 3) int64 [start, end, label], in_chunk mask)"""
        u64p_ = C.POINTER(C.c_uint64)
        ioff, iv, inc = u64p_(), C.POINTER(LcdNoisyIv)(), u8p()
        self.lib.lcd_chunk_intervals.argtypes = [C.c_void_p, C.POINTER(u64p_), C.POINTER(C.POINTER(LcdNoisyIv)), C.POINTER(u8p)]
        self.lib.lcd_chunk_intervals(self.h, C.byref(ioff), C.byref(iv), C.byref(inc))
        out = []
        for r in range(self.n):
            a, b = int(ioff[r]), int(ioff[r + 1])
            out.append((np.array([[iv[k].start, iv[k].end, iv[k].label] for k in range(a, b)], np.int64).reshape(-1, 3), np.array([inc[k] for k in range(a, b)], bool)))
        return out

    def region_slices(self, pair_read, pair_beg, pair_end, flank=10):
        pr = np.ascontiguousarray(pair_read, np.int32); pb = np.ascontiguousarray(pair_beg, np.int64); pe = np.ascontiguousarray(pair_end, np.int64)
        n = len(pr)
        rb = np.zeros(n, np.int32); re_ = np.zeros(n, np.int32); cv = np.zeros(n, np.int32)
        i64p = C.POINTER(C.c_int64)
        self.lib.lcd_chunk_region_slices.argtypes = [C.c_void_p, C.c_int, i32p, i64p, i64p, C.c_int, i32p, i32p, i32p]
        check(self.lib.lcd_chunk_region_slices(self.h, n, pr.ctypes.data_as(i32p), pb.ctypes.data_as(i64p), pe.ctypes.data_as(i64p), int(flank),
                                               rb.ctypes.data_as(i32p), re_.ctypes.data_as(i32p), cv.ctypes.data_as(i32p)), self.lib)
        return rb, re_, cv

    def add_region(self, batch, reg_beg, reg_end, read_ids, read_beg, read_end, cover, haps, phase_sets, ref):
        ids = np.ascontiguousarray(read_ids, np.int32); rb = np.ascontiguousarray(read_beg, np.int32); re_ = np.ascontiguousarray(read_end, np.int32)
        cv = np.ascontiguousarray(cover, np.int32); hp = np.ascontiguousarray(haps, np.int32); ps = np.ascontiguousarray(phase_sets, np.int64)
        rf = np.ascontiguousarray(ref, np.uint8)
        i64p = C.POINTER(C.c_int64)
        self.lib.lcd_batch_add_region_from_chunk_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, i32p, i32p, i32p, i32p, i32p, i64p, u8p, C.c_int]
        ri = check(self.lib.lcd_batch_add_region_from_chunk_dev(batch.h, self.h, int(reg_beg), int(reg_end), len(ids), ids.ctypes.data_as(i32p), rb.ctypes.data_as(i32p),
                                                                re_.ctypes.data_as(i32p), cv.ctypes.data_as(i32p), hp.ctypes.data_as(i32p), ps.ctypes.data_as(i64p), _p8(rf), len(rf)), self.lib)
        batch.n_reads.append(len(ids))
        return ri

    def clean_vars(self, ordered_read_ids, ref, ref_beg, ref_end, reg_beg, reg_end, pre_regs=(), low_comp=(), is_rev=None, opt=None):
        """lcd_chunk_clean_vars: steps 1.2 - 3.1 of collect_var_main on this chunk -> dict (clean_vars_dict)"""
        return chunk_clean_vars_batch([self], [dict(ordered_read_ids=ordered_read_ids, ref=ref, ref_beg=ref_beg, ref_end=ref_end, reg_beg=reg_beg, reg_end=reg_end,
                                                    pre_regs=pre_regs, low_comp=low_comp, is_rev=is_rev)], opt, single=True)[0]

    def close(self):
        if self.h:
            self.lib.lcd_chunk_destroy.argtypes = [C.c_void_p]
            self.lib.lcd_chunk_destroy(self.h)
            self.h = None


def digar_batch(pos0, cigars, quals, reg_beg, reg_end, whole_ref_len, is_ont=0, pal_flags=None, opt=None, cs=None, md=None, seqs=None, ref=None):
    """collect_digar_from_eqx_cigar (src/bam_utils.c:701) for a list of reads on the GPU: cigars[i] = uint32 BAM CIGAR words, quals[i] = phred bytes.
    The reference's three other sources (src/collect_var.c:1072-1079): cs=[bytes, ...] -> collect_digar_from_cs_tag (:844), md=[bytes, ...] ->
    collect_digar_from_MD_tag (:1010), seqs=[4-bit packed bases, ...] + ref=(ref_seq bytes, ref_beg, ref_end) -> collect_digar_from_ref_seq (:1179).
    -> list of dict(rc, digars (n,5), noisy (m,3), chunk_noisy (k,3), beg, end, n_cand), the layout of the oracle's wrapper"""
    lib = load_library()
    if opt is None:
        opt = LcdDigarOpt(); lib.lcd_digar_opt_default(C.byref(opt), int(is_ont))
    n = len(cigars)
    if n == 0:
        return []
    cg = [np.ascontiguousarray(c, np.uint32) for c in cigars]; ql = [np.ascontiguousarray(q, np.uint8) for q in quals]
    coff = np.concatenate([[0], np.cumsum([len(c) for c in cg])]).astype(np.uint64); qoff = np.concatenate([[0], np.cumsum([len(q) for q in ql])]).astype(np.uint64)
    cpool = np.concatenate(cg + [np.zeros(1, np.uint32)]); qpool = np.concatenate(ql + [np.zeros(1, np.uint8)])
    ncig = np.array([len(c) for c in cg], np.int32); qlen = np.array([len(q) for q in ql], np.int32)
    p0 = np.ascontiguousarray(pos0, np.int64)
    pf = np.ascontiguousarray(pal_flags if pal_flags is not None else np.zeros(n, np.uint8), np.uint8)
    status = np.zeros(n, np.int32); beg = np.zeros(n, np.int64); end = np.zeros(n, np.int64); ncand = np.zeros(n, np.int32)
    u64p_, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    doff, ioff = u64p_(), u64p_(); dg = C.POINTER(LcdDigar)(); iv = C.POINTER(LcdNoisyIv)(); inc = u8p()
    head = (C.byref(opt), n, p0.ctypes.data_as(i64p), cpool.ctypes.data_as(C.POINTER(C.c_uint32)), coff.ctypes.data_as(u64p_), ncig.ctypes.data_as(i32p))
    quals_ = (_p8(qpool), qoff.ctypes.data_as(u64p_), qlen.ctypes.data_as(i32p), _p8(pf))
    tail = (int(reg_beg), int(reg_end), int(whole_ref_len), C.byref(doff), C.byref(dg), C.byref(ioff), C.byref(iv), C.byref(inc), status.ctypes.data_as(i32p),
            beg.ctypes.data_as(i64p), end.ctypes.data_as(i64p), ncand.ctypes.data_as(i32p))
    if cs is not None or md is not None:
        tags = (C.c_char_p * n)(*[bytes(t) for t in (cs if cs is not None else md)])
        check(lib.lcd_digar_batch_tags(head[0], 1 if cs is not None else 2, *head[1:], tags, *quals_, *tail), lib)
    elif seqs is not None:
        sq = [np.ascontiguousarray(x, np.uint8) for x in seqs]
        soff = np.concatenate([[0], np.cumsum([len(x) for x in sq])]).astype(np.uint64); spool = np.concatenate(sq + [np.zeros(1, np.uint8)])
        ref_seq, ref_beg, ref_end = ref
        check(lib.lcd_digar_batch_ref(*head, _p8(spool), soff.ctypes.data_as(u64p_), *quals_, C.c_char_p(bytes(ref_seq)), int(ref_beg), int(ref_end), *tail), lib)
    else:
        check(lib.lcd_digar_batch(*head, *quals_, *tail), lib)
    out = []
    nd_tot, ni_tot = int(doff[n]), int(ioff[n])
    D = np.frombuffer((C.c_char * (24 * max(nd_tot, 1))).from_address(C.addressof(dg.contents)), dtype=np.dtype([("pos", "<i8"), ("type", "<i4"), ("len", "<i4"), ("qi", "<i4"), ("lq", "<i4")]), count=nd_tot).copy() if nd_tot else np.zeros(0, [("pos", "<i8"), ("type", "<i4"), ("len", "<i4"), ("qi", "<i4"), ("lq", "<i4")])
    I = np.frombuffer((C.c_char * (24 * max(ni_tot, 1))).from_address(C.addressof(iv.contents)), dtype=np.dtype([("st", "<i8"), ("en", "<i8"), ("label", "<i4"), ("pad", "<i4")]), count=ni_tot).copy() if ni_tot else np.zeros(0, [("st", "<i8"), ("en", "<i8"), ("label", "<i4"), ("pad", "<i4")])
    INC = np.array([inc[k] for k in range(ni_tot)], np.uint8)
    for r in range(n):
        d = D[int(doff[r]):int(doff[r + 1])]; v = I[int(ioff[r]):int(ioff[r + 1])]; m = INC[int(ioff[r]):int(ioff[r + 1])]
        noisy = np.stack([v["st"], v["en"], v["label"].astype(np.int64)], 1).reshape(-1, 3) if len(v) else np.zeros((0, 3), np.int64)
        out.append(dict(rc=int(status[r]), digars=np.stack([d["pos"], d["type"].astype(np.int64), d["len"].astype(np.int64), d["qi"].astype(np.int64), d["lq"].astype(np.int64)], 1).reshape(-1, 5),
                        noisy=noisy, chunk_noisy=noisy[m.astype(bool)].reshape(-1, 3), beg=int(beg[r]), end=int(end[r]), n_cand=int(ncand[r])))
    for p in (doff, ioff, dg, iv, inc):
        if p:
            _libc.free(C.cast(p, C.c_void_p))
    return out


def region_read_slices_batch(pair_read, pair_reg_beg, pair_reg_end, digars, qlens, flank=10):
    """collect_noisy_read_info's digar walk (src/align.c:1392-1456) for many (region, read) pairs in one launch (lcd_region_read_slices_batch):
    digars[r] = (n, >= 4) rows (pos, type, len, qi) of read r -> (read_beg, read_end, cover) arrays, one entry per pair"""
    lib = load_library()
    u64p_, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    n_reads = len(digars)
    off = np.zeros(n_reads + 1, np.uint64)
    for r in range(n_reads):
        off[r + 1] = off[r] + len(digars[r])
    pool = np.zeros((max(int(off[-1]), 1), 3), np.int64)      # lcd_digar_t: int64 pos | int32 type, len | int32 qi, is_low_qual
    v32 = pool.view(np.int32).reshape(len(pool), 6)
    for r in range(n_reads):
        d = np.asarray(digars[r], np.int64)
        if len(d):
            a, b = int(off[r]), int(off[r + 1])
            pool[a:b, 0] = d[:, 0]; v32[a:b, 2] = d[:, 1]; v32[a:b, 3] = d[:, 2]; v32[a:b, 4] = d[:, 3]
    pr = np.ascontiguousarray(pair_read, np.int32); pb = np.ascontiguousarray(pair_reg_beg, np.int64); pe = np.ascontiguousarray(pair_reg_end, np.int64)
    ql = np.ascontiguousarray(qlens, np.int32)
    n = len(pr)
    rb, re, cv = (np.zeros(max(n, 1), np.int32) for _ in range(3))
    check(lib.lcd_region_read_slices_batch(n, pr.ctypes.data_as(i32p), pb.ctypes.data_as(i64p), pe.ctypes.data_as(i64p), n_reads, off.ctypes.data_as(u64p_),
                                           C.cast(pool.ctypes.data, C.POINTER(LcdDigar)), ql.ctypes.data_as(i32p), int(flank), rb.ctypes.data_as(i32p),
                                           re.ctypes.data_as(i32p), cv.ctypes.data_as(i32p)), lib)
    return rb[:n], re[:n], cv[:n]


def pre_process_noisy_regs(chunk_noisy, low_comp, read_beg, read_end, read_ivs, min_alt_dp=2, min_af=0.2):
    """pre_process_noisy_regs (src/collect_var.c:557): chunk_noisy (n,3) in cr_add order, low_comp (m,2), per read beg/end and its own (k,>=2)
    interval array -> surviving regions (r,3)"""
    lib = load_library()
    def ivarr(a):
        a = np.asarray(a, np.int64).reshape(-1, a.shape[1] if hasattr(a, "shape") and a.ndim == 2 else 3) if len(a) else np.zeros((0, 3), np.int64)
        arr = (LcdNoisyIv * max(len(a), 1))()
        for i, row in enumerate(a):
            arr[i].start, arr[i].end, arr[i].label = int(row[0]), int(row[1]), int(row[2]) if len(row) > 2 else 0
        return arr, len(a)
    cn, n_noisy = ivarr(np.asarray(chunk_noisy, np.int64).reshape(-1, 3))
    lc = np.ascontiguousarray(np.asarray(low_comp, np.int64).reshape(-1, 2)); n_low = len(lc)
    if n_low == 0:
        lc = np.zeros((1, 2), np.int64)
    rb = np.ascontiguousarray(read_beg, np.int64); re_ = np.ascontiguousarray(read_end, np.int64)
    n_reads = len(rb)
    off = np.concatenate([[0], np.cumsum([len(x) for x in read_ivs])]).astype(np.uint64) if n_reads else np.zeros(1, np.uint64)
    flat = np.concatenate([np.asarray(x, np.int64).reshape(-1, 3) for x in read_ivs] + [np.zeros((0, 3), np.int64)]) if n_reads else np.zeros((0, 3), np.int64)
    ri, _ = ivarr(flat)
    i64p, u64p_ = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    out = C.POINTER(LcdNoisyIv)()
    if n_reads == 0:
        rb = np.zeros(1, np.int64); re_ = np.zeros(1, np.int64)
    n = check(lib.lcd_pre_process_noisy_regs(cn, n_noisy, lc.ctypes.data_as(i64p), n_low, n_reads, rb.ctypes.data_as(i64p), re_.ctypes.data_as(i64p), off.ctypes.data_as(u64p_), ri,
                                             int(min_alt_dp), float(min_af), C.byref(out)), lib)
    res = np.array([[out[i].start, out[i].end, out[i].label] for i in range(n)], np.int64).reshape(-1, 3)
    if out:
        _libc.free(C.cast(out, C.c_void_p))
    return res


def post_process_noisy_regs(regs, var_pos, var_ref_len, var_cate, flank=10):
    """post_process_noisy_regs (src/collect_var.c:640): regs (n,3) -> flank-extended, merged regions (m,3)"""
    lib = load_library()
    r = np.asarray(regs, np.int64).reshape(-1, 3)
    arr = (LcdNoisyIv * max(len(r), 1))()
    for i, row in enumerate(r):
        arr[i].start, arr[i].end, arr[i].label = int(row[0]), int(row[1]), int(row[2])
    vp = np.ascontiguousarray(var_pos, np.int64); vl = np.ascontiguousarray(var_ref_len, np.int32); vc = np.ascontiguousarray(var_cate, np.int32)
    if len(vp) == 0:
        vp = np.zeros(1, np.int64); vl = np.zeros(1, np.int32); vc = np.zeros(1, np.int32); nv = 0
    else:
        nv = len(vp)
    out = C.POINTER(LcdNoisyIv)()
    n = check(lib.lcd_post_process_noisy_regs(arr, len(r), nv, vp.ctypes.data_as(C.POINTER(C.c_int64)), vl.ctypes.data_as(i32p), vc.ctypes.data_as(i32p), int(flank), C.byref(out)), lib)
    res = np.array([[out[i].start, out[i].end, out[i].label] for i in range(n)], np.int64).reshape(-1, 3)
    if out:
        _libc.free(C.cast(out, C.c_void_p))
    return res


def cr_merge(ivs, fixed_merge_win=-1):
    """lcd_cr_merge: cr_merge (src/cgranges.c:289) of (n,3) (start, end, label) intervals -> merged (m,3)"""
    lib = load_library()
    r = np.asarray(ivs, np.int64).reshape(-1, 3)
    arr = (LcdNoisyIv * max(len(r), 1))()
    for i, row in enumerate(r):
        arr[i].start, arr[i].end, arr[i].label = int(row[0]), int(row[1]), int(row[2])
    out = C.POINTER(LcdNoisyIv)()
    lib.lcd_cr_merge.argtypes = [C.POINTER(LcdNoisyIv), C.c_int, C.c_int, C.POINTER(C.POINTER(LcdNoisyIv))]
    n = lib.lcd_cr_merge(arr, len(r), int(fixed_merge_win), C.byref(out))
    res = np.array([[out[i].start, out[i].end, out[i].label] for i in range(n)], np.int64).reshape(-1, 3)
    if out:
        _libc.free(C.cast(out, C.c_void_p))
    return res


def sdust(seq, T=5, W=20):
    """low-complexity intervals (src/sdust.c) of a code / letter sequence on the GPU -> (n, 2) array of (start, finish)"""
    lib = load_library()
    a = np.ascontiguousarray(seq, np.uint8)
    out = C.POINTER(C.c_int64)()
    n = check(lib.lcd_sdust(_p8(a), len(a), int(T), int(W), C.byref(out)), lib)
    res = np.array([out[i] for i in range(2 * n)], np.int64).reshape(-1, 2)
    if out:
        _libc.free(C.cast(out, C.c_void_p))
    return res


def sdust_batch(seqs, T=5, W=20):
    """lcd_sdust_batch: the low-complexity intervals of many sequences in one launch -> list of (n, 2) arrays"""
    lib = load_library()
    arrs = [np.ascontiguousarray(x, np.uint8) for x in seqs]
    n = len(arrs)
    ptrs = (u8p * n)(*[_p8(a) for a in arrs])
    lens = (C.c_int64 * n)(*[len(a) for a in arrs])
    outs = (C.POINTER(C.c_int64) * n)(); cnt = (C.c_int * n)()
    check(lib.lcd_sdust_batch(n, ptrs, lens, int(T), int(W), outs, cnt), lib)
    res = []
    for q in range(n):
        res.append(np.array([outs[q][i] for i in range(2 * cnt[q])], np.int64).reshape(-1, 2))
        if outs[q]:
            _libc.free(C.cast(outs[q], C.c_void_p))
    return res


def _hap_state(prob):
    R, V, TA = prob["n_reads"], prob["n_vars"], int(prob["alle_off"][-1])
    return dict(haps=np.zeros(R, np.int32), phase_sets=np.full(R, -1, np.int64), n_clean_agree_snps=np.zeros(R, np.int32),
                n_clean_conflict_snps=np.zeros(R, np.int32), var_phase_set=np.full(V, -1, np.int64),
                hap_to_cons_alle=np.full(V * 3, -1, np.int32), hap_to_alle_profile=np.zeros(3 * TA, np.int32))


def _fill_hap_struct(S, prob, state, keep):
    i32p, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    s = S()
    s.n_reads, s.n_vars, s.is_ont, s.n_cr = prob["n_reads"], prob["n_vars"], prob["is_ont"], len(prob["cr_read"])
    for name, ty in (("var_pos", i64p), ("var_type", i32p), ("var_cate", i32p), ("is_homopolymer_indel", i32p), ("total_cov", i32p),
                     ("alle_off", i32p), ("alle_covs", i32p), ("start_var_idx", i32p), ("end_var_idx", i32p), ("allele_off", i32p),
                     ("alleles", i32p), ("ordered_read_ids", i32p), ("cr_read", i32p)):
        a = np.ascontiguousarray(prob[name], np.int64 if ty is i64p else np.int32)
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        keep.append(a)
        setattr(s, name, a.ctypes.data_as(ty))
    sk = np.ascontiguousarray(prob["is_skipped"], np.uint8)
    keep.append(sk)
    s.is_skipped = sk.ctypes.data_as(u8p)
    for name, ty in (("haps", i32p), ("phase_sets", i64p), ("n_clean_agree_snps", i32p), ("n_clean_conflict_snps", i32p), ("var_phase_set", i64p),
                     ("hap_to_cons_alle", i32p), ("hap_to_alle_profile", i32p)):
        setattr(s, name, state[name].ctypes.data_as(ty))
    return s


def assign_hap_germline(prob, target_var_cate, state=None):
    """assign_hap_based_on_germline_het_vars_kmeans (src/assign_hap.c:473) on a flattened chunk; returns the mutated state dict"""
    from ._lib import LcdHapProblem
    lib = load_library()
    state = state or _hap_state(prob)
    keep = []
    s = _fill_hap_struct(LcdHapProblem, prob, state, keep)
    check(lib.lcd_assign_hap_germline(C.byref(s), int(target_var_cate)), lib)
    return state


def assign_hap_batch(probs, target_var_cates, states=None):
    """lcd_assign_hap_batch: K5 on several chunks in one launch (one wavefront per chunk); returns the mutated state dicts"""
    from ._lib import LcdHapProblem
    lib = load_library()
    states = states or [_hap_state(p) for p in probs]
    keep = []
    arr = (LcdHapProblem * len(probs))(*[_fill_hap_struct(LcdHapProblem, p, st, keep) for p, st in zip(probs, states)])
    cates = np.ascontiguousarray(target_var_cates, np.int32)
    check(lib.lcd_assign_hap_batch(len(probs), arr, cates.ctypes.data_as(C.POINTER(C.c_int))), lib)
    return states


# ---------------- chunk->ordered_read_ids: the NM tags of a BAM chunk's records and sort_chunk_reads ----------------
def chunk_read_nm(chunk):
    """lcd_chunk_read_nm: bam_get_NM per kept read of a DeviceChunk made from a BAM, computed on the records in HBM; LcdError (-4) for a host-array chunk"""
    lib = load_library()
    n = int(chunk.n)
    nm = np.zeros(max(1, n), np.int32)
    check(lib.lcd_chunk_read_nm(chunk.h, nm.ctypes.data_as(i32p)), lib)
    return nm[:n].copy()


def sort_chunk_reads(pos0, end_pos, nm, names):
    """lcd_sort_chunk_reads (sort_chunk_reads, src/bam_utils.c:1616-1656; host code): pos ascending, end descending, NM ascending, strcmp of the names, file order
    on a full tie -> the read ids in that order.  names: bytes / str per read."""
    lib = load_library()
    n = len(pos0)
    pos0 = np.ascontiguousarray(pos0, np.int64); end_pos = np.ascontiguousarray(end_pos, np.int64); nm = np.ascontiguousarray(nm, np.int32)
    raw = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
    off = np.zeros(max(1, n), np.uint64); pool = bytearray()
    for i, x in enumerate(raw):
        off[i] = len(pool); pool += x + b"\0"
    order = np.zeros(max(1, n), np.int32)
    z = lambda a, dt: a if a.size else np.zeros(1, dt)
    check(lib.lcd_sort_chunk_reads(n, z(pos0, np.int64).ctypes.data_as(C.POINTER(C.c_int64)), z(end_pos, np.int64).ctypes.data_as(C.POINTER(C.c_int64)),
                                   z(nm, np.int32).ctypes.data_as(i32p), off.ctypes.data_as(C.POINTER(C.c_uint64)), bytes(pool) + b"\0", order.ctypes.data_as(i32p)), lib)
    return order[:n].copy()


# ---------------- the first round of collect_var_main on a device-resident chunk (lcd_chunk_clean_vars) ----------------
def clean_opt(is_ont=0, **kw):
    """lcd_clean_opt_t with the defaults of src/call_var_main.c (HiFi or ONT); keyword arguments override fields"""
    lib = load_library()
    o = LcdCleanOpt()
    lib.lcd_clean_opt_default(C.byref(o), int(is_ont))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def clean_vars_dict(v):
    """an lcd_clean_vars_t (this library's or the test oracle's: same layout) -> dict of numpy copies"""
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n > 0 and p else np.zeros(0, dt)
    V, R = v.n_vars, v.n_reads
    alt_off = arr(v.alt_off, V + 1, np.uint64) if v.alt_off else np.zeros(1, np.uint64)
    aoff = arr(v.allele_off, R + 1, np.uint64) if v.allele_off else np.zeros(1, np.uint64)
    regs = np.array([(v.regs[i].start, v.regs[i].end, v.regs[i].label) for i in range(v.n_regs)], np.int64).reshape(-1, 3)
    arb = getattr(v, "alt_ref_base", None)    # (the test oracle's struct ends before this member; a NULL member counts as all 4)
    return dict(alt_ref_base=arr(arb, V, np.uint8) if arb else np.full(V, 4, np.uint8), n_vars=V, pos=arr(v.pos, V, np.int64), var_type=arr(v.var_type, V, np.int32), ref_len=arr(v.ref_len, V, np.int32), alt_len=arr(v.alt_len, V, np.int32),
                cate=arr(v.cate, V, np.int32), total_cov=arr(v.total_cov, V, np.int32), low_qual_cov=arr(v.low_qual_cov, V, np.int32),
                alle_covs=arr(v.alle_covs, 2 * V, np.int32), strand_alle_covs=arr(v.strand_alle_covs, 4 * V, np.int32), alt_off=alt_off,
                alt_pool=arr(v.alt_pool, int(alt_off[-1]), np.uint8), is_homopolymer_indel=arr(v.is_homopolymer_indel, V, np.int32), regs=regs, n_reads=R,
                start_var_idx=arr(v.start_var_idx, R, np.int32), end_var_idx=arr(v.end_var_idx, R, np.int32), allele_off=aoff,
                alleles=arr(v.alleles, int(aoff[-1]), np.int32), alt_qi=arr(v.alt_qi, int(aoff[-1]), np.int32), cr_read=arr(v.cr_read, v.n_cr, np.int32),
                qual_upload_bytes=int(v.qual_upload_bytes))


# every array of lcd_clean_vars_t (what "equal field for field" compares)
CLEAN_VARS_FIELDS = ("pos", "var_type", "ref_len", "alt_len", "cate", "total_cov", "low_qual_cov", "alle_covs", "strand_alle_covs", "alt_off", "alt_pool",
                     "is_homopolymer_indel", "regs", "start_var_idx", "end_var_idx", "allele_off", "alleles", "alt_qi", "cr_read")


def _clean_args(a, keep):
    i32p, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    ordered = np.ascontiguousarray(a["ordered_read_ids"], np.int32)
    ref = np.ascontiguousarray(a["ref"], np.uint8)
    pre = np.asarray(a.get("pre_regs", ()), np.int64).reshape(-1, 3)
    prearr = (LcdNoisyIv * max(1, len(pre)))(*[LcdNoisyIv(int(x[0]), int(x[1]), int(x[2]), 0) for x in pre])
    low = np.ascontiguousarray(np.asarray(a.get("low_comp", ()), np.int64).reshape(-1, 2))
    lowa = low.reshape(-1) if low.size else np.zeros(2, np.int64)
    rev = None if a.get("is_rev") is None else np.ascontiguousarray(a["is_rev"], np.uint8)
    keep += [ordered, ref, prearr, lowa, rev]
    return (ordered.ctypes.data_as(i32p), None if rev is None else _p8(rev), _p8(ref), int(a["ref_beg"]), int(a["ref_end"]), int(a["reg_beg"]), int(a["reg_end"]),
            C.cast(prearr, C.POINTER(LcdNoisyIv)), len(pre), lowa.ctypes.data_as(i64p), len(low))


def chunk_clean_vars_batch(chunks, args, opt=None, single=False):
    """lcd_chunk_clean_vars_batch over DeviceChunks; args[i] = dict(ordered_read_ids, ref, ref_beg, ref_end, reg_beg, reg_end, pre_regs (k,3), low_comp (n,2), is_rev)
    -> list of clean_vars_dict; single=True: one chunk through lcd_chunk_clean_vars"""
    lib = load_library()
    opt = opt if opt is not None else clean_opt()
    keep = []
    packs = [_clean_args(a, keep) for a in args]
    n = len(chunks)
    outs = (LcdCleanVars * n)()
    if single:
        check(lib.lcd_chunk_clean_vars(chunks[0].h, C.byref(opt), *packs[0], C.byref(outs[0])), lib)
    else:
        i32p, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
        col = lambda k, ty: (ty * n)(*[p[k] for p in packs])
        check(lib.lcd_chunk_clean_vars_batch(n, (C.c_void_p * n)(*[c.h for c in chunks]), C.byref(opt), col(0, i32p), col(1, u8p), col(2, u8p), col(3, C.c_int64),
                                             col(4, C.c_int64), col(5, C.c_int64), col(6, C.c_int64), col(7, C.POINTER(LcdNoisyIv)), col(8, C.c_int),
                                             col(9, i64p), col(10, C.c_int), outs), lib)
    res = []
    for i in range(n):
        res.append(clean_vars_dict(outs[i]))
        lib.lcd_clean_vars_free(C.byref(outs[i]))
    return res


def clean_vars_hap_problem(cv, ordered_read_ids, is_skipped, is_ont=0):
    """the K5 problem (assign_hap_germline's dict) over a clean_vars_dict, laid out by lcd_clean_vars_hap_problem (the C entry point fills the view; the
    arrays it points at are copied out)"""
    from ._lib import LcdHapProblem
    lib = load_library()
    V, R = cv["n_vars"], cv["n_reads"]
    keep = []
    def P(a, dt, ty):
        a = np.ascontiguousarray(a, dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ty))
    v = LcdCleanVars()
    v.n_vars, v.n_reads, v.n_cr = V, R, len(cv["cr_read"])
    v.pos = P(cv["pos"], np.int64, C.c_int64); v.var_type = P(cv["var_type"], np.int32, C.c_int); v.cate = P(cv["cate"], np.int32, C.c_int)
    v.is_homopolymer_indel = P(cv["is_homopolymer_indel"], np.int32, C.c_int); v.total_cov = P(cv["total_cov"], np.int32, C.c_int)
    v.alle_covs = P(cv["alle_covs"], np.int32, C.c_int); v.start_var_idx = P(cv["start_var_idx"], np.int32, C.c_int)
    v.end_var_idx = P(cv["end_var_idx"], np.int32, C.c_int); v.allele_off = P(cv["allele_off"], np.uint64, C.c_uint64)
    v.alleles = P(cv["alleles"], np.int32, C.c_int); v.cr_read = P(cv["cr_read"], np.int32, C.c_int)
    ordered = np.ascontiguousarray(ordered_read_ids, np.int32); skipped = np.ascontiguousarray(is_skipped, np.uint8)
    alle_off = np.zeros(V + 1, np.int32); allele_off = np.zeros(R + 1, np.int32)
    p = LcdHapProblem()
    check(lib.lcd_clean_vars_hap_problem(C.byref(v), int(is_ont), ordered.ctypes.data_as(C.POINTER(C.c_int)), _p8(skipped), alle_off.ctypes.data_as(C.POINTER(C.c_int)),
                                         allele_off.ctypes.data_as(C.POINTER(C.c_int)), C.byref(p)), lib)
    def out(ptr, n, dt):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n > 0 else np.zeros(0, dt)
    na = int(allele_off[-1])
    return dict(n_reads=p.n_reads, n_vars=p.n_vars, is_ont=p.is_ont, var_pos=out(p.var_pos, V, np.int64), var_type=out(p.var_type, V, np.int32),
                var_cate=out(p.var_cate, V, np.int32), is_homopolymer_indel=out(p.is_homopolymer_indel, V, np.int32), total_cov=out(p.total_cov, V, np.int32),
                alle_off=out(p.alle_off, V + 1, np.int32), alle_covs=out(p.alle_covs, int(alle_off[-1]), np.int32),
                start_var_idx=out(p.start_var_idx, R, np.int32), end_var_idx=out(p.end_var_idx, R, np.int32), allele_off=out(p.allele_off, R + 1, np.int32),
                alleles=out(p.alleles, na, np.int32), ordered_read_ids=out(p.ordered_read_ids, R, np.int32), is_skipped=out(p.is_skipped, R, np.uint8),
                cr_read=out(p.cr_read, p.n_cr, np.int32))


# ---------------- a pass's noisy-region variants merged into the chunk (lcd_merge_region_vars) ----------------
def _clean_vars_struct(cv, keep):
    """a clean_vars_dict -> LcdCleanVars over numpy copies (kept alive in `keep`)"""
    def P(a, dt, ty):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ty))
    v = LcdCleanVars()
    v.n_vars, v.n_reads, v.n_cr = int(cv["n_vars"]), int(cv["n_reads"]), len(cv["cr_read"])
    v.pos = P(cv["pos"], np.int64, C.c_int64)
    for k in ("var_type", "ref_len", "alt_len", "cate", "total_cov", "low_qual_cov", "alle_covs", "strand_alle_covs", "is_homopolymer_indel", "start_var_idx",
              "end_var_idx", "alleles", "alt_qi", "cr_read"):
        setattr(v, k, P(cv[k], np.int32, C.c_int))
    v.alt_off = P(cv["alt_off"], np.uint64, C.c_uint64); v.allele_off = P(cv["allele_off"], np.uint64, C.c_uint64); v.alt_pool = P(cv["alt_pool"], np.uint8, C.c_uint8)
    if cv.get("alt_ref_base") is not None:      # (absent: the member stays NULL = all 4)
        v.alt_ref_base = P(cv["alt_ref_base"], np.uint8, C.c_uint8)
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    ra = (LcdNoisyIv * max(1, len(regs)))(*[LcdNoisyIv(int(x[0]), int(x[1]), int(x[2]), 0) for x in regs])
    keep.append(ra)
    v.n_regs, v.regs = len(regs), C.cast(ra, C.POINTER(LcdNoisyIv))
    return v


def _region_vars_array(regions, keep):
    """RegionBatch.region_vars dicts -> (LcdRegionVars * n)"""
    from ._lib import LcdRegionVars
    arr = (LcdRegionVars * max(1, len(regions)))()
    for k, g in enumerate(regions):
        n, rows = int(g["n_vars"]), int(g.get("n_rows", len(g["row_read_ids"])))
        va = (LcdNoisyVar * max(1, n))()
        for i in range(max(n, 0)):
            x = va[i]
            x.pos, x.var_type, x.ref_len, x.alt_len, x.cate = int(g["pos"][i]), int(g["var_type"][i]), int(g["ref_len"][i]), int(g["alt_len"][i]), int(g["cate"][i])
            x.is_homopolymer_indel, x.total_cov = int(g["is_homopolymer_indel"][i]), int(g["total_cov"][i])
            if "alt_ref_base" in g:
                x.alt_ref_base = int(g["alt_ref_base"][i])
            x.alle_covs[0], x.alle_covs[1] = int(g["alle_covs"][i][0]), int(g["alle_covs"][i][1])
            a = np.ascontiguousarray(g["alt_seqs"][i], np.uint8)
            if a.size:
                keep.append(a)
                x.alt_seq = _p8(a)
        cols = [np.ascontiguousarray(g[name], np.int32).reshape(-1) for name in ("row_read_ids", "prof_start", "prof_end", "prof_alleles")]
        cols = [c if c.size else np.zeros(1, np.int32) for c in cols]
        keep += [va] + cols
        arr[k].n_vars, arr[k].vars, arr[k].n_rows = n, C.cast(va, C.POINTER(LcdNoisyVar)), rows
        arr[k].row_read_ids, arr[k].prof_start, arr[k].prof_end, arr[k].prof_alleles = [c.ctypes.data_as(i32p) for c in cols]
    keep.append(arr)
    return arr


def merge_region_vars_batch(cvs, regions, ordered, skipped, single=False, n_regions=None):
    """lcd_merge_region_vars_batch: cvs[i] = clean_vars_dict, regions[i] = list of RegionBatch.region_vars dicts in processing order, ordered[i] / skipped[i] = the
    chunk's ordered_read_ids / is_skipped -> list of (clean_vars_dict, cur_to_merged, [region_to_merged per region]); single=True: one chunk through
    lcd_merge_region_vars.  n_regions overrides the region counts handed to the library (tests of the argument checks)."""
    from ._lib import LcdRegionVars
    lib = load_library()
    n = len(cvs)
    keep = []
    cur = [_clean_vars_struct(cv, keep) for cv in cvs]
    regs = [_region_vars_array(r, keep) for r in regions]
    nreg = [len(r) for r in regions] if n_regions is None else list(n_regions)
    ords = [np.ascontiguousarray(o, np.int32) if len(o) else np.zeros(1, np.int32) for o in ordered]
    skips = [np.ascontiguousarray(s_, np.uint8) if len(s_) else np.zeros(1, np.uint8) for s_ in skipped]
    c2m = [np.full(max(1, cv["n_vars"]), -1, np.int32) for cv in cvs]
    r2m = [[np.full(max(1, int(g["n_vars"])), -1, np.int32) for g in r] for r in regions]
    r2m_p = [(i32p * max(1, len(r)))(*[a.ctypes.data_as(i32p) for a in r]) for r in r2m]
    outs = (LcdCleanVars * n)()
    if single:
        check(lib.lcd_merge_region_vars(C.byref(cur[0]), nreg[0], regs[0], ords[0].ctypes.data_as(i32p), _p8(skips[0]), C.byref(outs[0]), c2m[0].ctypes.data_as(i32p),
                                        r2m_p[0]), lib)
    else:
        check(lib.lcd_merge_region_vars_batch(n, (C.POINTER(LcdCleanVars) * n)(*[C.pointer(c) for c in cur]), (C.c_int * n)(*nreg),
                                              (C.POINTER(LcdRegionVars) * n)(*[C.cast(r, C.POINTER(LcdRegionVars)) for r in regs]),
                                              (i32p * n)(*[o.ctypes.data_as(i32p) for o in ords]), (u8p * n)(*[_p8(s_) for s_ in skips]), outs,
                                              (i32p * n)(*[a.ctypes.data_as(i32p) for a in c2m]), (C.POINTER(i32p) * n)(*[C.cast(p, C.POINTER(i32p)) for p in r2m_p])), lib)
    res = []
    for i in range(n):
        d = clean_vars_dict(outs[i])
        lib.lcd_clean_vars_free(C.byref(outs[i]))
        res.append((d, c2m[i][:cvs[i]["n_vars"]].copy(), [a[:max(0, int(g["n_vars"]))].copy() for a, g in zip(r2m[i], regions[i])]))
    return res


def merge_region_vars(cv, regions, ordered, skipped, n_regions=None):
    """lcd_merge_region_vars on one chunk -> (clean_vars_dict, cur_to_merged, [region_to_merged per region])"""
    return merge_region_vars_batch([cv], [regions], [ordered], [skipped], single=True, n_regions=None if n_regions is None else [n_regions])[0]


def sort_noisy_regs(regs):
    """lcd_sort_noisy_regs (sort_noisy_regs, src/collect_var.c:2745): regs (n, 3) start / end / label -> the processing order (indices)"""
    lib = load_library()
    regs = np.asarray(regs, np.int64).reshape(-1, 3)
    arr = (LcdNoisyIv * max(1, len(regs)))(*[LcdNoisyIv(int(x[0]), int(x[1]), int(x[2]), 0) for x in regs])
    order = np.zeros(max(1, len(regs)), np.int32)
    check(lib.lcd_sort_noisy_regs(arr, len(regs), order.ctypes.data_as(i32p)), lib)
    return order[:len(regs)].copy()


# ---------------- the noisy-region rounds of collect_var_main on device-resident chunks (lcd_chunk_plan_pass ... lcd_chunks_noisy_rounds) ----------------
PLAN_DONE_BEFORE, PLAN_SKIP_LONG, PLAN_SKIP_DEEP, PLAN_NO_READS, PLAN_SUBMIT = range(5)   # LCD_PLAN_*
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]


def pass_opt(**kw):
    """lcd_pass_opt_t with the defaults of src/call_var_main.h:36-42 (50000 / 1000 / 10); keyword arguments override fields"""
    from ._lib import LcdPassOpt
    o = LcdPassOpt()
    load_library().lcd_pass_opt_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _iv_array(regs, keep):
    regs = np.asarray(regs, np.int64).reshape(-1, 3)
    arr = (LcdNoisyIv * max(1, len(regs)))(*[LcdNoisyIv(int(x[0]), int(x[1]), int(x[2]), 0) for x in regs])
    keep.append(arr)
    return arr, len(regs)


def _pass_plan_struct(plan, keep):
    """a plan_pass dict -> LcdPassPlan over numpy copies"""
    from ._lib import LcdPassPlan
    def P(a, dt, ty):
        a = np.ascontiguousarray(a, dt).reshape(-1)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ty))
    pl = LcdPassPlan()
    pl.n_regs = len(plan["status"])
    pl.status = P(plan["status"], np.int32, C.c_int); pl.beg = P(plan["beg"], np.int64, C.c_int64); pl.end = P(plan["end"], np.int64, C.c_int64)
    pl.read_off = P(plan["read_off"], np.uint64, C.c_uint64)
    for k in ("read_ids", "read_beg", "read_end", "cover"):
        setattr(pl, k, P(plan[k], np.int32, C.c_int))
    return pl


def _pass_plan_dict(pl):
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n > 0 and p else np.zeros(0, dt)
    n = pl.n_regs
    off = arr(pl.read_off, n + 1, np.uint64) if pl.read_off else np.zeros(1, np.uint64)
    m = int(off[-1])
    return dict(status=arr(pl.status, n, np.int32), beg=arr(pl.beg, n, np.int64), end=arr(pl.end, n, np.int64), read_off=off.astype(np.int64),
                read_ids=arr(pl.read_ids, m, np.int32), read_beg=arr(pl.read_beg, m, np.int32), read_end=arr(pl.read_end, m, np.int32), cover=arr(pl.cover, m, np.int32))


def plan_pass_batch(chunks, args, opt=None, single=False, n_regs=None):
    """lcd_chunk_plan_pass_batch over DeviceChunks: args[i] = dict(regs (n, 3) start / end / label, done (n), ordered_read_ids, is_skipped, ref_beg, ref_end)
    -> list of dict(status, beg, end, read_off, read_ids, read_beg, read_end, cover); single=True: one chunk through lcd_chunk_plan_pass.  A chunk may be None
    and n_regs may override the region counts (tests of the argument checks)."""
    from ._lib import LcdPassPlan
    lib = load_library()
    opt = opt if opt is not None else pass_opt()
    n = len(chunks)
    keep = []
    ivs = [_iv_array(a["regs"], keep) for a in args]
    nreg = [x[1] for x in ivs] if n_regs is None else list(n_regs)
    nz = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(1, dt)
    done = [nz(a["done"], np.int32) for a in args]; ords = [nz(a["ordered_read_ids"], np.int32) for a in args]; skips = [nz(a["is_skipped"], np.uint8) for a in args]
    hs = [None if c is None else c.h for c in chunks]
    outs = (LcdPassPlan * n)()
    if single:
        check(lib.lcd_chunk_plan_pass(hs[0], C.byref(opt), nreg[0], ivs[0][0], done[0].ctypes.data_as(i32p), ords[0].ctypes.data_as(i32p), _p8(skips[0]),
                                      int(args[0]["ref_beg"]), int(args[0]["ref_end"]), C.byref(outs[0])), lib)
    else:
        check(lib.lcd_chunk_plan_pass_batch(n, (C.c_void_p * n)(*hs), C.byref(opt), (C.c_int * n)(*nreg),
                                            (C.POINTER(LcdNoisyIv) * n)(*[C.cast(x[0], C.POINTER(LcdNoisyIv)) for x in ivs]),
                                            (i32p * n)(*[d.ctypes.data_as(i32p) for d in done]), (i32p * n)(*[o.ctypes.data_as(i32p) for o in ords]),
                                            (u8p * n)(*[_p8(s) for s in skips]), (C.c_int64 * n)(*[int(a["ref_beg"]) for a in args]),
                                            (C.c_int64 * n)(*[int(a["ref_end"]) for a in args]), outs), lib)
    res = []
    for i in range(n):
        res.append(_pass_plan_dict(outs[i]))
        lib.lcd_pass_plan_free(C.byref(outs[i]))
    return res


def plan_pass(chunk, regs, done, ordered_read_ids, is_skipped, ref_beg, ref_end, opt=None, n_regs=None):
    """lcd_chunk_plan_pass: the plan of one noisy-region pass of a DeviceChunk (see plan_pass_batch)"""
    return plan_pass_batch([chunk], [dict(regs=regs, done=done, ordered_read_ids=ordered_read_ids, is_skipped=is_skipped, ref_beg=ref_beg, ref_end=ref_end)], opt,
                           single=True, n_regs=None if n_regs is None else [n_regs])[0]


_STATE_FIELDS = (("haps", np.int32), ("phase_sets", np.int64), ("n_clean_agree_snps", np.int32), ("n_clean_conflict_snps", np.int32), ("var_phase_set", np.int64),
                 ("hap_to_cons_alle", np.int32), ("hap_to_alle_profile", np.int32))


def _malloc_copy(a, ty):
    """a numpy array -> a malloc()'d copy (for structures the library takes ownership of)"""
    a = np.ascontiguousarray(a).reshape(-1)
    p = _libc.malloc(max(a.nbytes, 8))
    if a.nbytes:
        C.memmove(p, a.ctypes.data, a.nbytes)
    return C.cast(p, C.POINTER(ty))


def _hap_state_struct(state, n_reads, n_vars, keep=None):
    """a K5 state dict -> LcdHapState; keep=None: malloc()'d copies, else numpy copies kept alive in keep"""
    from ._lib import LcdHapState
    s = LcdHapState()
    s.n_reads, s.n_vars = int(n_reads), int(n_vars)
    for k, dt in _STATE_FIELDS:
        ty = C.c_int64 if dt is np.int64 else C.c_int
        a = np.ascontiguousarray(state[k], dt).reshape(-1)
        if keep is None:
            setattr(s, k, _malloc_copy(a, ty))
        else:
            a = a.copy() if a.size else np.zeros(1, dt)
            keep.append(a)
            setattr(s, k, a.ctypes.data_as(C.POINTER(ty)))
    return s


def _hap_state_dict(s):
    R, V = s.n_reads, s.n_vars
    size = dict(haps=R, phase_sets=R, n_clean_agree_snps=R, n_clean_conflict_snps=R, var_phase_set=V, hap_to_cons_alle=3 * V, hap_to_alle_profile=6 * V)
    return {k: (np.ctypeslib.as_array(getattr(s, k), shape=(size[k],)).astype(dt).copy() if size[k] > 0 else np.zeros(0, dt)) for k, dt in _STATE_FIELDS}


def hap_state_carry(state, n_merged_vars, cur_to_merged):
    """lcd_hap_state_carry: K5's state dict (assign_hap_germline) on the merged table of merge_region_vars: per-read arrays unchanged, per-variant arrays through
    cur_to_merged, fresh values for the variants that came from a region"""
    from ._lib import LcdHapState
    lib = load_library()
    keep = []
    c2m = np.ascontiguousarray(cur_to_merged, np.int32)
    old = _hap_state_struct(state, len(state["haps"]), len(state["var_phase_set"]), keep)
    out = LcdHapState()
    check(lib.lcd_hap_state_carry(C.byref(old), int(n_merged_vars), (c2m if c2m.size else np.zeros(1, np.int32)).ctypes.data_as(i32p), C.byref(out)), lib)
    res = _hap_state_dict(out)
    lib.lcd_hap_state_free(C.byref(out))
    return res


def _clean_vars_struct_malloc(cv):
    """a clean_vars_dict -> LcdCleanVars whose arrays are malloc()'d (lcd_clean_vars_free releases them)"""
    v = LcdCleanVars()
    v.n_vars, v.n_reads, v.n_cr = int(cv["n_vars"]), int(cv["n_reads"]), len(cv["cr_read"])
    v.pos = _malloc_copy(np.asarray(cv["pos"], np.int64), C.c_int64)
    for k in ("var_type", "ref_len", "alt_len", "cate", "total_cov", "low_qual_cov", "alle_covs", "strand_alle_covs", "is_homopolymer_indel", "start_var_idx",
              "end_var_idx", "alleles", "alt_qi", "cr_read"):
        setattr(v, k, _malloc_copy(np.asarray(cv[k], np.int32), C.c_int))
    v.alt_off = _malloc_copy(np.asarray(cv["alt_off"], np.uint64), C.c_uint64); v.allele_off = _malloc_copy(np.asarray(cv["allele_off"], np.uint64), C.c_uint64)
    v.alt_pool = _malloc_copy(np.asarray(cv["alt_pool"], np.uint8), C.c_uint8)
    if cv.get("alt_ref_base") is not None:
        v.alt_ref_base = _malloc_copy(np.asarray(cv["alt_ref_base"], np.uint8), C.c_uint8)
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    flat = np.zeros((max(1, len(regs)), 3), np.int64)    # lcd_noisy_iv_t: int64 start, end | int32 label, pad
    flat[:len(regs), :2] = regs[:, :2]; flat.view(np.int32).reshape(len(flat), 6)[:len(regs), 4] = regs[:, 2]
    v.n_regs, v.regs = len(regs), C.cast(_malloc_copy(flat, C.c_int64), C.POINTER(LcdNoisyIv))
    return v


class RefineLog:
    """lcd_refine_log_t: the (cluster, read) entries of the noisy regions a chunk's rounds resolved, in the reference's order"""

    def __init__(self):
        self.lib = load_library()
        self.h = self.lib.lcd_refine_log_create()
        if not self.h:
            raise LcdError("lcd_refine_log_create failed")

    def close(self):
        if self.h:
            self.lib.lcd_refine_log_free(self.h); self.h = None

    def __len__(self):
        return int(self.lib.lcd_refine_log_n_entries(self.h))

    def row_bytes(self):
        return int(self.lib.lcd_refine_log_row_bytes(self.h))

    def append(self, read_id, cover, read_beg, read_end, reg_beg, reg_end, target, query, pass_=0):
        from ._lib import LcdRefineEntry
        t = np.ascontiguousarray(target, np.uint8); q = np.ascontiguousarray(query, np.uint8)
        assert len(t) == len(q)
        e = LcdRefineEntry(int(read_id), int(cover), int(read_beg), int(read_end), len(t), int(pass_), int(reg_beg), int(reg_end), _p8(t), _p8(q))
        check(self.lib.lcd_refine_log_append(self.h, C.byref(e)), self.lib)

    def entries(self):
        """-> [dict(read_id, cover, read_beg, read_end, reg_beg, reg_end, pass_, target, query)] in log order"""
        from ._lib import LcdRefineEntry
        out = []
        for i in range(len(self)):
            e = LcdRefineEntry()
            check(self.lib.lcd_refine_log_entry(self.h, i, C.byref(e)), self.lib)
            row = lambda p: np.ctypeslib.as_array(p, shape=(max(e.aln_len, 1),))[:e.aln_len].copy() if e.aln_len else np.zeros(0, np.uint8)
            out.append(dict(read_id=e.read_id, cover=e.cover, read_beg=e.read_beg, read_end=e.read_end, reg_beg=e.reg_beg, reg_end=e.reg_end, pass_=e.pass_,
                            target=row(e.target), query=row(e.query)))
        return out

    def apply(self, digars, qlens):
        """lcd_refine_log_apply on per-read (n, 5) digar rows (DeviceChunk.digars()) -> ({read id: final (n, 5) rows} of the reads the log names, entries rejected)"""
        n = len(digars)
        off = np.concatenate([[0], np.cumsum([len(d) for d in digars])]).astype(np.uint64)
        dg = (LcdDigar * max(int(off[-1]), 1))()
        k = 0
        for d in digars:
            for x in np.asarray(d, np.int64).reshape(-1, 5):
                dg[k].pos, dg[k].type, dg[k].len, dg[k].qi, dg[k].is_low_qual = int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[4]); k += 1
        ql = np.ascontiguousarray(qlens, np.int32)
        nt, ids, toff, tdg, rej = C.c_int(0), i32p(), C.POINTER(C.c_uint64)(), C.POINTER(LcdDigar)(), C.c_int64(0)
        check(self.lib.lcd_refine_log_apply(self.h, n, off.ctypes.data_as(C.POINTER(C.c_uint64)), dg, ql.ctypes.data_as(i32p), C.byref(nt), C.byref(ids), C.byref(toff),
                                            C.byref(tdg), C.byref(rej)), self.lib)
        out = {}
        for t in range(nt.value):
            out[int(ids[t])] = np.array([[tdg[j].pos, tdg[j].type, tdg[j].len, tdg[j].qi, tdg[j].is_low_qual] for j in range(int(toff[t]), int(toff[t + 1]))], np.int64).reshape(-1, 5)
        for p_ in (ids, toff, tdg):
            if p_:
                _libc.free(C.cast(p_, C.c_void_p))
        return out, int(rej.value)


def chunks_noisy_rounds(chunks, items, opt=None, popt=None, logs=None):
    """lcd_chunks_noisy_rounds: DeviceChunks from "first round done" to the fixed point of collect_var_main's noisy-region loop (src/collect_var.c:2946-2977).
    items[i] = dict(cv = clean_vars_dict of the first round, state = K5 state after the clean-category call, ordered_read_ids, is_skipped, ref (codes),
    ref_beg, is_ont (optional)) -> list of dict(cv, state, done, n_passes, first_to_final).  logs = one RefineLog (or None) per chunk: lcd_chunks_noisy_rounds_log"""
    from ._lib import LcdRoundsChunk
    lib = load_library()
    opt = opt if opt is not None else default_opt()
    popt = popt if popt is not None else pass_opt()
    n = len(chunks)
    keep = []
    arr = (LcdRoundsChunk * max(1, n))()
    vs, ss = [], []
    for i, (ch, it) in enumerate(zip(chunks, items)):
        v = _clean_vars_struct_malloc(it["cv"]); s = _hap_state_struct(it["state"], it["cv"]["n_reads"], it["cv"]["n_vars"])
        vs.append(v); ss.append(s)
        ordered = np.ascontiguousarray(it["ordered_read_ids"], np.int32); skipped = np.ascontiguousarray(it["is_skipped"], np.uint8); ref = np.ascontiguousarray(it["ref"], np.uint8)
        keep += [ordered, skipped, ref]
        x = arr[i]
        x.chunk, x.vars, x.state = ch.h, C.pointer(v), C.pointer(s)
        x.ordered_read_ids, x.is_skipped, x.ref_seq = ordered.ctypes.data_as(i32p), _p8(skipped), _p8(ref)
        x.ref_beg, x.ref_end, x.is_ont = int(it["ref_beg"]), int(it["ref_beg"]) + len(ref) - 1, int(it.get("is_ont", 0))
    if logs is None:
        rc = lib.lcd_chunks_noisy_rounds(n, arr, C.byref(opt), C.byref(popt))
    else:
        assert len(logs) == n
        rc = lib.lcd_chunks_noisy_rounds_log(n, arr, C.byref(opt), C.byref(popt), (C.c_void_p * max(1, n))(*[g.h if g is not None else None for g in logs]))
    res = []
    try:
        check(rc, lib)
        for i in range(n):
            x = arr[i]
            nr, nf = vs[i].n_regs, x.n_first_vars
            res.append(dict(cv=clean_vars_dict(vs[i]), state=_hap_state_dict(ss[i]), n_passes=int(x.n_passes),
                            done=np.array([x.done[k] for k in range(nr)], np.int32), first_to_final=np.array([x.first_to_final[k] for k in range(nf)], np.int32)))
    finally:
        for i in range(n):
            lib.lcd_clean_vars_free(C.byref(vs[i])); lib.lcd_hap_state_free(C.byref(ss[i]))
            for p in (arr[i].done, arr[i].first_to_final):
                if p:
                    _libc.free(C.cast(p, C.c_void_p))
    return res


# ---------------- the head of collect_var_main on device-resident chunks (lcd_chunks_first_round) ----------------
def _bam_reads_struct(meta, keep):
    """DeviceChunk.meta -> LcdBamReads with the members the read order and the strands need (pos0, end_pos, flag, names)"""
    from ._lib import LcdBamReads
    m = LcdBamReads()
    n = len(meta["pos0"])
    pos0 = np.ascontiguousarray(meta["pos0"], np.int64); end = np.ascontiguousarray(meta["end_pos"], np.int64); flag = np.ascontiguousarray(meta["flag"], np.int32)
    off = np.zeros(max(1, n), np.uint64); pool = bytearray()
    for i, x in enumerate(meta["names"]):
        off[i] = len(pool); pool += (x.encode() if isinstance(x, str) else bytes(x)) + b"\0"
    buf = C.create_string_buffer(bytes(pool) + b"\0")
    z = lambda a, dt: a if a.size else np.zeros(1, dt)
    pos0, end, flag = z(pos0, np.int64), z(end, np.int64), z(flag, np.int32)
    keep += [pos0, end, flag, off, buf]
    m.n_reads = n
    m.pos0 = pos0.ctypes.data_as(C.POINTER(C.c_int64)); m.end_pos = end.ctypes.data_as(C.POINTER(C.c_int64)); m.flag = flag.ctypes.data_as(i32p)
    m.name_off = off.ctypes.data_as(C.POINTER(C.c_uint64)); m.name_pool = C.cast(buf, C.POINTER(C.c_char))
    return m


def _fill_first_chunk(x, ch, it, keep):
    """the input members of an lcd_first_chunk_t from a DeviceChunk and an item dict (see chunks_first_round)"""
    ref = np.ascontiguousarray(it["ref"], np.uint8)
    keep.append(ref)
    x.chunk = None if ch is None else ch.h
    x.ref_seq = _p8(ref); x.ref_beg = int(it["ref_beg"]); x.ref_end = int(it.get("ref_end", int(it["ref_beg"]) + len(ref) - 1))
    x.reg_beg, x.reg_end, x.is_ont = int(it["reg_beg"]), int(it["reg_end"]), int(it.get("is_ont", 0))
    if it.get("ordered_read_ids") is not None:
        o = np.ascontiguousarray(it["ordered_read_ids"], np.int32)
        o = o if o.size else np.zeros(1, np.int32)
        keep.append(o); x.ordered_read_ids = o.ctypes.data_as(i32p)
    if it.get("is_rev") is not None:
        r = np.ascontiguousarray(it["is_rev"], np.uint8)
        r = r if r.size else np.zeros(1, np.uint8)
        keep.append(r); x.is_rev = _p8(r)
    if it.get("meta", True) and ch is not None and getattr(ch, "meta", None) is not None:
        m = _bam_reads_struct(ch.meta, keep)
        keep.append(m); x.meta = C.pointer(m)


def _first_chunk_dict(x):
    """the out members of an lcd_first_chunk_t -> dict(ordered_read_ids, is_skipped, low_comp (n, 2), pre_regs (n, 3), cv, state)"""
    R = x.n_reads
    take = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(k,)).astype(dt).copy() if k > 0 else np.zeros(0, dt)
    return dict(ordered_read_ids=take(x.order, R, np.int32), is_skipped=take(x.is_skipped, R, np.uint8), low_comp=take(x.low_comp, 2 * x.n_low, np.int64).reshape(-1, 2),
                pre_regs=np.array([(x.pre_regs[k].start, x.pre_regs[k].end, x.pre_regs[k].label) for k in range(x.n_pre_regs)], np.int64).reshape(-1, 3),
                cv=clean_vars_dict(x.vars.contents), state=_hap_state_dict(x.state.contents))


def chunks_first_round(chunks, items, opt=None):
    """lcd_chunks_first_round: DeviceChunks -> "first round done" in one call.  items[i] = dict(ref (codes), ref_beg, reg_beg, reg_end, is_ont (0), ordered_read_ids
    (None: sort_chunk_reads from the chunk's meta and its NM tags), is_rev (None: from meta's flags when meta is used, else all forward), meta (True: hand the chunk's
    .meta to the library when it has one), ref_end (default ref_beg + len(ref) - 1)) -> list of dict(ordered_read_ids, is_skipped, low_comp (n, 2), pre_regs (n, 3),
    cv = clean_vars_dict, state = K5 state dict)"""
    from ._lib import LcdFirstChunk
    lib = load_library()
    opt = opt if opt is not None else clean_opt()
    n = len(chunks)
    keep = []
    arr = (LcdFirstChunk * max(1, n))()
    for i, (ch, it) in enumerate(zip(chunks, items)):
        _fill_first_chunk(arr[i], ch, it, keep)
    rc = lib.lcd_chunks_first_round(n, arr, C.byref(opt))
    res = []
    try:
        check(rc, lib)
        res = [_first_chunk_dict(arr[i]) for i in range(n)]
    finally:
        for i in range(n):
            lib.lcd_first_round_free(C.byref(arr[i]))
    return res


# ---------------- chunks -> stitched genotype records and VCF body lines (lcd_chunks_call, lcd_call_bam_regions) ----------------
def call_cfg(is_ont=0, clean=None, opt=None, pass_=None, call=None):
    """lcd_cfg_t with lcd_cfg_default's values; the keyword dicts override fields of the four option structs"""
    from ._lib import LcdCfg
    cfg = LcdCfg()
    load_library().lcd_cfg_default(C.byref(cfg), int(is_ont))
    for part, kw in (("clean", clean), ("opt", opt), ("pass_", pass_), ("call", call)):
        for k, v in (kw or {}).items():
            setattr(getattr(cfg, part), k, v)
    return cfg


def _var1_dict(v):
    return dict(cand_i=v.cand_i, pos=v.pos, PS=v.PS, type=v.type, ref_len=v.ref_len, n_alt=v.n_alt_allele, alt_len=list(v.alt_len)[:v.n_alt_allele],
                ref=bytes(v.ref_bases[j] for j in range(v.ref_len)), alt=[bytes(v.alt_bases[a][j] for j in range(v.alt_len[a])) for a in range(v.n_alt_allele)],
                GT=list(v.GT), DP=v.DP, AD=list(v.AD), QUAL=v.QUAL, GQ=v.GQ, is_sv=v.is_sv, is_clean=v.is_clean, alt_reads=[v.alt_read_i[j] for j in range(v.n_alt_reads)],
                tsd=bytes(v.tsd_seq[j] for j in range(v.tsd_len)), polya_len=v.polya_len, te_seq_i=v.te_seq_i, te_is_rev=v.te_is_rev, tsd_pos1=v.tsd_pos1, tsd_pos2=v.tsd_pos2)


def _call_result(lib, n, arr, recs, n_recs, text):
    try:
        chunks = []
        for i in range(n):
            d = _first_chunk_dict(arr[i].first)
            d.update(n_passes=int(arr[i].n_passes), flip_hap=int(arr[i].flip_hap), flip_pre_PS=int(arr[i].flip_pre_PS), flip_cur_PS=int(arr[i].flip_cur_PS),
                     n_records=int(arr[i].n_records), haps=d["state"]["haps"], phase_sets=d["state"]["phase_sets"])
            chunks.append(d)
        return dict(chunks=chunks, records=[_var1_dict(recs[i]) for i in range(n_recs.value)], vcf_body=C.string_at(text).decode() if text else "")
    finally:
        lib.lcd_call_free(n, arr, recs, n_recs.value, text)


class TeLib:
    """a TE library read from a FASTA file (te_lib_from_fasta): .names, .seq_lens in file order; check(seq) = lcd_check_te_seq -> (te_seq_i or -1, is_rev)"""

    def __init__(self, h, names, lens, n):
        self.h, self._names, self._lens, self.n = h, names, lens, n
        self.names = [names[i].decode() for i in range(n)]
        self.seq_lens = [int(lens[i]) for i in range(n)]

    def check(self, seq):
        lib = load_library()
        a = np.ascontiguousarray(seq, np.uint8)
        a = a if a.size else np.zeros(1, np.uint8)
        lib.lcd_check_te_seq.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, i32p]
        rev = C.c_int(0)
        return int(lib.lcd_check_te_seq(self.h, _p8(a), int(len(seq)), C.byref(rev))), int(rev.value)

    def close(self):
        if self.h:
            load_library().lcd_te_lib_from_fasta_free(self.h, self._names, self._lens, self.n)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def te_lib_from_fasta(path, kmer_len=0):
    """lcd_te_lib_from_fasta: the -T file (plain or gzip FASTA, read as kseq reads it) -> TeLib; kmer_len 0 = 15"""
    lib = load_library()
    h, names, lens, n = C.c_void_p(), C.POINTER(C.c_char_p)(), i32p(), C.c_int(0)
    check(lib.lcd_te_lib_from_fasta(str(path).encode(), int(kmer_len), C.byref(h), C.byref(names), C.byref(lens), C.byref(n)), lib)
    return TeLib(h, names, lens, n.value)


_RNAMES = {None: 0, "sv": 1, "all": 2}


def _vcf_fields(te_fasta, rnames, te_kmer_len=0):
    """the keywords te_fasta= / rnames=None|"sv"|"all" -> (LcdVcfFields, LcdVcfFieldsOut), or (None, None) without either: the entry point without options runs"""
    from ._lib import LcdVcfFields, LcdVcfFieldsOut
    if rnames not in _RNAMES:
        raise ValueError('rnames must be None, "sv" or "all"')
    if te_fasta is None and rnames is None:
        return None, None
    return LcdVcfFields(str(te_fasta).encode() if te_fasta is not None else None, int(te_kmer_len), _RNAMES[rnames]), LcdVcfFieldsOut()


def _fields_result(lib, res, vf, fo):
    """lcd_vcf_fields_out_t into a driver's result: "te_names", "n_mei_lines"; per record "te_name" (with a library) and "alt_read_names" (with a names mode: the list
    behind ALTREADS, [] for ".", None for a record the mode leaves out).  Frees *fo."""
    try:
        names = [fo.te_names[i].decode() for i in range(fo.n_te_seqs)]
        if vf.te_fasta_path is not None:
            res.update(te_names=names, n_mei_lines=int(fo.n_mei_lines))
        recs = res.get("records")
        if recs is not None and vf.te_fasta_path is not None:
            for r in recs:
                r["te_name"] = names[r["te_seq_i"]] if r["te_seq_i"] >= 0 else None
        if recs is not None and vf.rnames_mode:
            assert fo.n_rnames == len(recs)
            for i, r in enumerate(recs):
                v = fo.rnames[i]
                r["alt_read_names"] = None if v is None else [] if v == b"." else v.decode().split(",")
    finally:
        lib.lcd_vcf_fields_out_free(C.byref(fo))
    return res


def chunks_call(chunks, items, cfg=None, chrom="chr11", te_fasta=None, rnames=None):
    """lcd_chunks_call: DeviceChunks of one contig in genome order -> dict(chunks = per chunk the first-round dict with cv / state FINAL plus n_passes, flip_hap,
    flip_pre_PS, flip_cur_PS, n_records, haps, phase_sets; records = genotype records as dicts in chunk order; vcf_body).  items as for chunks_first_round.
    te_fasta= (the -T file) / rnames=None|"sv"|"all": lcd_chunks_call_fields, see _fields_result for what the result gains."""
    from ._lib import LcdCallChunk, LcdVar1
    lib = load_library()
    cfg = cfg if cfg is not None else call_cfg()
    n = len(chunks)
    keep = []
    arr = (LcdCallChunk * max(1, n))()
    for i, (ch, it) in enumerate(zip(chunks, items)):
        _fill_first_chunk(arr[i].first, ch, it, keep)
    recs, n_recs, text = C.POINTER(LcdVar1)(), C.c_int(0), C.c_void_p()
    vf, fo = _vcf_fields(te_fasta, rnames)
    if vf is not None:
        check(lib.lcd_chunks_call_fields(n, arr, C.byref(cfg), chrom.encode(), C.byref(vf), C.byref(recs), C.byref(n_recs), C.byref(text), C.byref(fo)), lib)
        return _fields_result(lib, _call_result(lib, n, arr, recs, n_recs, text), vf, fo)
    check(lib.lcd_chunks_call(n, arr, C.byref(cfg), chrom.encode(), C.byref(recs), C.byref(n_recs), C.byref(text)), lib)
    return _call_result(lib, n, arr, recs, n_recs, text)


call_chunks = chunks_call


def chunk_mod_pileup(chunk, haps, ref, ref_beg, ref_end, code="m", threshold=204, combine_strands=False):
    """DeviceChunk.mod_pileup"""
    return chunk.mod_pileup(haps, ref, ref_beg, ref_end, code, threshold, combine_strands)


class PhasedVcf:
    """lcd_phased_vcf_read (host only): the heterozygous phased sites of one sample of a VCF (plain, gzip or BGZF) as per-contig tables.  names: the contigs, in
    the order lcd_chunk_haplotag's `contig` counts them.  .stats: lcd_hapvcf_stats_t as a dict; .sites(contig): the table as a dict of arrays"""

    def __init__(self, path, names, sample=None, max_indel=50, snvs_only=False):
        from ._lib import LcdHapvcfOpt, LcdHapvcfStats
        lib = load_library()
        self.lib, self.names = lib, [str(n) for n in names]
        o = LcdHapvcfOpt(); lib.lcd_hapvcf_opt_default(C.byref(o))
        o.max_indel, o.snvs_only = int(max_indel), int(bool(snvs_only))
        arr = (C.c_char_p * max(len(self.names), 1))(*[n.encode() for n in self.names])
        st = LcdHapvcfStats()
        self.h = lib.lcd_phased_vcf_read(str(path).encode(), None if sample is None else str(sample).encode(), len(self.names), arr, C.byref(o), C.byref(st))
        if not self.h:
            raise LcdError(f"lcd_phased_vcf_read failed: error {lib.lcd_phased_vcf_errno()}: {lib.lcd_phased_vcf_error().decode()}")
        self.stats = {k: int(getattr(st, k)) for k, _t in st._fields_}

    def sites(self, contig):
        lib, c = self.lib, int(contig)
        n = int(lib.lcd_phased_vcf_n_sites(self.h, c))
        if n < 0:
            raise LcdError("PhasedVcf.sites: contig outside the tables'")
        nps, npool = int(lib.lcd_phased_vcf_n_phase_sets(self.h, c)), int(lib.lcd_phased_vcf_pool_size(self.h, c))
        a = dict(pos=np.zeros(n, np.int64), kind=np.zeros(n, np.uint8), hap_of_alt=np.zeros(n, np.uint8), len=np.zeros(n, np.int32), ref_code=np.zeros(n, np.uint8),
                 alt_code=np.zeros(n, np.uint8), ins_off=np.zeros(n, np.int64), ps_idx=np.zeros(n, np.int32), ps_value=np.zeros(nps, np.int64), pool=np.zeros(npool, np.uint8))
        u8p, i32p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_int64)
        ptr = lambda k, t: a[k].ctypes.data_as(t)
        check(lib.lcd_phased_vcf_sites_to_host(self.h, c, ptr("pos", i64p), ptr("kind", u8p), ptr("hap_of_alt", u8p), ptr("len", i32p), ptr("ref_code", u8p), ptr("alt_code", u8p),
                                               ptr("ins_off", i64p), ptr("ps_idx", i32p), ptr("ps_value", i64p), ptr("pool", u8p)), lib)
        a["max_footprint"] = int(lib.lcd_phased_vcf_max_footprint(self.h, c))
        return a

    def close(self):
        if self.h:
            self.lib.lcd_phased_vcf_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def phased_vcf_read(path, names, sample=None, max_indel=50, snvs_only=False):
    """PhasedVcf"""
    return PhasedVcf(path, names, sample, max_indel, snvs_only)


def _haplotag_stats(st):
    return {k: (list(getattr(st, k)) if k in ("n_verdict", "n_tagged") else getattr(st, k)) for k, _t in st._fields_}


def chunk_haplotag(chunk, vcf, contig, min_bq=0, min_diff=1, pairs=False):
    """lcd_chunk_haplotag: the kept records of a resolved chunk made from a BAM against the phased sites of contig `contig` (an index into vcf.names) ->
    dict(haps, phase_sets, n1, n2: one entry per kept read; stats); with pairs=True also first_site (per record), cand_off (records + 1) and verdict (one byte per
    candidate site: 0 NONE, 1 REF, 2 ALT, 3 OTHER, 4 LOWQ, 255 no pair)"""
    from ._lib import LcdHaplotagOpt, LcdHaplotagStats
    lib = load_library()
    o = LcdHaplotagOpt(); lib.lcd_haplotag_opt_default(C.byref(o))
    o.min_bq, o.min_diff = int(min_bq), int(min_diff)
    st = LcdHaplotagStats()
    h = lib.lcd_chunk_haplotag(chunk.h, vcf.h, int(contig), C.byref(o), C.byref(st))
    if not h:
        raise LcdError("lcd_chunk_haplotag failed: " + lib.lcd_last_error().decode())
    try:
        n = int(lib.lcd_haplotag_n_reads(h))
        haps, n1, n2, ps = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        i32p, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
        check(lib.lcd_haplotag_to_host(h, haps.ctypes.data_as(i32p), ps.ctypes.data_as(i64p), n1.ctypes.data_as(i32p), n2.ctypes.data_as(i32p)), lib)
        out = dict(haps=haps.tolist(), phase_sets=ps.tolist(), n1=n1.tolist(), n2=n2.tolist(), stats=_haplotag_stats(st))
        if pairs:
            nr, tot = int(lib.lcd_haplotag_n_records(h)), int(lib.lcd_haplotag_n_candidates(h))
            first, off, ver = np.zeros(nr, np.int64), np.zeros(nr + 1, np.int64), np.zeros(tot, np.uint8)
            check(lib.lcd_haplotag_pairs_to_host(h, first.ctypes.data_as(i64p), off.ctypes.data_as(i64p), ver.ctypes.data_as(C.POINTER(C.c_uint8))), lib)
            out.update(first_site=first.tolist(), cand_off=off.tolist(), verdict=ver)
        return out
    finally:
        lib.lcd_haplotag_free(h)


def _depth_stats(st):
    return {k: (list(getattr(st, k)) if k == "bases" else getattr(st, k)) for k, _t in st._fields_}


def chunk_depth(chunk, haps, skip_dels=False):
    """DeviceChunk.depth"""
    return chunk.depth(haps, skip_dels)


def depth_tile():
    """lcd_depth_tile (host only): the positions per workgroup of the depth track's row launches"""
    return int(load_library().lcd_depth_tile())


def _depth_arrays(rows):
    n = len(rows)
    beg = np.array([r[0] for r in rows] + [0], np.int64); end = np.array([r[1] for r in rows] + [0], np.int64)
    return n, beg, end, beg.ctypes.data_as(C.POINTER(C.c_int64)), end.ctypes.data_as(C.POINTER(C.c_int64))


def depth_windows(rows, window):
    """lcd_depth_windows (host only): rows [(beg, end, three depths)] that tile a span, in order -> the windows' rows [(beg, end, three sums of depth x positions)];
    window k of width `window` is [k * window + 1, (k + 1) * window]"""
    lib = load_library()
    n, beg, end, bp, ep = _depth_arrays(rows)
    dep = np.array([x for r in rows for x in r[2]] + [0] * 3, np.uint32)
    wb, we, ws = C.c_void_p(), C.c_void_p(), C.c_void_p()
    m = lib.lcd_depth_windows(n, bp, ep, dep.ctypes.data_as(C.POINTER(C.c_uint32)), int(window), C.byref(wb), C.byref(we), C.byref(ws))
    if m < 0:       # (host-only code: it sets no error text)
        raise LcdError(f"lcd_depth_windows: error {m}: a window below 1, or rows that are not in order and contiguous")
    try:
        b = np.ctypeslib.as_array(C.cast(wb, C.POINTER(C.c_int64)), (m + 1,)); e = np.ctypeslib.as_array(C.cast(we, C.POINTER(C.c_int64)), (m + 1,))
        v = np.ctypeslib.as_array(C.cast(ws, C.POINTER(C.c_uint64)), (3 * m + 3,))
        return [(int(b[k]), int(e[k]), tuple(int(x) for x in v[3 * k:3 * k + 3])) for k in range(m)]
    finally:
        _libc.free(wb); _libc.free(we); _libc.free(ws)


def depth_format(rows, chrom, windows=False, with_header=False):
    """lcd_depth_format (host only): the track's text for rows [(beg, end, three values)]; windows=True: the values are the 64-bit sums of depth_windows"""
    lib = load_library()
    n, beg, end, bp, ep = _depth_arrays(rows)
    vals = [x for r in rows for x in r[2]] + [0] * 3
    dep = np.array(vals, np.uint64 if windows else np.uint32)
    text = C.c_void_p()
    rc = lib.lcd_depth_format(n, bp, ep, None if windows else dep.ctypes.data_as(C.POINTER(C.c_uint32)), dep.ctypes.data_as(C.POINTER(C.c_uint64)) if windows else None,
                              _enc(chrom), int(bool(with_header)), C.byref(text))
    if rc < 0:
        raise LcdError(f"lcd_depth_format: error {rc}: a row with beg < 1 or end < beg")
    try:
        return C.string_at(text).decode()
    finally:
        _libc.free(text)


def mods_combine_rows(rows):
    """lcd_mods_combine_rows (host only): rows by position and strand -> the combined rows, keyed by the position of the CpG's C, strand '.'"""
    lib = load_library()
    n = len(rows)
    pos = np.array([r[0] for r in rows] + [0], np.int64); strand = C.create_string_buffer(b"".join(r[1].encode() for r in rows), n + 1)
    cnt = np.array([x for r in rows for x in r[2]] + [0] * 9, np.uint32)
    m = lib.lcd_mods_combine_rows(n, pos.ctypes.data_as(C.POINTER(C.c_int64)), strand, cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
    if m < 0:       # (host-only code: it sets no error text)
        raise LcdError(f"lcd_mods_combine_rows: error {m}: a strand outside + / -")
    return [(int(pos[k]), strand.raw[k:k + 1].decode(), tuple(int(x) for x in cnt[9 * k:9 * k + 9])) for k in range(m)]


def mods_format(rows, chrom, code="m", with_header=False):
    """lcd_mods_format (host only): the table's text for rows [(position, strand, nine counters)]"""
    lib = load_library()
    n = len(rows)
    pos = np.array([r[0] for r in rows] + [0], np.int64); strand = C.create_string_buffer(b"".join(r[1].encode() for r in rows), n + 1)
    cnt = np.array([x for r in rows for x in r[2]] + [0] * 9, np.uint32)
    text = C.c_void_p()
    rc = lib.lcd_mods_format(n, pos.ctypes.data_as(C.POINTER(C.c_int64)), strand, cnt.ctypes.data_as(C.POINTER(C.c_uint32)), _enc(chrom), ord(code) if len(code) == 1 else -1,
                             int(bool(with_header)), C.byref(text))
    if rc < 0:
        raise LcdError(f"lcd_mods_format: error {rc}: a code outside m / h or a strand outside + - .")
    try:
        return C.string_at(text).decode()
    finally:
        _libc.free(text)


def bgzf_deflate(data, block_payload=0, add_eof=1):
    """lcd_bgzf_deflate_dev: bytes -> dict(image = the BGZF file image compressed on the device, blocks = [(payload bytes, member bytes, kind 0 stored / 1 fixed /
    2 dynamic)], kernel_ms)"""
    lib = load_library()
    data = bytes(data)
    h = lib.lcd_bgzf_deflate_dev(data, len(data), int(block_payload), int(add_eof))
    if not h:
        raise LcdError("lcd_bgzf_deflate_dev failed: " + lib.lcd_last_error().decode())
    try:
        n = lib.lcd_deflated_size(h)
        buf = C.create_string_buffer(max(n, 1))
        check(lib.lcd_deflated_to_host(h, 0, n, buf), lib)
        blocks = []
        for i in range(lib.lcd_deflated_n_blocks(h)):
            pl, bs, kind = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
            check(lib.lcd_deflated_block_info(h, i, C.byref(pl), C.byref(bs), C.byref(kind)), lib)
            blocks.append((int(pl.value), int(bs.value), int(kind.value)))
        return dict(image=buf.raw[:n], blocks=blocks, kernel_ms=float(lib.lcd_deflated_kernel_ms(h)))
    finally:
        lib.lcd_deflated_free(h)


# ---------------- records as SAM text (bam_sam_kernel.hip) ----------------
class _SamNames:
    """lcd_sam_names_t for a `with` block: the contigs' names in HBM"""

    def __init__(self, names):
        self.lib = load_library()
        arr, n = _str_array(names)
        self.h = self.lib.lcd_sam_names_create(n, arr)
        if not self.h:
            raise LcdError("lcd_sam_names_create failed: " + self.lib.lcd_last_error().decode())

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.lcd_sam_names_free(self.h); self.h = None


def _sam_text(lib, h, what, st):
    """a lcd_sam_text_t handle -> (text bytes, stats dict); frees the handle"""
    from ._lib import LcdSamStats
    if not h:
        raise LcdError(what + " failed: " + lib.lcd_last_error().decode())
    try:
        n = lib.lcd_sam_text_size(h)
        buf = np.zeros(max(n, 1), np.uint8)
        check(lib.lcd_sam_text_to_host(h, 0, n, _p8(buf)), lib)
        return buf[:n].tobytes(), {k: getattr(st, k) for k, _t in LcdSamStats._fields_}
    finally:
        lib.lcd_sam_text_free(h)


def records_to_sam(records, names):
    """lcd_records_to_sam: host bytes of back-to-back block_size-prefixed BAM records + the contigs' names -> (the SAM lines formatted on the device, stats dict)"""
    from ._lib import LcdSamStats
    lib = load_library()
    rec = np.frombuffer(bytes(records), np.uint8)
    st = LcdSamStats()
    with _SamNames(names) as nm:
        h = lib.lcd_records_to_sam(_p8(rec) if len(rec) else None, len(rec), nm.h, C.byref(st))
        return _sam_text(lib, h, "lcd_records_to_sam", st)


def tagged_to_sam(chunk, haps, phase_sets, names, skip=None, order=None):
    """lcd_chunk_tag_records_sel + lcd_tagged_to_sam: a chunk's records with HP / PS rewritten, as SAM lines, without the records leaving HBM
    -> (text, number of records, stats dict)"""
    from ._lib import LcdSamStats
    lib = chunk.lib
    hp = np.concatenate([np.ascontiguousarray(haps, np.int32), np.zeros(1, np.int32)]); ps = np.concatenate([np.ascontiguousarray(phase_sets, np.int64), np.zeros(1, np.int64)])
    if len(hp) <= chunk.n or len(ps) <= chunk.n:
        raise ValueError("tagged_to_sam: haps / phase_sets shorter than the chunk's reads")
    sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
    od = np.ascontiguousarray(order, np.int32) if order is not None else None
    t = lib.lcd_chunk_tag_records_sel(chunk.h, hp.ctypes.data_as(i32p), ps.ctypes.data_as(C.POINTER(C.c_int64)), _p8(sk) if sk is not None else None,
                                      od.ctypes.data_as(i32p) if od is not None else None)
    if not t:
        raise LcdError("lcd_chunk_tag_records_sel failed: " + lib.lcd_last_error().decode())
    try:
        st = LcdSamStats()
        with _SamNames(names) as nm:
            text, stats = _sam_text(lib, lib.lcd_tagged_to_sam(t, nm.h, C.byref(st)), "lcd_tagged_to_sam", st)
        return text, int(lib.lcd_tagged_n_records(t)), stats
    finally:
        lib.lcd_tagged_free(t)


def write_phased_sam(in_bam_path, chunks, path, pg_line=None, sort_output=False, aln_format="sam", block_payload=0):
    """lcd_write_phased as SAM text (aln_format="bam": the BAM writer on the same chunks): chunks = [dict(chunk=DeviceChunk, haps, phase_sets, reg_beg, reg_end[, ref,
    ref_beg, ref_end])] in region order, each with its final haplotypes -- the fields of lcd_call_chunk_t the writer reads.  sort_output: lcd_writer_opt_t's.
    -> dict(bam_out = lcd_bam_out_t's counters, refine = lcd_refine_stats_t, sam = lcd_sam_stats_t)"""
    from ._lib import LCD_ALN_BAM, LCD_ALN_SAM, LcdBamOut, LcdCallChunk, LcdHapState, LcdRefineStats, LcdSamStats, LcdWriterOpt
    if aln_format not in ("sam", "bam"):
        raise ValueError("write_phased_sam: aln_format must be 'sam' or 'bam'")
    lib = load_library()
    n = len(chunks)
    arr = (LcdCallChunk * max(1, n))()
    keep = []
    for k, c in enumerate(chunks):
        ch = c["chunk"]
        hp = np.concatenate([np.ascontiguousarray(c["haps"], np.int32), np.zeros(1, np.int32)]); ps = np.concatenate([np.ascontiguousarray(c["phase_sets"], np.int64), np.zeros(1, np.int64)])
        if len(hp) <= ch.n or len(ps) <= ch.n:
            raise ValueError("write_phased_sam: haps / phase_sets shorter than the chunk's reads")
        s = LcdHapState(); s.n_reads = ch.n; s.haps = hp.ctypes.data_as(i32p); s.phase_sets = ps.ctypes.data_as(C.POINTER(C.c_int64))
        keep += [hp, ps, s]
        f = arr[k].first
        f.chunk, f.reg_beg, f.reg_end, f.n_reads, f.state = ch.h, int(c["reg_beg"]), int(c["reg_end"]), ch.n, C.pointer(s)
        if c.get("ref") is not None:
            rb = np.frombuffer(bytes(c["ref"]) if isinstance(c["ref"], (bytes, bytearray)) else np.ascontiguousarray(c["ref"], np.uint8).tobytes(), np.uint8).copy()
            keep.append(rb)
            f.ref_seq, f.ref_beg, f.ref_end = _p8(rb), int(c["ref_beg"]), int(c["ref_end"])
    bo = LcdBamOut(); bo.path = _enc(path); bo.pg_line = _enc(pg_line) if pg_line is not None else None; bo.block_payload = int(block_payload)
    rst, sst = LcdRefineStats(), LcdSamStats()
    wo = LcdWriterOpt(format=LCD_ALN_SAM if aln_format == "sam" else LCD_ALN_BAM, sort_output=int(bool(sort_output)), refine_stats=C.pointer(rst), sam_stats=C.pointer(sst))
    check(lib.lcd_write_phased(_enc(in_bam_path), n, arr, C.byref(bo), C.byref(wo)), lib)
    return dict(bam_out={k: getattr(bo, k) for k in ("n_records_out", "n_filtered_out", "bytes_inflated", "bytes_file", "ms_tag", "ms_deflate", "ms_download_write")},
                refine={k: getattr(rst, k) for k, _t in LcdRefineStats._fields_}, sam={k: getattr(sst, k) for k, _t in LcdSamStats._fields_})


def _split_stats(st):
    return {k: (list(getattr(st, k)) if k in ("n_hap", "bytes_fastq") else getattr(st, k)) for k, _t in st._fields_}


def chunk_split_reads(chunk, haps, phase_sets, skip=None, order=None, names=None, comment=False, list=False):
    """lcd_chunk_split_reads: the records of the chunk's table that skip / order name (merged_record_plan's outputs; None: all, in table order) as per-haplotype
    FASTQ entries and -- with list=True and names = the contigs' names -- haplotag list lines, formatted on the device.  haps / phase_sets per kept read.
    -> ([FASTQ bytes of stream 0 (none), 1, 2, the list's bytes (no header line)], stats dict; "n_hap" and "bytes_fastq" are lists of three)"""
    from ._lib import LcdSplitOpt, LcdSplitStats
    lib = chunk.lib
    hp = np.concatenate([np.ascontiguousarray(haps, np.int32), np.zeros(1, np.int32)]); ps = np.concatenate([np.ascontiguousarray(phase_sets, np.int64), np.zeros(1, np.int64)])
    if len(hp) <= chunk.n or len(ps) <= chunk.n:
        raise ValueError("chunk_split_reads: haps / phase_sets shorter than the chunk's reads")
    if list and names is None:
        raise ValueError("chunk_split_reads: list=True needs names= (the contigs' names)")
    sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
    od = np.ascontiguousarray(order, np.int32) if order is not None else None
    o = LcdSplitOpt(); lib.lcd_split_opt_default(C.byref(o)); o.comment, o.list = int(bool(comment)), int(bool(list))
    st = LcdSplitStats()

    def run(nm):
        h = lib.lcd_chunk_split_reads(chunk.h, hp.ctypes.data_as(i32p), ps.ctypes.data_as(C.POINTER(C.c_int64)), _p8(sk) if sk is not None else None,
                                      od.ctypes.data_as(i32p) if od is not None else None, nm, C.byref(o), C.byref(st))
        if not h:
            raise LcdError("lcd_chunk_split_reads failed: " + lib.lcd_last_error().decode())
        try:
            out = []
            for s in range(4):
                buf = np.zeros(max(1, int(lib.lcd_split_size(h, s))), np.uint8)
                n = int(lib.lcd_split_size(h, s))
                check(lib.lcd_split_to_host(h, s, 0, n, _p8(buf)), lib)
                out.append(buf[:n].tobytes())
            return out, _split_stats(st)
        finally:
            lib.lcd_split_free(h)
    if not list:
        return run(None)
    with _SamNames(names) as nm:
        return run(nm.h)


def split_paths(prefix, gz=False, other=()):
    """lcd_split_paths (host only): the FASTQ files of a prefix in stream order (none, h1, h2); LcdError when the prefix is empty or "-", or when two of them and the
    `other` output paths (None entries are skipped) are equal.  prefix None: only the others are compared -> []"""
    lib = load_library()
    oth = [(_enc(x) if x is not None else None) for x in other]
    arr = (C.c_char_p * max(1, len(oth)))(*oth)
    p = (C.c_void_p * 3)()
    rc = lib.lcd_split_paths(_enc(prefix) if prefix is not None else None, int(bool(gz)), len(oth), arr, p)
    if rc:
        raise LcdError(f"lcd_split_paths: error {rc}: an empty prefix or \"-\", or two outputs that name one file")
    try:
        return [C.string_at(p[k]).decode() for k in range(3) if p[k]]
    finally:
        for k in range(3):
            if p[k]:
                _libc_free(C.c_void_p(p[k]))


def split_offsets(stream, fq_len, list_len):
    """lcd_split_offsets (host only): the rows of a measure pass -> (fq_off per record inside its stream, list_off per record, the four totals)"""
    lib = load_library()
    sa = np.ascontiguousarray(stream, np.int32); fl = np.ascontiguousarray(fq_len, np.uint64); ll = np.ascontiguousarray(list_len, np.uint64)
    n = len(sa)
    assert len(fl) == n and len(ll) == n
    fo, lo, tot = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64), np.zeros(4, np.uint64)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib.lcd_split_offsets(n, sa.ctypes.data_as(i32p) if n else None, u64(fl) if n else None, u64(ll) if n else None, u64(fo), u64(lo), u64(tot))
    if rc:
        raise LcdError(f"lcd_split_offsets: error {rc}: a stream outside -1 ... 2, or lengths that overflow")
    return [int(x) for x in fo[:n]], [int(x) for x in lo[:n]], [int(x) for x in tot]


def _run_ext2_split(mods, depth, split):
    """_run_ext2 grown by split = dict([prefix, gz, comment, haplotag_list]) -> (the lcd_run_ext2_split_t, whose member x is handed to the drivers, and the three
    statistics structs it points to)"""
    from ._lib import LcdRunExt2Split, LcdSplitStats
    x, mst, dst = _run_ext2(mods, depth)
    xs = LcdRunExt2Split(); xs.x = x; xs.x.size = C.sizeof(LcdRunExt2Split)
    sst = LcdSplitStats()
    opt_s = lambda v: _enc(v) if v is not None else None
    xs.split_prefix, xs.split_gz, xs.split_comment = opt_s(split.get("prefix")), int(bool(split.get("gz", False))), int(bool(split.get("comment", False)))
    xs.haplotag_path, xs.split_stats = opt_s(split.get("haplotag_list")), C.pointer(sst)
    return xs, mst, dst, sst


def call_bam_regions(bam_path, bai_path, fasta_path, chrom, reg_beg, reg_end, min_mapq=30, cfg=None, bam_out=None, te_fasta=None, rnames=None, refine=False, mods=None, depth=None,
                     split=None):
    """lcd_call_bam_regions: regions of one contig of an indexed BAM + a FASTA with its .fai -> the dict of chunks_call.
    bam_out = dict(path[, pg_line, block_payload]): the phased alignment file is written too; the result gets "bam_out" = the counters and stage times of
    lcd_bam_out_t and "bam_out_rc" / "bam_out_error" (a failed output leaves the VCF side valid: it is returned, not raised).
    te_fasta= / rnames=: lcd_run_opt_t.fields (as chunks_call).  refine=True (with bam_out; not with te_fasta / rnames): lcd_aln_opt_t.refine -- the records are
    written with the alignments the call arrived at; the result gains "refine" = lcd_refine_stats_t's fields.
    mods = dict(path[, code, threshold, combine_strands]) (lcd_call_bam_regions_ext2): the contig's methylation table goes to path, every region's chunk piled up
    with the haplotypes the result returns for it; the result gains "mods" = the sums of lcd_mods_stats_t
    depth = dict(path[, window, skip_dels]): the contig's per-haplotype depth track goes to path (per base, or per window of `window` positions), from the records
    as stored and the same haplotypes; the result gains "depth" = the sums of lcd_depth_stats_t
    split = dict([prefix, gz, comment, haplotag_list]): the contig's per-haplotype read sets (prefix.none|h1|h2.fastq[.gz]) and / or the haplotag list, from the
    records the alignment output holds and the same haplotypes; the result gains "split" = the sums of lcd_split_stats_t"""
    from ._lib import LCD_ALN_BAM, LcdAlnOpt, LcdBamOut, LcdCallChunk, LcdRefineStats, LcdRunOpt, LcdRunOut, LcdVar1
    vf, fo = _vcf_fields(te_fasta, rnames)
    if refine and vf is not None:
        raise ValueError("call_bam_regions: refine= goes with neither te_fasta= nor rnames=")
    rst = LcdRefineStats() if refine and bam_out is not None else None
    lib = load_library()
    cfg = cfg if cfg is not None else call_cfg()
    n = len(reg_beg)
    arr = (LcdCallChunk * max(1, n))()
    rb = (C.c_int64 * max(1, n))(*[int(x) for x in reg_beg]); re_ = (C.c_int64 * max(1, n))(*[int(x) for x in reg_end])
    recs, n_recs, text = C.POINTER(LcdVar1)(), C.c_int(0), C.c_void_p()
    bo = None
    if bam_out is not None:
        bo = LcdBamOut(); bo.path = _enc(bam_out["path"]); bo.pg_line = _enc(bam_out["pg_line"]) if bam_out.get("pg_line") is not None else None
        bo.block_payload = int(bam_out.get("block_payload", 0))
    ao = LcdAlnOpt(LCD_ALN_BAM, int(rst is not None))
    ro = LcdRunOpt(fields=C.pointer(vf) if vf is not None else None, aln=C.pointer(ao))
    out = LcdRunOut(fields_out=C.pointer(fo) if vf is not None else None, refine_stats=C.pointer(rst) if rst is not None else None)
    args = (_enc(bam_path), _enc(bai_path), _enc(fasta_path), _enc(chrom), n, rb, re_, int(min_mapq), C.byref(cfg), arr, C.byref(recs), C.byref(n_recs),
            C.byref(text), C.byref(bo) if bo is not None else None, C.byref(ro), C.byref(out))
    mst = dst = spst = None
    if split is not None:
        ext2, mst, dst, spst = _run_ext2_split(mods, depth, split)
        rc = lib.lcd_call_bam_regions_ext2(*args, C.byref(ext2.x))
    elif mods is not None or depth is not None:
        ext2, mst, dst = _run_ext2(mods, depth)
        rc = lib.lcd_call_bam_regions_ext2(*args, C.byref(ext2))
    else:
        rc = lib.lcd_call_bam_regions(*args)
    err = lib.lcd_last_error().decode() if rc < 0 else ""
    if rc < 0 and (bo is None or (not text and not recs)):
        raise LcdError(f"liblcd_hotpath error {rc}: {err}")
    res = _call_result(lib, n, arr, recs, n_recs, text)
    if vf is not None:
        res = _fields_result(lib, res, vf, fo)
    if mst is not None:
        res["mods"] = {k: getattr(mst, k) for k, _t in mst._fields_}
    if dst is not None:
        res["depth"] = _depth_stats(dst)
    if spst is not None:
        res["split"] = _split_stats(spst)
    if bo is None:
        return res
    res.update(bam_out_rc=int(rc), bam_out_error=err, bam_out={k: getattr(bo, k) for k in ("n_records_out", "n_filtered_out", "bytes_inflated", "bytes_file", "ms_tag",
                                                                                               "ms_deflate", "ms_download_write")})
    if rst is not None:
        res["refine"] = {k: getattr(rst, k) for k, _t in LcdRefineStats._fields_}
    return res


def _run_ext2(mods, depth=None):
    """mods = dict(path[, code, threshold, combine_strands]) | None, depth = dict(path[, window, skip_dels]) | None -> (lcd_run_ext2_t, the lcd_mods_stats_t and the
    lcd_depth_stats_t it points to; None for the one that was not asked for)"""
    from ._lib import LcdDepthStats, LcdModsStats, LcdRunExt2
    x = LcdRunExt2(size=C.sizeof(LcdRunExt2))
    mst = dst = None
    if mods is not None:
        mst = LcdModsStats()
        code = mods.get("code", "m")
        x.mods_path, x.mods_code = _enc(mods["path"]), ord(code) if isinstance(code, str) and len(code) == 1 else -1
        x.mods_threshold, x.mods_combine_strands, x.mods_stats = int(mods.get("threshold", 204)), int(bool(mods.get("combine_strands", False))), C.pointer(mst)
    if depth is not None:
        dst = LcdDepthStats()
        x.depth_path, x.depth_window, x.depth_skip_dels, x.depth_stats = _enc(depth["path"]), int(depth.get("window", 0)), int(bool(depth.get("skip_dels", False))), C.pointer(dst)
    return x, mst, dst


# ---------------- a whole BAM in one call (lcd_call_files and what it is composed of) ----------------
def _enc(x):
    return x if isinstance(x, bytes) else str(x).encode()


def _str_array(xs):
    xs = [_enc(x) for x in (xs or [])]
    return (C.c_char_p * max(1, len(xs)))(*xs), len(xs)


def bam_contigs(bam_path):
    """lcd_bam_contigs -> [(name, length)] in header order"""
    lib = load_library()
    n, names, lens = C.c_int(0), C.POINTER(C.c_void_p)(), C.POINTER(C.c_int64)()
    check(lib.lcd_bam_contigs(_enc(bam_path), C.byref(n), C.byref(names), C.byref(lens)), lib)
    try:
        return [(C.string_at(names[i]).decode(), int(lens[i])) for i in range(n.value)]
    finally:
        lib.lcd_bam_contigs_free(n.value, names, lens)


def bam_sample_name(bam_path):
    """lcd_bam_sample_name -> the SM of the first @RG line that has one, or None"""
    lib = load_library()
    p = C.c_void_p()
    check(lib.lcd_bam_sample_name(_enc(bam_path), C.byref(p)), lib)
    if not p:
        return None
    try:
        return C.string_at(p).decode()
    finally:
        _libc.free(p)


def plan_chunks(contigs, contig_mode=0, exclude=(), regions=(), region_bed_path=None, chunk_len=0):
    """lcd_plan_chunks: contigs = [(name, length)] -> ([(tid, reg_beg, reg_end)], fallback flag)"""
    from ._lib import LcdChunkPlan
    lib = load_library()
    names, n = _str_array([c[0] for c in contigs])
    lens = (C.c_int64 * max(1, n))(*[int(c[1]) for c in contigs])
    exc, n_exc = _str_array(exclude)
    regs, n_regs = _str_array(regions)
    out = LcdChunkPlan()
    check(lib.lcd_plan_chunks(n, names, lens, int(contig_mode), n_exc, exc, n_regs, regs, _enc(region_bed_path) if region_bed_path is not None else None, int(chunk_len),
                              C.byref(out)), lib)
    try:
        return [(int(out.tid[i]), int(out.reg_beg[i]), int(out.reg_end[i])) for i in range(out.n)], int(out.fallback)
    finally:
        lib.lcd_chunk_plan_free(C.byref(out))


def stitch_chunks_carry(phases, update_reads=1, carry_in=None, carry_out=None, n=None):
    """lcd_stitch_chunks_carry on an array of _lib.LcdChunkPhase (mutated; its first n entries, default all); carry_in / carry_out: _lib.LcdStitchCarry or None
    -> the return code (0 or -6)"""
    lib = load_library()
    return lib.lcd_stitch_chunks_carry(phases, len(phases) if n is None else int(n), int(update_reads), C.byref(carry_in) if carry_in is not None else None,
                                       C.byref(carry_out) if carry_out is not None else None)


def _vcf_index_opt(fmt, index_path=None, slab_members=0, with_stats=True):
    """"tbi" / "csi" -> (lcd_vcf_index_opt_t, lcd_vcf_index_stats_t)"""
    from ._lib import LCD_VIDX_CSI, LCD_VIDX_TBI, LcdVcfIndexOpt, LcdVcfIndexStats
    if fmt not in ("tbi", "csi"):
        raise ValueError("the VCF index format must be 'tbi' or 'csi'")
    st = LcdVcfIndexStats()
    vo = LcdVcfIndexOpt(LCD_VIDX_CSI if fmt == "csi" else LCD_VIDX_TBI, _enc(index_path) if index_path is not None else None, int(slab_members), 0,
                        C.pointer(st) if with_stats else None)
    return vo, st


def _vcf_index_stats(st):
    from ._lib import LcdVcfIndexStats
    return {k: (getattr(st, k).decode() if k == "skip_reason" else getattr(st, k)) for k, _t in LcdVcfIndexStats._fields_ if k != "pad"}


def vcf_write(path, texts, bgzf=0, header_text=None, index=None, index_path=None, abort=False):
    """lcd_vcf_writer_open / _append per text / _close.  index "tbi" / "csi": lcd_vcf_writer_open_idx -- the index is written beside the file (or to index_path) at
    close; -> the dict of lcd_vcf_index_stats_t then, else None.  abort: lcd_vcf_writer_abort instead of close"""
    lib = load_library()
    vo, vst = _vcf_index_opt(index, index_path) if index is not None else (None, None)
    w = lib.lcd_vcf_writer_open_idx(_enc(path) if path is not None else None, int(bgzf), _enc(header_text) if header_text is not None else None,
                                    C.byref(vo) if vo is not None else None)
    if not w:
        raise LcdError("lcd_vcf_writer_open failed: " + lib.lcd_last_error().decode())
    for t in texts:
        rc = lib.lcd_vcf_writer_append(w, _enc(t))
        if rc:
            lib.lcd_vcf_writer_abort(w)
            check(rc, lib)
    if abort:
        lib.lcd_vcf_writer_abort(w)
    else:
        check(lib.lcd_vcf_writer_close(w), lib)
    return _vcf_index_stats(vst) if vst is not None else None


def chunk_open_from_bams(bam_paths, bai_paths, chrom, reg_beg, reg_end, min_mapq=30, is_ont=0, verify_crc=1):
    """lcd_chunk_open_from_bams -> DeviceChunk (DeviceChunk.open_from_bams)"""
    return DeviceChunk.open_from_bams(bam_paths, bai_paths, chrom, reg_beg, reg_end, min_mapq, is_ont, verify_crc)


def merged_record_plan(rec_file, rec_pos0, rec_endpos, has_prev=0, prev_beg=0, prev_end=0, sort_output=0):
    """lcd_merged_record_plan (pure host code): a chunk's record table in file-major order -> (skip mask, the records to write in output order).  rec_file None: one file"""
    lib = load_library()
    p0 = np.ascontiguousarray(rec_pos0, np.int64); e0 = np.ascontiguousarray(rec_endpos, np.int64)
    n = len(p0)
    assert len(e0) == n and (rec_file is None or len(rec_file) == n)
    rf = np.ascontiguousarray(rec_file, np.int32) if rec_file is not None else None
    skip = np.zeros(n + 1, np.uint8); order = np.zeros(n + 1, np.int32)
    i64p = C.POINTER(C.c_int64)
    m = check(lib.lcd_merged_record_plan(n, rf.ctypes.data_as(i32p) if rf is not None else None, p0.ctypes.data_as(i64p), e0.ctypes.data_as(i64p), int(has_prev), int(prev_beg),
                                         int(prev_end), int(sort_output), _p8(skip), order.ctypes.data_as(i32p)), lib)
    assert (order[m:n] == -1).all()
    return skip[:n].astype(bool), order[:m].copy()


def call_files(bams, fasta_path, bais=None, sort_output=False, index=None, **kw):
    """lcd_call_files: the alignment files of ONE sample (one BAM per SMRT cell / flow cell) + a FASTA -> one VCF and, with bam_out, one phased BAM holding every
    input's records (coordinate-sorted, and indexable, with sort_output).  bais None, or an entry None: <bam>.bai; every other keyword is call_file's.  The result has
    "n_reads_per_file" beside call_file's entries"""
    return call_file(list(bams), fasta_path, index=index, _inputs=dict(bais=bais, sort_output=sort_output), **kw)


def call_file(bam_path, fasta_path, bai_path=None, contig_mode=0, exclude=(), regions=(), region_bed_path=None, chunk_len=0, window_chunks=0, overlap=-1, loader_threads=0,
              min_mapq=30, vcf_path=None, vcf_bgzf=0, no_vcf_header=0, sample_name=None, source_version=None, cmdline=None, date_yyyymmdd=None, bam_out=None, cfg=None,
              keep_records=False, index=None, _inputs=None, te_fasta=None, rnames=None, refine=False, aln_format="bam", vcf_index=None, mods=None, depth=None,
              split=None, _haplotag=None):
    """lcd_call_files with the job's one file: a whole indexed BAM + a FASTA with its .fai -> the VCF file (vcf_path None: stdout) and, with bam_out = dict(path[,
    pg_line, block_payload]), the phased BAM.  -> dict of lcd_file_stats_t's counters; with keep_records also "chunks" (per planned chunk tid, reg_beg, reg_end, n_reads,
    n_passes, flip_hap, flip_pre_PS, flip_cur_PS, n_records), "records" (as chunks_call gives them) and, with bam_out, "bam_out" = its counters.
    index (default None: no lcd_index_opt_t): True, or a dict with build_missing_bai / build_missing_fai / write_out_bai / out_bai_path / slab_members; the result then
    has "index" = lcd_index_stats_t's fields (out_bai_skipped != 0: the output's index was not written, out_bai_skip_reason says why).
    te_fasta= (the -T file) / rnames=None|"sv"|"all" (--out-sv-rnames / --out-var-rnames): lcd_vcf_fields_t; the result gains "te_names" and "n_mei_lines" (with a
    library) and the kept records "te_name" / "alt_read_names" (see _fields_result).
    refine=True (the command line's --refine-bam; no effect without bam_out, not with te_fasta / rnames): lcd_aln_opt_t.refine; the result gains "refine" =
    lcd_refine_stats_t's fields.
    aln_format="sam" (the command line's --sam): bam_out's path gets SAM text ("-": stdout), block_payload is ignored, no output index; the result gains "sam" =
    lcd_sam_stats_t's fields.
    vcf_index=None | "tbi" | "csi" (the command line's --vcf-index; needs vcf_bgzf=1 and a vcf_path): <vcf_path>.tbi / .csi is written beside the VCF; the result
    gains "vcf_index" = lcd_vcf_index_stats_t's fields (skipped != 0: the VCF could not be indexed, skip_reason says why)"""
    from ._lib import LCD_ALN_BAM, LCD_ALN_SAM, LcdAlnOpt, LcdBamOut, LcdFileJob, LcdFileStats, LcdIndexOpt, LcdIndexStats, LcdRefineStats, LcdRunOpt, LcdRunOut, LcdSamStats
    if aln_format not in ("bam", "sam"):
        raise ValueError("call_file: aln_format must be 'bam' or 'sam'")
    lib = load_library()
    cfg = cfg if cfg is not None else call_cfg()
    job = LcdFileJob(); lib.lcd_file_job_default(C.byref(job))
    opt_s = lambda x: _enc(x) if x is not None else None
    if _inputs is None:
        job.bam_path, job.bai_path, job.fasta_path = _enc(bam_path), opt_s(bai_path), _enc(fasta_path)
    else:      # call_files: bam_path is the list of inputs
        from ._lib import LcdInputs
        job.fasta_path = _enc(fasta_path)
        inp = LcdInputs()
        in_bams, inp.n = _str_array(bam_path); inp.bam_paths = in_bams
        in_bais = None
        if _inputs["bais"] is not None:
            assert len(_inputs["bais"]) == inp.n
            in_bais = (C.c_char_p * max(1, inp.n))(*[opt_s(x) for x in _inputs["bais"]]); inp.bai_paths = in_bais
        inp.sort_output = int(bool(_inputs["sort_output"]))
        per_file = (C.c_int64 * max(1, inp.n))()
    exc, job.n_exclude = _str_array(exclude); job.exclude = exc
    regs, job.n_regions = _str_array(regions); job.regions = regs
    job.contig_mode, job.region_bed_path, job.chunk_len = int(contig_mode), opt_s(region_bed_path), int(chunk_len)
    job.window_chunks, job.overlap, job.loader_threads, job.min_mapq = int(window_chunks), int(overlap), int(loader_threads), int(min_mapq)
    job.vcf_path, job.vcf_bgzf, job.no_vcf_header = opt_s(vcf_path), int(vcf_bgzf), int(no_vcf_header)
    job.sample_name, job.source_version, job.cmdline, job.date_yyyymmdd = opt_s(sample_name), opt_s(source_version), opt_s(cmdline), opt_s(date_yyyymmdd)
    job.keep_records = int(bool(keep_records))
    bo = None
    if bam_out is not None:
        bo = LcdBamOut(); bo.path = _enc(bam_out["path"]); bo.pg_line = opt_s(bam_out.get("pg_line")); bo.block_payload = int(bam_out.get("block_payload", 0))
        job.bam_out = C.pointer(bo)
    st = LcdFileStats()
    ist, io = None, None
    if index:
        d = dict(build_missing_bai=1, build_missing_fai=1, write_out_bai=1 if bam_out is not None else 0) if index is True else dict(index)
        io = LcdIndexOpt(int(d.get("build_missing_bai", 0)), int(d.get("build_missing_fai", 0)), int(d.get("write_out_bai", 0)), opt_s(d.get("out_bai_path")), int(d.get("slab_members", 0)))
        ist = LcdIndexStats()
    vf, fo = _vcf_fields(te_fasta, rnames)
    if refine and vf is not None:
        raise ValueError("call_file: refine= goes with neither te_fasta= nor rnames=")
    rst = LcdRefineStats() if refine else None
    sst = LcdSamStats() if aln_format == "sam" else None
    ao = LcdAlnOpt(LCD_ALN_SAM if aln_format == "sam" else LCD_ALN_BAM, int(bool(refine)))
    ptr = lambda x: C.pointer(x) if x is not None else None
    vio, vist = _vcf_index_opt(vcf_index, with_stats=False) if vcf_index is not None else (None, None)
    ro = LcdRunOpt(idx=ptr(io), fields=ptr(vf), aln=C.pointer(ao))
    out = LcdRunOut(idx_stats=ptr(ist), n_reads_per_file=C.cast(per_file, C.POINTER(C.c_int64)) if _inputs is not None else None, fields_out=ptr(fo), refine_stats=ptr(rst), sam_stats=ptr(sst))
    args = (C.byref(inp) if _inputs is not None else None, C.byref(job), C.byref(cfg), C.byref(ro), C.byref(st), C.byref(out))
    ext, mst, dst, spst = None, None, None, None
    if vio is not None:
        from ._lib import LcdRunExt
        ext = LcdRunExt(vcf_idx=C.pointer(vio), vcf_idx_stats=C.pointer(vist))
    hvs = hts = None
    if _haplotag is not None:       # haplotag_file(s): the same run with lcd_chunk_haplotag as its middle stage (lcd_haplotag_files)
        from ._lib import LcdHaplotagRun, LcdHaplotagStats, LcdHapvcfStats
        if vio is not None:
            raise ValueError("haplotag_file: a haplotag run writes no VCF (vcf_index=)")
        hvs, hts = LcdHapvcfStats(), LcdHaplotagStats()
        hr = LcdHaplotagRun(size=C.sizeof(LcdHaplotagRun), vcf_path=_enc(_haplotag["vcf"]), sample=opt_s(_haplotag.get("sample")), max_indel=int(_haplotag.get("max_indel", 50)),
                            snvs_only=int(bool(_haplotag.get("snvs_only", False))), min_bq=int(_haplotag.get("min_bq", 0)), min_diff=int(_haplotag.get("min_diff", 1)),
                            vcf_stats=C.pointer(hvs), stats=C.pointer(hts))
        x2p = None
        if split is not None:
            ext2, mst, dst, spst = _run_ext2_split(mods, depth, split); x2p = C.byref(ext2.x)
        elif mods is not None or depth is not None:
            ext2, mst, dst = _run_ext2(mods, depth); x2p = C.byref(ext2)
        rc = lib.lcd_haplotag_files(args[0], args[1], args[2], C.byref(hr), args[3], args[4], args[5], x2p)
    elif split is not None:
        # split = dict([prefix, gz, comment, haplotag_list]) (the command line's --split-reads / --split-gz / --split-comment / --haplotag-list): the reads of
        # each haplotype as FASTQ files prefix.none|h1|h2.fastq[.gz] and / or the haplotag list (lcd_run_ext2_split_t), in the order of the output BAM; the result
        # gains "split" = the sums of lcd_split_stats_t over the chunks
        ext2, mst, dst, spst = _run_ext2_split(mods, depth, split)
        rc = lib.lcd_call_files_ext2(*args, C.byref(ext) if ext is not None else None, C.byref(ext2.x))
    elif mods is not None or depth is not None:
        # mods = dict(path[, code "m" | "h", threshold 128 ... 255, combine_strands]): the per-haplotype CpG methylation table (lcd_run_ext2_t); the result gains
        # "mods" = the sums of lcd_mods_stats_t over the chunks (n_rows: the data lines written)
        # depth = dict(path[, window 0 ... 2^30, skip_dels]) (the command line's --depth / --depth-window / --depth-skip-dels): the per-haplotype depth track, per
        # base or per window; the result gains "depth" = the sums of lcd_depth_stats_t over the chunks (n_rows: the data lines written)
        ext2, mst, dst = _run_ext2(mods, depth)
        rc = lib.lcd_call_files_ext2(*args, C.byref(ext) if ext is not None else None, C.byref(ext2))
    elif ext is not None:
        rc = lib.lcd_call_files_ext(*args, C.byref(ext))
    else:
        rc = lib.lcd_call_files(*args)
    try:
        check(rc, lib)
        res = {k: getattr(st, k) for k, _t in LcdFileStats._fields_[:14]}
        if _inputs is not None:
            res["n_reads_per_file"] = [int(per_file[f]) for f in range(inp.n)]
        if ist is not None:
            res["index"] = {k: (getattr(ist, k).decode() if k == "out_bai_skip_reason" else getattr(ist, k)) for k, _t in LcdIndexStats._fields_}
        if keep_records:
            res["chunks"] = [dict(tid=int(st.chunk_tid[i]), reg_beg=int(st.chunk_reg_beg[i]), reg_end=int(st.chunk_reg_end[i]), n_reads=int(st.chunk_n_reads[i]),
                                  n_passes=int(st.chunk_n_passes[i]), flip_hap=int(st.chunk_flip_hap[i]), flip_pre_PS=int(st.chunk_flip_pre_PS[i]),
                                  flip_cur_PS=int(st.chunk_flip_cur_PS[i]), n_records=int(st.chunk_n_records[i])) for i in range(st.n_chunks)]
            res["records"] = [_var1_dict(st.records[i]) for i in range(st.n_kept_records)]
        if bo is not None:
            res["bam_out"] = {k: getattr(bo, k) for k in ("n_records_out", "n_filtered_out", "bytes_inflated", "bytes_file", "ms_tag", "ms_deflate", "ms_download_write")}
        if vf is not None:
            res = _fields_result(lib, res, vf, fo)
        if rst is not None:
            res["refine"] = {k: getattr(rst, k) for k, _t in LcdRefineStats._fields_}
        if sst is not None:
            res["sam"] = {k: getattr(sst, k) for k, _t in LcdSamStats._fields_}
        if vist is not None:
            res["vcf_index"] = _vcf_index_stats(vist)
        if mst is not None:
            res["mods"] = {k: getattr(mst, k) for k, _t in mst._fields_}
        if dst is not None:
            res["depth"] = _depth_stats(dst)
        if spst is not None:
            res["split"] = _split_stats(spst)
        if hts is not None:
            res["haplotag"] = _haplotag_stats(hts)
            res["phased_vcf"] = {k: int(getattr(hvs, k)) for k, _t in hvs._fields_}
        return res
    finally:
        lib.lcd_file_stats_free(C.byref(st))


def haplotag_file(bam_path, fasta_path, phased_vcf, sample=None, max_indel=50, snvs_only=False, min_bq=0, min_diff=1, **kw):
    """lcd_haplotag_files with the job's one file: every read of an indexed BAM against the heterozygous phased sites of phased_vcf (plain, gzip or BGZF; sample None:
    the first), written through the outputs of call_file that hang on the reads' haplotypes -- bam_out (aln_format "bam" | "sam"), mods=, depth=, split= -- with
    call_file's input, region, index and run keywords.  No variant is called and no VCF is written; at least one output is needed.  -> call_file's counters (ms_call:
    the haplotag stage) with "haplotag" = the sums of lcd_haplotag_stats_t over the chunks and "phased_vcf" = lcd_hapvcf_stats_t"""
    for k in ("vcf_bgzf", "no_vcf_header", "sample_name", "source_version", "cmdline", "date_yyyymmdd", "keep_records", "_haplotag"):
        if k in kw:
            raise ValueError(f"haplotag_file: {k}= belongs to a calling run")
    return call_file(bam_path, fasta_path, _haplotag=dict(vcf=phased_vcf, sample=sample, max_indel=max_indel, snvs_only=snvs_only, min_bq=min_bq, min_diff=min_diff), **kw)


def haplotag_files(bams, fasta_path, phased_vcf, bais=None, sort_output=False, **kw):
    """haplotag_file over the alignment files of one sample (call_files' rules for the inputs and the merged output)"""
    return haplotag_file(list(bams), fasta_path, phased_vcf, _inputs=dict(bais=bais, sort_output=sort_output), **kw)


# ---------------- indexes: .bai on the device, .fai on the host ----------------
def bai_from_records(n_ref, refid, beg, end, flag, vbeg, vend):
    """lcd_bai_from_records (pure host code): a record table -> the bytes of its .bai"""
    lib = load_library()
    a = [np.ascontiguousarray(refid, np.int32), np.ascontiguousarray(beg, np.int64), np.ascontiguousarray(end, np.int64), np.ascontiguousarray(flag, np.int32),
         np.ascontiguousarray(vbeg, np.uint64), np.ascontiguousarray(vend, np.uint64)]
    n = len(a[0])
    assert all(len(x) == n for x in a)
    out, sz = C.c_void_p(), C.c_size_t()
    tys = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64]
    check(lib.lcd_bai_from_records(int(n_ref), n, *[x.ctypes.data_as(C.POINTER(t)) for x, t in zip(a, tys)], C.byref(out), C.byref(sz)), lib)
    try:
        return C.string_at(out.value, sz.value)
    finally:
        _libc_free(out)


def _libc_free(p):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free.restype = None
    libc.free(p)


def bai_build(bam_path, out_path=None, slab_members=0, verify_crc=0):
    """lcd_bai_build: the .bai of a BAM of any size, built on the device (out_path None: <bam>.bai) -> dict of lcd_bai_stats_t"""
    from ._lib import LcdBaiOpt, LcdBaiStats
    lib = load_library()
    opt, st = LcdBaiOpt(int(slab_members), int(verify_crc)), LcdBaiStats()
    check(lib.lcd_bai_build(_enc(bam_path), _enc(out_path if out_path is not None else bam_path + ".bai"), C.byref(opt), C.byref(st)), lib)
    return {k: getattr(st, k) for k, _t in LcdBaiStats._fields_}


def tbx_from_records(fmt, names, tid, beg, end, vbeg, vend, max_contig_len=0):
    """lcd_tbx_from_records (pure host code): a table of data lines -> the UNCOMPRESSED bytes of its .tbi / .csi"""
    from ._lib import LCD_VIDX_CSI, LCD_VIDX_TBI
    lib = load_library()
    a = [np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(beg, np.int64), np.ascontiguousarray(end, np.int64), np.ascontiguousarray(vbeg, np.uint64),
         np.ascontiguousarray(vend, np.uint64)]
    n = len(a[0])
    assert all(len(x) == n for x in a)
    nm, n_ref = _str_array(names)
    out, sz = C.c_void_p(), C.c_size_t()
    tys = [C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64]
    check(lib.lcd_tbx_from_records(LCD_VIDX_CSI if fmt == "csi" else LCD_VIDX_TBI, n_ref, nm, int(max_contig_len), n, *[x.ctypes.data_as(C.POINTER(t)) for x, t in zip(a, tys)],
                                   C.byref(out), C.byref(sz)), lib)
    try:
        return C.string_at(out.value, sz.value)
    finally:
        _libc_free(out)


def vcf_index_build(path, out_path=None, fmt="tbi", slab_members=0):
    """lcd_vcf_index_build: the .tbi / .csi of a BGZF-compressed VCF of any size, built on the device (out_path None: <path>.tbi / <path>.csi) -> dict of
    lcd_vcf_index_stats_t"""
    from ._lib import LcdVcfIndexStats
    lib = load_library()
    vo, _ = _vcf_index_opt(fmt, slab_members=slab_members, with_stats=False)
    st = LcdVcfIndexStats()
    check(lib.lcd_vcf_index_build(_enc(path), _enc(out_path) if out_path is not None else None, C.byref(vo), C.byref(st)), lib)
    return _vcf_index_stats(st)


def fai_build(fasta_path, out_path=None):
    """lcd_fai_build (host code): <fasta>.fai (or out_path) -> the number of sequences"""
    lib = load_library()
    return check(lib.lcd_fai_build(_enc(fasta_path), _enc(out_path) if out_path is not None else None), lib)
