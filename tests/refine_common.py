"""Pure-Python oracle of the refined alignment output (lcd_chunk_refine_records): refine_bam1 + update_bam1_tags (src/bam_utils.c:1718-1942) on one record body,
written from the rules R1-R5 and the project rules of include/lcd_hotpath.h, on top of bam_out_common.tag_aux (HP / PS) and bam_src_common.aux_walk.
  * digars are rows [pos (1-based), type, len, qi(, is_low_qual)] as lcd_digar_batch returns them; the window is codes 0-4 with ref[0] = position ref_beg and the
    reference's bounds test `ref_beg <= pos < ref_end` on the project's INCLUSIVE ref_end (the window's last base reads as N);
  * every decision leaves a named entry in `trace`, so that a test can prove from the oracle's own trace that each condition of its case table was reached;
  * digars_from_cigar / md_events / cs_events read a CIGAR + bases, an MD string and a cs string back into one alignment (tests only: the checks that a refined
    record still describes the alignment its digars describe)."""
import re
import struct

import numpy as np

import bam_out_common as bo

EQ, X, INS, DEL, SOFT, HARD = 7, 8, 1, 2, 4, 5
REASONS = ("no_digars", "qlen_mismatch", "bad_pos", "too_many_ops", "cg_cigar")


def digars_cigar(d):
    """R2: longcalld_push_cigar per digar, then a hard clip as the first / last word becomes a soft clip -> list of words"""
    out = []
    for _, t, l, *_ in d:
        if out and (out[-1] & 0xf) == t:
            out[-1] += int(l) << 4
        else:
            out.append((int(l) << 4) | int(t))
    for k in (0, -1):
        if out and (out[k] & 0xf) == HARD:
            out[k] = (out[k] & ~0xf) | SOFT
    return out


def digars_nm(d):
    return sum(int(l) for _, t, l, *_ in d if t in (X, INS, DEL))


def digar2qlen(d):
    if len(d) == 0:
        return 0
    _, t, l, qi, *_ = d[-1]
    return int(qi) + (int(l) if t in (EQ, 0, X, INS, SOFT, HARD) else 0)


def _ref_code(ref, ref_beg, ref_end, p):
    if ref is not None and ref_beg <= p < ref_end:
        c = int(ref[p - ref_beg])
        return c if c < 4 else 4
    return 4


def digars_md(d, ref, ref_beg, ref_end):
    out, eq = [], 0
    for pos, t, l, *_ in d:
        if t == EQ:
            eq += int(l)
        elif t in (X, DEL):
            out.append(b"%d" % eq + (b"^" if t == DEL else b"") + bytes(b"ACGTN"[_ref_code(ref, ref_beg, ref_end, int(pos) + j)] for j in range(int(l)))); eq = 0
    if eq > 0:
        out.append(b"%d" % eq)
    return b"".join(out)


def digars_cs(d, bases, ref, ref_beg, ref_end):
    """bases: the read's codes 0-4 (seq_nt16_int of the record's 4-bit bases)"""
    rb = lambda q: b"acgtn"[int(bases[q]) if 0 <= q < len(bases) else 4]
    out = []
    for pos, t, l, qi, *_ in d:
        pos, l, qi = int(pos), int(l), int(qi)
        if t == EQ:
            out.append(b":%d" % l)
        elif t == X:
            out.append(b"".join(b"*" + bytes([b"acgtn"[_ref_code(ref, ref_beg, ref_end, pos + j)], rb(qi + j)]) for j in range(l)))
        elif t == INS:
            out.append(b"+" + bytes(rb(qi + j) for j in range(l)))
        elif t == DEL:
            out.append(b"-" + bytes(b"acgtn"[_ref_code(ref, ref_beg, ref_end, pos + j)] for j in range(l)))
    return b"".join(out)


def reg2bin(beg, end):
    end -= 1
    for sh, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return off + (beg >> sh)
    return 0


def core(body):
    refid, pos, lname, mapq, bin_, nc, flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    c0 = 32 + lname
    s0 = c0 + 4 * nc
    a0 = s0 + (lseq + 1) // 2 + lseq
    return dict(refid=refid, pos=pos, lname=lname, mapq=mapq, bin=bin_, nc=nc, flag=flag, lseq=lseq, c0=c0, s0=s0, a0=a0,
                cig=list(struct.unpack("<%dI" % nc, body[c0:s0])) if s0 <= len(body) else [], fits=lseq >= 0 and a0 <= len(body))


def read_codes(body):
    x = core(body)
    pk = np.frombuffer(body[x["s0"]:x["s0"] + (x["lseq"] + 1) // 2], np.uint8)
    nib = np.stack([pk >> 4, pk & 15], 1).reshape(-1)[:x["lseq"]]
    lut = np.full(16, 4, np.uint8); lut[[1, 2, 4, 8]] = [0, 1, 2, 3]
    return lut[nib]


def unrefined_reason(body, digars, skipped):
    """the FIRST reason that leaves a kept record with HP / PS only, or None"""
    x = core(body)
    if skipped or digars is None or len(digars) == 0:
        return "no_digars"
    if not x["fits"] or digar2qlen(digars) != x["lseq"]:
        return "qlen_mismatch"
    if int(digars[0][0]) < 1:
        return "bad_pos"
    n_ops = 1 + sum(1 for a, b in zip(digars[:-1], digars[1:]) if a[1] != b[1])
    if n_ops > 65535:
        return "too_many_ops"
    f = bo.field_spans(body[x["a0"]:])
    cg = next((ty for tag, ty, *_ in f if tag == b"CG"), None)
    if x["nc"] == 2 and x["cig"][0] == ((x["lseq"] << 4) | SOFT) and (x["cig"][1] & 0xf) == 3 and cg == "B":
        return "cg_cigar"
    return None


def refine_record(body, kept, digars, skipped, ref, ref_beg, ref_end, hap=0, ps=0, trace=None):
    """one record body -> (the rewritten body, state) with state in 'filtered' / 'changed' / 'identical' / one of REASONS"""
    trace = trace if trace is not None else []
    if not kept:
        trace.append("filtered")
        return bo.tag_record(body, False, trace=trace), "filtered"
    why = unrefined_reason(body, digars, skipped)
    if why:
        trace.append("unrefined:" + why)
        return bo.tag_record(body, True, hap, ps, trace), why
    x = core(body)
    words = digars_cigar(digars)
    new_pos = int(digars[0][0]) - 1
    rl = sum(w >> 4 for w in words if (w & 0xf) in (0, 2, 3, 7, 8))
    moved = new_pos != x["pos"]
    if moved:
        trace.append("pos_moved")
    if any((a & 0xf) == HARD for a in (int(digars[0][1]), int(digars[-1][1]))):
        trace.append("hard_to_soft")
    head = lambda nc: body[:4] + struct.pack("<iBBHH", new_pos, x["lname"], x["mapq"], reg2bin(new_pos, new_pos + max(rl, 1)), nc) + body[14:x["c0"]]
    if words == x["cig"]:
        trace.append("identical")
        out = (head(x["nc"]) if moved else body[:x["c0"]]) + body[x["c0"]:]
        return bo.tag_record(out, True, hap, ps, trace), "identical"
    trace.append("changed")
    if any((w & 0xf) == 0 for w in x["cig"]):
        trace.append("M_input")
    aux = body[x["a0"]:]
    first = {}
    for tag, ty, val, b, e in bo.field_spans(aux):
        if tag in (b"NM", b"MD", b"cs") and tag not in first:
            first[tag] = (ty, val, b, e)
    dels, app = [], b""
    f = first.get(b"NM")
    nm = digars_nm(digars)
    if f is None:
        trace.append("NM:absent")
    elif bo.aux2i(f[0], f[1]) == nm:
        trace.append("NM:kept:" + f[0])
    else:
        trace.append("NM:replaced:" + f[0]); dels.append(f[2:]); app += b"NMi" + struct.pack("<i", nm)
    for tag, text in ((b"MD", lambda: digars_md(digars, ref, ref_beg, ref_end)), (b"cs", lambda: digars_cs(digars, read_codes(body), ref, ref_beg, ref_end))):
        f, name = first.get(tag), tag.decode()
        if f is None:
            trace.append(name + ":absent")
        elif f[0] != "Z":
            trace.append(name + ":not_Z:" + f[0])
        elif bytes(f[1]) == text():
            trace.append(name + ":kept")
        else:
            trace.append(name + ":replaced"); dels.append(f[2:]); app += tag + b"Z" + text() + b"\0"
    new_aux, p = b"", 0
    for b, e in sorted(dels):
        new_aux += aux[p:b]; p = e
    new_aux += aux[p:] + app
    out = head(len(words)) + struct.pack("<%dI" % len(words), *words) + body[x["s0"]:x["a0"]] + new_aux
    return bo.tag_record(out, True, hap, ps, trace), "changed"


def refined_stream(recs, digars_of, skipped, ref, ref_beg, ref_end, haps, phase_sets, skip=None, order=None, trace=None):
    """lcd_chunk_refine_records on bam_out_common.region_records' list [(body, chunk read id | -1)]; digars_of[r] = the final digars of read r ->
    (bytes, number of records, stats dict, [state per record written])"""
    idx = [i for i in range(len(recs)) if skip is None or not skip[i]]
    if order is not None:
        idx = [int(i) for i in order[:len(idx)]]
    out, states = b"", []
    st = dict(n_records=0, n_kept=0, n_refined=0, n_identical=0, n_unrefined=0, n_pos_moved=0, n_no_digars=0, n_qlen_mismatch=0, n_bad_pos=0, n_too_many_ops=0,
              n_cg_cigar=0, n_nm_replaced=0, n_md_replaced=0, n_cs_replaced=0)
    for i in idx:
        body, r = recs[i]
        t = []
        new, state = refine_record(body, r >= 0, digars_of[r] if r >= 0 else None, bool(skipped[r]) if r >= 0 else False, ref, ref_beg, ref_end,
                                   int(haps[r]) if r >= 0 else 0, int(phase_sets[r]) if r >= 0 else 0, t)
        out += struct.pack("<i", len(new)) + new
        states.append(state)
        st["n_records"] += 1; st["n_kept"] += r >= 0
        st["n_refined"] += state == "changed"; st["n_identical"] += state == "identical"; st["n_pos_moved"] += "pos_moved" in t
        if state in REASONS:
            st["n_unrefined"] += 1; st["n_" + state] += 1
        for k in ("NM", "MD", "cs"):
            st["n_%s_replaced" % k.lower()] += any(e.startswith(k + ":replaced") for e in t)
        if trace is not None:
            trace += t
    return out, len(idx), st, states


# ---------------- reading an alignment back (tests) ----------------
def expand_cigar(pos0, words, bases, ref, ref_beg):
    """a CIGAR with = / X / I / D / S against the window and the read's codes -> per-base events [(kind, ref position (1-based), read index)]; '=' / 'X' are
    re-decided from the bases, so the result says what the record's bytes describe, not what its words claim"""
    ev, p, q = [], pos0 + 1, 0
    for w in words:
        op, l = w & 0xf, w >> 4
        if op in (EQ, X, 0):
            for j in range(l):
                ev.append(("=" if int(bases[q + j]) == int(ref[p + j - ref_beg]) else "X", p + j, q + j))
            p += l; q += l
        elif op == INS:
            ev += [("I", p, q + j) for j in range(l)]; q += l
        elif op == DEL:
            ev += [("D", p + j, q) for j in range(l)]; p += l
        elif op == SOFT:
            q += l
    return ev


def digar_events(d):
    ev = []
    for pos, t, l, qi, *_ in d:
        pos, l, qi = int(pos), int(l), int(qi)
        if t in (EQ, X):
            ev += [("=" if t == EQ else "X", pos + j, qi + j) for j in range(l)]
        elif t == INS:
            ev += [("I", pos, qi + j) for j in range(l)]
        elif t == DEL:
            ev += [("D", pos + j, qi) for j in range(l)]
    return ev


def md_ref_events(md):
    """an MD string -> the reference-consuming columns in order: '=' per matched base, ('X', letter) per mismatch, ('D', letter) per deleted base"""
    out = []
    for num, dele, sub in re.findall(rb"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            out += ["="] * int(num)
        elif dele:
            out += [("D", bytes([c])) for c in dele]
        else:
            out.append(("X", sub))
    return out


def cs_events(cs):
    """a cs string -> columns in order: '=' per matched base, ('X', ref, read), ('I', base), ('D', base)"""
    out = []
    for num, sub, ins, dele in re.findall(rb":(\d+)|\*([a-z][a-z])|\+([a-z]+)|-([a-z]+)", cs):
        if num:
            out += ["="] * int(num)
        elif sub:
            out.append(("X", sub[:1], sub[1:]))
        elif ins:
            out += [("I", bytes([c])) for c in ins]
        else:
            out += [("D", bytes([c])) for c in dele]
    return out


# ---------------- the refine log: the rounds loop composed from the oracles, with ref<->read strings on ----------------
def update_digars(oracle, digars, qlen, e):
    """oracle/digar_rewrite.c on one log entry -> (rc, new rows | None)"""
    import ctypes as C
    from longcalld_amd._lib import LcdDigar
    rows = [tuple(int(v) for v in d[:5]) for d in digars]
    arr = (LcdDigar * max(len(rows), 1))(*[LcdDigar(*d) for d in rows])
    out, n = C.POINTER(LcdDigar)(), C.c_int(0)
    t, q = np.ascontiguousarray(e["target"], np.uint8), np.ascontiguousarray(e["query"], np.uint8)
    u8p = C.POINTER(C.c_uint8)
    fn = oracle.lib().lcdo_update_digars_from_msa1
    fn.restype = C.c_int
    rc_ = fn(arr, len(rows), int(qlen), len(t), t.ctypes.data_as(u8p), q.ctypes.data_as(u8p), int(e["cover"]), C.c_int64(int(e["reg_beg"])), C.c_int64(int(e["reg_end"])),
             int(e["read_beg"]), int(e["read_end"]), C.byref(out), C.byref(n))
    res = [(out[i].pos, out[i].type, out[i].len, out[i].qi, out[i].is_low_qual) for i in range(n.value)] if rc_ == 0 else None
    if out:
        libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]; libc.free(C.cast(out, C.c_void_p))
    return rc_, res


def apply_log(oracle, digars, qlens, log):
    """the log applied front to back on a running copy (rc 1 keeps the old list, rc 2 is untouched) -> ({read id: final rows} of the reads the log names, rejected)"""
    cur, rej = {}, 0
    for e in log:
        r = int(e["read_id"])
        if r not in cur:
            cur[r] = [tuple(int(v) for v in d[:5]) for d in digars[r]]
        rc, new = update_digars(oracle, cur[r], qlens[r], e)
        if rc == 0:
            cur[r] = new
        rej += rc == 1
    return cur, rej


def oracle_rounds_log(oracle, ch, digs, cv, state, ordered, skipped, max_len=50000, max_cov=1000, flank=10, slices_from_refined=False):
    """pass_plan_common.oracle_rounds with opt.collect_ref_read_aln_str: the same loop, and per region that resolves one log entry per (cluster, read) in
    update_digars_from_aln_str's order.  slices_from_refined: the read slices of every region are cut from the digars refined SO FAR (what the reference does)
    instead of the original ones (what the device does) -> (oracle_rounds' dict, log, slices [(region beg, read, cover, read_beg, read_end, bases)], final digars)"""
    import merge_vars_common as mc
    import pass_plan_common as pc
    from longcalld_amd.jobs import GERMLINE_ALL
    rb = [d["beg"] for d in digs]; re_ = [d["end"] for d in digs]
    o, ref = ch["ref_beg"], ch["ref"]
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    order = pc.sort_noisy_regs(regs)
    done = np.zeros(len(regs), np.int32)
    state = {k: v.copy() for k, v in state.items()}
    opt = oracle.default_opt(); opt.collect_ref_read_aln_str = 1
    cur = [[tuple(int(v) for v in x[:5]) for x in d["digars"]] for d in digs]
    log, slices, n_passes = [], [], 0
    f2f = np.arange(cv["n_vars"], dtype=np.int32)
    while len(regs) and n_passes < 20:
        n_passes += 1
        status, begs, ends, lists = pc.oracle_plan(regs, done, ordered, skipped, rb, re_, o, o + len(ref) - 1, max_len, max_cov)
        new_done, got = False, []
        for i in order:
            if status[i] in (pc.SKIP_LONG, pc.SKIP_DEEP):
                done[i] = 1; new_done = True
            if status[i] != pc.SUBMIT:
                continue
            beg, end, ids = int(begs[i]), int(ends[i]), lists[i]
            seqs, quals, covers, sl = [], [], [], {}
            for r in ids:
                rd = ch["reads"][r]
                src = np.asarray(cur[r], np.int64).reshape(-1, 5) if slices_from_refined else np.asarray(digs[r]["digars"])
                r0, r1, c = oracle.read_region_slice(src[:, :4], len(rd["qual"]), beg, end, flank)
                seqs.append(rd["seq"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
                quals.append(rd["qual"][r0:r1 + 1].copy() if r1 >= r0 else np.zeros(0, np.uint8))
                covers.append(c); sl[int(r)] = (int(c), int(r0), int(r1))
                slices.append((beg, int(r), int(c), int(r0), int(r1), seqs[-1].tobytes()))
            idv = np.asarray(ids, np.int32)
            reg = dict(reg_len=end - beg + 1, read_ids=idv, seqs=seqs, quals=quals, covers=np.asarray(covers, np.int32), haps=state["haps"][idv],
                       phase_sets=state["phase_sets"][idv], ref=ref[beg - o:end - o + 1])
            res = oracle.collect_noisy_reg_aln_strs(reg, opt)
            if res["n_cons"] == 0:
                continue
            v = oracle.make_vars_from_msa_cons_aln(res, beg, ref, o)
            v["row_read_ids"] = np.concatenate([np.asarray(res["clu_read_ids"][c], np.int32) for c in range(res["n_cons"])] + [np.zeros(0, np.int32)])
            for c in range(res["n_cons"]):
                for j, rid in enumerate(res["clu_read_ids"][c]):
                    s = res["aln_strs"][c][2 * j + 2]
                    cvr, r0, r1 = sl[int(rid)]
                    e = dict(read_id=int(rid), cover=cvr, read_beg=r0, read_end=r1, reg_beg=beg, reg_end=end, pass_=n_passes - 1, target=s["target"], query=s["query"])
                    log.append(e)
                    rc, new = update_digars(oracle, cur[int(rid)], len(ch["reads"][int(rid)]["qual"]), e)
                    if rc == 0:
                        cur[int(rid)] = new
            done[i] = 1; new_done = True
            got.append(v)
        if any(v["n_vars"] > 0 for v in got):
            merged, c2m, _ = mc.oracle_merge(cv, got, ordered, skipped)
            state = pc.carry(state, merged["n_vars"], c2m)
            state = oracle.assign_hap_germline(pc.py_hap_problem(merged, ordered, skipped, ch.get("is_ont", 0)), GERMLINE_ALL, state=state)
            cv, f2f = merged, np.asarray(c2m, np.int32)[f2f]
        if not new_done:
            break
    return dict(cv=cv, state=state, done=done, n_passes=n_passes, first_to_final=f2f), log, slices, cur
