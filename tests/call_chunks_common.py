"""Helpers of the read-order and alt_ref_base tests: sort_chunk_reads' comparator (src/bam_utils.c:1616-1656) restated in Python, a writer for a small BAM whose
records carry chosen names and auxiliary fields (the BGZF / index pieces are those of tests/test_io.py), the NM cases of the device walk, and the alt_ref_base
column of a merge (make_cand_vars0, src/collect_var.c:1755-1756) written beside the pure-Python merge oracle of tests/merge_vars_common.py."""
import struct

import numpy as np

from test_io import _bgzf, _write_bai

CDIFF, CINS, CDEL = 8, 1, 2


# ---------------- comp_bam_read_sort ----------------
def read_sort_key(pos, end, nm, name):
    """pos ascending, end DESCENDING, NM ascending, strcmp of the names (bytes compare as unsigned chars; names hold no NUL)"""
    return (int(pos), -int(end), int(nm), name.encode() if isinstance(name, str) else bytes(name))


def python_order(pos, end, nm, names):
    """the read ids in sort_chunk_reads' order; Python's sort is stable: a full tie keeps file order (the project rule)"""
    keys = [read_sort_key(p, e, m, s) for p, e, m, s in zip(pos, end, nm, names)]
    return np.array(sorted(range(len(keys)), key=keys.__getitem__), np.int32)


# ---------------- a BAM with chosen names and auxiliary fields ----------------
def write_aux_bam(path, recs, chrom="chr11", ref_len=100000, block=1500):
    """recs: dicts(name, pos0, qlen, aux bytes[, flag]) in coordinate order; every read is `<qlen>=` with bases A and quality 30.  Adds u0 (the offset of the record's
    block_size word in the uncompressed stream) and aux0 (the offset of its first auxiliary byte) to each dict."""
    refs = [(chrom, ref_len)]
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n"
    d = b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", len(refs))
    for nm, ln in refs:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    out = []
    for r in recs:
        name = r["name"].encode() + b"\0"
        qlen = int(r["qlen"])
        cig = np.array([(qlen << 4) | 7], "<u4")
        packed = np.full((qlen + 1) // 2, 0x11, np.uint8)
        if qlen & 1:
            packed[-1] = 0x10
        fixed = struct.pack("<iiBBHHHiiii", 0, int(r["pos0"]), len(name), 60, 4680, 1, int(r.get("flag", 0)), qlen, -1, -1, 0) + name + cig.tobytes() + \
            packed.tobytes() + np.full(qlen, 30, np.uint8).tobytes()
        body = fixed + bytes(r["aux"])
        r["u0"] = len(d); r["aux0"] = len(d) + 4 + len(fixed)
        d += struct.pack("<i", len(body)) + body
        out.append(dict(tid=0, pos=int(r["pos0"]), end=int(r["pos0"]) + qlen, u0=r["u0"], u1=len(d)))
    coffs = []
    open(path, "wb").write(_bgzf(d, block=block, offsets=coffs))
    coffs.append(coffs[-1] + 1)
    for x in out:
        x["vbeg"] = (coffs[x["u0"] // block] << 16) | (x["u0"] % block)
        x["vend"] = (coffs[x["u1"] // block] << 16) | (x["u1"] % block) if x["u1"] < len(d) else ((coffs[(len(d) - 1) // block] << 16) | ((len(d) - 1) % block + 1))
    _write_bai(path + ".bai", len(refs), out)
    return recs


def nm_records():
    """16 records: (name, pos0, qlen, aux bytes, the NM bam_get_NM gives).  Four records share each start; inside a group NM and the names decide the order, and in
    the second group the ends differ.  The names' lengths differ, so the records and their auxiliary fields start at every byte offset modulo 4."""
    f = lambda tag, ty, fmt, v: tag + ty + struct.pack(fmt, v)
    rg = b"RGZgrp1\0"
    cs = b"csZ" + b":100*ag" * 700 + b"\0"                          # 4 900 bytes in front of the NM field
    spec = [
        ("a", 400, f(b"NM", b"c", "<b", 5), 5),
        ("bb", 400, rg + f(b"NM", b"c", "<b", -3), -3),              # a negative c
        ("ccc", 400, f(b"NM", b"C", "<B", 200), 200),
        ("dddd", 400, f(b"xs", b"s", "<h", -7) + f(b"NM", b"s", "<h", -300), -300),
        ("r10", 300, f(b"NM", b"S", "<H", 40000), 40000),           # (second group: the longer reads come first)
        ("r9", 500, f(b"NM", b"i", "<i", 70000), 70000),
        ("e", 401, f(b"NM", b"I", "<I", 3000000000), 3000000000 - (1 << 32)),   # wraps in the reference's int
        ("ff", 401, b"NMZ12\0", 0),                                  # a Z-typed NM: 0
        ("zz", 350, rg + f(b"xf", b"f", "<f", 1.5), 0),              # no NM (its name puts it behind the two `same` records of equal NM)
        ("r9", 350, cs + f(b"NM", b"i", "<i", 7), 7),                # behind a long cs:Z field
        ("same", 350, b"XBBi" + struct.pack("<I", 1000) + b"\1\0\0\0" + f(b"NM", b"i", "<i", 9), 0),   # the B array runs past the record: the NM behind it does not exist
        ("same", 350, b"XZZabc" + b"NMC\x09", 0),                    # a Z value without its NUL inside the record
        ("g", 351, b"NMAx", 0),                                      # another type: 0
        ("hh", 351, f(b"NM", b"C", "<B", 4) + f(b"NM", b"C", "<B", 9), 4),   # the first NM field decides
        ("iii", 351, b"XBBS" + struct.pack("<IHHH", 3, 1, 2, 3) + f(b"NM", b"s", "<h", 17), 17),
        ("jjjj", 351, f(b"NM", b"f", "<f", 2.0), 0),
    ]
    return [dict(name=s[0], pos0=1000 + 50 * (i // 4), qlen=s[1], aux=s[2], nm=s[3]) for i, s in enumerate(spec)]


# ---------------- alt_ref_base through a merge ----------------
def merged_alt_ref_base(cv, regions, cur_to_merged, region_to_merged, n_merged):
    """the column lcd_merge_region_vars must give, from the maps of the merge: a kept table entry carries its value (4 where the table has no column), a kept region
    entry 0 for an X variant and the region's alt_ref_base for an insertion / deletion; an equal region entry was dropped (map -1) and changes nothing"""
    out = np.full(n_merged, 255, np.uint8)
    cur = cv.get("alt_ref_base")
    for i, m in enumerate(cur_to_merged):
        out[m] = 4 if cur is None else cur[i]
    for reg, r2m in zip(regions, region_to_merged):
        for j, m in enumerate(r2m):
            if m >= 0:
                out[m] = 0 if int(reg["var_type"][j]) == CDIFF else int(reg["alt_ref_base"][j])
    assert (out != 255).all()
    return out


# ---------------- the head of collect_var_main composed by hand ----------------
def low_comp_of(sdust, ch):
    """chunk->low_comp_cr: sdust over the bases of [reg_beg, reg_end], cr_add(reg_beg + start - 1, reg_beg + finish - 1)"""
    o = ch["ref_beg"]
    low = sdust(ch["ref"][ch["reg_beg"] - o:ch["reg_end"] - o + 1], 5, 20)
    return np.stack([ch["reg_beg"] + low[:, 0] - 1, ch["reg_beg"] + low[:, 1] - 1], 1).astype(np.int64).reshape(-1, 2)


def pre_inputs(digs, ordered, skipped):
    """pre_process_noisy_regs' inputs: the reads in ordered_read_ids order with the skipped ones left out (collect_digars_from_bam's cr_add order)"""
    kept = [int(r) for r in ordered if not skipped[r]]
    chunk_noisy = np.concatenate([digs[r]["chunk_noisy"].reshape(-1, 3) for r in kept] + [np.zeros((0, 3), np.int64)])
    return chunk_noisy, [digs[r]["beg"] for r in kept], [digs[r]["end"] for r in kept], [digs[r]["noisy"].reshape(-1, 3) for r in kept]


def first_round_chain(lcd, oracle, ch, digs, ordered, dev=None):
    """the first round composed by hand: the oracles' side (dev None) or the library's single exports on the device chunk"""
    import clean_vars_common as cc
    import pass_plan_common as pc
    from longcalld_amd import jobs
    is_ont = ch.get("is_ont", 0)
    skipped = np.array([d["rc"] != 0 for d in digs], np.uint8)
    low = low_comp_of(oracle.ref_sdust if dev is None else lcd.sdust, ch)
    pre = (oracle.ref_pre_process_noisy_regs if dev is None else lcd.pre_process_noisy_regs)(pre_inputs(digs, ordered, skipped)[0], low, *pre_inputs(digs, ordered, skipped)[1:])
    pre = np.asarray(pre, np.int64).reshape(-1, 3)
    opt = lcd.clean_opt(is_ont)
    if dev is None:
        cv = cc.run_oracle(ch, digs, opt, pre_regs=pre, low_comp=low, ordered=ordered)
    else:
        cv = dev.clean_vars(ordered, ch["ref"], ch["ref_beg"], ch["ref_beg"] + len(ch["ref"]) - 1, ch["reg_beg"], ch["reg_end"], pre, low,
                            is_rev=np.array([x["is_rev"] for x in ch["reads"]], np.uint8), opt=opt)
    st = pc.fresh_state(len(digs), cv["n_vars"])
    if cv["n_vars"] > 0:
        if dev is None:
            st = oracle.assign_hap_germline(pc.py_hap_problem(cv, ordered, skipped, is_ont), jobs.GERMLINE_CLEAN)
        else:
            st = lcd.assign_hap_germline(lcd.clean_vars_hap_problem(cv, ordered, skipped, is_ont), jobs.GERMLINE_CLEAN)
    return dict(is_skipped=skipped, low_comp=low, pre_regs=pre, cv=cv, state=st)


# ---------------- the whole path composed from the oracles ----------------
# two-chunk seeds: make_diploid_chunk(seed, ref_len=12000, depth=12) cut at its midpoint, noisy regions up to 600 bases.  tests/test_call_chunks_oracle.py proves from
# the oracle's own output that the stitch of SEED_FLIP joins the chunks and swaps the second one's haplotypes and that of SEED_JOIN joins them as they are
SEED_FLIP, SEED_JOIN, TWO_CHUNK_MAX_LEN = 1, 3, 600


def planted_anchor_chunk(seed=77, ins_len=5):
    """one chunk in which a noisy-region insertion's anchor base is not the reference base: haplotype 1 carries a cluster of 8 SNPs in 64 bases (the noisy region) and,
    inside it, a 5-base insertion immediately right of a SNP that BOTH haplotypes carry.  The second consensus pins that SNP to its reference column, so the
    insertion cannot be moved in front of it and its record's first ALT base is the SNP's base (cand_var_t.alt_ref_base, src/collect_var.c:1544)"""
    import clean_vars_common as cc
    rng = np.random.default_rng(seed)
    L = 6000
    ref = rng.integers(0, 4, L).astype(np.uint8)
    hap1 = {3000 + 8 * k: ("X", int((ref[3000 + 8 * k] + 1 + k % 3) % 4)) for k in range(8)}
    x = int((ref[3035] + 2) % 4)
    both = {3035: ("X", x), 1000: ("X", int((ref[1000] + 1) % 4)), 5000: ("X", int((ref[5000] + 1) % 4))}
    hap1[3036] = ("I", [int((x + 1) % 4)] * ins_len)
    hap1.update({1500: ("X", int((ref[1500] + 1) % 4)), 4500: ("X", int((ref[4500] + 1) % 4))})
    reads = []
    for i in range(14):
        ev = dict(both)
        if i % 2 == 0:
            ev.update(hap1)
        reads.append(dict(cc.read_from_hap(ref, 300 + 40 * i, 5200 - 30 * i, ev), is_rev=0))
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=L, whole_ref_len=L, is_ont=0), 3036   # (the record's position: the SNP's, 1-based)


def anchor_differs(records):
    """the gap records whose first ALT base is not their first REF base"""
    return [r for r in records if r["type"] in (CINS, CDEL) and any(a[:1] != r["ref"][:1] for a in r["alt"])]


def two_chunks(seed):
    import clean_vars_common as cc
    return split_chunk(cc.make_diploid_chunk(seed, ref_len=12000, depth=12), [6000])


def read_end(r):
    """bam_endpos of a record dict (0-based exclusive = 1-based inclusive end)"""
    return int(r["pos0"]) + sum(int(c) >> 4 for c in r["cigar"] if (int(c) & 0xf) in (0, 2, 3, 7, 8))


def split_chunk(ch, cuts):
    """one seeded chunk -> chunks of the same contig in genome order: regions [reg_beg, cuts[0]], [cuts[0] + 1, cuts[1]], ..., each with the reads the loader would
    give it (pos0 < reg_end and bam_endpos > reg_beg - 1, file order) and the whole reference window"""
    bounds = [ch["reg_beg"] - 1] + list(cuts) + [ch["reg_end"]]
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        rb, re_ = lo + 1, hi
        reads = [r for r in ch["reads"] if r["pos0"] < re_ and read_end(r) > rb - 1]
        out.append(dict(ch, reads=reads, reg_beg=rb, reg_end=re_))
    return out


def ovlp_with_region(read_beg, read_end_, reg_beg, reg_end):
    """is_ovlp_with_prev_region / _next_region (src/bam_utils.c:1586-1614) on [pos0 + 1, bam_endpos]"""
    return not (read_end_ < reg_beg or read_beg > reg_end)


def overlap_lists(chs):
    """per chunk (up, down): its reads, in file order, that overlap the previous / the next chunk's region"""
    res = []
    for c, ch in enumerate(chs):
        up = [i for i, r in enumerate(ch["reads"]) if c > 0 and ovlp_with_region(r["pos0"] + 1, read_end(r), chs[c - 1]["reg_beg"], chs[c - 1]["reg_end"])]
        down = [i for i, r in enumerate(ch["reads"]) if c + 1 < len(chs) and ovlp_with_region(r["pos0"] + 1, read_end(r), chs[c + 1]["reg_beg"], chs[c + 1]["reg_end"])]
        res.append((np.array(up, np.int32), np.array(down, np.int32)))
    return res


def oracle_rounds_arb(oracle, ch, digs, cv, state, ordered, skipped, max_len=50000):
    """pass_plan_common.oracle_rounds with cand_var_t.alt_ref_base carried beside the table: 4 for the first round's variants, the value of
    oracle.make_vars_from_msa_cons_aln through the maps of the merge oracle (merged_alt_ref_base above) -> oracle_rounds' dict, cv with the column"""
    import merge_vars_common as mc
    import pass_plan_common as pc
    from longcalld_amd.jobs import GERMLINE_ALL
    rb = [d["beg"] for d in digs]; re_ = [d["end"] for d in digs]
    o, ref = ch["ref_beg"], ch["ref"]
    regs = np.asarray(cv["regs"], np.int64).reshape(-1, 3)
    order = pc.sort_noisy_regs(regs)
    done = np.zeros(len(regs), np.int32)
    cv = dict(cv, alt_ref_base=np.full(cv["n_vars"], 4, np.uint8))
    state = {k: v.copy() for k, v in state.items()}
    n_passes = 0
    while len(regs) and n_passes < 20:
        n_passes += 1
        status, begs, ends, lists = pc.oracle_plan(regs, done, ordered, skipped, rb, re_, o, o + len(ref) - 1, max_len, 1000)
        new_done, got = False, []
        for i in order:
            if status[i] in (pc.SKIP_LONG, pc.SKIP_DEEP):
                done[i] = 1; new_done = True
            if status[i] != pc.SUBMIT:
                continue
            n_cons, v = pc.oracle_region(oracle, ch, digs, int(begs[i]), int(ends[i]), lists[i], state, 10)
            if n_cons == 0:
                continue
            done[i] = 1; new_done = True
            got.append(v)
        if any(v["n_vars"] > 0 for v in got):
            plain = {k: v for k, v in cv.items() if k != "alt_ref_base"}
            merged, c2m, r2m = mc.oracle_merge(plain, got, ordered, skipped)
            merged["alt_ref_base"] = merged_alt_ref_base(cv, got, c2m, r2m, merged["n_vars"])
            state = pc.carry(state, merged["n_vars"], c2m)
            state = oracle.assign_hap_germline(pc.py_hap_problem(merged, ordered, skipped, ch.get("is_ont", 0)), GERMLINE_ALL, state=state)
            cv = merged
        if not new_done:
            break
    return dict(cv=cv, state=state, done=done, n_passes=n_passes)


def emit_records(lib, prefix, ch, cv, state, ordered, skipped):
    """make_variants + annotate_te (no TE library) + the VCF lines of one chunk through `lib` (the product's or the oracle's: tests/emit_common.py)"""
    import emit_common as ec
    import pass_plan_common as pc
    from longcalld_amd import _lib, align
    keep = []
    prob = pc.py_hap_problem(cv, ordered, skipped, ch.get("is_ont", 0))
    st = {k: np.ascontiguousarray(v).copy() for k, v in state.items()}
    keep.append(st)
    hs = align._fill_hap_struct(_lib.LcdHapProblem, prob, st, keep)
    extra = dict(var_ref_len=cv["ref_len"], var_alt_len=cv["alt_len"], alt_off=np.asarray(cv["alt_off"], np.uint64), alt_pool=np.concatenate([cv["alt_pool"], np.zeros(1, np.uint8)]),
                 alt_ref_base=np.concatenate([cv["alt_ref_base"], np.zeros(1, np.uint8)]))
    if cv["n_vars"] == 0:
        return [], ""
    return ec.make_variants(lib, prefix, hs, ec.default_call_opt(), extra, np.ascontiguousarray(ch["ref"], np.uint8).tobytes(), ch["ref_beg"], ch["reg_beg"], ch["reg_end"],
                            te=dict(lib=None, names=[]))


def stitch(lib, prefix, chs, finals):
    """stitch_var_main over the chunks' final states (mutated: haps, phase_sets, var_phase_set, hap_to_cons_alle) -> per chunk (flip_hap, flip_pre_PS, flip_cur_PS)"""
    import emit_common as ec
    lists = overlap_lists(chs)
    ds = []
    for ch, f, (up, down) in zip(chs, finals, lists):
        st = f["state"]
        for k in ("haps", "phase_sets", "var_phase_set", "hap_to_cons_alle"):
            st[k] = np.ascontiguousarray(st[k]).copy()
        ds.append(dict(tid=0, ordered_read_ids=np.ascontiguousarray(f["ordered"], np.int32), is_skipped=np.ascontiguousarray(f["skipped"], np.uint8), haps=st["haps"],
                       phase_sets=st["phase_sets"], var_phase_set=st["var_phase_set"], hap_to_cons_alle=st["hap_to_cons_alle"], up_ovlp=up, down_ovlp=down))
    flips = [(0, -1, -1)]
    for i in range(1, len(ds)):
        rc, fl = ec.flip(lib, prefix, ds[i - 1], ds[i], 1)
        assert rc == 0, rc
        flips.append(fl if fl[1] != -7 else (0, -1, -1))      # (emit_common.flip presets -7: the pair was not joined)
    return flips


def shift_chunk(ch, new_ref_beg, tail=60000):
    """the chunk moved along its contig so that its reference window starts at new_ref_beg (a test FASTA then need not hold megabases in front of it)"""
    d = new_ref_beg - ch["ref_beg"]
    reads = [dict(r, pos0=r["pos0"] + d) for r in ch["reads"]]
    return dict(ch, reads=reads, ref_beg=new_ref_beg, reg_beg=ch["reg_beg"] + d, reg_end=ch["reg_end"] + d, whole_ref_len=new_ref_beg + len(ch["ref"]) - 1 + tail)


def write_fasta(path, chrom, ch, width=60):
    """a FASTA + .fai of the chunk's contig: N in front of and behind the chunk's reference window"""
    seq = np.full(ch["whole_ref_len"], 4, np.uint8)
    seq[ch["ref_beg"] - 1:ch["ref_beg"] - 1 + len(ch["ref"])] = ch["ref"]
    text = np.frombuffer(b"ACGTN", np.uint8)[seq].tobytes().decode()
    head = f">{chrom}\n"
    with open(path, "w") as f:
        f.write(head)
        for i in range(0, len(text), width):
            f.write(text[i:i + width] + "\n")
    with open(path + ".fai", "w") as f:
        f.write(f"{chrom}\t{len(text)}\t{len(head)}\t{width}\t{width + 1}\n")


def stepped_call(lcd, oracle, prod, chs, devs, popt):
    """the library's single exports composed by hand: first round (first_round_chain on the device chunk), pass_plan_common.stepped_rounds, lcd_flip_variant_hap,
    lcd_make_variants + lcd_annotate_te + lcd_format_vcf_te -> oracle_call's dict"""
    import clean_vars_common as cc
    import pass_plan_common as pc
    finals = []
    for ch, dev in zip(chs, devs):
        digs = cc.read_digars(ch, oracle, ch.get("is_ont", 0))
        ordered = np.arange(len(ch["reads"]), dtype=np.int32)
        first = first_round_chain(lcd, oracle, ch, digs, ordered, dev)
        r = pc.stepped_rounds(lcd, dev, first["cv"], first["state"], ordered, first["is_skipped"], ch["ref"], ch["ref_beg"], popt, ch.get("is_ont", 0))
        finals.append(dict(cv=r["cv"], state=r["state"], n_passes=r["n_passes"], ordered=ordered, skipped=first["is_skipped"]))
    flips = stitch(prod, "lcd_", chs, finals)
    records, text = [], ""
    for ch, f, fl in zip(chs, finals, flips):
        recs, t = emit_records(prod, "lcd_", ch, f["cv"], f["state"], f["ordered"], f["skipped"])
        f["flip"], f["n_records"] = fl, len(recs)
        records += recs; text += t
    return dict(chunks=finals, records=records, vcf_body=text)


def same_call(got, want, state_keys=None):
    """lcd.chunks_call's / call_bam_regions' dict against oracle_call's / stepped_call's: per chunk the final table, state, n_passes and flip; the records; the text"""
    import clean_vars_common as cc
    import pass_plan_common as pc
    assert len(got["chunks"]) == len(want["chunks"])
    for g, w in zip(got["chunks"], want["chunks"]):
        assert g["n_passes"] == w["n_passes"], (g["n_passes"], w["n_passes"])
        cc.same_clean_vars(g["cv"], w["cv"])
        assert g["cv"]["alt_ref_base"].tolist() == np.asarray(w["cv"]["alt_ref_base"]).tolist()
        pc.same_state(g["state"], w["state"], state_keys or pc.STATE_KEYS)
        assert (g["flip_hap"], g["flip_pre_PS"], g["flip_cur_PS"]) == tuple(int(x) for x in w["flip"]), ((g["flip_hap"], g["flip_pre_PS"], g["flip_cur_PS"]), w["flip"])
        assert g["n_records"] == w["n_records"]
    assert len(got["records"]) == len(want["records"])
    for x, y in zip(got["records"], want["records"]):
        assert x == y, (x, y)
    assert got["vcf_body"] == want["vcf_body"]


def oracle_call(lcd, oracle, chs, max_len=50000, orders=None):
    """chunks of one contig through the oracles end to end -> dict(chunks = per chunk dict(cv, state, n_passes, flip, ordered, skipped, n_records), records, vcf_body)"""
    finals = []
    for ci, ch in enumerate(chs):
        digs = [oracle.collect_digar_from_eqx_cigar(r["pos0"], r["cigar"], r["qual"], ch["reg_beg"], ch["reg_end"], ch["whole_ref_len"], opt=oracle.digar_opt(ch.get("is_ont", 0)))
                for r in ch["reads"]]
        ordered = np.arange(len(ch["reads"]), dtype=np.int32) if orders is None else np.asarray(orders[ci], np.int32)
        first = first_round_chain(lcd, oracle, ch, digs, ordered)
        rounds = oracle_rounds_arb(oracle, ch, digs, first["cv"], first["state"], ordered, first["is_skipped"], max_len)
        finals.append(dict(cv=rounds["cv"], state=rounds["state"], n_passes=rounds["n_passes"], ordered=ordered, skipped=first["is_skipped"]))
    flips = stitch(oracle.lib(), "lcdo_", chs, finals)
    records, text = [], ""
    for ch, f, fl in zip(chs, finals, flips):
        recs, t = emit_records(oracle.lib(), "lcdo_", ch, f["cv"], f["state"], f["ordered"], f["skipped"])
        f["flip"], f["n_records"] = fl, len(recs)
        records += recs; text += t
    return dict(chunks=finals, records=records, vcf_body=text)

