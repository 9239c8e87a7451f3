"""Pure-Python oracle of the phased alignment output (lcd_chunk_tag_records, lcd_write_phased): the HP:i / PS:i rewrite of write_read_to_bam
(src/bam_utils.c:1944-2006) on one record, a region's record stream with its skip counts, and the pieces the GPU tests need to read a BGZF / BAM file back.
Written from the rules of include/lcd_hotpath.h, on bam_src_common.aux_walk (bam_aux_get's walk).  Every decision leaves a named entry in `trace`, so that
tests/test_bam_out_oracle.py can prove from the oracle's own trace that each condition of its case table was reached.
  * a tag is WANTED for a kept record when hap != 0 (HP) / ps > 0 (PS); the first field of that name stays where it is when bam_aux2i of it equals the wanted value,
    else it is deleted and HP:i / PS:i (4 bytes, the low 32 bits) is appended -- HP first, then PS; an unwanted tag's first field is deleted; later fields of the
    same name stay; a filtered record loses its first HP and first PS field;
  * bam_aux2i: types c C s S i I give their value, any other type 0;
  * the iterator's overlap test applies whatever the flags say; a record with the unmapped flag, or whose CIGAR consumes no reference, spans one base."""
import struct
import zlib

from bam_src_common import aux_walk

FILTER_FLAGS = 0x4 | 0x100 | 0x800


def aux2i(ty, val):
    fmt = dict(c="<b", C="<B", s="<h", S="<H", i="<i", I="<I").get(ty)
    return struct.unpack(fmt, bytes(val))[0] if fmt else 0


def parse(body):
    """the fixed fields of a record body (without its block_size word) -> dict(pos0, end (bam_endpos by the project's rule), flag, mapq, name, aux0)"""
    refid, pos, lname, mapq, _bin, nc, flag, lseq = struct.unpack("<iiBBHHHi", body[:20])
    cig = struct.unpack("<%dI" % nc, body[32 + lname:32 + lname + 4 * nc])
    rl = sum(c >> 4 for c in cig if (c & 0xf) in (0, 2, 3, 7, 8))
    end = pos + 1 if (flag & 4) or rl == 0 else pos + rl
    return dict(refid=refid, pos0=pos, end=end, flag=flag, mapq=mapq, name=body[32:32 + lname - 1], aux0=32 + lname + 4 * nc + (lseq + 1) // 2 + lseq)


def field_spans(aux):
    """aux_walk's fields with their [beg, end) in the auxiliary block"""
    out, p = [], 0
    for tag, ty, val in aux_walk(aux):
        n = 3 + len(val) + (1 if ty in "ZH" else 0)
        out.append((tag, ty, val, p, p + n)); p += n
    return out


def tag_aux(aux, kept, hap=0, ps=0, trace=None):
    """the auxiliary block of one record after the rewrite"""
    trace = trace if trace is not None else []
    first = {}
    for tag, ty, val, b, e in field_spans(aux):
        if tag in (b"HP", b"PS") and tag not in first:
            first[tag] = (ty, val, b, e)
    dels, app = [], b""
    for tag, want, value in ((b"HP", bool(kept) and hap != 0, hap), (b"PS", bool(kept) and ps > 0, ps)):
        f, name = first.get(tag), tag.decode()
        if not kept:
            trace.append(f"{name}:filtered_{'deleted' if f else 'absent'}")
            if f:
                dels.append(f[2:])
        elif want and f and aux2i(f[0], f[1]) == value:
            trace.append(f"{name}:kept_in_place:{f[0]}")
        elif want:
            trace.append(f"{name}:replaced:{f[0]}" if f else f"{name}:appended_absent")
            if f:
                dels.append(f[2:])
            app += tag + b"i" + struct.pack("<I", value & 0xffffffff)
        else:
            trace.append(f"{name}:unwanted_{'deleted:' + f[0] if f else 'absent'}")
            if f:
                dels.append(f[2:])
    out, p = b"", 0
    for b, e in sorted(dels):
        out += aux[p:b]; p = e
    return out + aux[p:] + app


def tag_record(body, kept, hap=0, ps=0, trace=None):
    """a record body -> the rewritten body (everything in front of the auxiliary block is untouched)"""
    a0 = parse(body)["aux0"]
    return body[:a0] + tag_aux(body[a0:], kept, hap, ps, trace)


def region_records(bodies, reg_beg, reg_end, min_mapq, refid=0):
    """the records the iterator of region [reg_beg, reg_end] (1-based) yields, in file order -> [(body, chunk read id | -1)]; sorted input: the walk stops at the
    first record at or behind reg_end"""
    out, n_kept = [], 0
    for body in bodies:
        x = parse(body)
        if x["refid"] != refid:
            continue
        if x["pos0"] >= reg_end:
            break
        if x["end"] <= reg_beg - 1:
            continue
        kept = not (x["flag"] & FILTER_FLAGS) and x["mapq"] >= min_mapq
        out.append((body, n_kept if kept else -1))
        n_kept += kept
    return out


def skip_counts(recs, prev_beg, prev_end):
    """(n_skip_kept, n_skip_filtered) of a region whose predecessor is [prev_beg, prev_end]: is_ovlp_with_prev_region on [pos0 + 1, bam_endpos]"""
    sk = sf = 0
    for body, r in recs:
        x = parse(body)
        if not (x["end"] < prev_beg or x["pos0"] + 1 > prev_end):
            if r >= 0:
                sk += 1
            else:
                sf += 1
    return sk, sf


def tagged_stream(recs, haps, phase_sets, n_skip_kept=0, n_skip_filtered=0, trace=None):
    """lcd_chunk_tag_records on region_records' list -> (bytes, number of records written)"""
    out, n, sk, sf = b"", 0, n_skip_kept, n_skip_filtered
    for body, r in recs:
        if r >= 0 and sk > 0:
            sk -= 1; continue
        if r < 0 and sf > 0:
            sf -= 1; continue
        new = tag_record(body, r >= 0, int(haps[r]) if r >= 0 else 0, int(phase_sets[r]) if r >= 0 else 0, trace)
        out += struct.pack("<i", len(new)) + new; n += 1
    return out, n


# ---------------- reading files back ----------------
def bgzf_members(image):
    """a BGZF image member by member -> [dict(payload bytes, bsize, crc, isize, comp = the raw deflate stream)]; asserts the container fields of SAM spec 4.1, that
    the stream ends exactly at its last byte and that no member is larger than 64 KB"""
    out, o = [], 0
    while o < len(image):
        assert image[o:o + 4] == b"\x1f\x8b\x08\x04" and image[o + 10:o + 16] == b"\x06\x00BC\x02\x00", o
        bsize = struct.unpack("<H", image[o + 16:o + 18])[0] + 1
        assert bsize <= 65536 and o + bsize <= len(image)
        comp = image[o + 18:o + bsize - 8]
        crc, isize = struct.unpack("<II", image[o + bsize - 8:o + bsize])
        d = zlib.decompressobj(-15)
        data = d.decompress(comp)
        assert d.eof and d.unused_data == b"" and len(data) == isize and zlib.crc32(data) & 0xffffffff == crc, o
        # no unused trailing bits beyond the final byte: the stream cut by its last byte no longer ends
        if comp:
            d2 = zlib.decompressobj(-15); d2.decompress(comp[:-1])
            assert not d2.eof, o
        out.append(dict(payload=data, bsize=bsize, crc=crc, isize=isize, comp=comp))
        o += bsize
    assert o == len(image)
    return out


def bam_split(stream):
    """an inflated BAM stream -> (header block bytes, [record bodies])"""
    assert stream[:4] == b"BAM\x01"
    o = 8 + struct.unpack("<i", stream[4:8])[0]
    n_ref = struct.unpack("<i", stream[o:o + 4])[0]; o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack("<i", stream[o:o + 4])[0] + 4
    hdr, bodies = stream[:o], []
    while o < len(stream):
        bs = struct.unpack("<i", stream[o:o + 4])[0]
        bodies.append(stream[o + 4:o + 4 + bs]); o += 4 + bs
    assert o == len(stream)
    return hdr, bodies


def header_with_pg(hdr, pg_line):
    """the header block with one line appended to its text"""
    l_text = struct.unpack("<i", hdr[4:8])[0]
    text = hdr[8:8 + l_text]
    add = (b"" if not text or text.endswith(b"\n") else b"\n") + pg_line + b"\n"
    return hdr[:4] + struct.pack("<i", l_text + len(add)) + text + add + hdr[8 + l_text:]
