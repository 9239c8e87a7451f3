"""lcd_write_phased / lcd_bam_writer_open as SAM text on the MI355X: the synthetic BAM of tests/test_gpu_bam_tags.py through chunk creation, a fixed haplotype state
and the writer.  The file is the oracle's header plus the oracle's lines of bam_out_common.tagged_stream's records, and it is the oracle formatting of the records
decoded from what the BAM format writes for the same chunks (the BAM path against the SAM path) -- with one chunk, with two (the overlap skip), with
sort_output, with a refine log on the chunk (refine_common's records), and with a header that has @SQ lines and NUL padding."""
import struct

import pytest

import bam_out_common as bo
import refine_cases as rcases
import refine_common as rc
import sam_out_common as so
import test_gpu_bam_tags as tg
from bam_src_common import CONTIG, TLEN, _bgzf, record, write_bam

pytestmark = pytest.mark.gpu
PG = b"@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:call --sam"
NAMES = [CONTIG.encode()]


def inflate(path):
    return b"".join(m["payload"] for m in bo.bgzf_members(open(path, "rb").read()))


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_writer")
    path = str(d / "t.bam")
    cs = tg.cases()
    recs = [record(tg._read(i, 500 + 230 * i, qlen, flag), [(qlen << 4) | 7], [(None, None, aux)], mapq=mapq) for i, (_, aux, qlen, flag, mapq, _, _) in enumerate(cs)]
    write_bam(path, recs, block=9000)
    return dict(dir=d, path=path, cs=cs, bodies=[r["body"] for r in recs], hdr=bo.bam_split(inflate(path))[0])


def chunks_of(lcd, bam, regions):
    """-> (the writer's chunk dicts, the oracle's record stream of all regions with the overlap skip)"""
    out, stream, prev = [], b"", None
    for beg, end in regions:
        ch = lcd.DeviceChunk.from_bam(bam["path"], bam["path"] + ".bai", CONTIG, beg, end, min_mapq=tg.MIN_MAPQ)
        sk, sf = bo.skip_counts(bo.region_records(bam["bodies"], beg, end, tg.MIN_MAPQ), *prev) if prev else (0, 0)
        (want, _n), haps, ps = tg.expected(bam["cs"], bam["bodies"], beg, end, sk, sf)
        assert ch.n == len(haps)
        out.append(dict(chunk=ch, haps=haps, phase_sets=ps, reg_beg=beg, reg_end=end)); stream += want; prev = (beg, end)
    return out, stream


def bodies_of_stream(s):
    return bo.bam_split(b"BAM\x01" + struct.pack("<ii", 0, 0) + s)[1]


def close(chunks):
    for c in chunks:
        c["chunk"].close()


@pytest.mark.parametrize("regions", [[(1, 29000)], [(1, 5000), (5001, 29000)]], ids=["one_chunk", "two_chunks"])
def test_the_file_is_the_oracle_s_header_and_lines(lcd, bam, regions):
    chunks, stream = chunks_of(lcd, bam, regions)
    bodies = bodies_of_stream(stream)
    assert len(bodies) == 40                                             # the second chunk left out what the first one wrote
    if len(regions) == 2:
        assert len(bodies_of_stream(chunks_of_oracle_without_skip(bam, regions))) > 40
    out = str(bam["dir"] / f"o{len(regions)}.sam")
    st = lcd.write_phased_sam(bam["path"], chunks, out, pg_line=PG)
    text, wst = so.sam_text(bodies, NAMES)
    head = so.sam_header(bam["hdr"], PG)
    assert head == b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % (NAMES[0], TLEN) + PG + b"\n"      # (the test BAM's header has no @SQ line)
    got = open(out, "rb").read()
    assert got[:len(head)] == head
    for k, (g, w) in enumerate(zip(got[len(head):].split(b"\n"), text.split(b"\n"))):
        assert g == w, k
    assert got == head + text
    assert {k: v for k, v in st["sam"].items() if not k.startswith("ms_")} == wst and wst["n_walk_stopped"] == 2
    b = st["bam_out"]
    assert b["bytes_file"] == len(got) and b["ms_deflate"] == 0 and b["bytes_inflated"] == len(stream) and b["n_records_out"] + b["n_filtered_out"] == 40
    # the BAM path on the same chunks: its records, decoded and formatted by the oracle, are the SAM path's lines
    out_bam = str(bam["dir"] / f"o{len(regions)}.bam")
    stb = lcd.write_phased_sam(bam["path"], chunks, out_bam, pg_line=PG, aln_format="bam")
    hdr_b, bodies_b = bo.bam_split(inflate(out_bam))
    assert bodies_b == bodies and so.sam_text(bodies_b, NAMES)[0] == got[len(head):] and so.sam_header(hdr_b, None) == head
    assert stb["bam_out"]["n_records_out"] == b["n_records_out"] and stb["bam_out"]["ms_deflate"] > 0 and stb["sam"]["n_records"] == 0
    # sort_output on a sorted input: the same lines, through open / append / close
    out_s = str(bam["dir"] / f"s{len(regions)}.sam")
    sts = lcd.write_phased_sam(bam["path"], chunks, out_s, pg_line=PG, sort_output=True)
    assert open(out_s, "rb").read() == got and {k: v for k, v in sts["sam"].items() if not k.startswith("ms_")} == wst
    close(chunks)


def chunks_of_oracle_without_skip(bam, regions):
    return b"".join(tg.expected(bam["cs"], bam["bodies"], b, e)[0][0] for b, e in regions)


def test_sort_orders_the_lines_by_position(lcd, bam):
    """the plan with sort_output on a chunk whose table is not in position order is the writer's business (lcd_merged_record_plan, tested on the CPU); here: the SAM
    writer uses it -- tagged_to_sam with a reversed order gives the oracle's lines in that order"""
    ch = lcd.DeviceChunk.from_bam(bam["path"], bam["path"] + ".bai", CONTIG, 1, 29000, min_mapq=tg.MIN_MAPQ)
    (want, n), haps, ps = tg.expected(bam["cs"], bam["bodies"], 1, 29000)
    bodies = bodies_of_stream(want)
    order = list(range(n))[::-1]
    text, n_got, st = lcd.tagged_to_sam(ch, haps, ps, NAMES, order=order)
    assert n_got == n and text == so.sam_text(bodies[::-1], NAMES)[0] and st["n_records"] == n
    skip = [1 if i % 3 == 0 else 0 for i in range(n)]
    text, n_got, _ = lcd.tagged_to_sam(ch, haps, ps, NAMES, skip=skip)
    assert n_got == n - sum(skip) and text == so.sam_text([b for i, b in enumerate(bodies) if not skip[i]], NAMES)[0]
    text, n_got, st = lcd.tagged_to_sam(ch, haps, ps, NAMES, skip=[1] * n)
    assert (text, n_got, st["n_records"]) == (b"", 0, 0)
    ch.close()


def test_path_minus_is_stdout(lcd, bam, capfdbinary):
    chunks, stream = chunks_of(lcd, bam, [(3001, 6000)])
    capfdbinary.readouterr()
    st = lcd.write_phased_sam(bam["path"], chunks, "-", pg_line=PG)
    got = capfdbinary.readouterr().out
    assert got == so.sam_header(bam["hdr"], PG) + so.sam_text(bodies_of_stream(stream), NAMES)[0] and st["bam_out"]["bytes_file"] == len(got)
    close(chunks)


def test_a_header_with_sq_lines_and_nul_padding(lcd, bam, tmp_path):
    """the header comes from in_bam_path alone: a second file with the same table whose text has @SQ, no final newline and NUL padding"""
    text = b"@HD\tVN:1.6\n@SQ\tSN:%s\tLN:%d\tM5:abc\n@RG\tID:g\tSM:s" % (NAMES[0], TLEN) + b"\0" * 5
    blk = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", len(NAMES[0]) + 1) + NAMES[0] + b"\0" + struct.pack("<i", TLEN)
    hdr_only = str(tmp_path / "h.bam")
    open(hdr_only, "wb").write(_bgzf(blk, block=9000, offsets=[]))
    chunks, stream = chunks_of(lcd, bam, [(3001, 6000)])
    for pg, name in ((PG, "pg.sam"), (None, "nopg.sam")):
        out = str(tmp_path / name)
        lcd.write_phased_sam(hdr_only, chunks, out, pg_line=pg)
        head = so.sam_header(blk, pg)
        assert head == b"@HD\tVN:1.6\n@SQ\tSN:%s\tLN:%d\tM5:abc\n@RG\tID:g\tSM:s\n" % (NAMES[0], TLEN) + (pg + b"\n" if pg else b"")
        assert open(out, "rb").read() == head + so.sam_text(bodies_of_stream(stream), NAMES)[0]
    close(chunks)


def test_a_refine_log_on_the_chunk(lcd, oracle, tmp_path):
    """a chunk with a refine log: the writer rewrites its records from the reads' final digars (here the chunk's own: the log is empty), then formats them"""
    path = str(tmp_path / "r.bam")
    cs = rcases.build()
    write_bam(path, [c["rec"] for c in cs], block=9000, tlen=rcases.TLEN)
    _digars_of, _skipped, _touched, kept = rcases.resolve(cs, oracle)
    ch = lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, 1, rcases.TLEN, min_mapq=rcases.MIN_MAPQ, src=(rcases.letters(), 1, rcases.TLEN, 0))
    lib = lcd.load_library()
    assert lib.lcd_chunk_set_refine(ch.h, 1) == 0
    recs = bo.region_records([c["rec"]["body"] for c in cs], 1, rcases.TLEN, rcases.MIN_MAPQ)
    haps = [cs[i]["hap"] for i in kept]; ps = [cs[i]["ps"] for i in kept]
    own = [d.tolist() for d in ch.digars()]
    want, n_want, st_want, _ = rc.refined_stream(recs, own, ch.read_info()["status"] != 0, rcases.WIN, rcases.REF_BEG, rcases.REF_END, haps, ps)
    plain = bo.tagged_stream(recs, haps, ps)[0]
    assert want != plain and st_want["n_refined"] > 0
    out = str(tmp_path / "r.sam")
    st = lcd.write_phased_sam(path, [dict(chunk=ch, haps=haps, phase_sets=ps, reg_beg=1, reg_end=rcases.TLEN, ref=rcases.WIN, ref_beg=rcases.REF_BEG, ref_end=rcases.REF_END)], out)
    got = open(out, "rb").read()
    head = so.sam_header(bo.bam_split(inflate(path))[0], None)
    text, wst = so.sam_text(bodies_of_stream(want), NAMES)
    assert got == head + text and text != so.sam_text(bodies_of_stream(plain), NAMES)[0]
    assert st["refine"]["n_refined"] == st_want["n_refined"] and st["refine"]["n_records"] == n_want == st["sam"]["n_records"] and st["sam"]["bytes_text"] == len(text)
    assert st["sam"]["n_cg_cigar"] == wst["n_cg_cigar"]
    ch.close()
