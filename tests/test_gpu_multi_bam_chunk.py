"""lcd_chunk_open_from_bams on the MI355X: one chunk from several BAMs of one sample -- their region images appended, one inflate, one walk launch, the reads
file-major -- against lcd_chunk_open_from_bam on every file alone: read_info, digars, NM, sources and meta of the merged chunk are the concatenation, in file order,
of what the files give on their own.  Regions [1, 6000] and [6001, 12000] of the seeded contig of tests/test_gpu_call_file.py, dealt out to two files with records
the loader filters over the border."""
import numpy as np
import pytest

import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc
import multi_bam_common as mb

pytestmark = pytest.mark.gpu

REGIONS = [(1, 6000), (6001, 12000)]
META_KEYS = ("pos0", "end_pos", "mapq", "flag", "n_cigar", "qlen")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi_chunk")
    ch = cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12)
    other = cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12)
    fa, fb = mb.deal(ch["reads"], "chr1", 2, borders=[6000])
    p = {k: str(d / f"{k}.bam") for k in ("A", "B", "E", "O", "Bm")}
    ctg = lambda r1, r2: [("chr1", 12000, r1), ("chr2", 12000, r2)]
    mb.write_bam(p["A"], ctg(fa, []))
    chr2 = [dict(r, name=f"chr2_r{i}") for i, r in enumerate(other["reads"])]
    mb.write_bam(p["B"], ctg(fb, chr2), block=7000)                                  # (another block size: the files' members differ in length; records of a later contig follow)
    mb.write_bam(p["E"], ctg([], []))                                                # the header and no record
    mb.write_bam(p["O"], ctg([], chr2))                                              # reads on another contig only
    mb.write_bam(p["Bm"], ctg([dict(r, cigar=fc.m_cigar(r["cigar"])) for r in fb], []))                    # file B with plain-M CIGARs
    return dict(paths=p, ref=ch["ref"], files=dict(A=fa, B=fb, E=[], O=[], Bm=fb))


def src_of(data):
    return (data["ref"], 1, len(data["ref"]), 0)


def view(lcd, chunk):
    """everything the test compares, on the host"""
    info = chunk.read_info()
    v = dict(n=chunk.n, meta={k: chunk.meta[k].tolist() for k in META_KEYS}, names=list(chunk.meta["names"]), info={k: info[k].tolist() for k in info},
             digars=[x.tolist() for x in chunk.digars()], nm=lcd.chunk_read_nm(chunk).tolist(), source=chunk.sources()["source"].tolist(),
             head=(chunk.meta["tid"], chunk.meta["n_targets"], chunk.meta["target_len"]))
    return v


@pytest.fixture(scope="module")
def alone(lcd, data):
    """per file and region: lcd_chunk_open_from_bam + resolve on the file alone (the reference of every case; computed once)"""
    out = {}
    for k, path in data["paths"].items():
        for reg in REGIONS:
            c = lcd.DeviceChunk.open_from_bam(path, path + ".bai", "chr1", *reg, min_mapq=30)
            c.resolve(src_of(data))
            out[k, reg] = view(lcd, c)
            hp = np.arange(c.n) % 3; ps = np.where(hp > 0, 1000 + np.arange(c.n), 0)
            out[k, reg]["tagged"] = c.tag_records(hp, ps)
            c.close()
    return out


def concat(parts):
    w = dict(n=sum(p["n"] for p in parts), meta={k: [x for p in parts for x in p["meta"][k]] for k in META_KEYS}, names=[x for p in parts for x in p["names"]],
             info={k: [x for p in parts for x in p["info"][k]] for k in parts[0]["info"]}, digars=[x for p in parts for x in p["digars"]],
             nm=[x for p in parts for x in p["nm"]], source=[x for p in parts for x in p["source"]], head=parts[0]["head"])
    return w


@pytest.mark.parametrize("case", ["A+B", "A+B+E", "E+A+B", "A+O", "O+A+B", "B+A", "A+Bm", "Bm+A"])
@pytest.mark.parametrize("reg", REGIONS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_merged_chunk_is_the_concatenation_of_its_files(lcd, data, alone, case, reg):
    keys = case.split("+")
    paths = [data["paths"][k] for k in keys]
    c = lcd.chunk_open_from_bams(paths, None if case != "B+A" else [p + ".bai" for p in paths], "chr1", *reg, min_mapq=30)
    try:
        assert c.n_files == len(keys)
        want_files = [f for f, k in enumerate(keys) for _ in range(alone[k, reg]["n"])]
        assert c.file_of_read.tolist() == want_files and c.n == len(want_files)
        c.resolve(src_of(data))
        got, want = view(lcd, c), concat([alone[k, reg] for k in keys])
        for k in ("n", "meta", "names", "head", "nm", "source", "info"):
            assert got[k] == want[k], k
        assert got["digars"] == want["digars"]
        # the data is what the case says: both files contribute, the filtered records exist, the plain-M file is compared with the reference
        rows, reads = mb.chunk_table([data["files"][k] for k in keys], *reg)
        assert [r["name"] for r in reads] == got["names"] and got["meta"]["pos0"] == [r["pos0"] for r in reads]
        assert sum(1 for r in rows if r["read"] < 0) >= 2 and len({r["file"] for r in rows}) == sum(1 for k in keys if data["files"][k])
        if "Bm" in keys:
            assert set(got["source"]) == {0, 3}                                       # LCD_SRC_EQX and LCD_SRC_REF in one chunk
        # the record table behind the reads: every file's records, kept and filtered, in file-major order (table order, nothing left out)
        hp = np.arange(c.n) % 3; ps = np.where(hp > 0, 1000 + np.arange(c.n), 0)
        stream, n_rec = c.tag_records(hp, ps)
        assert n_rec == len(rows)
        assert c.tag_records_sel(hp, ps) == (stream, n_rec)
        skip, order = mb.python_plan(rows, 1, reg[0] - 6000, reg[0] - 1, 1)
        assert lcd.merged_record_plan([r["file"] for r in rows], [r["pos0"] for r in rows], [r["end"] for r in rows], 1, reg[0] - 6000, reg[0] - 1, 1)[1].tolist() == order
        sel, n_sel = c.tag_records_sel(hp, ps, skip, order)
        bodies = split_records(stream)
        assert n_sel == len(order) and split_records(sel) == [bodies[i] for i in order]
    finally:
        c.close()


def split_records(stream):
    import struct
    out, o = [], 0
    while o < len(stream):
        bs = struct.unpack("<i", stream[o:o + 4])[0]
        out.append(stream[o + 4:o + 4 + bs]); o += 4 + bs
    assert o == len(stream)
    return out


@pytest.mark.parametrize("reg", REGIONS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_one_file_is_the_old_export(lcd, data, alone, reg):
    for k in ("A", "Bm", "E"):
        path = data["paths"][k]
        c = lcd.chunk_open_from_bams([path], [path + ".bai"], "chr1", *reg, min_mapq=30)
        try:
            assert c.n_files == 1 and not c.file_of_read.any()
            c.resolve(src_of(data))
            got = view(lcd, c)
            for key in got:
                assert got[key] == alone[k, reg][key], (k, key)
            hp = np.arange(c.n) % 3; ps = np.where(hp > 0, 1000 + np.arange(c.n), 0)
            assert c.tag_records(hp, ps) == alone[k, reg]["tagged"]                   # the record stream, byte for byte
        finally:
            c.close()


def test_errors(lcd, data, tmp_path):
    p = data["paths"]
    with pytest.raises(lcd.LcdError, match="absent.bai"):                             # the message names the file
        lcd.chunk_open_from_bams([p["A"], p["B"]], [None, str(tmp_path / "absent.bai")], "chr1", 1, 6000)
    with pytest.raises(lcd.LcdError, match="chrZ"):
        lcd.chunk_open_from_bams([p["A"], p["B"]], None, "chrZ", 1, 6000)
    c = lcd.chunk_open_from_bams([p["A"], p["B"]], None, "chr1", 1, 6000)
    c.resolve(src_of(data))
    n_rec = c.tag_records(np.zeros(c.n, np.int32), np.zeros(c.n, np.int64))[1]
    with pytest.raises(lcd.LcdError, match="exactly once"):
        c.tag_records_sel(np.zeros(c.n, np.int32), np.zeros(c.n, np.int64), np.zeros(n_rec, np.uint8), np.zeros(n_rec, np.int32))
    c.close()
