"""lcd_call_files with lcd_index_opt_t on the seeded multi-contig file of tests/test_gpu_call_file.py: the output BAM's .bai (built by the writer from the tagged stream in HBM)
against the oracle's index of the written file, for every schedule; region queries on the output through lcd_bam_load_region_indexed; an output that is not sorted
gets no index and says so; missing input indexes are built on request, change no result byte and are not touched again."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import bai_common as bc
import call_chunks_common as kc
import call_file_common as fc
import clean_vars_common as cc

pytestmark = pytest.mark.gpu

CHUNK_LEN = 6000
PG = "@PG\tID:longcalld_amd\tPN:longcalld_amd"
ORDER = ["chr1", "chr2", "chr3", "chr4", "chrM"]


def cfg_of(lcd):
    return lcd.call_cfg(0, pass_=dict(max_noisy_reg_len=kc.TWO_CHUNK_MAX_LEN))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the file of tests/test_gpu_call_file.py: chr1 / chr2 the seeded 12 kb diploid contigs, chr3 18 kb, chr4 12 kb without a read, chrM 6 kb"""
    d = tmp_path_factory.mktemp("call_file_index")
    chs = dict(chr1=cc.make_diploid_chunk(kc.SEED_FLIP, ref_len=12000, depth=12), chr2=cc.make_diploid_chunk(kc.SEED_JOIN, ref_len=12000, depth=12),
               chr3=cc.make_diploid_chunk(41, ref_len=18000, depth=12), chrM=cc.make_diploid_chunk(43, ref_len=6000, depth=12, read_len=(1000, 3000)))
    refs = dict({k: v["ref"] for k, v in chs.items()}, chr4=np.random.default_rng(4).integers(0, 4, 12000).astype(np.uint8))
    reads = {k: (chs[k]["reads"] if k in chs else []) for k in ORDER}
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    fc.write_multi_bam(bam, [(k, len(refs[k]), reads[k]) for k in ORDER], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    fc.write_multi_fasta(fa, [(k, refs[k]) for k in ORDER])
    return dict(dir=d, bam=bam, fa=fa, refs=refs, reads=reads, contigs=[(k, len(refs[k])) for k in ORDER])


def run(lcd, data, tag, bam=None, fa=None, index=None, **kw):
    vcf, out = str(data["dir"] / f"{tag}.vcf"), str(data["dir"] / f"{tag}.bam")
    res = lcd.call_file(bam or data["bam"], fa or data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, bam_out=dict(path=out, pg_line=PG), cfg=cfg_of(lcd), no_vcf_header=1,
                        contig_mode=2, index=index, **kw)
    res["text"], res["bam"], res["image"] = open(vcf).read(), out, open(out, "rb").read()
    return res


@pytest.fixture(scope="module")
def schedules(lcd, data):
    return {(w, o): run(lcd, data, f"w{w}o{o}", index=dict(write_out_bai=1), window_chunks=w, overlap=o) for w in (2, 0) for o in (0, 1)}


def test_the_output_index_equals_the_oracle_for_every_schedule(lcd, data, schedules):
    first = None
    for key, res in schedules.items():
        assert res["index"]["wrote_out_bai"] == 1 and res["index"]["out_bai_skipped"] == 0, res["index"]
        got = open(res["bam"] + ".bai", "rb").read()
        s = bc.scan_bam(res["image"])                                                    # the written file, re-read with zlib
        assert len(s["recs"]) > 100 and s["recs"] == sorted(s["recs"], key=lambda x: (x["tid"], x["pos"]))
        assert got == bc.oracle_bai(len(s["refs"]), s["recs"]), key
        assert res["index"]["out_bai_bytes"] == len(got) and res["index"]["out_n_indexed"] == len(s["recs"])
        first = first or (got, res["image"])
        assert (got, res["image"]) == first                                              # identical across the four schedules
    assert not os.path.exists(run(lcd, data, "plain")["bam"] + ".bai")                   # without the option nothing is written


def test_region_queries_on_the_output(lcd, data, schedules):
    from longcalld_amd._lib import LcdBamReads
    lib = lcd.load_library()
    lib.lcd_bam_load_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_bam_load_region_indexed.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(LcdBamReads)]
    lib.lcd_bam_reads_free.argtypes = [C.POINTER(LcdBamReads)]
    res = schedules[(2, 0)]
    s = bc.scan_bam(res["image"])
    rng = np.random.default_rng(5)
    hit = 0
    for k in range(100):
        t = int(rng.choice([0, 1, 2, 3, 4]))
        ln = data["contigs"][t][1]
        b = int(rng.integers(0, ln)); e = min(ln, b + int(rng.integers(1, 4000)))
        a, q = LcdBamReads(), LcdBamReads()
        n = lib.lcd_bam_load_region(res["bam"].encode(), ORDER[t].encode(), b + 1, e, 0, 1, C.byref(a))
        m = lib.lcd_bam_load_region_indexed(res["bam"].encode(), (res["bam"] + ".bai").encode(), ORDER[t].encode(), b + 1, e, 0, C.byref(q))
        want = [s["recs"][i] for i in bc.records_by_scan(s, t, b, e) if not s["recs"][i]["flag"] & (4 | 256 | 2048)]
        assert n == m == len(want), (t, b, e)
        assert [q.pos0[i] for i in range(m)] == [x["pos"] for x in want] == [a.pos0[i] for i in range(n)]
        hit += bool(want)
        lib.lcd_bam_reads_free(C.byref(a)); lib.lcd_bam_reads_free(C.byref(q))
    assert hit > 50


def test_an_unsorted_output_is_completed_without_an_index(lcd, data):
    """lcd_plan_chunks sorts and merges the regions of a contig, so the plan alone never puts a contig's chunks out of order; an input whose records are out of order
    inside a region does: the writer's stream then violates rule 3"""
    reads = dict(data["reads"])
    r3 = list(reads["chr3"])
    k = next(i for i in range(len(r3) - 1, 0, -1) if r3[i]["pos0"] != r3[i - 1]["pos0"])     # the last two records of chr3 with different positions change places
    r3[k - 1], r3[k] = r3[k], r3[k - 1]
    reads["chr3"] = r3
    bam = str(data["dir"] / "unsorted.bam")
    fc.write_multi_bam(bam, [(c, len(data["refs"][c]), reads[c]) for c in ORDER], header_text=fc.DEFAULT_HEADER + b"@RG\tID:x\tSM:sample7\n")
    res = run(lcd, data, "unsorted_out", bam=bam, index=dict(write_out_bai=1), window_chunks=2, overlap=0)
    s = bc.scan_bam(res["image"])                                                        # the BAM is complete: header, records, ONE EOF member at the end
    assert s["tab"][-1][2] == 0 and sum(1 for _c, _u, n in s["tab"] if n == 0) == 1 and len(s["recs"]) > 100
    with pytest.raises(bc.BaiRefused):
        bc.oracle_bai(len(s["refs"]), s["recs"])                                         # the oracle refuses the written file too
    assert not os.path.exists(res["bam"] + ".bai")
    assert res["index"]["out_bai_skipped"] == bc.ERR_ORDER and res["index"]["wrote_out_bai"] == 0 and "record " in res["index"]["out_bai_skip_reason"]


def test_missing_input_indexes_are_built_once_and_change_nothing(lcd, data):
    want = run(lcd, data, "with_indexes", window_chunks=2, overlap=0)
    d = data["dir"] / "bare"
    d.mkdir()
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    shutil.copy(data["bam"], bam); shutil.copy(data["fa"], fa)
    with pytest.raises(lcd.LcdError, match="error -30:.*in.bam.bai"):
        run(lcd, data, "bare0", bam=bam, fa=fa, window_chunks=2, overlap=0)              # idx == NULL: as before
    with pytest.raises(lcd.LcdError, match="error -30:.*ref.fa.fai.*build_missing_fai"):   # the message names the option that would have built it
        run(lcd, data, "bare1", bam=bam, fa=fa, index=dict(build_missing_bai=1), window_chunks=2, overlap=0)
    os.remove(bam + ".bai")
    got = run(lcd, data, "bare2", bam=bam, fa=fa, index=dict(build_missing_bai=1, build_missing_fai=1), window_chunks=2, overlap=0)
    assert got["index"]["built_bai"] == 1 and got["index"]["built_fai"] == 1
    assert got["text"] == want["text"] and got["image"] == want["image"]
    s = bc.scan_bam(open(bam, "rb").read())
    assert open(bam + ".bai", "rb").read() == bc.oracle_bai(len(s["refs"]), s["recs"])
    assert open(fa + ".fai").read() == open(data["fa"] + ".fai").read()                  # the generator's own .fai is the oracle's
    stamp = (os.stat(bam + ".bai").st_mtime_ns, os.stat(fa + ".fai").st_mtime_ns)
    again = run(lcd, data, "bare3", bam=bam, fa=fa, index=dict(build_missing_bai=1, build_missing_fai=1), window_chunks=2, overlap=0)
    assert again["index"]["built_bai"] == 0 and again["index"]["built_fai"] == 0
    assert (os.stat(bam + ".bai").st_mtime_ns, os.stat(fa + ".fai").st_mtime_ns) == stamp and again["image"] == want["image"]
    with pytest.raises(lcd.LcdError, match="error -30:.*nowhere"):                       # an unwritable location names its path
        run(lcd, data, "bare4", bam=bam, fa=fa, bai_path=str(d / "nowhere" / "x.bai"), index=dict(build_missing_bai=1), window_chunks=2, overlap=0)
