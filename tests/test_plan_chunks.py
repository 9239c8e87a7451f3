"""lcd_plan_chunks (collect_regions, src/call_var_main.c:404-634, and the fallback of :744-749) against the rules restated in Python
(tests/call_file_common.py::python_plan): contig classes, -E, region strings, BED files, the fallback.  Host code: no device is needed."""
import pytest

import call_file_common as fc

L = 1000
NAMES = ["chr1", "chr2", "chr22", "chr23", "chrX", "chrY", "chrM", "MT", "1", "X", "chr1_random", "chrUn_x", "hs37d5"]
LENS = [1, L - 1, L, L + 1, 5 * L // 2]


def contigs(rot=0):
    return [(n, LENS[(i + rot) % len(LENS)]) for i, n in enumerate(NAMES)]


def both(lcd, ctg, tmp_path=None, bed_text=None, **kw):
    bed = None
    if bed_text is not None:
        bed = str(tmp_path / "regions.bed")
        open(bed, "w").write(bed_text)
    got = lcd.plan_chunks(ctg, kw.get("mode", 0), kw.get("exclude", ()), kw.get("regions", ()), bed, kw.get("chunk_len", L))
    want = fc.python_plan(ctg, kw.get("mode", 0), kw.get("exclude", ()), kw.get("regions", ()), bed_text, kw.get("chunk_len", L))
    assert got == want, (kw, bed_text)
    return got


def test_classify_chromosome_as_written():
    cls = {n: fc.classify(n) for n in NAMES}
    assert cls == {"chr1": 0, "chr2": 0, "chr22": 0, "chr23": 0, "chrX": 1, "chrY": 1, "chrM": 2, "MT": 2, "1": 0, "X": 1, "chr1_random": 2, "chrUn_x": 2, "hs37d5": 2}


@pytest.mark.parametrize("rot", range(5))
@pytest.mark.parametrize("mode", [fc.CTG_AUTOSOME_XY, fc.CTG_AUTOSOME, fc.CTG_ALL])
def test_whole_genome_modes_and_every_length(lcd, mode, rot):
    ctg = contigs(rot)
    plan, fb = both(lcd, ctg, mode=mode)
    assert fb == 0
    kept = {n for n in NAMES if mode == fc.CTG_ALL or fc.classify(n) == 0 or (mode == fc.CTG_AUTOSOME_XY and fc.classify(n) == 1)}
    assert {NAMES[t] for t, _, _ in plan} == kept                                  # chr23 and "1" are autosomes, chr1_random is not
    for tid, (nm, ln) in enumerate(ctg):
        mine = [(b, e) for t, b, e in plan if t == tid]
        if nm in kept:
            assert len(mine) == -(-ln // L) and mine[0][0] == 1 and mine[-1][1] == ln and all(e - b + 1 <= L for b, e in mine)
            assert all(mine[i + 1][0] == mine[i][1] + 1 for i in range(len(mine) - 1))
    assert [t for t, _, _ in plan] == sorted(t for t, _, _ in plan)                 # header order


def test_default_chunk_len_is_500000(lcd):
    plan, _ = both(lcd, [("chr1", 1200000)], chunk_len=0)
    assert plan == [(0, 1, 500000), (0, 500001, 1000000), (0, 1000001, 1200000)]


@pytest.mark.parametrize("mode", [fc.CTG_AUTOSOME_XY, fc.CTG_AUTOSOME, fc.CTG_ALL])
def test_excluded_names(lcd, mode):
    plan, fb = both(lcd, contigs(3), mode=mode, exclude=["chr2", "X", "hs37d5", "nope"])
    assert fb == 0 and not {NAMES[t] for t, _, _ in plan} & {"chr2", "X", "hs37d5"}


REGION_CASES = [
    ["chr22"],                                   # chr
    ["chr23:300"],                               # chr:beg
    ["chr23:300-700"],                           # chr:beg-end
    ["hs37d5:1,200-2,400"],                      # from its own begin; the classes are off
    ["chr23:5000"],                              # beg past the contig end
    ["chr23:200-99999"],                         # end past the length
    ["hs37d5:100-1500", "hs37d5:1400-2300"],     # two overlapping regions
    ["hs37d5:100-300", "hs37d5:301-500"],        # adjacent, not overlapping
    ["chrY:2-5", "chr2:1-1", "chr1_random:10-2000", "chr2:700-800"],   # out of header order
    ["chr77:1-100", "chr22:10-20"],              # an unknown contig
    ["chr77", "zz:1-5"],                         # only unknown contigs: the fallback
    ["chrM", "MT:1-1"],                          # 'other' contigs are planned when named
    ["chr23:0-10", "chr23:-5-3"],                # non-positive begins are clamped / unparsable
]


@pytest.mark.parametrize("rot", [0, 2, 4])
@pytest.mark.parametrize("regions", REGION_CASES, ids=[",".join(r) for r in REGION_CASES])
def test_region_strings(lcd, regions, rot):
    for mode in (fc.CTG_AUTOSOME_XY, fc.CTG_AUTOSOME):                              # regions switch the classes off
        both(lcd, contigs(rot), mode=mode, regions=regions)
    both(lcd, contigs(rot), regions=regions, exclude=["hs37d5", "chr22"])           # ... but not -E


def test_region_examples_by_hand(lcd):
    ctg = [("chr1", 2500), ("chr2", 999), ("chrM", 1001)]
    assert lcd.plan_chunks(ctg, regions=["chr1:300"], chunk_len=L) == ([(0, 300, 1299), (0, 1300, 2299), (0, 2300, 2500)], 0)
    assert lcd.plan_chunks(ctg, regions=["chrM:990-5000", "chr1:10-20"], chunk_len=L) == ([(0, 10, 20), (2, 990, 1001)], 0)
    assert lcd.plan_chunks(ctg, regions=["chr1:100-1500", "chr1:1400-2300"], chunk_len=L) == ([(0, 100, 1099), (0, 1100, 2099), (0, 2100, 2300)], 0)
    assert lcd.plan_chunks(ctg, regions=["chr1:3000"], chunk_len=L) == ([(0, 1, 1000), (0, 1001, 2000), (0, 2001, 2500), (1, 1, 999), (2, 1, 1000), (2, 1001, 1001)], 1)


BED_CASES = [
    "chr22\n",                                                   # one column
    "chr23\t299\n",                                              # two columns: 0-based begin, to the contig's end
    "chr23\t299\t700\n",                                         # three columns
    "# a comment\nchr23\t0\t10\n#chr22\t0\t5\n",                  # '#' lines
    "chr77\t0\t10\nchr22\t4\t9\n",                               # an unknown contig
    "chr23\t700\t300\nchr23\t10\t20\n",                          # beg > end
    "chr23\t-1\t5\nchr23\t3\t0\nchr22\t0\t1\n",                  # non-positive bounds
    "hs37d5\t99\t1500\nchr2\t0\t1\nhs37d5\t1399\t2300",          # overlapping, out of order, a last line without a newline
    "chr23\t5\t10\textra\tcolumns\n",
    "chr77\t0\t10\n",                                            # nothing usable: the fallback
    "",
]


@pytest.mark.parametrize("rot", [0, 2, 4])
@pytest.mark.parametrize("bed", BED_CASES, ids=[repr(b)[:40] for b in BED_CASES])
def test_bed_files(lcd, tmp_path, bed, rot):
    both(lcd, contigs(rot), tmp_path, bed_text=bed, mode=fc.CTG_AUTOSOME)
    both(lcd, contigs(rot), tmp_path, bed_text=bed, exclude=["chr23"])


def test_strings_win_over_a_bed_file(lcd, tmp_path):
    bed = str(tmp_path / "r.bed")
    open(bed, "w").write("chr2\t0\t5\n")
    got = lcd.plan_chunks(contigs(), regions=["chr22:1-2"], region_bed_path=bed, chunk_len=L)
    assert got == fc.python_plan(contigs(), regions=["chr22:1-2"], bed_text="chr2\t0\t5\n", chunk_len=L) == ([(2, 1, 2)], 0)


def test_a_missing_bed_file_is_an_error(lcd, tmp_path):
    with pytest.raises(lcd.LcdError, match="-30"):
        lcd.plan_chunks(contigs(), region_bed_path=str(tmp_path / "absent.bed"), chunk_len=L)


@pytest.mark.parametrize("mode", [fc.CTG_AUTOSOME_XY, fc.CTG_AUTOSOME])
def test_fallback_plans_every_contig_and_sets_the_flag(lcd, mode):
    ctg = [("chrM", 2500), ("chrUn_x", 1), ("hs37d5", 1001)]
    plan, fb = both(lcd, ctg, mode=mode)
    assert fb == 1 and plan == [(0, 1, 1000), (0, 1001, 2000), (0, 2001, 2500), (1, 1, 1), (2, 1, 1000), (2, 1001, 1001)]
    plan, fb = both(lcd, ctg, mode=mode, exclude=["chrM"])                           # -E still applies
    assert fb == 1 and plan == [(1, 1, 1), (2, 1, 1000), (2, 1001, 1001)]
    assert both(lcd, [("chrX", 10)], mode=fc.CTG_AUTOSOME) == ([(0, 1, 10)], 1)
    assert both(lcd, [("chrX", 10)], mode=fc.CTG_AUTOSOME_XY) == ([(0, 1, 10)], 0)


def test_bad_arguments(lcd):
    for kw in (dict(contig_mode=7), dict(chunk_len=-1)):
        with pytest.raises(lcd.LcdError, match="-4"):
            lcd.plan_chunks(contigs(), **kw)
