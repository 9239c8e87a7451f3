"""lcd_chunk_mod_pileup over two adjacent chunks of one contig that share reads: every (record, site) pair is counted by exactly one chunk -- the one whose region
holds the site -- for all its kept records, so the chunks' rows joined in plan order are the table of the whole stretch, and no site appears twice."""
import pytest

import mods_common as mc
from bam_src_common import CONTIG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_chunks(lcd, tmp_path_factory):
    s = mc.seeded(seed=23, n_reads=160)
    path = str(tmp_path_factory.mktemp("mods2") / "two.bam")
    mc.write_bam(path, s["recs"], block=9000, tlen=s["tlen"])
    rb, re_ = s["first"] + 1, s["first"] + s["span"]
    cut = next(p for p in range(s["first"] + s["span"] // 2, re_) if s["ref"][p - 1] == 1 and s["ref"][p] == 2)     # the C of a CpG: the cut goes through it
    regs = [(rb, cut), (cut + 1, re_)]
    chunks = [lcd.DeviceChunk.from_bam(path, path + ".bai", CONTIG, a, b, min_mapq=30, src=(s["ref"], 1, s["tlen"], 0)) for a, b in regs]
    yield s, regs, chunks
    for c in chunks:
        c.close()


@pytest.mark.parametrize("combine", [False, True])
def test_the_union_of_two_chunks_is_the_whole_stretch(lcd, two_chunks, combine):
    s, regs, chunks = two_chunks
    import bam_out_common as bo
    shared = {id(b) for b, r in bo.region_records(s["bodies"], *regs[0], 30) if r >= 0} & {id(b) for b, r in bo.region_records(s["bodies"], *regs[1], 30) if r >= 0}
    assert len(shared) >= 10                                                      # reads that both chunks hold
    # a read's hap is the same in both chunks here, so the whole stretch as ONE chunk is the yardstick
    haps = [mc.haps_for(s["bodies"], a, b, 2) for a, b in regs]
    got = [c.mod_pileup(h, s["ref"], 1, s["tlen"], combine_strands=combine) for c, h in zip(chunks, haps)]
    whole_haps = mc.haps_for(s["bodies"], regs[0][0], regs[1][1], 2)
    want_rows, want_st = mc.pileup(s["bodies"], s["ref"], 1, regs[0][0], regs[1][1], whole_haps, combine=combine)
    rows = mc.merge_rows([g[0] for g in got])
    assert rows == want_rows
    assert sum(g[1]["n_counted"] for g in got) == want_st["n_counted"]
    keys = [(p, x) for g in got for p, x, _ in g[0]]
    if combine:
        assert got[0][0][-1][0] == got[1][0][0][0] == regs[0][1]                  # the cut CpG: one row in each chunk, the same key, added by the join
        assert len(set(keys)) == len(keys) - 1
    else:
        assert len(set(keys)) == len(keys)                                        # no site twice


def test_each_chunk_counts_with_its_own_haps(lcd, two_chunks):
    s, regs, chunks = two_chunks
    for k, (c, (a, b)) in enumerate(zip(chunks, regs)):
        haps = mc.haps_for(s["bodies"], a, b, 5 + k)                              # the shared reads get another hap in the second chunk
        rows, st = c.mod_pileup(haps, s["ref"], 1, s["tlen"])
        want_rows, want_st = mc.pileup(s["bodies"], s["ref"], 1, a, b, haps)
        assert rows == want_rows and {x: st[x] for x in mc.STAT_KEYS} == want_st
        assert want_st["n_outside"] > 0
