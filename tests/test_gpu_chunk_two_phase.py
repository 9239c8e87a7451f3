"""Two-phase chunk creation on the MI355X: lcd_chunk_open_from_bam (region image, inflate, record walk, loader's rule, meta) followed by lcd_chunk_resolve (sources,
reference comparison, cs / MD words, digars) equals lcd_chunk_create_from_bam_src in everything a chunk exposes, on the mixed-kind records of
tests/bam_src_common.py (HiFi and ONT) and on an EQX file; an opened handle has no digars until it is resolved."""
import numpy as np
import pytest

import bam_src_common as bs

pytestmark = pytest.mark.gpu

RB, RE = 6000, 24000            # the chunk region and the reference window of tests/test_gpu_bam_sources.py
WB, WE = 5000, 25000


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("two_phase")
    out = {}
    for kind in ("mixed", "eqx"):
        path = str(d / f"{kind}.bam")
        bs.write_bam(path, bs.records_as(kind, sa=kind == "mixed"))
        out[kind] = path
    ref, _ = bs.seeded()
    out["window"] = bs.ref_letters(ref)[WB - 1:WE]
    return out


def view(lcd, dev):
    """everything the exports show of a chunk"""
    info = dev.read_info(); so = dev.sources()
    return dict(n=dev.n, digars=dev.digars(), info=info, ivs=dev.intervals(), source=so["source"], pal=so["is_ont_palindrome"], tag_bytes=so["tag_bytes_d2h"],
                nm=lcd.chunk_read_nm(dev), meta=dev.meta)


def same_view(a, b):
    assert a["n"] == b["n"] and a["n"] > 0
    assert len(a["digars"]) == len(b["digars"]) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a["digars"], b["digars"]))
    for k in ("status", "beg", "end", "n_cand", "n_digars"):
        assert (a["info"][k] == b["info"][k]).all(), k
    for (na, ia), (nb, ib) in zip(a["ivs"], b["ivs"]):
        assert na.shape == nb.shape and (na == nb).all() and (np.asarray(ia) == np.asarray(ib)).all()
    assert (a["source"] == b["source"]).all() and (a["pal"] == b["pal"]).all() and a["tag_bytes"] == b["tag_bytes"]
    assert np.asarray(a["nm"]).tolist() == np.asarray(b["nm"]).tolist()
    for k, v in a["meta"].items():
        assert (np.asarray(v) == np.asarray(b["meta"][k])).all() if not isinstance(v, (int, list)) else v == b["meta"][k], k


@pytest.mark.parametrize("kind,is_ont,with_src", [("mixed", 0, True), ("mixed", 1, True), ("eqx", 0, True), ("eqx", 0, False), ("mixed", 0, False)])
def test_open_then_resolve_equals_the_one_call(lcd, files, kind, is_ont, with_src):
    path = files[kind]
    src = (files["window"], WB, WE, is_ont) if with_src else None
    one = lcd.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30, is_ont=is_ont, src=src)
    two = lcd.DeviceChunk.open_from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30, is_ont=is_ont)
    assert two.n == one.n and two.meta["names"] == one.meta["names"]                 # the reads' span is known before any digar exists
    assert two.resolve(src) == 0
    a, b = view(lcd, one), view(lcd, two)
    same_view(a, b)
    if kind == "mixed" and with_src:
        assert set(a["source"].tolist()) == {0, 1, 2, 3} and a["tag_bytes"] > 0      # every source took part
    if kind == "mixed" and not with_src:
        assert (a["info"]["status"] == -2).any()                                     # 'M' reads without a source, as before
    one.close(); two.close()


def test_an_unresolved_handle_is_refused_and_freed(lcd, files):
    path = files["mixed"]
    dev = lcd.DeviceChunk.open_from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30)
    assert dev.n > 0
    with pytest.raises(lcd.LcdError, match="-4.*not resolved"):
        dev.read_info()
    with pytest.raises(lcd.LcdError, match="-4.*not resolved"):
        dev.digars()
    dev.close()                                                                       # lcd_chunk_destroy on an opened handle
    dev = lcd.DeviceChunk.open_from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30)
    assert dev.resolve((files["window"], WB, WE, 0)) == 0
    with pytest.raises(lcd.LcdError, match="-4"):                                    # resolve twice
        dev.resolve((files["window"], WB, WE, 0))
    assert len(dev.read_info()["status"]) == dev.n                                   # ... and the chunk is still whole
    dev.close()
    one = lcd.DeviceChunk.from_bam(path, path + ".bai", bs.CONTIG, RB, RE, min_mapq=30)
    with pytest.raises(lcd.LcdError, match="-4"):                                    # a chunk of the one-call form is resolved already
        one.resolve(None)
    one.close()


def test_an_empty_region_opens_and_resolves(lcd, files):
    path = files["eqx"]
    dev = lcd.DeviceChunk.open_from_bam(path, path + ".bai", bs.CONTIG, bs.TLEN - 5, bs.TLEN, min_mapq=30)
    assert dev.n == 0 and dev.resolve(None) == 0 and dev.read_info()["status"].tolist() == []
    dev.close()
