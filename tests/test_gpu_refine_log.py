"""lcd_chunks_noisy_rounds_log on the MI355X: the rounds driver with a refine-log sink -- the log equals the one the loop composed from the oracles writes
(entries, order, slices, rows); variants, state and done are those of the run without a sink; the log applied on the host (lcd_refine_log_apply) gives the
oracle's final digars; and those, handed to lcd_chunk_refine_records' oracle, change CIGARs inside noisy regions."""
import numpy as np
import pytest

import clean_vars_common as cc
import pass_plan_common as pc
import refine_common as rc
from test_gpu_noisy_rounds import _item, first_round

pytestmark = pytest.mark.gpu


def _same_log(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for f in ("read_id", "cover", "read_beg", "read_end", "reg_beg", "reg_end", "pass_"):
            assert g[f] == w[f], (k, f, g[f], w[f])
        assert g["target"].tobytes() == np.asarray(w["target"], np.uint8).tobytes() and g["query"].tobytes() == np.asarray(w["query"], np.uint8).tobytes(), k


@pytest.mark.parametrize("which", ["hg002", "seeded"])
def test_g2_log_equals_the_oracles_and_the_call_is_unchanged(lcd, oracle, which):
    ch = cc.events_chunk() if which == "hg002" else cc.make_diploid_chunk(201, ref_len=12000)
    max_len = 3000 if which == "hg002" else 600
    f = first_round(lcd, oracle, ch)
    popt = lcd.pass_opt(max_noisy_reg_len=max_len)
    plain = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], popt=popt)[0]
    log = lcd.RefineLog()
    before = lcd.copy_counters()
    got = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], popt=popt, logs=[log])[0]
    assert lcd.copy_counters() == before                                         # no digar and no base crossed PCIe: only the rows
    pc.same_rounds(got, plain); pc.same_state(got["state"], plain["state"])       # the call never sees a refined digar
    want, wlog, wsl, wdig = rc.oracle_rounds_log(oracle, f["ch"], f["digs"], f["want"], f["ex"], f["ordered"], f["skipped"], max_len=max_len)
    pc.same_rounds(got, want)
    entries = log.entries()
    print(which, "entries", len(entries), "reads", len({e["read_id"] for e in entries}), "row bytes", log.row_bytes(), "passes", got["n_passes"])
    assert len(entries) > 50 and log.row_bytes() == 2 * sum(len(e["target"]) for e in entries)
    _same_log(entries, wlog)
    # the log on the host: the oracle's final digars
    digs = [np.asarray(d["digars"], np.int64).reshape(-1, 5) for d in f["digs"]]
    qlens = [len(r["qual"]) for r in f["ch"]["reads"]]
    touched, rej = log.apply(digs, qlens)
    wt, wrej = rc.apply_log(oracle, digs, qlens, wlog)
    assert sorted(touched) == sorted(wt) and rej == wrej
    changed = 0
    for r in touched:
        assert [tuple(x) for x in touched[r].tolist()] == list(wt[r]) == list(wdig[r]), r
        changed += rc.digars_cigar(touched[r]) != rc.digars_cigar(digs[r])
    assert changed > 0
    # an empty sink list is the old entry point; the old entry point keeps its answer
    same = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], popt=popt, logs=[None])[0]
    pc.same_rounds(same, plain)
    o = lcd.default_opt(); o.collect_ref_read_aln_str = 1
    with pytest.raises(lcd.LcdError, match="not supported"):
        lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], opt=o, popt=popt)
    log.close(); f["dev"].close()
