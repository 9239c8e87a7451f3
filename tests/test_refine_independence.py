"""C2, the premise of the refined-alignment design, on the CPU: calling never needs to see refined digars.  The rounds loop composed from the oracles
(refine_common.oracle_rounds_log, ref<->read strings on) runs twice per chunk -- read slices cut from the ORIGINAL digars (what the device does) and from the digars
refined SO FAR (what the reference does) -- on the bundled HG002 chunk and on two seeded bam_src_common chunks.  Every region's (cover, read_beg, read_end, slice
bases) of every read, the logs and the final digars must be equal.  The inputs must exercise the premise: the oracle's own log has to show a read with two resolved
regions and a left- or right-cover read in a resolved cluster before anything is compared."""
import numpy as np
import pytest

import bam_src_common as bs
import call_chunks_common as kc
import clean_vars_common as cc
import refine_common as rc

RIGHT_COVER, LEFT_COVER, BOTH_COVER = 4, 8, 12        # the cover flag of collect_noisy_read_info (src/align.c: LONGCALLD_NOISY_LEFT_COVER / RIGHT_COVER)
_state = {}


def seeded_chunk(seed):
    ref, al = bs.seeded(seed, 60)
    reads = []
    for a in al:
        pk = np.asarray(a["bseq"], np.uint8)
        nib = np.stack([pk >> 4, pk & 15], 1).reshape(-1)[:a["qlen"]]
        lut = np.full(16, 4, np.uint8); lut[[1, 2, 4, 8]] = [0, 1, 2, 3]
        reads.append(dict(pos0=a["pos0"], cigar=a["eqx"], seq=lut[nib], qual=a["qual"], bseq=a["bseq"], is_rev=1 if a["flag"] & 16 else 0))
    return dict(reads=reads, ref=ref, ref_beg=1, reg_beg=1, reg_end=bs.TLEN, whole_ref_len=bs.TLEN, is_ont=0)


def both_ways(lcd, oracle, name):
    if name not in _state:
        ch, max_len = (cc.events_chunk(), 3000) if name == "hg002" else (seeded_chunk(7 if name == "seeded7" else 8), 50000)
        digs = cc.read_digars(ch, oracle)
        ordered = np.arange(len(ch["reads"]), dtype=np.int32)
        first = kc.first_round_chain(lcd, oracle, ch, digs, ordered)
        args = (oracle, ch, digs, first["cv"], first["state"], ordered, first["is_skipped"])
        _state[name] = (rc.oracle_rounds_log(*args, max_len=max_len), rc.oracle_rounds_log(*args, max_len=max_len, slices_from_refined=True))
    return _state[name]


def counts(log):
    regions_of = {}
    for e in log:
        regions_of.setdefault(e["read_id"], set()).add(e["reg_beg"])
    return sum(1 for v in regions_of.values() if len(v) >= 2), sum(1 for e in log if e["cover"] in (LEFT_COVER, RIGHT_COVER))


def test_c2_the_inputs_exercise_the_premise(lcd, oracle):
    tot = np.zeros(2, np.int64)
    for name in ("hg002", "seeded7", "seeded8"):
        (_, log, _, _), _ = both_ways(lcd, oracle, name)
        n_two, n_part = counts(log)
        print(name, "entries", len(log), "reads with two resolved regions", n_two, "left / right cover entries", n_part)
        assert n_two >= 1 and n_part >= 1, name
        tot += (n_two, n_part)
    assert tot[0] >= 1 and tot[1] >= 1, tot


@pytest.mark.parametrize("name", ["hg002", "seeded7", "seeded8"])
def test_c2_slices_logs_and_final_digars_do_not_depend_on_the_rewrite(lcd, oracle, name):
    (want, log, slices, final), (want2, log2, slices2, final2) = both_ways(lcd, oracle, name)
    assert len(log) > 0
    assert len(slices) == len(slices2)
    for a, b in zip(slices, slices2):
        assert a == b, (a[:5], b[:5])
    assert len(log) == len(log2)
    for a, b in zip(log, log2):
        assert {k: a[k] for k in a if k not in ("target", "query")} == {k: b[k] for k in b if k not in ("target", "query")}
        assert np.asarray(a["target"]).tobytes() == np.asarray(b["target"]).tobytes() and np.asarray(a["query"]).tobytes() == np.asarray(b["query"]).tobytes()
    assert final == final2
    assert want["n_passes"] == want2["n_passes"] and want["done"].tolist() == want2["done"].tolist() and want["cv"]["n_vars"] == want2["cv"]["n_vars"]
