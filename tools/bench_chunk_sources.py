"""Chunks from any BAM, measured: ONE set of seeded alignments (a 500 kb chunk at 30x, HiFi shape as tools/bench_f3.py: 10 - 20 kb reads, an event every ~500
bases) written four times -- as an EQX BAM, an 'M' + cs BAM, an 'M' + MD BAM and a plain-'M' BAM -- and each turned into an lcd_chunk_t by
lcd_chunk_create_from_bam_src, which picks the read's digar source as the reference does; beside them lcd_chunk_create_from_bam on the EQX file (the unchanged
entry point).  Per route the median of `repeats` timed calls after one warm-up, the spread of the repeats, and the stage split the library keeps
(lcd_chunk_stage_ms: aux fields, reference comparison, tag download + host parse, digars).  The four chunks must agree read for read.  One JSON line.
usage: python tools/bench_chunk_sources.py [n_reads, default 1000] [repeats, default 7]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT); sys.path.insert(0, os.path.join(_ROOT, "tests"))
from longcalld_amd import align as lcd  # noqa: E402
import bam_src_common as bs  # noqa: E402

SPAN, START, PAD = 500000, 20000, 20000


def make_alignments(n_reads, rng):
    ref = rng.integers(0, 4, START + SPAN + PAD + 20000).astype(np.uint8)
    pos = np.sort(rng.integers(START - 10000, START + SPAN, n_reads))
    qv = np.array([93, 93, 93, 93, 80, 70, 60, 50, 40, 30, 20, 10], np.uint8)
    al = []
    for i in range(n_reads):
        rlen = int(rng.integers(10000, 20000))
        ops, left = [], rlen
        while left > 0:                     # '=' runs of at least 3 bases between single-base events; the read ends in a '=' run
            ln = int(min(left, 2 + rng.geometric(1 / 500.0)))
            if left - ln <= 3:
                ln = left
            ops.append((7, ln, None)); left -= ln
            if left > 0:
                op = int(rng.choice([8, 1, 2], p=[0.5, 0.25, 0.25]))
                ops.append((op, 1, None)); left -= 1 if op != 1 else 0
        a = bs.build_on_ref(rng, ref, int(pos[i]), ops)
        a["qual"] = qv[np.minimum(rng.geometric(0.45, a["qlen"]) - 1, len(qv) - 1)]; a["flag"] = 0; a["name"] = b"m64011_190830_220126/%d/ccs" % i
        al.append(a)
    return ref, al


def measure(n=1000, reps=7, tmp=None):
    tmp = tmp or tempfile.mkdtemp(prefix="chunk_src_")
    rng = np.random.default_rng(3)
    ref, al = make_alignments(n, rng)
    tlen = len(ref)
    nm = ("NM", "i", 3)
    kinds = dict(eqx=lambda a: (a["eqx"], [nm]), cs=lambda a: (a["mcig"], [nm, ("cs", "Z", a["cs"])]), md=lambda a: (a["mcig"], [nm, ("MD", "Z", a["md"])]), ref=lambda a: (a["mcig"], [nm]))
    paths = {}
    for k, f in kinds.items():
        paths[k] = os.path.join(tmp, f"chunk_src_{k}.bam")
        bs.write_bam(paths[k], [bs.record(a, *f(a)) for a in al], block=65280, tlen=tlen)
    beg, end = START, START + SPAN
    src = (ref, 1, tlen, 0)
    res = dict(reads_in_file=n, repeats=reps, file_mb={k: round(os.path.getsize(p) / 2**20, 1) for k, p in paths.items()})
    routes = [("old_entry_eqx", "eqx", None)] + [(k, k, src) for k in kinds]
    times = {r[0]: [] for r in routes}; stages = {r[0]: [] for r in routes}
    info = {}
    for rep in range(reps + 1):
        for name, k, s in routes:
            t0 = time.perf_counter()
            ch = lcd.DeviceChunk.from_bam(paths[k], paths[k] + ".bai", bs.CONTIG, beg, end, min_mapq=30, src=s)
            t1 = time.perf_counter()
            if rep:
                times[name].append((t1 - t0) * 1e3); stages[name].append(ch.stage_ms())
            else:
                info[name] = (ch.read_info(), ch.sources())
            ch.close()
    base = info["old_entry_eqx"][0]
    res["reads_in_region"] = int(len(base["status"]))
    res["chunks_agree"] = bool(all(all((info[r][0][k] == base[k]).all() for k in base) for r in times))
    res["sources"] = {r: np.bincount(info[r][1]["source"], minlength=4).tolist() for r in times}
    res["tag_mb_d2h"] = {r: round(info[r][1]["tag_bytes_d2h"] / 2**20, 2) for r in times}
    med = lambda v: sorted(v)[len(v) // 2]
    res["ms"] = {r: round(med(v), 2) for r, v in times.items()}
    res["ms_min_max"] = {r: [round(min(v), 2), round(max(v), 2)] for r, v in times.items()}
    res["stage_ms"] = {r: [round(med([s[j] for s in v]), 2) for j in range(4)] for r, v in stages.items() if r != "old_entry_eqx"}
    res["stage_names"] = ["aux", "refcmp", "tag_d2h_parse", "digars"]
    res["ratio_to_eqx_route"] = {r: round(res["ms"][r] / res["ms"]["eqx"], 2) for r in times}
    return res


if __name__ == "__main__":
    print(json.dumps(measure(int(sys.argv[1]) if len(sys.argv) > 1 else 1000, int(sys.argv[2]) if len(sys.argv) > 2 else 7)))
