"""Measurement of the VCF index (no threshold).  About 10^6 seeded VCF lines are written through the project's own writer (-O z); then
  * lcd_vcf_index_build on that file: ms_read, ms_inflate, ms_lines, ms_entry, ms_finish, ms_wall (median of the repeats after a warm-up call), at the default slab
    and at a smaller one;
  * the writer on the same appends without and with the index: wall-clock per file, median of the repeats, and their ratio.
One JSON line.  The stage times are wall-clock around each stage's launches, copies and synchronisations (what the stats structs carry), not kernel-only HIP-event
times: a stage here is a handful of short kernels with host decisions between them.

    python tools/bench_vcf_index.py [--lines 1000000] [--append 20000] [--repeats 5] [--out DIR]

Every GPU step runs in a child process of its own under its own time limit; the parent never opens the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS = [(f"chr{k}", 240000000 - 9000000 * k) for k in range(1, 23)]
HEADER = "##fileformat=VCFv4.2\n" + "".join(f"##contig=<ID={n},length={ln}>\n" for n, ln in CONTIGS) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n"


def make_text(path, n_lines, seed=1):
    """the body lines, in order: SNVs and short indels of the usual 100 - 300 bytes, now and then a deletion with END= and an insertion with a few kilobytes of ALT"""
    rng = np.random.default_rng(seed)
    per = n_lines // len(CONTIGS)
    with open(path, "w") as f:
        for name, ln in CONTIGS:
            pos = np.sort(rng.integers(1, ln - 200000, per))
            kind = rng.random(per)
            dp = rng.integers(10, 60, per)
            out = []
            for p, k, d in zip(pos.tolist(), kind.tolist(), dp.tolist()):
                if k < 0.9:
                    out.append(f"{name}\t{p}\t.\tA\tG\t{d}\tPASS\tDP={d};AF=0.5;CLEAN\tGT:PS:DP:AD\t0|1:{p}:{d}:{d // 2},{d - d // 2}\n")
                elif k < 0.97:
                    out.append(f"{name}\t{p}\t.\t{'ACGTTGCA' * (1 + d % 6)}\tA\t{d}\tPASS\tDP={d};SVTYPE=DEL;CIEND=0,3\tGT:PS:DP\t1|0:{p}:{d}\n")
                elif k < 0.995:
                    out.append(f"{name}\t{p}\t.\tN\t<DEL>\t{d}\tPASS\tSVTYPE=DEL;SVLEN=-{d * 900};END={p + d * 900}\tGT\t0/1\n")
                else:
                    out.append(f"{name}\t{p}\t.\tG\tG{'ACGT' * (d * 20)}\t{d}\tPASS\tSVTYPE=INS;END={p}\tGT:ALTREADS\t0/1:{'m64011/1234/ccs,' * d}\n")
            f.write("".join(out))
    return per * len(CONTIGS)


def appends_of(path, n_append):
    lines = open(path).readlines()
    return ["".join(lines[k:k + n_append]) for k in range(0, len(lines), n_append)]


def step_write(text_path, out_path, n_append, repeats, index):
    from longcalld_amd import align
    texts = appends_of(text_path, n_append)
    ms, st = [], None
    for r in range(repeats + 1):                              # the first call warms up: allocations, code upload
        t0 = time.perf_counter()
        st = align.vcf_write(out_path, texts, bgzf=1, header_text=HEADER, index=index)
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(ms_median=statistics.median(ms[1:]), ms_all=[round(x, 1) for x in ms[1:]], n_appends=len(texts), index_stats=st)))


def step_build(path, slab, repeats, fmt):
    from longcalld_amd import align
    align.vcf_index_build(path, path + ".warm", fmt=fmt, slab_members=slab)
    runs = [align.vcf_index_build(path, path + f".{slab}.{fmt}", fmt=fmt, slab_members=slab) for _ in range(repeats)]
    med = {k: statistics.median(r[k] for r in runs) for k in ("ms_read", "ms_inflate", "ms_lines", "ms_entry", "ms_finish", "ms_wall")}
    print(json.dumps(dict(med, **{k: runs[0][k] for k in ("n_lines", "n_data_lines", "n_contigs", "n_chunks", "n_slabs", "n_members", "bytes_in", "bytes_inflated", "bytes_index", "bytes_file")})))


def child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"step {args} failed with status {r.returncode}: {r.stderr[-600:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1000000); ap.add_argument("--append", type=int, default=20000); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="out"); ap.add_argument("--step"); ap.add_argument("--path"); ap.add_argument("--dst"); ap.add_argument("--slab", type=int, default=0)
    ap.add_argument("--index"); ap.add_argument("--fmt", default="tbi")
    a = ap.parse_args()
    if a.step == "write":
        return step_write(a.path, a.dst, a.append, a.repeats, a.index)
    if a.step == "build":
        return step_build(a.path, a.slab, a.repeats, a.fmt)
    os.makedirs(a.out, exist_ok=True)
    text, plain, idxd = (os.path.join(a.out, f"bench_vcf_index_{a.lines}.{s}") for s in ("txt", "plain.vcf.gz", "idx.vcf.gz"))
    t0 = time.perf_counter()
    n = make_text(text, a.lines)
    res = dict(bench="vcf_index", n_lines=n, text_mb=round(os.path.getsize(text) / 2 ** 20, 1), make_s=round(time.perf_counter() - t0, 1))
    limit = 180 + a.lines // 5000
    common = ["--path", text, "--append", str(a.append), "--repeats", str(a.repeats)]
    res["write_plain"] = child(["--step", "write", "--dst", plain] + common, limit)
    res["write_tbi"] = child(["--step", "write", "--dst", idxd, "--index", "tbi"] + common, limit)
    res["write_csi"] = child(["--step", "write", "--dst", idxd, "--index", "csi"] + common, limit)
    res["write_ratio_tbi"] = round(res["write_tbi"]["ms_median"] / res["write_plain"]["ms_median"], 3)
    res["write_ratio_csi"] = round(res["write_csi"]["ms_median"] / res["write_plain"]["ms_median"], 3)
    res["file_mb"] = round(os.path.getsize(plain) / 2 ** 20, 1)
    for slab in (0, 256):
        for fmt in ("tbi", "csi"):
            res[f"build_{fmt}_{slab}"] = child(["--step", "build", "--path", plain, "--slab", str(slab), "--repeats", str(a.repeats), "--fmt", fmt], limit)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
