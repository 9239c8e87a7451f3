"""Measurement of the .bai builder (no threshold): per-stage times of lcd_bai_build on a seeded HiFi-shape BAM for slab_members at the default and at two smaller
values, the records per second of the serial record walk on its own, and the existing host path over the same file (lcd_bam_load_region across each contig with
its host-thread inflate) as the comparison.  One JSON line.

    python tools/bench_bai.py [--mb 256] [--threads 16] [--out DIR]

Every GPU step runs in a child process of its own under its own time limit; the parent never opens the device."""
import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS = [("chr1", 120000000), ("chr2", 120000000), ("chr3", 120000000)]


def member(payload, level=1):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


def make_bam(path, mb, seed=1):
    """HiFi shape: ~20 kb reads (=/X/I/D CIGARs of a few hundred operations, 4-bit bases, qualities), 30x-like spacing, three contigs"""
    rng = np.random.default_rng(seed)
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n"
    d = bytearray(b"BAM\x01" + struct.pack("<i", len(hdr)) + hdr + struct.pack("<i", len(CONTIGS)))
    for nm, ln in CONTIGS:
        d += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    pool = []
    for _ in range(32):                                      # record bodies behind the fixed fields
        qlen = int(rng.integers(12000, 28000))
        ops, left = [], qlen
        while left > 0:
            ln = int(min(left, rng.integers(20, 400))); ops.append((ln << 4) | 7); left -= ln
            if left > 0:
                op = int(rng.choice([8, 1, 2])); k = int(rng.integers(1, 4))
                if op != 2:
                    k = min(k, left); left -= k
                ops.append((k << 4) | op)
        cig = np.array(ops, "<u4")
        rl = int(sum(c >> 4 for c in ops if (c & 15) in (2, 7, 8)))
        pool.append((qlen, rl, cig.tobytes() + rng.integers(0, 256, (qlen + 1) // 2).astype(np.uint8).tobytes() + rng.integers(20, 60, qlen).astype(np.uint8).tobytes(), len(cig)))
    target, n, per = mb << 20, 0, None
    per = target // len(CONTIGS)
    with open(path, "wb") as f:
        for tid, (_nm, ln) in enumerate(CONTIGS):
            pos, done = 1000, 0
            while done < per and pos < ln - 40000:
                qlen, rl, tail, nc = pool[n % len(pool)]
                name = f"m64011_{n}/ccs".encode() + b"\0"
                body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), 60, 4680, nc, 16 if n & 1 else 0, qlen, -1, -1, 0) + name + tail + b"NMi" + struct.pack("<i", 7)
                d += struct.pack("<i", len(body)) + body
                done += 4 + len(body); n += 1; pos += int(rng.integers(300, 1100))
                while len(d) >= 65280:
                    f.write(member(bytes(d[:65280]))); del d[:65280]
        if d:
            f.write(member(bytes(d)))
        f.write(member(b""))
    return n


def step_build(path, slab_members):
    from longcalld_amd import align
    align.bai_build(path, path + f".warm{slab_members}.bai", slab_members=slab_members)                 # first call: allocations, code upload
    best = None
    for _ in range(3):
        st = align.bai_build(path, path + f".{slab_members}.bai", slab_members=slab_members)
        if best is None or st["ms_wall"] < best["ms_wall"]:
            best = st
    print(json.dumps(best))


def step_host(path, threads):
    from longcalld_amd import _lib, align
    lib = align.load_library()
    lib.lcd_bam_load_region.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(_lib.LcdBamReads)]
    lib.lcd_bam_reads_free.argtypes = [C.POINTER(_lib.LcdBamReads)]
    t0, n = time.perf_counter(), 0
    for nm, ln in CONTIGS:
        r = _lib.LcdBamReads()
        k = lib.lcd_bam_load_region(path.encode(), nm.encode(), 1, ln, 0, threads, C.byref(r))
        assert k >= 0
        n += k
        lib.lcd_bam_reads_free(C.byref(r))
    print(json.dumps(dict(ms=(time.perf_counter() - t0) * 1e3, n_reads=n, threads=threads)))


def child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"step {args} failed with status {r.returncode}: {r.stderr[-600:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--out", default="out")
    ap.add_argument("--step"); ap.add_argument("--path"); ap.add_argument("--slab", type=int, default=0)
    a = ap.parse_args()
    if a.step == "build":
        return step_build(a.path, a.slab)
    if a.step == "host":
        return step_host(a.path, a.threads)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"bench_bai_{a.mb}.bam")
    t0 = time.perf_counter()
    n = make_bam(path, a.mb)
    res = dict(bench="bai", inflated_mb=a.mb, file_mb=round(os.path.getsize(path) / 2 ** 20, 1), n_records=n, make_s=round(time.perf_counter() - t0, 1), build={})
    limit = 120 + a.mb                                       # seconds per GPU step
    for slab in (0, 1024, 256):
        st = child(["--step", "build", "--path", path, "--slab", str(slab)], limit)
        res["build"][str(slab)] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()}
    d = res["build"]["0"]
    res["walk_records_per_s"] = round(d["n_records"] / max(d["ms_walk"], 1e-9) * 1e3)
    res["host_load_region"] = child(["--step", "host", "--path", path, "--threads", str(a.threads)], limit)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
