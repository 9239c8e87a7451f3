"""The read sets' prefix sums, paths and option check (longcalld_amd/csrc/lcd_split_format.cpp, a translation unit without a HIP call) under AddressSanitizer +
UBSan: tests/c/split_sanitize.cpp is a stand-alone program with its own main, compiled here together with that file by the host compiler and run on the CPU over
the case table's rows, seeded rows and lengths near 2^64; what it prints must be the Python rules' numbers.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np

import split_common as sc
from conftest import ROOT


def _rows_of(table, haps, pss, comment, with_list):
    """the measure pass's rows of a record table, from the oracle: (stream, entry length, line length)"""
    rows = []
    for body, r in table:
        fq, lst, st = sc.split_text([(body, 0 if r >= 0 else -1)], [haps[r] if r >= 0 else 0], [pss[r] if r >= 0 else 0], names=[sc.CONTIG] if with_list else None, comment=comment)
        s = -1 if not st["n_selected"] else st["n_hap"].index(1)
        rows.append((s, sum(len(f) for f in fq), len(lst)))
    return rows


def _tables():
    t = sc.build_cases()
    out = [_rows_of(t["table"], t["haps"], t["phase_sets"], c, l) for c in (False, True) for l in (False, True)]
    for seed in range(12):
        recs, rb, re_ = sc.seeded_chunk(seed, n_rec=30)
        x = sc.table_of(recs, rb, re_)
        out.append(_rows_of(x["table"], x["haps"], x["phase_sets"], seed % 2 == 0, seed % 3 != 0))
    rng = np.random.default_rng(1)
    out.append([(int(rng.integers(-1, 3)), int(rng.integers(0, 1 << 50)), int(rng.integers(0, 1 << 20))) for _ in range(4000)])
    out.append([(0, (1 << 63) - 1, 1 << 62), (0, 1 << 63, 1 << 62), (-1, (1 << 64) - 1, (1 << 64) - 1), (1, (1 << 64) - 1, (1 << 63) - 1), (2, 0, 0)])
    out.append([(-1, 5, 5)] * 3)
    out.append([])
    return out


def test_offsets_and_paths_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (the project's own build needs one)"
    exe = str(tmp_path / "split_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "split_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_split_format.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    tables = _tables()
    path = str(tmp_path / "tables.txt")
    with open(path, "w") as f:
        for rows in tables:
            f.write("T\n" + "".join(f"{s} {a} {b}\n" for s, a, b in rows))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    body, tail = run.stdout.split("--end--\n")
    got = body.split("--table--\n")
    assert len(got) == len(tables) > 15
    for text, rows in zip(got, tables):
        fo, lo, tot = sc.offsets([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
        assert text == "".join(f"{a} {b}\n" for a, b in zip(fo, lo)) + "= %d %d %d %d\n" % tuple(tot)
    lines = tail.splitlines()
    assert lines[:12] == [p for pre in ("p", "dir.with.dots/x") for gz in (False, True) for p in sc.paths(pre, gz)]
    assert lines[-1].split()[1:] == ["checks", "ok"] and int(lines[-1].split()[0]) >= 100
