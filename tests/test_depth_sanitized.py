"""The depth track's window rule, formatter and option check (longcalld_amd/csrc/lcd_depth_format.cpp, a translation unit without a HIP call) under AddressSanitizer +
UBSan: tests/c/depth_sanitize.cpp is a stand-alone program with its own main, compiled here together with that file by the host compiler and run on the CPU over the
case table's rows, seeded rows, windows that cut rows and sums near 2^63; what it prints must be the Python rules' text.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import depth_common as dc
from conftest import ROOT


def _tables():
    t = dc.build_cases()
    out = []
    for sd in (False, True):
        rows, _ = dc.depth_rows(t["bodies"], t["reg_beg"], t["reg_end"], t["haps"], skip_dels=sd)
        out += [(W, rows) for W in (1, 7, 1000, 1 << 30)]
    for seed in range(20):
        recs, rb, re_ = dc.seeded_chunk(seed)
        rows, _ = dc.depth_rows([r["body"] for r in recs], rb, re_, dc.haps_of(recs, rb, re_))
        out.append((1 + 5 * seed, rows))
    # windows that cut long rows many times; the widest depths over spans whose sums come near 2^63
    out.append((3, [(2, 40, (1, 2, 3)), (41, 41, (0, 0, 0)), (42, 100, (7, 0, 9))]))
    out.append((1 << 30, [(1, 1 << 31, (0xffffffff, 0xfffffffe, 1)), ((1 << 31) + 1, (1 << 31) + 5, (0, 0xffffffff, 0))]))
    out.append((1 << 29, [((1 << 40) - 3, (1 << 40) + (1 << 30), (0xffffffff, 1, 0xffffffff))]))
    return out


def test_windows_and_formatter_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (the project's own build needs one)"
    exe = str(tmp_path / "depth_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "depth_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_depth_format.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    tables = _tables()
    path = str(tmp_path / "tables.txt")
    with open(path, "w") as f:
        for W, rows in tables:
            f.write(f"T {W}\n" + "".join(f"{b} {e} {d[0]} {d[1]} {d[2]}\n" for b, e, d in rows))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    body, tail = run.stdout.split("--end--\n")
    got = body.split("--table--\n")
    assert len(got) == len(tables) > 20
    for text, (W, rows) in zip(got, tables):
        base, win = text.split("--windows--\n")
        assert base == dc.HEADER + dc.format_rows(rows, "chrS"), W
        assert win == dc.HEADER_W + dc.format_rows(dc.windows(rows, W), "chrS"), W
    assert tail.split()[1:] == ["checks", "ok"] and int(tail.split()[0]) >= 100
