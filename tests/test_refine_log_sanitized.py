"""C5: the host-only log application (longcalld_amd/csrc/lcd_refine_log.cpp with lcd_update_digars_from_msa1 of lcd_emit.cpp, translation units without a HIP
call) under AddressSanitizer + UBSan: tests/c/refine_log_sanitize.cpp is a stand-alone program with its own main, compiled here by the host compiler and run as a
subprocess over the logs of tests/test_refine_independence.py's chunks; it exits 0 and prints the oracle's final digars.  Nothing loaded into Python is sanitized."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import refine_common as rc
from conftest import ROOT
from test_refine_independence import both_ways


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("san") / "refine_log_sanitize")
    src = os.path.join(ROOT, "longcalld_amd", "csrc")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "refine_log_sanitize.cpp"), os.path.join(src, "lcd_refine_log.cpp"), os.path.join(src, "lcd_emit.cpp"), "-lz", "-o", out],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return out


@pytest.mark.parametrize("name", ["hg002", "seeded7", "seeded8"])
def test_c5_log_application_under_host_sanitizers(lcd, oracle, exe, tmp_path, name):
    import clean_vars_common as cc
    from test_refine_independence import seeded_chunk
    (_, log, _, final), _ = both_ways(lcd, oracle, name)
    ch = cc.events_chunk() if name == "hg002" else seeded_chunk(7 if name == "seeded7" else 8)
    digs = cc.read_digars(ch, oracle)
    w = [struct.pack("<q", len(digs))]
    for d, r in zip(digs, ch["reads"]):
        rows = np.asarray(d["digars"], np.int64).reshape(-1, 5)
        w.append(struct.pack("<qq", len(r["qual"]), len(rows)) + rows.astype("<i8").tobytes())
    w.append(struct.pack("<q", len(log)))
    for e in log:
        t, q = np.asarray(e["target"], np.uint8).tobytes(), np.asarray(e["query"], np.uint8).tobytes()
        w.append(struct.pack("<8q", e["read_id"], e["cover"], e["read_beg"], e["read_end"], e["reg_beg"], e["reg_end"], e["pass_"], len(t)) + t + q)
    path = str(tmp_path / "dump.bin")
    open(path, "wb").write(b"".join(w))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-300:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    _, wrej = rc.apply_log(oracle, [np.asarray(d["digars"]).tolist() for d in digs], [len(r["qual"]) for r in ch["reads"]], log)
    assert lines[0] == "rejected %d" % wrej
    k, touched = 1, {}
    while k < len(lines):
        r, n = map(int, lines[k].split())
        touched[r] = [tuple(map(int, x.split())) for x in lines[k + 1:k + 1 + n]]; k += 1 + n
    assert sorted(touched) == sorted({e["read_id"] for e in log}) and len(touched) > 20
    for r, rows in touched.items():
        assert rows == [tuple(x) for x in final[r]], (name, r)
