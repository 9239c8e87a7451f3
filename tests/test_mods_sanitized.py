"""The methylation table's formatter, strand combination and option check (longcalld_amd/csrc/lcd_mods_format.cpp, a translation unit without a HIP call) under
AddressSanitizer + UBSan: tests/c/mods_sanitize.cpp is a stand-alone program, compiled here together with that file by the host compiler and run on the CPU over the
rows of the case table; what it prints must be the oracle's text."""
import os
import shutil
import subprocess

import mods_common as mc
from conftest import ROOT


def test_formatter_and_combination_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (the project's own build needs one)"
    exe = str(tmp_path / "mods_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "mods_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_mods_format.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    t = mc.build_cases()
    rows, _ = mc.pileup(t["bodies"], t["ref"], 1, t["reg_beg"], t["reg_end"], t["haps"])
    path = str(tmp_path / "rows.txt")
    with open(path, "w") as f:
        for p, s, v in rows:
            f.write(f"{p} {s} " + " ".join(str(x) for x in v) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    text, rest = run.stdout.split("--combined--\n")
    comb, tail = rest.split("--end--\n")
    assert text == mc.HEADER + mc.format_rows(rows, "chrS") and comb == mc.format_rows(mc.combine_rows(rows), "chrS")
    assert tail.split()[1:] == ["checks", "ok"] and int(tail.split()[0]) >= 20
