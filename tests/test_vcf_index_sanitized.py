"""The finisher of the VCF indexes (longcalld_amd/csrc/lcd_index_host.cpp, a translation unit without a HIP call) under AddressSanitizer + UBSan:
tests/c/vcf_index_sanitize.cpp is a stand-alone program with its own main, compiled here together with that file by the host compiler and run on the CPU as a child
process.  It compares lcd_tbx_from_records with a second, naive implementation on zero records and one, an end of exactly 2^29 and of 2^29 + 1, depth-6 CSI bins and
10^5 seeded records."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_finisher_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "vcf_index_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "vcf_index_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_index_host.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert run.stdout.split()[1:] == ["checks", "ok"] and int(run.stdout.split()[0]) >= 25
