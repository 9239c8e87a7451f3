"""The TE file reader and the formatter with read names (longcalld_amd/csrc/lcd_emit.cpp, a translation unit without a HIP call) under AddressSanitizer + UBSan on
their corner cases: tests/c/vcf_fields_sanitize.cpp is a stand-alone program, compiled here together with that file by the host compiler and run on the CPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_reader_and_formatter_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "vcf_fields_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "vcf_fields_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_emit.cpp"), "-lz", "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert run.stdout.split()[1:] == ["checks", "ok"] and int(run.stdout.split()[0]) >= 20
