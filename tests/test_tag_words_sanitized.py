"""The host parsers of the cs / MD digar sources (longcalld_amd/csrc/tag_words.h: cs_to_words, md_to_words) under AddressSanitizer + UBSan on truncated and
garbage tag bytes: tests/c/tag_words_fuzz.cpp is a stand-alone program, compiled here with the host compiler and run on the CPU.  Chunks made from a BAM hand
these parsers whatever bytes a file's cs / MD fields hold."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_tag_parsers_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tag_words_fuzz")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "tag_words_fuzz.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    n, ok = int(run.stdout.split()[0]), int(run.stdout.split()[2])
    assert n > 100000 and 3000 * 2 <= ok < n        # the well-formed cs / MD tags parse; truncated and garbage ones mostly do not
