"""longcalld_amd/csrc/sam_fmt.h on the CPU: tests/c/sam_float_check.cpp (a program of its own that includes the header the kernel includes) built with
-fsanitize=address,undefined and run.  It compares fmt_g with snprintf("%g") on every 1021st bit pattern, the 1024 lowest and highest mantissas of every sign and
exponent, the floats within 3 ulps of d * 10^k (d in 1, 9.999994, 9.999995, 9.999996; k = -45 ... 38), and the integer formatters on each side of every digit-count
step.  The sweep of all 2^32 patterns is run by hand (`sam_float_check full`); its result stands in profiles/NOTES_sam_out.md."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fmt_g_equals_printf_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/c/sam_float_check.cpp"
    exe = str(tmp_path / "sam_float_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "longcalld_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "sam_float_check.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n, d = r.stdout.split()[0], r.stdout.split()[2]
    assert int(n) > 5000000 and int(d) == 0, r.stdout
