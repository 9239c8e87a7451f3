"""The phased-VCF reader (longcalld_amd/csrc/lcd_phased_vcf.cpp, a translation unit without a HIP call) under AddressSanitizer + UBSan: tests/c/haplotag_vcf_sanitize.cpp
is a stand-alone program with its own main, compiled here together with that file by the host compiler and run on the CPU over crafted inputs -- truncated lines,
empty fields, 10 kb alleles, a gzip member cut short, no trailing newline; what it prints must be the Python reader's dump, an error where the Python reader raises
one, with the same code.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import haplotag_common as hc
from conftest import ROOT


def test_reader_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (the project's own build needs one)"
    exe = str(tmp_path / "haplotag_vcf_sanitize")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "haplotag_vcf_sanitize.cpp"), os.path.join(ROOT, "longcalld_amd", "csrc", "lcd_phased_vcf.cpp"), "-lz", "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    files = hc.crafted_files()
    t = hc.build_cases()
    files.append(("case_table", t["vcf"].encode(), dict(names=[hc.CONTIG], sample=None, max_indel=50, snvs_only=0)))
    want, lines = [], []
    for name, data, kw in files:
        path = str(tmp_path / (name + ".vcf"))
        open(path, "wb").write(data)
        lines.append(" ".join([path, kw["sample"] or "-", str(kw["max_indel"]), str(kw["snvs_only"])] + kw["names"]) + "\n")
        try:
            want.append(hc.dump(*hc.read_vcf(hc.vcf_bytes(path), kw["names"], kw["sample"], kw["max_indel"], bool(kw["snvs_only"]))))
        except hc.VcfError as e:
            want.append("error %d\n" % e.code)
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("".join(lines))
    run = subprocess.run([exe, lst], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    got = run.stdout.split("--end--\n")
    assert got[-1] == "%d files ok\n" % len(files)
    assert len(got) == len(files) + 1
    for (name, _, _), g, w in zip(files, got, want):
        assert g == w, name
    n_err = sum(w.startswith("error") for w in want)
    assert 7 <= n_err < len(files) - 10                          # both kinds of ending are exercised
    assert want[[f[0] for f in files].index("gzip_cut_short")] == "error -30\n"
