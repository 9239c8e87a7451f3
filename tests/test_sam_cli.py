"""The command line of the SAM text output (no GPU): --sam FILE is parsed and listed, the reference's -S / --out-sam stay refused with a line that names --sam,
--sam with -b and --sam - with the VCF on stdout are refused with status 2 and one line, before the library is imported."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def one_refusal(r):
    return r.returncode == 2 and r.stdout == "" and len(r.stderr.strip().splitlines()) == 1


def test_help_lists_sam():
    r = cli("--help")
    assert r.returncode == 0 and "--sam FILE" in r.stdout and "-S (use --sam)" in r.stdout and "--sam gets no index" in r.stdout


@pytest.mark.parametrize("args", [["-S", "out.sam"], ["--out-sam", "out.sam"], ["--out-sam=out.sam"]], ids=lambda a: a[0])
def test_the_reference_s_spellings_stay_refused_and_name_the_new_one(args):
    r = cli("call", *args, "ref.fa", "in.bam")
    assert one_refusal(r) and "not supported" in r.stderr and "--sam FILE" in r.stderr


def test_the_cram_refusal_names_both_outputs():
    r = cli("call", "-C", "out.cram", "ref.fa", "in.bam")
    assert one_refusal(r) and "not supported" in r.stderr and "-b or --sam" in r.stderr


@pytest.mark.parametrize("args", [["--sam", "o.sam", "-b", "o.bam"], ["-b", "o.bam", "--sam=o.sam"], ["--out-bam", "o.bam", "--sam", "-"]], ids=lambda a: " ".join(a))
def test_sam_with_b_is_refused(args):
    r = cli("call", *args, "-o", "o.vcf", "ref.fa", "in.bam")
    assert one_refusal(r) and "--sam" in r.stderr and "-b" in r.stderr


@pytest.mark.parametrize("args", [["--sam", "-"], ["--sam=-", "-o", "-"], ["--sam", "-", "--out-vcf=-"]], ids=lambda a: " ".join(a))
def test_sam_on_stdout_needs_the_vcf_in_a_file(args):
    r = cli("call", *args, "ref.fa", "in.bam")
    assert one_refusal(r) and "stdout" in r.stderr


def test_both_refusals_come_before_the_library_is_imported(tmp_path):
    """a child process whose longcalld_amd.align cannot be imported still gets the one line and status 2"""
    code = ("import sys, importlib.abc\n"
            "class Block(importlib.abc.MetaPathFinder):\n"
            "    def find_spec(self, name, path, target=None):\n"
            "        if name == 'longcalld_amd.align': raise ImportError('the library is imported')\n"
            "sys.meta_path.insert(0, Block())\n"
            "from longcalld_amd import cli\n"
            "sys.exit(cli.main(sys.argv[1:]))\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["call", "--sam", "-", "ref.fa", "in.bam"], ["call", "--sam", "a.sam", "-b", "a.bam", "ref.fa", "in.bam"]):
        r = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=env, cwd=ROOT)
        assert one_refusal(r), r.stderr


def test_sam_is_parsed_and_the_run_fails_on_the_input(tmp_path):
    """--sam FILE with -o FILE, --refine-bam, --sort-merged and --make-index is accepted: the run gets as far as the missing input"""
    r = cli("call", "--sam", str(tmp_path / "o.sam"), "-o", str(tmp_path / "o.vcf"), "--refine-bam", "--sort-merged", str(tmp_path / "missing_ref.fa"), str(tmp_path / "missing_in.bam"))
    assert r.returncode == 1 and "not supported" not in r.stderr and "missing_in.bam" in r.stderr and not os.path.exists(str(tmp_path / "o.sam"))
