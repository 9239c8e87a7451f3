"""The command line of the per-haplotype read sets (no GPU): --split-reads PREFIX, --split-gz, --split-comment and --haplotag-list FILE are parsed and listed,
the keyword split= is built from them, and every refusal is one line with status 2 before the library is imported and before anything is created."""
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


def test_help_lists_the_options():
    r = cli("--help")
    assert r.returncode == 0
    for w in ("--split-reads PREFIX", "--split-gz", "--split-comment", "--haplotag-list FILE", "PREFIX.h1.fastq", "PREFIX.none.fastq", "#readname haplotype phaseset chromosome",
              "as it was sequenced", "in the order of the output BAM"):
        assert w in r.stdout, w


@pytest.mark.parametrize("args,word", [(["--split-gz"], "need --split-reads"), (["--split-comment"], "need --split-reads"), (["--haplotag-list", "l.tsv", "--split-gz"], "need --split-reads"),
                                       (["--split-reads", "-"], "stdout"), (["--split-reads="], "stdout"), (["--split-reads"], "needs a value"), (["--haplotag-list", "-"], "stdout"),
                                       (["--haplotag-list="], "stdout"), (["--haplotag-list"], "needs a value"),
                                       (["--split-reads", "p", "--haplotag-list", "p.h1.fastq"], "name one file"),
                                       (["--split-reads", "p", "--split-gz", "--haplotag-list", "p.none.fastq.gz"], "name one file"),
                                       (["--split-reads", "p", "-b", "p.h2.fastq"], "name one file"), (["--split-reads", "p", "--sam", "p.h2.fastq"], "name one file"),
                                       (["--split-reads", "p", "--mods", "p.none.fastq"], "name one file"), (["--split-reads", "p", "--depth", "p.h1.fastq"], "name one file"),
                                       (["--haplotag-list", "same", "--depth", "same"], "name one file"), (["--haplotag-list", "same", "--mods", "same"], "name one file"),
                                       (["--haplotag-list", "same", "-b", "same"], "name one file")],
                         ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_refusals(args, word, tmp_path):
    r = cli("call", "ref.fa", "in.bam", "-o", str(tmp_path / "o.vcf"), *args)
    assert one_refusal(r) and word in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_an_output_equal_to_the_vcf_is_refused(tmp_path):
    for args in (["--split-reads", "p", "-o", "p.h1.fastq"], ["--haplotag-list", "x.tsv", "-o", "x.tsv"]):
        r = cli("call", "ref.fa", "in.bam", *args)
        assert one_refusal(r) and "name one file" in r.stderr, r.stderr


def test_the_refusals_come_before_the_library_is_imported():
    code = ("import sys, importlib.abc\n"
            "class Block(importlib.abc.MetaPathFinder):\n"
            "    def find_spec(self, name, path, target=None):\n"
            "        if name == 'longcalld_amd.align': raise ImportError('the library is imported')\n"
            "sys.meta_path.insert(0, Block())\n"
            "from longcalld_amd import cli\n"
            "sys.exit(cli.main(sys.argv[1:]))\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["call", "--split-gz", "ref.fa", "in.bam"], ["call", "--split-reads", "-", "ref.fa", "in.bam"], ["call", "--split-reads", "p", "--haplotag-list", "p.h1.fastq", "ref.fa", "in.bam"]):
        r = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=env, cwd=ROOT)
        assert one_refusal(r), r.stderr


def test_parsing_and_the_keyword():
    from longcalld_amd import cli as c
    o, pos = c.parse(["--split-reads", "out/p", "--split-gz", "--split-comment", "--haplotag-list=l.tsv", "ref.fa", "in.bam"])
    assert pos == ["ref.fa", "in.bam"] and c.split_option(o) == dict(prefix="out/p", gz=True, comment=True, haplotag_list="l.tsv")
    o, _ = c.parse(["--split-reads=p", "ref.fa", "in.bam"])
    assert c.split_option(o) == dict(prefix="p", gz=False, comment=False, haplotag_list=None)
    o, _ = c.parse(["--haplotag-list", "l.tsv", "ref.fa", "in.bam"])
    assert c.split_option(o) == dict(prefix=None, gz=False, comment=False, haplotag_list="l.tsv")
    o, _ = c.parse(["--split-reads", "p", "--depth", "d.bed", "--mods", "t.tsv", "-b", "o.bam", "-o", "-", "ref.fa", "in.bam"])
    assert c.split_option(o)["prefix"] == "p" and c.depth_option(o)["path"] == "d.bed" and c.mods_option(o)["path"] == "t.tsv"
    o, _ = c.parse(["--split-reads", "p", "--haplotag-list", "p.h1.fastq.gz", "ref.fa", "in.bam"])       # (without --split-gz that is another file)
    assert c.split_option(o)["haplotag_list"] == "p.h1.fastq.gz"
    o, _ = c.parse(["ref.fa", "in.bam"])
    assert c.split_option(o) is None
    assert {"--split-gz", "--split-comment"} <= c.FLAGS and c.VALUED["--split-reads"] == "split_reads" and c.VALUED["--haplotag-list"] == "haplotag_list"


def test_the_options_are_accepted_and_the_run_fails_on_the_input(tmp_path):
    r = cli("call", "--split-reads", str(tmp_path / "p"), "--split-gz", "--split-comment", "--haplotag-list", str(tmp_path / "l.tsv"), "--depth", str(tmp_path / "d.bed"),
            "-o", str(tmp_path / "o.vcf"), str(tmp_path / "missing_ref.fa"), str(tmp_path / "missing_in.bam"))
    assert r.returncode == 1 and "not supported" not in r.stderr and "missing_in.bam" in r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if "fastq" in f or f == "l.tsv"]
