"""The command line of the depth track (no GPU): --depth FILE, --depth-window INT and --depth-skip-dels are parsed and listed, and every refusal is one line with
status 2 before the library is imported."""
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
    for w in ("--depth FILE", "--depth-window INT", "--depth-skip-dels", "depth_all depth_h1 depth_h2 depth_unassigned", "bases_all bases_h1 bases_h2 bases_unassigned",
              "as stored in the input", "--refine-bam does not change it", "beside --mods"):
        assert w in r.stdout, w


@pytest.mark.parametrize("args,word", [(["--depth-window", "1000"], "need --depth"), (["--depth-skip-dels"], "need --depth"), (["--depth", "-"], "stdout"), (["--depth="], "stdout"),
                                       (["--depth"], "needs a value"), (["--depth", "d.bed", "--depth-window", "1k"], "not a number"), (["--depth", "d.bed", "--depth-window", "0.5"], "not a number"),
                                       (["--depth", "d.bed", "--depth-window", "-1"], "0 ... 2^30"), (["--depth", "d.bed", "--depth-window", str((1 << 30) + 1)], "0 ... 2^30"),
                                       (["--depth", "same.tsv", "--mods", "same.tsv"], "name one file")],
                         ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_refusals(args, word, tmp_path):
    r = cli("call", "ref.fa", "in.bam", "-o", str(tmp_path / "o.vcf"), *args)
    assert one_refusal(r) and word in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_refusals_come_before_the_library_is_imported():
    code = ("import sys, importlib.abc\n"
            "class Block(importlib.abc.MetaPathFinder):\n"
            "    def find_spec(self, name, path, target=None):\n"
            "        if name == 'longcalld_amd.align': raise ImportError('the library is imported')\n"
            "sys.meta_path.insert(0, Block())\n"
            "from longcalld_amd import cli\n"
            "sys.exit(cli.main(sys.argv[1:]))\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["call", "--depth-skip-dels", "ref.fa", "in.bam"], ["call", "--depth", "-", "ref.fa", "in.bam"], ["call", "--depth", "d", "--depth-window", "x", "ref.fa", "in.bam"]):
        r = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=env, cwd=ROOT)
        assert one_refusal(r), r.stderr


def test_parsing():
    from longcalld_amd import cli as c
    o, pos = c.parse(["--depth", "d.bed", "--depth-window=5000", "--depth-skip-dels", "ref.fa", "in.bam"])
    assert pos == ["ref.fa", "in.bam"] and c.depth_option(o) == dict(path="d.bed", window=5000, skip_dels=True)
    o, _ = c.parse(["--depth=d.bed", "ref.fa", "in.bam"])
    assert c.depth_option(o) == dict(path="d.bed", window=0, skip_dels=False)
    o, _ = c.parse(["--depth", "d.bed", "--depth-window", str(1 << 30), "--mods", "t.tsv", "ref.fa", "in.bam"])
    assert c.depth_option(o) == dict(path="d.bed", window=1 << 30, skip_dels=False) and c.mods_option(o)["path"] == "t.tsv"
    o, _ = c.parse(["ref.fa", "in.bam"])
    assert c.depth_option(o) is None


def test_the_options_are_accepted_and_the_run_fails_on_the_input(tmp_path):
    r = cli("call", "--depth", str(tmp_path / "d.bed"), "--depth-window", "1000", "--depth-skip-dels", "--mods", str(tmp_path / "t.tsv"), "-o", str(tmp_path / "o.vcf"),
            str(tmp_path / "missing_ref.fa"), str(tmp_path / "missing_in.bam"))
    assert r.returncode == 1 and "not supported" not in r.stderr and "missing_in.bam" in r.stderr and not os.path.exists(str(tmp_path / "d.bed"))
