"""The command line of the methylation table (no GPU): --mods FILE and its --mod-* options are parsed and listed, the reference's -m / --methylation are refused
with a line that names --mods FILE, and every refusal is one line with status 2 before the library is imported."""
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
    for w in ("--mods FILE", "--mod-code m|h", "--mod-threshold INT", "--mod-combine-strands", "-m/--methylation (use --mods FILE)", "n_all mod_all n_h1 mod_h1 n_h2 mod_h2 n_filtered"):
        assert w in r.stdout, w


@pytest.mark.parametrize("args", [["-m"], ["--methylation"]], ids=lambda a: a[0])
def test_the_reference_s_spelling_is_refused_and_names_the_new_one(args):
    r = cli("call", *args, "ref.fa", "in.bam")
    assert one_refusal(r) and "not supported" in r.stderr and "--mods FILE" in r.stderr


@pytest.mark.parametrize("args,word", [(["--mod-code", "h"], "need --mods"), (["--mod-threshold=200"], "need --mods"), (["--mod-combine-strands"], "need --mods"),
                                       (["--mods", "t.tsv", "--mod-code", "a"], "m or h"), (["--mods", "t.tsv", "--mod-code", "mh"], "m or h"),
                                       (["--mods", "t.tsv", "--mod-threshold", "127"], "128 ... 255"), (["--mods", "t.tsv", "--mod-threshold", "256"], "128 ... 255"),
                                       (["--mods", "t.tsv", "--mod-threshold", "0.8"], "not a number"), (["--mods", "-"], "stdout"), (["--mods="], "stdout"), (["--mods"], "needs a value")],
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
    for args in (["call", "-m", "ref.fa", "in.bam"], ["call", "--mod-code", "h", "ref.fa", "in.bam"], ["call", "--mods", "t", "--mod-threshold", "9", "ref.fa", "in.bam"]):
        r = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=env, cwd=ROOT)
        assert one_refusal(r), r.stderr


def test_parsing():
    from longcalld_amd import cli as c
    o, pos = c.parse(["--mods", "t.tsv", "--mod-code=h", "--mod-threshold", "230", "--mod-combine-strands", "ref.fa", "in.bam"])
    assert pos == ["ref.fa", "in.bam"] and c.mods_option(o) == dict(path="t.tsv", code="h", threshold=230, combine_strands=True)
    o, _ = c.parse(["--mods=t.tsv", "ref.fa", "in.bam"])
    assert c.mods_option(o) == dict(path="t.tsv", code="m", threshold=204, combine_strands=False)
    o, _ = c.parse(["ref.fa", "in.bam"])
    assert c.mods_option(o) is None


def test_the_options_are_accepted_and_the_run_fails_on_the_input(tmp_path):
    r = cli("call", "--mods", str(tmp_path / "t.tsv"), "--mod-code", "h", "--mod-threshold", "128", "--mod-combine-strands", "-o", str(tmp_path / "o.vcf"),
            str(tmp_path / "missing_ref.fa"), str(tmp_path / "missing_in.bam"))
    assert r.returncode == 1 and "not supported" not in r.stderr and "missing_in.bam" in r.stderr and not os.path.exists(str(tmp_path / "t.tsv"))
