"""python -m longcalld_amd.cli haplotag: the parser's refusals (one line, status 2, before the library is loaded or an input is looked at), its own options, and
what `call` still refuses and accepts (no GPU needed)."""
import pytest

from longcalld_amd import cli

BASE = ["haplotag", "ref.fa", "in.bam", "phased.vcf.gz"]


def _run(capsys, argv):
    rc = cli.main(argv)
    out = capsys.readouterr()
    return rc, out.out, out.err


@pytest.mark.parametrize("extra,word", [
    (["-o", "x.vcf"], "-o"), (["--out-vcf=x.vcf"], "--out-vcf"), (["-O", "z"], "-O"), (["--vcf-index", "tbi"], "--vcf-index"), (["--refine-bam"], "--refine-bam"),
    (["--te-lib", "te.fa"], "--te-lib"), (["--var-rnames"], "--var-rnames"), (["--sv-rnames"], "--sv-rnames"), (["-c", "3"], "-c"), (["-d", "2"], "-d"), (["-a", "0.2"], "-a"),
    (["-C", "50"], "-C"), (["-l", "30"], "-l"), (["--min-cov", "3"], "--min-cov"), (["-n", "S"], "-n"), (["-H"], "-H"), (["--amb-base"], "--amb-base")])
def test_call_only_options_are_refused(capsys, extra, word):
    rc, out, err = _run(capsys, BASE + ["-b", "o.bam"] + extra)
    assert rc == 2 and out == "" and err.count("\n") == 1 and err.startswith("longcalld_amd haplotag: ") and word in err and "no VCF" in err


@pytest.mark.parametrize("extra,word", [
    ([], "no output"), (["--tag-min-diff", "0", "-b", "o.bam"], "--tag-min-diff"), (["--tag-max-indel", "0", "-b", "o.bam"], "--tag-max-indel"),
    (["--tag-min-diff", "x", "-b", "o.bam"], "not a number"), (["-B", "255", "-b", "o.bam"], "-B"), (["-b", "o.bam", "--sam", "o.sam"], "one alignment output"),
    (["--depth", "-"], "--depth needs a file"), (["--depth-window", "5", "-b", "o.bam"], "need --depth"), (["--mods", "t.tsv", "--mod-code", "x"], "--mod-code"),
    (["--split-gz", "-b", "o.bam"], "need --split-reads"), (["--haplotag-list", "o.bam", "-b", "o.bam"], "name one file"),
    (["--vcf-sample"], "needs a value"), (["--no-such-option", "-b", "o.bam"], "unknown option"), (["-s", "-b", "o.bam"], "somatic")])
def test_other_refusals(capsys, extra, word):
    rc, out, err = _run(capsys, BASE + extra)
    assert rc == 2 and out == "" and err.count("\n") == 1 and err.startswith("longcalld_amd haplotag: ")
    assert word in err


def test_too_few_arguments_print_the_usage(capsys):
    rc, out, err = _run(capsys, ["haplotag", "ref.fa", "in.bam", "-b", "o.bam"])
    assert rc == 2 and err == cli.USAGE
    rc, out, err = _run(capsys, ["haplotag", "--help"])
    assert rc == 0 and out == cli.USAGE and "haplotag [options] ref.fa in.bam phased.vcf[.gz] [region ...]" in out
    for word in ("--vcf-sample", "--tag-snvs-only", "--tag-max-indel INT [50]", "--tag-min-diff INT [1]"):
        assert word in cli.USAGE


def test_the_options_are_parsed():
    o, pos = cli.parse(["ref.fa", "in.bam", "p.vcf", "chr1:1-500", "--vcf-sample", "HG002", "--tag-snvs-only", "--tag-max-indel=20", "--tag-min-diff", "2", "-M", "20", "-B5",
                        "--haplotag-list", "l.tsv", "--add-bam", "b.bam", "--sort-merged"], haplotag=True)
    assert pos == ["ref.fa", "in.bam", "p.vcf", "chr1:1-500"]
    assert (o["vcf_sample"], o["tag_max_indel"], o["tag_min_diff"], o["min_mapq"], o["min_bq"], o["haplotag_list"], o["add_bam"]) == ("HG002", "20", "2", "20", "5", "l.tsv", ["b.bam"])
    assert {"--tag-snvs-only", "--sort-merged"} <= o["flags"]


def test_call_does_not_take_the_new_options(capsys):
    for extra in (["--vcf-sample", "S"], ["--tag-snvs-only"], ["--tag-max-indel", "9"], ["--tag-min-diff", "2"]):
        rc, out, err = _run(capsys, ["call", "ref.fa", "in.bam"] + extra)
        assert rc == 2 and "unknown option" in err and err.startswith("longcalld_amd call: ")
    o, pos = cli.parse(["ref.fa", "in.bam", "-o", "x.vcf", "-c", "3"])
    assert (o["out_vcf"], o["min_cov"]) == ("x.vcf", "3")
    rc, out, err = _run(capsys, ["tag"])
    assert rc == 2 and "call, haplotag, index, faidx" in err


def test_a_missing_input_is_the_library_s_error(capsys, tmp_path):
    """past the parser: the run is refused by the library because the input is missing, and nothing is created"""
    rc, out, err = _run(capsys, ["haplotag", str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "p.vcf"), "-b", str(tmp_path / "o.bam")])
    assert rc == 1 and out == "" and "in.bam" in err and list(tmp_path.iterdir()) == []
