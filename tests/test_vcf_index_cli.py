"""The command line of the VCF index: --vcf-index is parsed and refused without -O z / -o FILE, `index --csi` is parsed, `index` decides by content, and the old
spellings behave as before.  No device is needed: every refusal comes before the library is used."""
import gzip
import os
import subprocess
import sys

import vcf_index_common as vc
from conftest import ROOT


def cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)


def test_vcf_index_is_parsed():
    from longcalld_amd import cli as m
    o, pos = m.parse(["-O", "z", "-o", "out.vcf.gz", "--vcf-index", "tbi", "ref.fa", "in.bam"])
    assert o["vcf_index"] == "tbi" and o["out_type"] == "z" and pos == ["ref.fa", "in.bam"]
    assert m.parse(["--vcf-index=csi", "ref.fa", "in.bam"])[0]["vcf_index"] == "csi"
    assert "vcf_index" not in m.parse(["--make-index", "ref.fa", "in.bam"])[0]
    assert m.parse(["ref.fa", "in.bam", "--vcf-index"]) == 2
    for word in ("--vcf-index tbi|csi", "index [--csi] in.vcf.gz", "--make-index", "it does not index the VCF"):
        assert word in m.USAGE, word


def test_vcf_index_is_refused_without_a_compressed_file():
    for args in (["--vcf-index", "tbi", "-o", "o.vcf"], ["--vcf-index", "tbi", "-O", "v", "-o", "o.vcf"], ["--vcf-index", "csi", "-O", "z"], ["--vcf-index", "csi", "-O", "z", "-o", "-"]):
        r = cli("call", *args, "ref.fa", "in.bam")
        assert r.returncode == 2 and r.stderr.count("\n") == 1 and "--vcf-index needs -O z and -o FILE" in r.stderr, (args, r.stderr)
    r = cli("call", "--vcf-index", "bai", "-O", "z", "-o", "o.vcf.gz", "ref.fa", "in.bam")
    assert r.returncode == 2 and "--vcf-index can only be tbi or csi" in r.stderr
    assert not os.path.exists(os.path.join(ROOT, "o.vcf")) and not os.path.exists(os.path.join(ROOT, "o.vcf.gz"))


def test_index_spellings(tmp_path):
    from longcalld_amd import cli as m
    assert m.parse_index(["index", "--csi", "x.vcf.gz"]) == ("index-csi", ["x.vcf.gz"]) and m.parse_index(["index", "x.vcf.gz", "--csi", "o.csi"]) == ("index-csi", ["x.vcf.gz", "o.csi"])
    # the old spellings, as before
    assert m.parse_index(["index", "in.bam"]) == ("index", ["in.bam"]) and m.parse_index(["index", "in.bam", "o.bai"]) == ("index", ["in.bam", "o.bai"])
    assert m.parse_index(["faidx", "ref.fa"]) == ("faidx", ["ref.fa"])
    assert m.parse_index(["index"]) == 2 and m.parse_index(["faidx", "a", "b"]) == 2 and m.parse_index(["index", "--fast", "in.bam"]) == 2 and m.parse_index(["faidx", "--csi", "a"]) == 2
    assert m.parse_index(["index", "--csi"]) == 2


def test_index_decides_by_content(tmp_path):
    from longcalld_amd import cli as m
    import bai_common as bc
    text = vc.seeded_text(3, 10)
    files = {"a.bam": (vc.build_gz(text), "vcf"), "b.vcf.gz": (bc.build_bam([("c", 100)], []), "bam"), "c.vcf.gz": (gzip.compress(text), "vcf"), "d.bam": (text, "vcf"),
             "e.vcf.gz": (vc.build_gz(b"hello\n"), None), "f": (b"", None)}
    for name, (content, kind) in files.items():
        open(tmp_path / name, "wb").write(content)
        assert m.file_kind(str(tmp_path / name)) == kind, name
    assert m.file_kind(str(tmp_path / "absent")) is None
    r = cli("index", "--csi", str(tmp_path / "b.vcf.gz"))                                 # a BAM, whatever its name
    assert r.returncode == 2 and "only BAI is built for a BAM" in r.stderr and not os.path.exists(str(tmp_path / "b.vcf.gz.csi"))
    assert cli("index", "--csi", str(tmp_path / "e.vcf.gz")).returncode == 2
    # an uncompressed and a plain-gzip VCF reach the builder, which says which of the two the file is (host code: before any device call)
    for name, word in (("d.bam", "plain text"), ("c.vcf.gz", "plain gzip")):
        r = cli("index", str(tmp_path / name))
        assert r.returncode == 1 and "error -33:" in r.stderr and word in r.stderr, r.stderr
        assert not os.path.exists(str(tmp_path / name) + ".tbi")
    r = cli("index", str(tmp_path / "absent.bam"))                                        # as before: the BAM path and its message
    assert r.returncode == 1 and "absent.bam" in r.stderr
