"""call_file(..., vcf_bgzf=1, vcf_index="tbi" | "csi") on the seeded multi-contig input of tests/test_gpu_call_file.py: the VCF equals the run without the option byte
for byte, the index equals the oracle's index of that file and does not depend on window_chunks or overlap, and the command line's `index` reproduces it."""
import os
import subprocess
import sys

import pytest

import vcf_index_common as vc
from conftest import ROOT
from test_gpu_call_file import CHUNK_LEN, HEADER_ARGS, cfg_of, data  # noqa: F401  (data: the module-scoped input fixture)

pytestmark = pytest.mark.gpu


def run(lcd, data, tag, **kw):
    vcf = str(data["dir"] / f"{tag}.vcf.gz")
    res = lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, vcf_path=vcf, vcf_bgzf=1, cfg=cfg_of(lcd), sample_name="s", **HEADER_ARGS, **kw)
    return vcf, res


def logical(index_bytes, gz):
    """the parsed index with every virtual offset replaced by the offset of the INFLATED text it denotes: what the index says, free of where the run's appends cut
    the file into members (an append makes members of its own, so a file's bytes -- and with them the virtual offsets -- follow window_chunks with or without an index)"""
    tab = vc.members_of(gz)[0]
    u_of = {c: u for c, u, _n in tab}
    u_of[len(gz)] = tab[-1][1] + tab[-1][2]
    at = lambda v: u_of[v >> 16] + (v & 0xffff)
    idx = vc.parse_index(index_bytes)
    for r in idx["refs"]:
        r["bins"] = {b: (at(ch[0][0]), at(ch[-1][1])) for b, ch in r["bins"].items()}     # (how many chunks a bin has follows the members: the merge rule; its span does not)
        r["meta"] = dict(r["meta"], off_beg=at(r["meta"]["off_beg"]), off_end=at(r["meta"]["off_end"]))
        if "lin" in r:
            r["lin"] = [at(v) if v else 0 for v in r["lin"]]
        if "loff" in r:
            r["loff"] = {b: at(v) for b, v in r["loff"].items()}
    return idx


CONFIGS = [(4, 0), (4, 1), (1, 0)]        # (window_chunks, overlap)


@pytest.fixture(scope="module")
def bases(lcd, data):
    """the runs WITHOUT the option, one per configuration, made once: the bytes of their .vcf.gz"""
    out = {}
    for k, (window, overlap) in enumerate(CONFIGS):
        base, _ = run(lcd, data, f"base{k}", window_chunks=window, overlap=overlap)
        assert not os.path.exists(base + ".tbi") and not os.path.exists(base + ".csi")
        out[window, overlap] = open(base, "rb").read()
    return out


@pytest.mark.parametrize("fmt", [vc.TBI, vc.CSI])
def test_the_vcf_is_unchanged_and_the_index_is_the_oracles(lcd, data, bases, fmt):
    """Figures that decide what can be asked: the .vcf.gz of window_chunks 4 and 1 differ from byte 871 on WITHOUT the option (every append is compressed into
    members of its own), so the index bytes cannot be equal across window_chunks; what is equal is the inflated text and the index with its offsets taken back to
    that text (logical).  Across overlap, at one window_chunks, the bytes of both files are equal."""
    seen = {}
    for k, (window, overlap) in enumerate(CONFIGS):
        gz = bases[window, overlap]
        scan = vc.scan_vcf(gz, fmt)
        assert len(scan["lines"]) > 20 and len(scan["names"]) >= 3 and scan["max_clen"] == 18000
        vcf, res = run(lcd, data, f"{fmt}{k}", window_chunks=window, overlap=overlap, vcf_index=fmt)
        assert open(vcf, "rb").read() == gz, (fmt, window, overlap)                    # the VCF equals the run without the option, byte for byte
        image = open(f"{vcf}.{fmt}", "rb").read()
        assert vc.ends_with_eof_member(image) and vc.inflate(image) == vc.oracle_index(scan, fmt), (fmt, window, overlap)
        vi = res["vcf_index"]
        assert (vi["wrote"], vi["skipped"], vi["n_data_lines"], vi["n_contigs"]) == (1, 0, len(scan["lines"]), len(scan["names"]))
        seen[window, overlap] = (gz, image, vc.inflate(gz), logical(vc.inflate(image), gz))
    assert seen[4, 0][:2] == seen[4, 1][:2]                                             # overlap: the same bytes, VCF and index
    assert seen[4, 0][0] != seen[1, 0][0] and seen[4, 0][2:] == seen[1, 0][2:]          # window_chunks: other members, the same text, the same index over that text


def test_the_command_line_reproduces_the_index(lcd, data, bases):
    """`index` on a copy whose name says nothing: BAM or VCF is decided by content"""
    gz = bases[4, 0]
    copy = str(data["dir"] / "no_suffix_tells")
    open(copy, "wb").write(gz)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args, suffix, fmt in ((["index", copy], ".tbi", vc.TBI), (["index", "--csi", copy], ".csi", vc.CSI)):
        r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", *args], capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert vc.inflate(open(copy + suffix, "rb").read()) == vc.oracle_index(vc.scan_vcf(gz, fmt), fmt)


def test_refused_without_a_compressed_file(lcd, data):
    with pytest.raises(lcd.LcdError) as e:
        lcd.call_file(data["bam"], data["fa"], chunk_len=CHUNK_LEN, vcf_path=str(data["dir"] / "p.vcf"), vcf_bgzf=0, cfg=cfg_of(lcd), vcf_index="tbi")
    assert "error -4:" in str(e.value) and not os.path.exists(str(data["dir"] / "p.vcf"))


def test_the_command_line_call_leaves_the_index_beside_an_unchanged_vcf(lcd, data):
    """call ... -O z -o out.vcf.gz --vcf-index tbi (-H: the header would carry the command line, which names the flag)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for tag, extra in (("cli_plain", []), ("cli_tbi", ["--vcf-index", "tbi"])):
        out = str(data["dir"] / f"{tag}.vcf.gz")
        r = subprocess.run([sys.executable, "-m", "longcalld_amd.cli", "call", data["fa"], data["bam"], "-H", "-O", "z", "-o", out, "--chunk-len", str(CHUNK_LEN), *extra],
                           capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0 and "without an index" not in r.stderr, r.stderr
        outs.append(out)
    gz = open(outs[1], "rb").read()
    assert gz == open(outs[0], "rb").read() and not os.path.exists(outs[0] + ".tbi")
    scan = vc.scan_vcf(gz)
    assert len(scan["lines"]) > 20 and scan["max_clen"] == 0
    assert vc.inflate(open(outs[1] + ".tbi", "rb").read()) == vc.oracle_tbi(scan)
