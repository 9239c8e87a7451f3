"""lcd_fai_build (host code) against a Python oracle written from the rules of include/lcd_hotpath.h: seeded multi-sequence FASTA files covering every accepted and
refused shape, the widths 1, 60 and 61, a sequence of exactly one full line; byte equality with the reference's bundled chr11_2M.fa.fai where the checkout
exists; lcd_fasta_fetch through a built .fai against the generator's own sequences."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

REF_FA = "/root/reference/test_data/chr11_2M.fa"


def make_fasta(rng, widths, nl=b"\n", last_newline=True, blank_tail=0, lengths=None):
    """-> (bytes, [(name, sequence bytes)], expected .fai text): one sequence per width; lengths[i] (default random) bases cut into lines of widths[i]"""
    out, seqs, fai = b"", [], ""
    for i, w in enumerate(widths):
        n = lengths[i] if lengths else int(rng.integers(1, 5 * w + 2))
        seq = bytes(rng.choice(list(b"ACGTNacgt"), n).astype(np.uint8))
        name = f"seq{i}"
        head = f">{name}" + (" some description\there" if i % 2 else "")
        out += head.encode() + nl
        fai += f"{name}\t{n}\t{len(out)}\t{min(w, n)}\t{min(w, n) + len(nl)}\n"
        lines = [seq[o:o + w] for o in range(0, n, w)]
        out += nl.join(lines) + nl
        seqs.append((name, seq))
    out += nl * blank_tail
    if not last_newline:
        out = out[:-len(nl)]
        n_last = len(seqs[-1][1])
        if n_last <= widths[-1]:                           # the only line of the last sequence lost its line end: one byte is counted for it (PROJECT RULE)
            rows = fai.splitlines()
            f = rows[-1].split("\t"); f[4] = str(int(f[3]) + 1); rows[-1] = "\t".join(f)
            fai = "\n".join(rows) + "\n"
    return out, seqs, fai


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("last_newline,blank_tail", [(True, 0), (False, 0), (True, 3)])
def test_accepted_shapes_equal_the_oracle_and_fetch_through_them(lcd, tmp_path, nl, last_newline, blank_tail):
    lib = lcd.load_library()
    lib.lcd_fasta_fetch.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(C.c_uint8))]
    lib.lcd_fasta_fetch.restype = C.c_int64
    code = {c: k for k, cs in enumerate(("Aa", "Cc", "Gg", "Tt")) for c in cs.encode()}
    for seed in range(6):
        rng = np.random.default_rng(50 + seed)
        widths = [1, 60, 61] + [int(rng.integers(2, 90)) for _ in range(3)]
        lengths = [int(rng.integers(1, 6)), 60, 61 * 3] + [int(rng.integers(1, 400)) for _ in range(3)]     # (seq1: exactly one full line; seq2: full lines only)
        data, seqs, want = make_fasta(rng, widths, nl, last_newline, blank_tail, lengths)
        fa = str(tmp_path / f"f{seed}.fa")
        open(fa, "wb").write(data)
        assert lcd.fai_build(fa) == len(seqs)
        assert open(fa + ".fai").read() == want
        for name, seq in seqs:                                  # the fetch through the built index returns the generator's bases
            for _ in range(4):
                b = int(rng.integers(1, len(seq) + 1)); e = int(rng.integers(b, len(seq) + 1))
                p = C.POINTER(C.c_uint8)()
                n = lib.lcd_fasta_fetch(fa.encode(), name.encode(), b, e, C.byref(p))
                assert n == e - b + 1
                assert [p[k] for k in range(n)] == [code.get(c, 4) for c in seq[b - 1:e]]
    other = str(tmp_path / "elsewhere.fai")
    assert lcd.fai_build(fa, other) == len(seqs) and open(other).read() == want


def test_shorter_last_line_and_empty_sequence(lcd, tmp_path):
    fa = str(tmp_path / "s.fa")
    open(fa, "w").write(">a\nACGT\nACGT\nAC\n>empty\n>b d\nGGG\n\n")
    assert lcd.fai_build(fa) == 3
    assert open(fa + ".fai").read() == "a\t10\t3\t4\t5\nempty\t0\t23\t0\t0\nb\t3\t28\t3\t4\n"


@pytest.mark.parametrize("text,word", [
    (b">a\nACGT\nAC\nACGT\n", "a has lines of different length"),           # a short line in the middle
    (b">a\nACGT\nACGTA\n", "a has lines of different length"),              # a longer line
    (b">ok\nAC\n>b\nACGT\n\nACGT\n", "b has lines of different length"),      # a blank line inside a sequence
    (b">a\nAC\n>b\nAC\n>a\nAC\n", "duplicate sequence name a"),
    (b"ACGT\n>a\nAC\n", "does not start with '>'"),
    (b"", "does not start with '>'"),
    (b">\nAC\n", "without a name"),
    (b"\x1f\x8b\x08\x04" + bytes(30), "compressed"),
], ids=["short_middle", "long_line", "blank_inside", "duplicate", "no_header", "empty_file", "no_name", "compressed"])
def test_refused_shapes(lcd, tmp_path, text, word):
    fa = str(tmp_path / "bad.fa")
    open(fa, "wb").write(text)
    with pytest.raises(lcd.LcdError, match="error -52:") as e:
        lcd.fai_build(fa)
    assert word in str(e.value)
    assert not os.path.exists(fa + ".fai")


def test_unreadable_and_unwritable_paths_are_minus_30(lcd, tmp_path):
    with pytest.raises(lcd.LcdError, match="error -30:.*absent.fa"):
        lcd.fai_build(str(tmp_path / "absent.fa"))
    fa = str(tmp_path / "x.fa")
    open(fa, "w").write(">a\nAC\n")
    with pytest.raises(lcd.LcdError, match="error -30:.*no_such_dir"):
        lcd.fai_build(fa, str(tmp_path / "no_such_dir" / "x.fai"))


@pytest.mark.skipif(not os.path.exists(REF_FA), reason="the reference's bundled FASTA exists in the build container only")
def test_bundled_fasta_index_is_byte_equal(lcd, tmp_path):
    fa = str(tmp_path / "chr11_2M.fa")
    shutil.copy(REF_FA, fa)
    os.chmod(fa, 0o644)
    assert lcd.fai_build(fa) == 1
    assert open(fa + ".fai", "rb").read() == open(REF_FA + ".fai", "rb").read()
