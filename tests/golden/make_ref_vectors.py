#!/usr/bin/env python
"""Generates tests/golden/ref_vectors.npz: the answers of the REFERENCE's own edlib and cgranges (oracle/_ref, built by oracle/Makefile where the reference
tree is present) to every call the live-reference oracle tests make, so that those tests run where oracle/_ref cannot be built (tests/ref_vectors.py).

Run where the reference tree exists, after build():  python tests/golden/make_ref_vectors.py
The file is data only: each call's result, keyed by the call's function name and argument bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pyoracle  # noqa: E402
import ref_vectors  # noqa: E402
import test_oracle_cgranges as tc  # noqa: E402
import test_oracle_edlib as te  # noqa: E402


def main():
    pyoracle.build()
    assert pyoracle.ref_cgranges() is not None and pyoracle.ref_edlib() is not None, "oracle/_ref not built: run make -C oracle where the reference tree exists"
    rec = ref_vectors.Recorder(pyoracle)
    tc.test_sorted_order_matches_reference_cgranges(rec)
    tc.test_overlap_reports_in_sorted_index_order(rec)
    tc.test_post_process_noisy_regs_host_glue(rec)
    te.test_oracle_matches_live_reference_edlib(pyoracle, rec)
    te.test_oracle_hw_mode_matches_reference_golden_vectors_and_live_edlib(pyoracle, rec)
    np.savez_compressed(ref_vectors.PATH, **rec.tab)
    print(f"{ref_vectors.PATH}: {len(rec.tab)} arrays, {os.path.getsize(ref_vectors.PATH)} bytes")


if __name__ == "__main__":
    main()
