"""Generator of tests/golden/bai_hg002.npz (data only): the record table and the BGZF member table of the reference's bundled HG002_chr11_hifi_test.bam, read by
the plain gzip decoding of tests/bai_common.py, and the bytes of the .bai samtools wrote for it.  Run where the reference checkout exists:
    python tests/golden/make_bai_fixture.py [reference root]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bai_common as bc  # noqa: E402


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    path = os.path.join(root, "test_data", "HG002_chr11_hifi_test.bam")
    bam = open(path, "rb").read()
    s = bc.scan_bam(bam)
    r = s["recs"]
    np.savez_compressed(os.path.join(HERE, "bai_hg002.npz"),
                        n_ref=np.int64(len(s["refs"])), ref_lens=np.array([l for _n, l in s["refs"]], np.int64), fsize=np.int64(len(bam)),
                        members=np.array(s["tab"], np.int64),
                        tid=np.array([x["tid"] for x in r], np.int32), pos=np.array([x["pos"] for x in r], np.int64), end=np.array([x["end"] for x in r], np.int64),
                        flag=np.array([x["flag"] for x in r], np.int32), u0=np.array([x["u0"] for x in r], np.int64), u1=np.array([x["u1"] for x in r], np.int64),
                        vbeg=np.array([x["vbeg"] for x in r], np.uint64), vend=np.array([x["vend"] for x in r], np.uint64),
                        samtools_bai=np.frombuffer(open(path + ".bai", "rb").read(), np.uint8))
    print(len(r), "records,", len(s["tab"]), "members")


if __name__ == "__main__":
    main()
