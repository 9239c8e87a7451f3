"""Chains for the PLAIN rows of the single-wavefront POA rows (poa_kernel.hip align_lean): rows with one usable predecessor, the row before, which take that
row's values from registers and run as a loop of their own inside each 64-row plan window.

The reads are 130 - 200 bases, so a graph spans more than two plan windows and nothing larger: runs that cross row 64 and row 128, a last window that ends at the
end node, windows that stay and move, bands that drift, runs that end and restart at bubbles, rows that store their ring slot for a general row to read, a band
that outgrows the 64-lane window, the certified-band instantiation, and a code region that runs out in the middle of a run.  CASES is the table that the CPU
test (tests/test_plain_row_cases_oracle.py: planned class, length of the oracle's MSA) and the GPU test (tests/test_gpu_plain_rows.py: parity with the oracle and
with the generic rows) share; oracle results are computed once per (reads, mode) and never changed."""
import numpy as np

L = 170            # backbone: rows 1 .. 170 of the graph, i.e. plan windows [1, 64], [65, 128] and a short one that ends at the end node
N_READS = 6
SEED = 11

K1 = dict(threads=64, wmax=64, cert=0)                       # K1, reads < 1 400 bases: the 64-column window, one cell per lane
K2_CERT = dict(threads=64, wmax=512, cert=1, solo=0)         # K2, certified band, clean reads: intervals in the one-cell rows first
# LCD_CELL_SHRINK: the DP region is sized this many times too small.  At 12 a chain of these reads gets about 2 400 code bytes for a read that needs about
# 28 bytes x 170 rows: the region runs out near row 90, inside a run of plain rows in the second plan window, and the chain ends LCD_OK after taking a larger one
SHRINK = {"LCD_CELL_SHRINK": "12"}


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def _backbone():
    """170 bases without a repeated neighbour: gap placements do not tie, so the reads below differ from it exactly where they say"""
    rng = np.random.default_rng(SEED)
    return _u8(np.cumsum(rng.integers(1, 4, L)) % 4)     # (every base differs from the one before by 1 - 3)


def _identical():
    h = _backbone()
    return [h.copy() for _ in range(N_READS)]


def _indel12():
    """the third read carries a 12-base insertion mid-read (the window stays while the read runs ahead of the graph), the fifth a 12-base deletion"""
    h = _backbone()
    rng = np.random.default_rng(SEED + 1)
    reads = [h.copy() for _ in range(N_READS)]
    reads[2] = _u8(np.concatenate([h[:85], rng.integers(0, 4, 12), h[85:]]))
    reads[4] = _u8(np.concatenate([h[:80], h[92:]]))
    return reads


def _snps():
    """one SNP per read at its own column: a bubble per read after the first -- rows with two predecessors, rows whose ring slot is kept, runs that end and
    restart inside a plan window"""
    h = _backbone()
    reads = [h.copy() for _ in range(N_READS)]
    for k, col in enumerate((0, 23, 59, 66, 101, 131)):
        if k:
            reads[k][col] = (reads[k][col] + 2) % 4
    return reads


def _ins40():
    """a 40-base insertion in the fourth read of a 150-base backbone: its band reaches the last lane of the 64-column window"""
    h = _backbone()[:150]
    rng = np.random.default_rng(SEED + 2)
    reads = [h.copy() for _ in range(N_READS)]
    reads[3] = _u8(np.concatenate([h[:70], rng.integers(0, 4, 40), h[70:]]))
    return reads


READS = {"identical": _identical, "indel12": _indel12, "snps": _snps, "ins40": _ins40}


def _case(name, mode, reads, planned, env=None, also=()):
    """planned: what the planner's probe must report under `env`; also: further environments the GPU test runs the same job under"""
    return dict(name=name, mode=mode, reads=reads, planned=planned, env=env or {}, also=list(also))


CASES = [
    _case("k1_identical", 0, "identical", K1, also=[SHRINK]),
    _case("k1_indel12", 0, "indel12", K1),
    _case("k1_snps", 0, "snps", K1, also=[SHRINK]),
    _case("k1_ins40", 0, "ins40", K1),
    _case("k2_cert_identical", 1, "identical", K2_CERT, env={"LCD_CERT": "1"}),
    _case("k2_cert_snps", 1, "snps", K2_CERT, env={"LCD_CERT": "1"}),
]
SWITCHES = sorted({k for c in CASES for env in [c["env"]] + c["also"] for k in env} | {"LCD_DBG"})

_reads, _oracle = {}, {}


def case_reads(case):
    if case["reads"] not in _reads:
        _reads[case["reads"]] = READS[case["reads"]]()
    return _reads[case["reads"]]


def case_oracle(case):
    """the oracle's K1 (mode 0, every read full-cover) or K2 (mode 1) chain of the case, computed once per (reads, mode)"""
    from oracle import pyoracle
    k = (case["reads"], case["mode"])
    if k not in _oracle:
        reads = case_reads(case)
        _oracle[k] = pyoracle.poa_aln_msa_cons(reads, 2) if case["mode"] == 1 else pyoracle.poa_partial_aln_msa_cons(reads, [12] * len(reads))
    return _oracle[k]


def plan_case(case, env=None):
    """the chain_plan_cases entry of a case: poa_batch plans without a submission around the chain (n_chains = 2^40)"""
    import chain_plan_cases as P
    return P.chain(case["name"], case["mode"], 0, 0, lens=[len(r) for r in case_reads(case)], n_chains=1 << 40, env=dict(case["env"], **(env or {})))
