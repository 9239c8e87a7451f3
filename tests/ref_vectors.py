"""The reference's own edlib / cgranges for the oracle tests: live from oracle/_ref where that was built (the reference tree is present), else the answers those
libraries gave to the same calls, committed as tests/golden/ref_vectors.npz by tests/golden/make_ref_vectors.py.  A call is looked up by its function name
and the exact bytes of its arguments; a call the file does not hold fails (regenerate the file where the reference tree is present)."""
import hashlib
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.npz")
NAMES = ("ref_cr_sorted_order", "ref_cr_overlap", "ref_post_process_noisy_regs", "ref_edlib_nw", "ref_edlib_hw")


def key(name, args):
    h = hashlib.sha1(name.encode())
    for a in args:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode()); h.update(a.tobytes())
    return h.hexdigest()


def _to_arrays(k, out):
    """one call's result -> {npz name: array}: an array as itself, a tuple element by element (k.0, k.1, ...)"""
    if isinstance(out, tuple):
        return {f"{k}.{i}": np.asarray(x) for i, x in enumerate(out)}
    return {k: np.asarray(out)}


class Recorded:
    """the oracle module with its ref_* calls answered from the committed vectors"""

    def __init__(self, oracle):
        self._oracle = oracle
        self._tab = dict(np.load(PATH))

    def __getattr__(self, name):
        if name not in NAMES:
            return getattr(self._oracle, name)

        def answer(*args):
            k = key(name, args)
            if k in self._tab:
                return self._tab[k]
            parts = []
            while f"{k}.{len(parts)}" in self._tab:
                x = self._tab[f"{k}.{len(parts)}"]
                parts.append(x.item() if x.ndim == 0 else x)
            assert parts, f"{name}: no committed answer for this call (python tests/golden/make_ref_vectors.py)"
            return tuple(parts)
        return answer


class Recorder:
    """the live oracle, every ref_* call's result kept for the vectors file (tests/golden/make_ref_vectors.py)"""

    def __init__(self, oracle):
        self._oracle = oracle
        self.tab = {}

    def __getattr__(self, name):
        fn = getattr(self._oracle, name)
        if name not in NAMES:
            return fn

        def call(*args):
            out = fn(*args)
            self.tab.update(_to_arrays(key(name, args), out))
            return out
        return call


def reference(oracle):
    """the live libraries where oracle/_ref holds both, else their committed answers"""
    if oracle.ref_cgranges() is not None and oracle.ref_edlib() is not None:
        return oracle
    return Recorded(oracle)
