"""The table behind tests/test_chain_plan.py: inputs of the two planning probes (lcd_plan_chain_probe, lcd_plan_wfa_probe), and the switch rows.

The expected outputs are in tests/golden/chain_plan.json.  They were written by THIS file run as a program against a library built from the commit before the
planner moved into lcd_plan.cpp, with nothing added but the two probes calling that commit's own static functions (profiles/NOTES_chain_plan.md has the diff):

    python tests/chain_plan_cases.py <that liblcd_hotpath.so> tests/golden/chain_plan.json

Every distinct environment runs in a child process of its own, because that commit froze most switches at their first read.  The code under test never writes
the golden.  Boundaries: both sides of every comparison in chain_caps / chain_class / wfa_plan / wfa_class that a chain's shape can cross at default switches."""
import ctypes as C
import json
import os
import subprocess
import sys

CHAIN_OUT = ("threads", "wmax", "lds_bytes", "ring_k", "ring16", "solo", "cert", "node_cap", "edge_cap", "cell_cap", "spill_x", "min_w")
WFA_OUT = ("lds", "s_cap", "blk_rows", "n_ckpt", "ws_bytes", "class")
DEFAULT_SCORING = (6, 6, 2, 24, 1)   # mismatch, o1, e1, o2, e2


def chain(name, mode, n, maxl, *, ont=0, lens=None, scale=1, cert_level=-1, solo=-1, n_chains=1000, hints=None, opt=None, env=None):
    """one chain: `n` reads of `maxl` bases (or `lens`); K1 is mode 0, K2 mode 1"""
    return dict(kind="chain", name=name, mode=mode, lens=list(lens) if lens else [maxl] * n, ont=ont, scale=scale, cert_level=cert_level, solo=solo,
                n_chains=n_chains, hints=hints, opt=opt or {}, env=env or {})


def wfa(name, plen, tlen, s_want, *, anchor=0, hint=-1, scoring=DEFAULT_SCORING, env=None):
    return dict(kind="wfa", name=name, plen=plen, tlen=tlen, s_want=s_want, anchor=anchor, hint=hint, scoring=list(scoring), env=env or {})


def _cases():
    c = []
    # K1 chains of clean reads: the window (64 -> 128 -> 256 columns) and the workgroup (64 -> 128 threads) by the longest read
    for m in (200, 1399, 1400, 4599, 4600, 9399, 9400, 20000):
        c.append(chain(f"k1_clean_{m}", 0, 6, m))
    # K2 chains with full rows: the class by the longest read + 2 guard columns
    for m in (100, 254, 255, 510, 511, 1022, 1023, 2046, 2047, 5000):
        c.append(chain(f"k2_full_{m}", 1, 6, m, cert_level=0))
        c.append(chain(f"k2_cert0_{m}", 1, 6, m, env={"LCD_CERT": "0"}))
    # K2 chains over the certified band, clean reads: 16-bit ring while the int16 bound holds, no band from 65 535 bases on
    for m in (1000, 14420, 14421, 14999, 15000, 65534, 65535):   # (default scoring: a gap over 1.1 x maxl + 64 rows and columns leaves int16 between 14 420 and 14 421)
        c.append(chain(f"k2_cert_1read_{m}", 1, 1, m))
    for m in (14999, 15000):   # chain_class's own cut at 15 000 bases lies above that: only LCD_RING16=2 (16-bit whatever the bounds say) reaches it
        c.append(chain(f"k2_cert_ring16_forced_{m}", 1, 1, m, env={"LCD_RING16": "2"}))
    for m in (1000, 10281, 10282):   # three reads: 2 x maxl + (1.1 x maxl + 64) x ilog2(3) + 64 crosses 32 000 between these two
        c.append(chain(f"k2_cert_3reads_{m}", 1, 3, m))
    c.append(chain("k2_cert_uneven", 1, 0, 0, lens=[900, 1500, 1200, 300, 1499]))
    c.append(chain("k2_cert_int16_fails_scoring", 1, 5, 1000, opt={"gap_ext1": 20, "gap_ext2": 20}))
    c.append(chain("k2_cert_min_af", 1, 40, 800, opt={"min_af": 0.25}))
    # noisy reads (is_ont): K1 ring slots -- LCD_RING_K from LCD_RING_K_LEN bases on, below it what the bucket has room for (LCD_RING_K_FREE: 8, 4, 2 slots here)
    for m in (500, 1000, 1400, 1499, 1500, 4000):
        c.append(chain(f"ont_k1_{m}", 0, 8, m, ont=1))
    # ... small graphs: the spill floor up to node_cap 1 024 (4 reads of 701 bases: 1 024 nodes; of 702: 1 025)
    for m in (100, 701, 702):
        c.append(chain(f"ont_small_k1_{m}", 0, 4, m, ont=1))
        c.append(chain(f"ont_small_k2_{m}", 1, 4, m, ont=1))
    # ... K2: full rows, or the band in the systolic rows (LCD_CERT_SYS, reads of at least 256 bases), or LCD_CERT=2
    for m in (255, 256, 3000):
        c.append(chain(f"ont_k2_{m}", 1, 10, m, ont=1))
        c.append(chain(f"ont_k2_sys_{m}", 1, 10, m, ont=1, env={"LCD_CERT_SYS": "1"}))
    c.append(chain("ont_k2_cert2_3000", 1, 10, 3000, ont=1, env={"LCD_CERT": "2"}))
    # long chains: reads x longest read against LCD_SOLO_RL, the chains of the submission against LCD_SOLO_CYC_MIN; and the caller's own choice (solo 0 / 1)
    for n in (24, 25):
        for nch in (15999, 16000):
            c.append(chain(f"long_k2_{n}x4000_of_{nch}", 1, n, 4000, n_chains=nch))
            c.append(chain(f"long_k1_{n}x4000_of_{nch}", 0, n, 4000, n_chains=nch))
    for solo in (0, 1):
        c.append(chain(f"chosen_solo{solo}_k2_10x3000", 1, 10, 3000, solo=solo, n_chains=20000))
        c.append(chain(f"chosen_solo{solo}_k2_30x4000", 1, 30, 4000, solo=solo, n_chains=20000))
        c.append(chain(f"chosen_solo{solo}_k2_full_30x4000", 1, 30, 4000, solo=solo, cert_level=0, n_chains=20000))
        c.append(chain(f"chosen_solo{solo}_ont_k1_30x4000", 0, 30, 4000, solo=solo, ont=1, n_chains=20000))
    c.append(chain("long_k2_20x6000", 1, 20, 6000, n_chains=100))
    # retries: the capacity scale, the learned levels, the certified-band level
    for s in (1, 2, 4):
        c.append(chain(f"scale{s}_k1", 0, 6, 2000, scale=s))
        c.append(chain(f"scale{s}_k2", 1, 6, 2000, scale=s))
        c.append(chain(f"scale{s}_ont_k2", 1, 6, 2000, scale=s, ont=1))
        c.append(chain(f"scale{s}_tiny", 1, 2, 40, scale=s, cert_level=0))
    for h in (0, 1, 2):
        c.append(chain(f"cellhint_k1_{h}", 0, 6, 2000, hints=[h, 0, 0]))
        c.append(chain(f"cellhint_k2_{h}", 1, 6, 2000, hints=[0, h, 0], cert_level=0))
        c.append(chain(f"cellhint_ont_k2_{h}", 1, 6, 2000, hints=[0, h, 0], ont=1))
        c.append(chain(f"nodehint_k1_{h}", 0, 6, 2000, hints=[0, 0, h]))
        c.append(chain(f"nodehint_k2_{h}", 1, 6, 2000, hints=[0, 0, h]))
    for lvl in (-1, 0, 1, 2):
        c.append(chain(f"certlevel{lvl}_clean", 1, 6, 2000, cert_level=lvl))
        c.append(chain(f"certlevel{lvl}_ont", 1, 6, 2000, cert_level=lvl, ont=1))
        c.append(chain(f"certlevel{lvl}_k1", 0, 6, 2000, cert_level=lvl))
    # WFA jobs at the default scoring (36 ring rows of 2 s + 3 columns): the 16 KB bucket up to s = 55, the 32 KB bucket up to 112, the HBM ring beyond;
    # decision bytes above 16 MB (s ~ 4 100) are checkpointed
    for s in (8, 55, 56, 112, 113, 1000, 4000, 5000, 20000):
        c.append(wfa(f"wfa_s{s}", 10000, 10000, s))
    c.append(wfa("wfa_short_pair_bound_by_lengths", 20, 30, 500))
    c.append(wfa("wfa_default_bound_clean", 3000, 2900, 0))
    c.append(wfa("wfa_default_bound_sv_gap", 4000, 1500, 0))
    for h in (0, 1, 2):
        c.append(wfa(f"wfa_anchor_hint{h}", 3000, 2900, 0, anchor=1, hint=h))
        c.append(wfa(f"wfa_anchor_short_hint{h}", 300, 290, 0, anchor=1, hint=h))
    c.append(wfa("wfa_other_scoring", 5000, 5000, 100, scoring=(4, 4, 2, 12, 1)))
    return c


CASES = _cases()

# (b) every planning switch: one value that is not its default and one input whose plan it changes (against `base`, the defaults unless given)
_long = chain("sw_long_k2_25x4000_of_100", 1, 25, 4000, n_chains=100)
_clean_k2 = chain("sw_clean_k2_5x1000", 1, 5, 1000)
SWITCH_ROWS = [
    ("LCD_CERT", {"LCD_CERT": "0"}, {}, _clean_k2),
    ("LCD_CERT_SOLO_LEN", {"LCD_CERT_SOLO_LEN": "500"}, {}, _clean_k2),
    ("LCD_CERT_SYS", {"LCD_CERT_SYS": "1"}, {}, chain("sw_ont_k2_10x3000", 1, 10, 3000, ont=1)),
    ("LCD_CERT_BAND", {"LCD_CERT_BAND": "2000"}, {}, chain("sw_clean_k2_5x3000", 1, 5, 3000)),
    ("LCD_CERT_RING", {"LCD_CERT_RING": "1024"}, {}, _clean_k2),
    ("LCD_BAND_MARGIN", {"LCD_BAND_MARGIN": "40"}, {}, chain("sw_clean_k1_6x1000", 0, 6, 1000)),
    ("LCD_SOLO_RL", {"LCD_SOLO_RL": "50000"}, {}, chain("sw_k2_24x4000", 1, 24, 4000)),
    ("LCD_SOLO_MW", {"LCD_SOLO_MW": "1"}, {}, _long),
    ("LCD_SOLO_CYC", {"LCD_SOLO_CYC": "0"}, {}, chain("sw_long_k2_25x4000_of_16000", 1, 25, 4000, n_chains=16000)),
    ("LCD_SOLO_CYC_MIN", {"LCD_SOLO_CYC_MIN": "10"}, {}, _long),
    ("LCD_SOLO_CAP", {"LCD_SOLO_CAP": "0"}, {}, chain("sw_long_k2_20x6000", 1, 20, 6000, n_chains=100)),
    ("LCD_SOLO_KB", {"LCD_SOLO_KB": "30"}, {}, _long),   # (30: rounded up to the 32 KB bucket)
    ("LCD_ISO_KB", {"LCD_ISO_KB": "48"}, {}, chain("sw_k2_24x4000_iso", 1, 24, 4000)),
    ("LCD_ISO_RL", {"LCD_ISO_KB": "48", "LCD_ISO_RL": "50000"}, {"LCD_ISO_KB": "48"}, chain("sw_k2_15x4000", 1, 15, 4000)),
    ("LCD_LDS_CAP_KB", {"LCD_LDS_CAP_KB": "16"}, {}, chain("sw_clean_k1_6x3000", 0, 6, 3000)),
    ("LCD_RING_K", {"LCD_RING_K": "4"}, {}, chain("sw_ont_k1_8x2000", 0, 8, 2000, ont=1)),
    ("LCD_RING_K_LEN", {"LCD_RING_K_LEN": "3000"}, {}, chain("sw_ont_k1_8x2000_len", 0, 8, 2000, ont=1)),
    ("LCD_RING_K_FREE", {"LCD_RING_K_FREE": "0"}, {}, chain("sw_ont_k1_8x500", 0, 8, 500, ont=1)),
    ("LCD_RING_K_MAXLDS_KB", {"LCD_RING_K_MAXLDS_KB": "4"}, {}, chain("sw_ont_k1_8x500_maxlds", 0, 8, 500, ont=1)),
    ("LCD_RING16", {"LCD_RING16": "0"}, {}, _clean_k2),
    ("LCD_CELL_SHRINK", {"LCD_CELL_SHRINK": "24"}, {}, _clean_k2),
    ("LCD_NODE_HINT", {"LCD_NODE_HINT": "2"}, {}, _clean_k2),
    ("LCD_CELL_HINT", {"LCD_CELL_HINT": "2"}, {}, chain("sw_clean_k1_6x2000", 0, 6, 2000)),
    ("LCD_WFA_BUCKETS_KB", {"LCD_WFA_BUCKETS_KB": "8,64"}, {}, wfa("sw_wfa_s150", 10000, 10000, 150)),
    ("LCD_WFA_LDS_MAX_KB", {"LCD_WFA_LDS_MAX_KB": "0"}, {}, wfa("sw_wfa_s50", 10000, 10000, 50)),
    ("LCD_WFA_BLOCK_KB", {"LCD_WFA_BLOCK_KB": "8"}, {}, wfa("sw_wfa_s200", 10000, 10000, 200)),
]
# (c) the lifetime test's three probes of one input
LIFETIME_CASE = chain("lifetime_clean_k1_6x1000", 0, 6, 1000)
LIFETIME_ENV = {"LCD_LDS_CAP_KB": "16", "LCD_BAND_MARGIN": "40"}
PROCESS_SWITCHES = ("LCD_WFA_BUCKETS_KB",)   # of the planning switches, the ones a process reads once: their rows run in a child process


def key(case, env):
    return case["name"] + "".join(f"|{k}={v}" for k, v in sorted(env.items()))


def all_keyed():
    """every (case, environment) pair the golden holds"""
    out = [(c, c["env"]) for c in CASES]
    for _, env, base, case in SWITCH_ROWS:
        out += [(case, env), (case, base)]
    out += [(LIFETIME_CASE, {}), (LIFETIME_CASE, LIFETIME_ENV)]
    seen, uniq = set(), []
    for c, e in out:
        if key(c, e) not in seen:
            seen.add(key(c, e)); uniq.append((c, e))
    return uniq


def open_lib(path):
    from longcalld_amd._lib import LcdOpt
    lib = C.CDLL(path)
    i32p, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    lib.lcd_opt_default.argtypes = [C.POINTER(LcdOpt)]
    lib.lcd_plan_chain_probe.argtypes = [C.POINTER(LcdOpt), C.c_int, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_longlong, i32p, i64p]
    lib.lcd_plan_wfa_probe.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, i32p, i64p]
    return lib


def probe(lib, case):
    """the probe's output for one case, with the environment as it is now"""
    from longcalld_amd._lib import LcdOpt
    if case["kind"] == "wfa":
        out = (C.c_int64 * len(WFA_OUT))()
        sc = (C.c_int * 5)(*case["scoring"])
        assert lib.lcd_plan_wfa_probe(case["plen"], case["tlen"], case["s_want"], case["anchor"], case["hint"], sc, out) == 0
        return list(out)
    o = LcdOpt()
    lib.lcd_opt_default(C.byref(o))
    o.is_ont = case["ont"]
    for k, v in case["opt"].items():
        setattr(o, k, v)
    lens = (C.c_int * max(1, len(case["lens"])))(*case["lens"])
    hints = (C.c_int * 3)(*case["hints"]) if case["hints"] else None
    out = (C.c_int64 * len(CHAIN_OUT))()
    assert lib.lcd_plan_chain_probe(C.byref(o), case["mode"], len(case["lens"]), lens, case["scale"], case["cert_level"], case["solo"], case["n_chains"], hints, out) == 0
    return list(out)


def probe_in_child(lib_path, cases, env):
    """the probes' outputs for `cases` in a fresh process whose LCD_* environment is exactly `env`"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("LCD_")}
    e.update(env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path], input=json.dumps(cases), capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def _main(argv):
    if argv[1] == "--child":
        lib = open_lib(argv[2])
        print(json.dumps([probe(lib, c) for c in json.load(sys.stdin)]))
        return
    lib_path, out_path = os.path.abspath(argv[1]), argv[2]
    by_env = {}
    for c, e in all_keyed():
        by_env.setdefault(tuple(sorted(e.items())), []).append(c)
    golden = {}
    for env, cases in by_env.items():
        for c, r in zip(cases, probe_in_child(lib_path, cases, dict(env))):
            golden[key(c, dict(env))] = r
    with open(out_path, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(golden)} probe results from {len(by_env)} processes -> {out_path}")


if __name__ == "__main__":
    _main(sys.argv)
