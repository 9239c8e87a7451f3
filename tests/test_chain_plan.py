"""What the host plans for a POA chain and a WFA job (csrc/lcd_plan.cpp), observed through the two probes on a machine without a GPU.

Every GPU test compares results with the oracle, and a chain's class changes speed only: these tests are what notices a planning default that slipped.  The
expected values (tests/golden/chain_plan.json) come from the commit before the planner was moved, see tests/chain_plan_cases.py."""
import json
import os
import re

import pytest

import chain_plan_cases as T
from conftest import ROOT

CSRC = os.path.join(ROOT, "longcalld_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "chain_plan.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from longcalld_amd import _lib
    return T.open_lib(_lib.LIB_PATH)


@pytest.fixture
def clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("LCD_")]:
        monkeypatch.delenv(k)
    return monkeypatch


def _named(case, out):
    return dict(zip(T.CHAIN_OUT if case["kind"] == "chain" else T.WFA_OUT, out))


def _probe_with(lib, mp, case, env):
    """probe `case` in this process with exactly `env` set (the switches are read per call), or in a child where a switch is read once per process"""
    if any(k in T.PROCESS_SWITCHES for k in env):
        from longcalld_amd import _lib
        return T.probe_in_child(_lib.LIB_PATH, [case], env)[0]
    with mp.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        return T.probe(lib, case)


# ---- (a) characterisation: every boundary of the planner, against the commit before ----
def test_golden_covers_the_table(golden):
    assert sorted(golden) == sorted(T.key(c, e) for c, e in T.all_keyed())


@pytest.mark.parametrize("case", T.CASES, ids=[T.key(c, c["env"]) for c in T.CASES])
def test_plan_matches_parent(lib, golden, clean_env, case):
    got = _probe_with(lib, clean_env, case, case["env"])
    assert _named(case, got) == _named(case, golden[T.key(case, case["env"])])


# ---- the switch table, as the header declares it ----
_COMMENT = re.compile(r"\s*(LCD_\w+)\s*\|\s*(call|process)\s*\|\s*([^|]+?)\s*\|\s*(.+)$")
_DECL = re.compile(r".*?(\w+)\s*(?:=\s*(.+?)|\{(.*)\})\s*$")


def switch_table():
    """{environment name: (member, C++ default, lifetime, default as documented, meaning)} from csrc/lcd_switches.h"""
    tab = {}
    for ln in open(os.path.join(CSRC, "lcd_switches.h")):
        code, _, comment = ln.partition("//")
        m = _COMMENT.match(comment)
        if not m or not code.strip():
            continue
        d = _DECL.match([x for x in code.split(";") if x.strip()][-1].strip())   # (the documented member is the last one a line declares)
        assert d, f"lcd_switches.h: a switch line the test cannot read: {ln.strip()[:120]}"
        name, life, doc_default, meaning = m.groups()
        assert name not in tab, name
        tab[name] = (d.group(1), (d.group(2) if d.group(2) is not None else d.group(3)).strip(), life, doc_default, meaning.strip())
    return tab


def test_switch_table_is_the_only_reader_of_the_environment():
    tab = switch_table()
    assert len(tab) >= 55
    hdr = open(os.path.join(CSRC, "lcd_switches.h")).read()
    read_names = set(re.findall(r'"(LCD_\w+)"', hdr[hdr.index("HostSwitches::from_env() {"):]))
    assert read_names == set(tab), (read_names ^ set(tab))
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".cpp", ".h", ".hip")) and fn != "lcd_switches.h":
            for name in re.findall(r'getenv\("(\w+)"\)', open(os.path.join(CSRC, fn)).read()):
                assert name in ("LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE"), f"{fn} reads {name} from the environment"


def _planning_switches():
    """environment names of the switches chain_caps, chain_class, wfa_plan and wfa_class read: every `sw.<member>` of lcd_plan.cpp"""
    tab = switch_table()
    by_member = {v[0]: k for k, v in tab.items()}
    hdr = open(os.path.join(CSRC, "lcd_switches.h")).read()
    names = set()
    for tok in set(re.findall(r"\bsw\.(\w+)", open(os.path.join(CSRC, "lcd_plan.cpp")).read())):
        if tok in by_member:
            names.add(by_member[tok])
            continue
        body = re.search(r"\b%s\(\) const \{([^\n]*)\}" % tok, hdr)   # an accessor of the table: the members it reads
        assert body, f"lcd_plan.cpp reads sw.{tok}, which the switch table does not declare"
        used = {by_member[w] for w in re.findall(r"\b\w+\b", body.group(1)) if w in by_member}
        assert used, tok
        names |= used
    return names


# ---- (b) every switch the planner reads is wired: a value that is not the default changes a plan, the way it did in the parent ----
def test_every_planning_switch_has_a_row(golden):
    rows = {name for name, _, _, _ in T.SWITCH_ROWS}
    missing = sorted(_planning_switches() - rows)
    assert not missing, f"planning switches without a row in chain_plan_cases.SWITCH_ROWS: {missing}"
    for name, env, base, case in T.SWITCH_ROWS:
        assert name in env and name not in base
        assert golden[T.key(case, env)] != golden[T.key(case, base)], f"{name}: the row's plan does not differ from its base"


@pytest.mark.parametrize("row", T.SWITCH_ROWS, ids=[r[0] for r in T.SWITCH_ROWS])
def test_switch_changes_the_plan_as_in_parent(lib, golden, clean_env, row):
    name, env, base, case = row
    for e in (env, base):
        assert _named(case, _probe_with(lib, clean_env, case, e)) == _named(case, golden[T.key(case, e)]), (name, e)


# ---- (c) lifetime: a call-lifetime switch changed inside a process is seen by the next call (the parent kept what its first call saw) ----
def test_call_switches_are_read_at_every_call(lib, golden, clean_env):
    case = T.LIFETIME_CASE
    first = T.probe(lib, case)
    for k, v in T.LIFETIME_ENV.items():
        clean_env.setenv(k, v)
    second = T.probe(lib, case)
    for k in T.LIFETIME_ENV:
        clean_env.delenv(k)
    third = T.probe(lib, case)
    assert _named(case, first) == _named(case, golden[T.key(case, {})])
    assert _named(case, second) == _named(case, golden[T.key(case, T.LIFETIME_ENV)])
    assert _named(case, third) == _named(case, golden[T.key(case, {})])
    assert second != first


# ---- (d) INTEGRATION.md's switch section says what the table says ----
def _doc_rows():
    """[(names, defaults)] of the switch section's table rows that document environment switches"""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = txt[txt.index("Run-time switches (environment"):]
    rows = []
    for ln in sec.splitlines():
        cells = [c.strip() for c in ln.split("|")]
        if len(cells) < 5 or "-D" in cells[1] or not re.search(r"`LCD_\w+", cells[1]):
            continue
        names = re.findall(r"`(LCD_\w+)(?:=[^`]*)?`", cells[1])
        rows.append((names, [d.strip() for d in cells[2].split(", ")] if len(names) > 1 else [cells[2]]))
    return sec, rows


def test_integration_md_matches_the_switch_table():
    tab = switch_table()
    sec, rows = _doc_rows()
    documented = {}
    for names, defaults in rows:
        assert len(names) == len(defaults), f"INTEGRATION.md: {names} against defaults {defaults}"
        for n, d in zip(names, defaults):
            assert n not in documented, f"INTEGRATION.md documents {n} twice"
            documented[n] = d
    assert sorted(documented) == sorted(tab), sorted(set(documented) ^ set(tab))
    for name, (member, cxx_default, life, doc_default, _) in tab.items():
        assert documented[name] == doc_default, f"{name}: INTEGRATION.md says {documented[name]!r}, lcd_switches.h says {doc_default!r}"
        try:
            want = float(doc_default)
        except ValueError:
            continue   # (a default that is not a number: "unset", "CUs / 2", ...)
        got = {"true": 1.0, "false": 0.0}.get(cxx_default)
        if got is None:
            got = float(eval(cxx_default, {"__builtins__": {}}))   # the initialiser is a number or a shift of numbers
        assert got == want, f"{name}: initialised with {cxx_default}, documented as {doc_default}"
    # no switch in the section that the table lacks (build switches -DLCD_* and the LCD_ERR_* status names are not environment switches)
    loose = set(re.findall(r"(?<!-D)\bLCD_[A-Z0-9_]+\b", sec)) - set(tab)
    loose = {n for n in loose if not n.startswith("LCD_ERR_") and ("-D" + n) not in sec}
    assert not loose, f"INTEGRATION.md names switches the table lacks: {sorted(loose)}"
    for life in ("call", "process"):
        assert f"**{life}**" in sec   # the lifetime rule is stated there
    assert "SubmitEnv" not in sec and "ProcessEnv" not in sec and "ChainEnv" not in sec
