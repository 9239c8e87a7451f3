#!/usr/bin/env python3
"""Issue slots per row of the plain-row loops of the POA chain kernel, from the device assembly.  Needs no GPU.

Compiles longcalld_amd/csrc/poa_kernel.hip to gfx950 assembly with the Makefile's flags (into a temporary directory; --asm FILE reads a listing made
elsewhere), finds the plain-row loops by their marker comments (LCD_ROW_MARK in the source: `; LCD_ROW_MARK <loop> top` opens a row, `<loop> slot` sits in the
block that stores the row to its ring slot) and prints, per instantiation of align_lean, the instructions of ONE row on its common path -- a row that does not
store its ring slot, whose cells do store their codes -- by class: vector (v_*), scalar side (s_*; of these the nops, waits and branches), memory (everything
else: ds_*, global_*, ...).  Then the VGPR count, occupancy and scratch size of lcd_poa_chain_kernel<64>.

The common path is the longest cycle from the loop's header back to it that stays inside the loop, avoids the ring-slot block and falls through every
s_cbranch_execz.  Instructions are classified by the prefix of their mnemonic and nothing else."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "longcalld_amd", "csrc")
KERNEL = "_Z20lcd_poa_chain_kernelILi64EE"


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()
    arch = os.environ.get("ARCH", var("ARCH"))
    return os.environ.get("HIPCC", var("HIPCC")), var("CXXFLAGS").replace("$(ARCH)", arch).split()


def compile_asm(out):
    hipcc, flags = makefile_flags()
    cmd = [hipcc] + flags + ["-Wno-inline-asm", "-S", "--offload-device-only", "poa_kernel.hip", "-o", out]
    subprocess.check_call(cmd, cwd=CSRC)


def functions(lines):
    """-> [(symbol, first line, last line)] of the listing's functions"""
    out, cur = [], None
    for i, l in enumerate(lines):
        m = re.match(r"^(\S+):\s+; @", l)
        if m:
            cur = (m.group(1), i)
        elif cur and l.startswith("\t.size\t" + cur[0] + ","):
            out.append((cur[0], cur[1], i)); cur = None
    return out


def blocks(lines, a, b):
    """the function's basic blocks in text order: [dict(name, loop, header, ins=[mnemonic, operands], marks=[...])]"""
    out = [dict(name="entry", loop=None, header=False, ins=[], marks=[])]
    for l in lines[a + 1:b]:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; %(bb\.\d+):(.*)$", l)
        if m:
            lp = re.search(r"in Loop: Header=(BB\d+_\d+)", m.group(2))
            out.append(dict(name=m.group(1), loop=lp.group(1) if lp else None, header="Loop Header" in m.group(2), ins=[], marks=[]))
            continue
        s = l.strip()
        mk = re.match(r"^; LCD_ROW_MARK (.*)$", s)
        if mk:
            out[-1]["marks"].append(mk.group(1)); continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        s = s.split(";")[0].split()
        if s:
            out[-1]["ins"].append((s[0], " ".join(s[1:])))
    return out


def common_path(bl, loop_name):
    """-> the instructions of one row on its common path, or None"""
    top = next((i for i, b in enumerate(bl) if loop_name + " top" in b["marks"]), None)
    if top is None:
        return None
    hdr = bl[top]["name"].lstrip(".L") if bl[top]["header"] else bl[top]["loop"]
    index = {b["name"]: i for i, b in enumerate(bl)}
    h = index[".L" + hdr]
    inside = lambda i: i == h or bl[i]["loop"] == hdr
    slot = {i for i, b in enumerate(bl) if loop_name + " slot" in b["marks"]}

    def succ(i):
        ins = bl[i]["ins"]
        if ins and ins[-1][0] == "s_branch":
            return [index[ins[-1][1]]]
        nxt = [i + 1] if i + 1 < len(bl) else []
        if ins and ins[-1][0].startswith("s_cbranch"):
            return nxt if ins[-1][0] == "s_cbranch_execz" else nxt + [index[ins[-1][1]]]
        return nxt

    best = None
    def walk(i, seen, acc):
        nonlocal best
        acc = acc + bl[i]["ins"]
        for j in succ(i):
            if j == h:
                if best is None or len(acc) > len(best):
                    best = acc
            elif inside(j) and j not in slot and j not in seen:
                walk(j, seen | {j}, acc)
    walk(h, {h}, [])
    return best


def classify(path):
    c = dict(total=len(path), vector=0, scalar=0, memory=0, nop=0, wait=0, branch=0)
    for mn, _ in path:
        if mn.startswith("v_"):
            c["vector"] += 1
        elif mn.startswith("s_"):
            c["scalar"] += 1
            c["nop"] += mn == "s_nop"
            c["wait"] += mn.startswith("s_waitcnt")
            c["branch"] += mn.startswith("s_cbranch") or mn == "s_branch"
        else:
            c["memory"] += 1
    return c


def kernel_info(lines):
    at = next((i for i, l in enumerate(lines) if l.startswith("\t.size\t" + KERNEL)), None)
    info = {}
    if at is not None:
        for l in lines[at:at + 60]:
            m = re.match(r"^; (NumVgprs|Occupancy|ScratchSize): (\d+)", l)
            if m:
                info.setdefault(m.group(1), int(m.group(2)))
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--list", action="store_true", help="print the common path of every loop found")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = args.asm
        if not path:
            path = os.path.join(tmp, "poa_kernel.s")
            compile_asm(path)
        lines = open(path).read().split("\n")
    print(f"{'function':<22} {'loop':<10} {'slots':>5} {'vector':>6} {'scalar':>6} {'memory':>6}   of scalar: {'nop':>3} {'wait':>4} {'branch':>6}")
    found = 0
    for sym, a, b in functions(lines):
        m = re.search(r"align_leanILi(\d)ELi(\d)EE", sym)
        if not m:
            continue
        bl = blocks(lines, a, b)
        for loop in ("plain_c1", "plain_cn"):
            p = common_path(bl, loop)
            if p is None:
                continue
            found += 1
            c = classify(p)
            print(f"{'align_lean<%s, %s>' % m.groups():<22} {loop:<10} {c['total']:>5} {c['vector']:>6} {c['scalar']:>6} {c['memory']:>6}   {'':<10} {c['nop']:>3} {c['wait']:>4} {c['branch']:>6}")
            if args.list:
                for mn, ops in p:
                    print("    ", mn, ops)
    k = kernel_info(lines)
    print("lcd_poa_chain_kernel<64>: " + ", ".join(f"{n} {k.get(n, '?')}" for n in ("NumVgprs", "Occupancy", "ScratchSize")))
    return 0 if found else 1


if __name__ == "__main__":
    sys.exit(main())
