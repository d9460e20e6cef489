#!/usr/bin/env python3
"""The passes of a quad kernel in its disassembly (tools/quad_isa.sh leaves okx_quad_cold_u.s / okx_quad_solve_u.s in its
cache directory): every loop (a backward branch and its target) and every skipped region (a forward branch over it) of at
least MIN instructions, with its instruction mix.  In okx_quad_cold_u the fast loop's full pass is the first large loop and
the confirming pass the large skipped region right behind it; the general loop follows with both once more.
   python3 tools/quad_passes.py /tmp/okx_isa_dw/okx_quad_cold_u.s [MIN = 300]"""
import re
import sys

path = sys.argv[1]
least = int(sys.argv[2]) if len(sys.argv) > 2 else 300
KINDS = (("v_rsq_f64", r"v_rsq_f64"), ("v_rcp_f64", r"v_rcp_f64"), ("dpp", r"dpp"), ("accvgpr", r"accvgpr"), ("cndmask", r"cndmask"),
         ("fp64", r"v_(fma|mul|add|fmac)_f64"))
ops, offset_of = [], {}
base = None
for line in open(path):
    m = re.match(r"^\s+([a-z]\S*).*//\s*([0-9A-Fa-f]+):", line)
    if not m:
        continue
    addr = int(m.group(2), 16)
    base = addr if base is None else base
    offset_of[addr - base] = len(ops)
    target = re.search(r"<\S+\+0x([0-9a-f]+)>\s*$", line) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
    ops.append((m.group(1), line, int(target.group(1), 16) if target else None))
regions = []
for i, (op, _, target) in enumerate(ops):
    if target is None or target not in offset_of:
        continue
    j = offset_of[target]
    if j <= i and i - j >= least:
        regions.append((j, i, "loop"))
    elif j > i and j - i >= least:
        regions.append((i + 1, j - 1, "skipped region"))
print(f"{path}: {len(ops)} instructions")
for lo, hi, what in sorted(regions):
    text = [ops[k][1] for k in range(lo, hi + 1)]
    mix = "  ".join(f"{name} {sum(bool(re.search(rx, t.split('//')[0])) for t in text)}" for name, rx in KINDS)
    print(f"  {what:14s} instructions {lo:5d}..{hi:5d}  {hi - lo + 1:5d}  {mix}")
