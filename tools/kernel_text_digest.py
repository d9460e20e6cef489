#!/usr/bin/env python3
"""Digest of the device code of every HIP unit of libokx.so (no GPU): each ``.hip`` file ``make`` builds an object from
is compiled with that object's own command line plus ``-S --cuda-device-only``, and every function symbol of the assembly
is hashed over its instruction text - comments and assembler directives dropped, local labels renumbered in the order the
function first names them (their numbers carry the function's position in its unit).  The record is sorted JSON:
``functions`` {symbol: sha256} and ``units`` {file: [symbols]}.  A change that only moves host code between units leaves
``functions`` identical to the parent commit's, and every symbol in exactly one unit.
  python tools/kernel_text_digest.py [--csrc DIR] [out.json]      (default: the package's csrc, standard output)"""
import concurrent.futures
import hashlib
import json
import os
import re
import shlex
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_lines(csrc):
    """{unit: the words of the command `make` would compile its object with} for the .hip files the library is built from"""
    dry = subprocess.run(["make", "-n", "-B"], cwd=csrc, capture_output=True, text=True, check=True).stdout
    lines = {}
    for line in dry.splitlines():
        m = re.search(r"\s-c\s+(\w+)\.hip\b", line)
        if m:
            lines[m.group(1)] = shlex.split(line)
    return lines


def assembly(csrc, unit, words):
    """The unit's device assembly: its compile line with -S --cuda-device-only in the place of -c ... -o object."""
    words = list(words)
    at = words.index("-o")
    del words[at:at + 2]
    words.remove("-c")
    proc = subprocess.run(words + ["-S", "--cuda-device-only", "-o", "-"], cwd=csrc, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"{unit}.hip: {proc.stderr[-2000:]}")
    return proc.stdout


def functions(text):
    names = set(re.findall(r"^\s*\.type\s+(\w+),@function", text, re.M))
    out, name, body, labels = {}, None, None, None
    for line in text.splitlines():
        if name is None:
            m = re.match(r"(\w+):", line)
            if m and m.group(1) in names:
                name, body, labels = m.group(1), [], {}
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
            name = None
            continue
        code = line.split(";")[0].strip()
        if not code or (code.startswith(".") and not code.startswith(".L")):
            continue
        body.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), code))
    return out


def main():
    args = sys.argv[1:]
    csrc = os.path.join(REPO, "open_kinematics_amd", "csrc")
    if len(args) > 1 and args[0] == "--csrc":
        csrc = os.path.abspath(args[1])
        del args[:2]
    lines = compile_lines(csrc)
    names = sorted(lines)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(names))) as pool:
        texts = list(pool.map(lambda unit: assembly(csrc, unit, lines[unit]), names))
    record = {"functions": {}, "units": {}}
    for unit, text in zip(names, texts):
        found = functions(text)
        record["units"][unit + ".hip"] = sorted(found)
        for symbol, digest in found.items():
            if record["functions"].setdefault(symbol, digest) != digest:
                record["functions"][symbol] = "differs between units"
    out = json.dumps(record, indent=1, sort_keys=True) + "\n"
    if args:
        with open(args[0], "w") as fh:
            fh.write(out)
    else:
        sys.stdout.write(out)


if __name__ == "__main__":
    main()
