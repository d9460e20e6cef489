#!/usr/bin/env python3
"""Digest of everything the two kernel generators emit through ``okx_quad_source`` / ``okx_lane_source`` (no GPU): for every
program fixture of tests/golden, both line-row forms, with OKX_DEV unset and with each generator switch of
tests/test_dev_switches.py::GENERATOR_SWITCHES on the fixture named there, ``{case: sha256(text) | "refused: <message>"}``
as sorted JSON.  A change that only restructures the generators leaves this file identical to the parent commit's; the
generated text is the kernel cache key (okx_jit.cpp), so identical text means identical code objects.  Every OKX_DEV
setting runs in a fresh child process.  ``--with a,b`` adds the switches a and b to every run without naming them in the case
keys: the record of a build whose new text sits behind switches (``--with quad_serial_chains``) is then the
same file as the parent commit's record when those switches restore the parent's text.
  python tools/generated_source_digest.py [--with switch,...] [out.json]      (default: standard output)"""
import ctypes as C
import glob
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
ENTRIES = ("okx_quad_source", "okx_lane_source")
MODES = ("pinned", "softnorm")


def generator_switches():
    spec = importlib.util.spec_from_file_location("test_dev_switches", os.path.join(REPO, "tests", "test_dev_switches.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return [(switch, fixture, entry) for switch, fixture, entry, _ in module.GENERATOR_SWITCHES]


def program_fixtures():
    import numpy as np

    names = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        if os.path.basename(path).startswith("rebind_"):
            continue  # rebind_<name>.npz carries the program of <name>.npz (tests/test_rebind_topologies.py holds them equal)
        with np.load(path, allow_pickle=False) as arrays:
            if "prog_row_type" in arrays.files:
                names.append(os.path.splitext(os.path.basename(path))[0])
    return names


def digest(fixture, mode, entry):
    import numpy as np

    from open_kinematics_amd import _abi, _lib
    from open_kinematics_amd.program import ConstraintProgram

    arrays = dict(np.load(os.path.join(GOLDEN, fixture + ".npz"), allow_pickle=False))
    program = ConstraintProgram.from_arrays(arrays, prefix="prog_").with_line_mode(mode)
    host = _abi.HostProgram(program)
    fn = getattr(_lib.load(), entry)
    size = fn(host.byref(), None, 0)
    if size < 0:
        return f"refused: {_lib.last_error()}"
    buf = C.create_string_buffer(size)
    if fn(host.byref(), buf, size) != size:
        raise RuntimeError(f"{entry}({fixture}, {mode}): the size changed between two calls")
    return hashlib.sha256(buf.value).hexdigest()


def child(cases, tag):
    """The digests of `cases` under this process's OKX_DEV, recorded under the switch `tag`."""
    return {f"{fixture}|{mode}|{entry}|{tag}": digest(fixture, mode, entry) for fixture, mode, entry in cases}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        json.dump(child(json.loads(sys.argv[2]), sys.argv[3]), sys.stdout)
        return
    always = ""
    if len(sys.argv) > 2 and sys.argv[1] == "--with":
        always = sys.argv[2]
        del sys.argv[1:3]
    fixtures = program_fixtures()
    runs = [("", [(f, m, e) for f in fixtures for m in MODES for e in ENTRIES])]
    runs += [(switch, [(fixture, m, entry) for m in MODES]) for switch, fixture, entry in generator_switches()]
    record = {}
    for switch, cases in runs:
        env = {k: v for k, v in os.environ.items() if k != "OKX_DEV"}
        if switch or always:
            env["OKX_DEV"] = ",".join(item for item in (switch, always) if item)
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(cases), switch], env=env,
                              capture_output=True, text=True)
        if proc.returncode != 0:
            raise SystemExit(f"OKX_DEV={switch!r}: {proc.stderr[-2000:]}")
        record.update(json.loads(proc.stdout))
    text = json.dumps(record, indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
