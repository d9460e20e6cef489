"""
Batched norm chains of the quad generator (``csrc/okx_quadgen.cpp``: up to four distance / angle rows share ONE chain of
`+ EPS_SQ`, fast_sqrt_rsqrt and `- EPS`, lane k of the quad working on row k) and the switch that restores the serial text,
``OKX_DEV=quad_serial_chains``: the generated source is deterministic with and without the switch (the text is the kernel
cache key), the two texts differ where they should, the helpers are defined only where they are used, and every text
passes the device compiler's front end (``hipcc -fsyntax-only`` for gfx950).  CPU only.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from open_kinematics_amd import _abi, _lib

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIXTURES = ["c1_dw_corner", "c3_axle_grid", "c4_macpherson_grid", "rows_all_classes"]
SWITCHES = ["quad_serial_chains"]
CHAIN_ROW_TYPES = (0, 1, 2, 3)  # distance, spherical, angle, three-point angle: the rows whose chains are batched


def _source(program, entry: str = "okx_quad_source") -> str:
    lib = _lib.load()
    host = _abi.HostProgram(program)
    fn = getattr(lib, entry)
    size = fn(host.byref(), None, 0)
    if size < 0:
        raise ValueError(_lib.last_error())
    buf = C.create_string_buffer(size)
    assert fn(host.byref(), buf, size) == size
    return buf.value.decode()


def _front_end_accepts(source: str, tmp_path, tag: str) -> None:
    path = tmp_path / f"{tag}.hip"
    path.write_text(source)
    proc = subprocess.run([HIPCC, "-fsyntax-only", "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17",
                           "-include", "hip/hip_runtime.h", "-Wno-unused-command-line-argument", str(path)],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_sources_are_deterministic_and_compile_with_and_without_the_switches(golden, monkeypatch, tmp_path, fixture):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    _, program = golden(fixture)
    program = program.with_line_mode("pinned")
    texts = {}
    for switch in [""] + SWITCHES + [",".join(SWITCHES)]:
        if switch:
            monkeypatch.setenv("OKX_DEV", switch)
        else:
            monkeypatch.delenv("OKX_DEV", raising=False)
        first, second = _source(program), _source(program)
        assert first == second, f"OKX_DEV={switch!r}: the same setting must give the same text every time"
        texts[switch] = first
    monkeypatch.delenv("OKX_DEV", raising=False)
    default, serial = texts[""], texts["quad_serial_chains"]
    assert texts[",".join(SWITCHES)] == serial
    # the serial text knows nothing of the batches: no helper, no call
    assert "qsum_t" not in serial and "QB3" not in serial
    # the default text batches this program's chains and defines the helpers it calls, once
    assert default != serial
    assert default.count("DEV double qsum_t4(") == 1 and "= qsum_t" in default
    for tag, text in (("default", default), ("serial", serial)):
        _front_end_accepts(text, tmp_path, f"{fixture}_{tag}")


@pytest.mark.parametrize("fixture", ["c1_dw_corner", "c4_macpherson_grid", "rows_all_classes"])
def test_one_chain_per_batch_of_four_rows(golden, monkeypatch, fixture):
    """Single mode: the residual-only pass of the module (`okx_quad_eval`'s neighbour, the confirming pass) runs
    ceil(rows / 4) batched chains - a last batch of one row keeps its serial chain - and every batched row fetches its
    results from its own lane."""
    monkeypatch.delenv("OKX_DEV", raising=False)
    _, program = golden(fixture)
    program = program.with_line_mode("pinned")
    rows = int(sum(int(t) in CHAIN_ROW_TYPES for t in program.row_type))
    text = _source(program)
    start = text.index("okx_quad_eval")  # one kernel's text: one evaluation
    body = text[start:text.index("__global__", start + 1)] if "__global__" in text[start + 1:] else text[start:]
    sizes = [int(k) for k in re.findall(r"= qsum_t([234])\(", body)]
    n_eval = max(1, body.count("double ss = 0.0, mres_new = 0.0;"))
    per_eval = sizes[:len(sizes) // n_eval]
    full, rest = divmod(rows, 4)
    assert per_eval == [4] * full + ([rest] if rest >= 2 else [])
