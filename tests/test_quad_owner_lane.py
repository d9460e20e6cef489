"""
Two generator switches of the quad kernels (``csrc/okx_quadgen.cpp``; ``tools/README.md``), each of which restores the
earlier text of one cross-lane move whose result only the owning lane reads:

  quad_full_diag_update  the LDL^T trailing update (and pair mode's rank-one terms of the joining rows) broadcasts lane 2's
                         operand ahead of entry 2 of a diagonal block (default: lane 2's own register - only lane 2 reads
                         that entry)
  quad_full_diag_rows    the same for the J^T J contribution of a row that touches one free block

Every text is deterministic (the text is the kernel cache key), each switch changes it, every text passes the device
compiler's front end, both switches together give the text of the commit before them for every fixture and every
other generator switch (``tools/generated_source_digest.py``; that commit's record is ``tests/golden/owner_lane_parent_digest.json``),
and ``okx_quad_eval`` - which stores whole diagonal blocks of J^T J - never takes the rows' change.  CPU only.
"""

import importlib.util
import json
import os

import pytest

import ctypes as C
import shutil
import subprocess

from open_kinematics_amd import _abi, _lib

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SWITCHES = ["quad_full_diag_update", "quad_full_diag_rows"]
ALL = ",".join(SWITCHES)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(program) -> str:
    lib = _lib.load()
    host = _abi.HostProgram(program)
    size = lib.okx_quad_source(host.byref(), None, 0)
    if size < 0:
        raise ValueError(_lib.last_error())
    buf = C.create_string_buffer(size)
    assert lib.okx_quad_source(host.byref(), buf, size) == size
    return buf.value.decode()


def _front_end_accepts(source: str, tmp_path, tag: str) -> None:
    path = tmp_path / f"{tag}.hip"
    path.write_text(source)
    proc = subprocess.run([HIPCC, "-fsyntax-only", "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17",
                           "-include", "hip/hip_runtime.h", "-Wno-unused-command-line-argument", str(path)],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]


@pytest.mark.parametrize("mode", ["pinned", "softnorm"])
@pytest.mark.parametrize("fixture", ["c1_dw_corner", "c3_axle_grid"])
@pytest.mark.parametrize("switch", SWITCHES)
def test_each_switch_gives_deterministic_source_that_differs_and_compiles(golden, monkeypatch, tmp_path, switch, fixture, mode):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    _, program = golden(fixture)
    program = program.with_line_mode(mode)
    monkeypatch.delenv("OKX_DEV", raising=False)
    default = _source(program)
    assert default == _source(program)
    monkeypatch.setenv("OKX_DEV", switch)
    first, second = _source(program), _source(program)
    assert first == second, "the same switch must give the same text every time"
    assert first != default
    monkeypatch.setenv("OKX_DEV", f"{switch}=0")
    assert _source(program) == default
    _front_end_accepts(first, tmp_path, f"{switch}_{fixture}_{mode}")


def test_both_switches_together_restore_the_parent_commits_text(monkeypatch):
    """Every case of the digest tool's record, computed here in one process (the switches are read at every generation)."""
    spec = importlib.util.spec_from_file_location("generated_source_digest", os.path.join(REPO, "tools", "generated_source_digest.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(REPO, "tests", "golden", "owner_lane_parent_digest.json"), encoding="utf-8") as fh:
        parent = json.load(fh)
    fixtures = tool.program_fixtures()
    runs = [("", [(f, m, e) for f in fixtures for m in tool.MODES for e in tool.ENTRIES])]
    runs += [(switch, [(fixture, m, entry) for m in tool.MODES]) for switch, fixture, entry in tool.generator_switches()]
    record = {}
    for switch, cases in runs:
        monkeypatch.setenv("OKX_DEV", ",".join(item for item in (switch, ALL) if item))
        record.update(tool.child(cases, switch))
    assert sorted(record) == sorted(parent)
    assert [key for key in sorted(parent) if record[key] != parent[key]] == []


def _eval_kernel(source: str) -> str:
    start = source.index("okx_quad_eval(QEvalArgs a) {")
    return source[start:source.index("\n}\n", start)]


@pytest.mark.parametrize("fixture", ["c1_dw_corner", "c4_macpherson_grid", "rows_all_classes"])
def test_the_parity_kernel_keeps_whole_diagonal_blocks(golden, monkeypatch, fixture):
    """okx_quad_eval stores every lane's entries of the diagonal blocks: its body is the same text with and without
    quad_full_diag_rows (broadcasts ahead of every entry), while the solve kernels' text changes."""
    _, program = golden(fixture)
    monkeypatch.delenv("OKX_DEV", raising=False)
    default = _source(program)
    monkeypatch.setenv("OKX_DEV", "quad_full_diag_rows")
    full = _source(program)
    assert full != default
    assert _eval_kernel(default) == _eval_kernel(full)
    assert "a.ata[" in _eval_kernel(default)


@pytest.mark.parametrize("fixture", ["c1_dw_corner", "c3_axle_grid", "rows_all_classes"])
def test_the_default_text_names_every_residual(golden, monkeypatch, fixture):
    """`const double r{i} =` for every row (what tests/test_quadgen.py looks for)."""
    _, program = golden(fixture)
    monkeypatch.delenv("OKX_DEV", raising=False)
    default = _source(program)
    rows = 0
    while f"const double r{rows} =" in default:
        rows += 1
    # (pair mode solves the half program: its rows, without the row that joins the halves)
    assert rows >= (int(len(program.row_type)) if fixture != "c3_axle_grid" else (int(len(program.row_type)) - 1) // 2)
