"""
GPU: the launch branches of okx_api.hip that no other test reaches - the lane kernel's nested and coarse-to-fine start
modes (generated under their developer switches only), the per-geometry first-step scratch of a captured launch that
finds it too small, and the lane-group packed interpreter kernel (auto selection takes it only without a quad kernel).  Smallest shapes that reach them; answers against independent cold solves and the oracle.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd import _lib
from open_kinematics_amd._abi import LaunchCaps

pytestmark = pytest.mark.gpu

NESTED, REFINED = 2, 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def _start_mode(dp, n_problems: int) -> tuple:
    """(family, start mode) the launch path plans for a forced lane launch of `n_problems` with chain_len = -1"""
    lib = _lib.load()
    caps = LaunchCaps()
    assert lib.okx_debug_program_caps(dp._handle, C.byref(caps)) == 0, _lib.last_error()
    opts = dp.default_opts()
    opts.kernel, opts.chain_len = 4, -1
    out = (C.c_int32 * 6)()
    assert lib.okx_debug_plan_launch(C.byref(caps), C.byref(opts), n_problems, 0, 0, C.byref(out)) == 0, _lib.last_error()
    return out[0], out[2]


def test_nested_and_refined_starts_give_the_cold_solves_answers(monkeypatch):
    """chain_len = -1 on a lane module that carries both start modes: a span of 256 steps runs the nested bodies (with
    their ring), one of 260 - no multiple of 256, a multiple of 4 - the four strided launches of the coarse-to-fine start.
    Records and compact output; 1e-9 mm against cold solves of the same kernel and against the oracle (tests/test_gpu_lane.py)."""
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.workloads import macpherson_grid_problem
    from oracle.oracle import Oracle

    monkeypatch.setenv("OKX_DEV", "lane_nested,lane_refine")
    program, targets = macpherson_grid_problem(13, 20)  # 260 problems, rows of 20 steer steps
    dp = DeviceProgram(program, "cuda:0")
    assert dp.lane_threshold > 0, f"lane kernel not loaded: {dp.lane_note}"
    t = torch.as_tensor(targets, device="cuda:0")
    cold = dp.solve(t, kernel="lane", chain_len=1, predictor=False)
    assert np.all((cold.info()["flags"] & 7) == 1)
    sub = slice(None, None, 8)
    orc = Oracle(program).sweep(targets[sub], 1e-15, 1e-15, 1e-15, warm_start=False)
    for n, mode in ((256, NESTED), (260, REFINED)):
        assert _start_mode(dp, n) == (4, mode)
        guard = torch.full((n + 1, program.n_out, 3), -7.0, dtype=torch.float64, device="cuda:0")
        res = dp.solve(t[:n], kernel="lane", chain_len=-1, out=guard[:n])
        free = dp.solve(t[:n], kernel="lane", chain_len=-1, output="free")
        torch.cuda.synchronize()
        assert np.all((res.info()["flags"] & 7) == 1), mode
        assert float((res.positions - cold.positions[:n]).abs().max()) <= 1e-9, mode
        assert float((guard[n] + 7.0).abs().max()) == 0.0, "wrote past the batch"
        assert np.max(np.abs(res.positions.cpu().numpy()[sub] - orc.positions[: len(range(n)[sub])])) <= 1e-9, mode
        assert float((free.free - res.positions[:, dp.free_out_index]).abs().max()) <= 1e-9, mode


def test_captured_ensemble_launch_with_too_small_a_first_step_scratch(golden):
    """Per-geometry first-step tables live in a grow-only scratch of the program that is never grown inside a stream
    capture: a captured launch that finds it too small runs without the shared first step, one that finds it large enough
    fills it inside the graph.  Both replay to the plain launch's answers."""
    from open_kinematics_amd.batch import DeviceProgram

    arrays, program = golden("c5_ensemble")
    pinned = program.with_line_mode("pinned")
    dp = DeviceProgram(pinned, "cuda:0")
    gpos, gparam = dp.rebind(torch.as_tensor(arrays["hardpoints"], device="cuda:0"))
    g, s = arrays["targets_abs"].shape[:2]
    assert s >= 4  # (fewer steps per geometry take no table at all)
    t = torch.as_tensor(np.ascontiguousarray(arrays["targets_abs"]).reshape(g * s, -1), device="cuda:0")
    kw = dict(geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, kernel="quad", chain_len=1, predictor=False)
    no_table = dp.solve(t, shared_first_step=False, **kw)  # (warm: lazy loads happen outside the capture; no scratch yet)
    torch.cuda.synchronize()
    assert np.all((no_table.info()["flags"] & 7) == 1)
    ref = arrays["ref_tight_pos"].reshape(g * s, -1, 3)
    assert np.max(np.abs(no_table.positions.cpu().numpy() - ref)) <= 6e-8  # reference's own floor (tests/test_gpu_lane.py)
    out = torch.empty_like(no_table.positions)
    stream = torch.cuda.Stream()
    for scratch in ("too small", "large enough"):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            dp.solve(t, out=out, **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        if scratch == "too small":  # the launch the graph holds ran the heads' own first pass: the bits of that launch
            assert torch.equal(out, no_table.positions)
            plain = dp.solve(t, **kw)  # outside a capture: grows the scratch, shares the first step
            torch.cuda.synchronize()
            assert float((plain.positions - no_table.positions).abs().max()) <= 1e-9
        else:
            assert torch.equal(out, plain.positions)


@pytest.mark.parametrize("name", ["c4_macpherson_grid", "c1_dw_corner"])
def test_packed_interpreter_kernel_matches_the_single_kernel_and_the_oracle(golden, name):
    """kernel = "packed": four (15 unknowns) / three (18) problems per wavefront; a batch that leaves the last wavefront part
    empty.  Same algorithm as the one-problem-per-wavefront kernel; 1e-9 mm against the oracle (tests/test_gpu_lane.py)."""
    from open_kinematics_amd.batch import DeviceProgram
    from oracle.oracle import Oracle

    arrays, program = golden(name)
    pinned = program.with_line_mode("pinned")
    dp = DeviceProgram(pinned, "cuda:0")
    targets = arrays["targets_abs"][:41]
    assert dp.plan_launch(len(targets), kernel="packed")[0] == "packed"
    t = torch.as_tensor(targets, device="cuda:0")
    guard = torch.full((len(targets) + 1, pinned.n_out, 3), -7.0, dtype=torch.float64, device="cuda:0")
    packed = dp.solve(t, kernel="packed", out=guard[:-1])
    single = dp.solve(t, kernel="single")
    torch.cuda.synchronize()
    assert np.all((packed.info()["flags"] & 7) == 1)
    assert float((guard[-1] + 7.0).abs().max()) == 0.0, "wrote past the batch"
    assert float((packed.positions - single.positions).abs().max()) <= 1e-10
    orc = Oracle(pinned).sweep(targets, 1e-15, 1e-15, 1e-15, warm_start=False)
    assert np.max(np.abs(packed.positions.cpu().numpy() - orc.positions)) <= 1e-9
