"""
The quad kernels' default text (``csrc/okx_quadgen.cpp``: entry 2 of a diagonal block updated from lane 2's own register)
against the text with both switches of ``tests/test_quad_owner_lane.py`` on - the text of the commit before them: every
lane's entry kept valid behind a broadcast.  The default text performs, on the lanes whose results are read,
exactly the other text's IEEE operations on the same operands, so EVERYTHING must agree bit for bit: positions and every
info field, converged or not; the evaluated launch's metrics and tangents; the tangent kernel; okx_quad_eval's residuals,
normal equations and step.  The two texts are two separately created programs (the switches are read when a program's
kernels are generated); build() leaves both in the kernel cache.
"""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FULL = "quad_full_diag_update,quad_full_diag_rows"
INFO = [("max_residual", "f8"), ("cost", "f8"), ("last_step", "f8"), ("iterations", "i4"), ("nfev", "i4"), ("flags", "i4"), ("reserved", "i4")]
FIELDS = ("flags", "nfev", "iterations", "cost", "max_residual", "last_step")


class _BothTexts:
    """The default and the switched-text program of one constraint program, created once and closed together."""

    def __init__(self, program, roles=None):
        from open_kinematics_amd.batch import DeviceProgram

        kept = os.environ.pop("OKX_DEV", None)
        try:
            self.owner = DeviceProgram(program, "cuda:0")
            if roles is not None:
                self.owner.enable_evaluation(roles)
            os.environ["OKX_DEV"] = FULL
            self.full = DeviceProgram(program, "cuda:0")
            if roles is not None:
                self.full.enable_evaluation(roles)
        finally:
            os.environ.pop("OKX_DEV", None)
            if kept is not None:
                os.environ["OKX_DEV"] = kept
        for dp in (self.owner, self.full):
            assert dp.kernel == "quad", dp.kernel_note

    def solve(self, targets, **kw):
        """[(positions or free coordinates, info records)] of the default and of the switched text."""
        output = kw.get("output", "records")
        t = torch.as_tensor(np.ascontiguousarray(targets), device="cuda:0")
        results = []
        for dp in (self.owner, self.full):
            res = dp.solve(t, predictor=False, kernel="quad", **kw)
            torch.cuda.synchronize()
            pos = (res.positions if output == "records" else res.free).cpu().numpy()
            results.append((pos, np.frombuffer(res.info_raw.cpu().numpy().tobytes(), dtype=INFO).copy()))
        return results

    def close(self):
        self.owner.close()
        self.full.close()


def _assert_identical(owner, full):
    (po, io), (pf, if_) = owner, full
    for field in FIELDS:
        assert np.array_equal(io[field], if_[field], equal_nan=True), field
    assert np.array_equal(po, pf, equal_nan=True)
    return (if_["flags"] & 7) == 1


@pytest.fixture(scope="module")
def double_wishbone():
    from open_kinematics_amd.workloads import bump_sweep_problem

    both = _BothTexts(bump_sweep_problem(4)[0])
    assert both.owner.has_cold_body and both.full.has_cold_body
    yield both
    both.close()


def test_double_wishbone_17_problems(double_wishbone):
    """The second wave unit has one live quad."""
    from open_kinematics_amd.workloads import bump_sweep_problem

    assert _assert_identical(*double_wishbone.solve(bump_sweep_problem(17)[1], chain_len=1)).all()


@pytest.mark.parametrize("options", [dict(chain_len=1), dict(chain_len=4), dict(chain_len=4, shared_first_step=False),
                                     dict(chain_len=1, output="free")],
                         ids=["cold", "general_chains_of_4", "no_shared_first_step", "free_output"])
def test_double_wishbone_64_problems(double_wishbone, options):
    from open_kinematics_amd.workloads import bump_sweep_problem

    assert _assert_identical(*double_wishbone.solve(bump_sweep_problem(64)[1], **options)).all()


def test_a_nan_target_and_a_target_beyond_reach(double_wishbone):
    """The fast loop's hand-over to the general loop, rejected steps and failed factorisations: flags, evaluation counts
    and whatever positions were left are the same."""
    from open_kinematics_amd.workloads import bump_sweep_problem

    targets = np.array(bump_sweep_problem(17)[1], dtype=np.float64, copy=True)
    targets[5, -1] = np.nan
    targets[11, -1] += 4000.0                                    # (mm of wheel travel: many times the links' length)
    for chain_len in (1, 4):
        ok = _assert_identical(*double_wishbone.solve(targets, chain_len=chain_len))
        assert not ok[5] and not ok[11] and ok[:5].all()


def test_macpherson_17_problems():
    from open_kinematics_amd.workloads import macpherson_grid_problem

    program, targets = macpherson_grid_problem(6, 3)
    both = _BothTexts(program)
    try:
        for chain_len in (1, 4):
            assert _assert_identical(*both.solve(targets[:17], chain_len=chain_len)).all()
    finally:
        both.close()


def test_pair_mode_rocker_axle_9_problems():
    from open_kinematics_amd.workloads import axle_grid_problem

    program, targets = axle_grid_problem(3, 3)
    both = _BothTexts(program)
    try:
        for chain_len in (1, 4):
            assert _assert_identical(*both.solve(targets, chain_len=chain_len)).all()
    finally:
        both.close()


def test_the_evaluated_launch_and_the_tangent_kernel():
    """17 double-wishbone states: the evaluation epilogue's undamped factorisation (metrics, derivative columns, tangents)
    and okx_tangent_batch on the solved states."""
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.workloads import bump_sweep_problem, geometry_path

    program, targets = bump_sweep_problem(17)
    both = _BothTexts(program, corner_roles(load_geometry(geometry_path("geometry.yaml")), program))
    try:
        t = torch.as_tensor(np.ascontiguousarray(targets), device="cuda:0")
        results = []
        for dp in (both.owner, both.full):
            res = dp.solve_evaluated(t, tangents=True, predictor=False, kernel="quad", chain_len=1)
            tan, tinfo = dp.tangents(res.positions)
            torch.cuda.synchronize()
            results.append([v.cpu().numpy() for v in (res.positions, res.info_raw, res.eval, res.tangents, tan, tinfo)])
        for o, f in zip(*results):
            assert np.array_equal(o, f, equal_nan=True)
        assert np.isfinite(results[0][3]).all() and np.abs(results[0][4]).max() > 0.0
    finally:
        both.close()


def test_every_row_class_through_the_evaluation_hook(golden):
    """okx_quad_eval on one row of each constraint class: residuals, J^T J (whole diagonal blocks), J^T r and the step."""
    arrays, program = golden("rows_all_classes")
    x, t = arrays["eval_x"], arrays["eval_targets"]
    both = _BothTexts(program)
    try:
        owner = [v.cpu().numpy() for v in both.owner.quad_eval(x, t, 1.0)]
        full = [v.cpu().numpy() for v in both.full.quad_eval(x, t, 1.0)]
    finally:
        both.close()
    assert len(owner) == 4
    for o, f in zip(owner, full):
        assert np.array_equal(o, f)
    assert np.isfinite(owner[3]).all()                           # (the damped factorisation went through: a real step)
