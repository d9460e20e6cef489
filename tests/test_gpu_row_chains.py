"""
The quad kernels with batched norm chains (the default text of ``csrc/okx_quadgen.cpp``: four rows' `+ EPS_SQ`,
fast_sqrt_rsqrt, `- EPS` chains run as ONE chain on the four lanes of a quad) against the serial text
(``OKX_DEV=quad_serial_chains``: every lane runs every row's chain) on the same inputs.  A batch performs, per row, exactly
the serial text's IEEE operations on the serial text's inputs, so EVERYTHING must agree bit for bit: positions and every info
field - flags, nfev, iterations, cost, max_residual, last_step - converged or not.  The two texts are two separately created
programs (the switch is read when a program's kernels are generated); build() leaves both in the kernel cache.

Remainders of the last batch (rows whose chains are batched: distance, spherical, angle, three-point angle), by fixture:
  0  the double wishbone corner (bump sweep / c1_dw_corner: 15 distance + 1 angle = 16) and the MacPherson corner (12)
  1  the half program of the rocker axle (c3_axle_grid, pair mode: 28 distance + 1 angle = 29; a batch of one stays serial)
  2  t_corner_strut_rocker (25 distance + 1 angle = 26)
  3  t_corner_rocker (22 + 1 = 23) and rows_all_classes (4 distance + spherical + angle + three-point angle = 7)
"""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SERIAL = "quad_serial_chains"
INFO = [("max_residual", "f8"), ("cost", "f8"), ("last_step", "f8"), ("iterations", "i4"), ("nfev", "i4"), ("flags", "i4"), ("reserved", "i4")]
FIELDS = ("flags", "nfev", "iterations", "cost", "max_residual", "last_step")
CHAIN_ROW_TYPES = (0, 1, 2, 3)


class _BothTexts:
    """The default and the serial-text program of one constraint program, created once and closed together."""

    def __init__(self, program):
        from open_kinematics_amd.batch import DeviceProgram

        kept = os.environ.pop("OKX_DEV", None)
        try:
            self.batched = DeviceProgram(program, "cuda:0")
            os.environ["OKX_DEV"] = SERIAL
            self.serial = DeviceProgram(program, "cuda:0")
        finally:
            os.environ.pop("OKX_DEV", None)
            if kept is not None:
                os.environ["OKX_DEV"] = kept
        for dp in (self.batched, self.serial):
            assert dp.kernel == "quad", dp.kernel_note

    def solve(self, targets, **kw):
        """[(positions or None, info records)] of the batched and of the serial text."""
        output = kw.get("output", "records")
        t = torch.as_tensor(np.ascontiguousarray(targets), device="cuda:0")
        results = []
        for dp in (self.batched, self.serial):
            res = dp.solve(t, predictor=False, kernel="quad", **kw)
            torch.cuda.synchronize()
            pos = None if output == "none" else (res.positions if output == "records" else res.free).cpu().numpy()
            results.append((pos, np.frombuffer(res.info_raw.cpu().numpy().tobytes(), dtype=INFO).copy()))
        return results

    def close(self):
        self.batched.close()
        self.serial.close()


def _assert_identical(batched, serial):
    (pb, ib), (ps, is_) = batched, serial
    for field in FIELDS:
        assert np.array_equal(ib[field], is_[field], equal_nan=True), field
    if pb is not None:
        assert np.array_equal(pb, ps, equal_nan=True)
    return (is_["flags"] & 7) == 1


def _chain_rows(program) -> int:
    return int(sum(int(t) in CHAIN_ROW_TYPES for t in program.row_type))


@pytest.fixture(scope="module")
def double_wishbone():
    from open_kinematics_amd.workloads import bump_sweep_problem

    both = _BothTexts(bump_sweep_problem(2)[0])
    assert both.batched.has_cold_body and both.serial.has_cold_body
    yield both
    both.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_double_wishbone_sweeps_cold_and_chained_every_output(double_wishbone, n):
    """Partial quads in a wavefront, a partial last wavefront, quads that finish early while others iterate; the cold body
    (independent solves) and the general body (chains of four); records, free coordinates, no positions."""
    from open_kinematics_amd.workloads import bump_sweep_problem

    program, targets = bump_sweep_problem(n)
    assert _chain_rows(program) % 4 == 0                         # (remainder 0)
    for chain_len in (1, 4):
        for output in ("records", "free", "none"):
            ok = _assert_identical(*double_wishbone.solve(targets, chain_len=chain_len, output=output))
            assert ok.all(), (chain_len, output)


def test_a_grid_beyond_the_reach(double_wishbone):
    """64 problems out to and beyond the mechanism's limits: rejected steps, failures, and the fast loop's hand-over to the
    general loop - flags, evaluation counts and the converged positions (here: everything) are the same."""
    from open_kinematics_amd.workloads import bump_sweep_problem

    _, base = bump_sweep_problem(2)
    bump, rack = np.meshgrid(np.linspace(-260.0, 260.0, 8), np.linspace(-120.0, 120.0, 8), indexing="ij")
    t = np.stack([base[0, 0] + rack.ravel(), 0.5 * (base[0, 1] + base[1, 1]) + bump.ravel()], axis=1)
    batched, serial = double_wishbone.solve(t, chain_len=1)
    ok = _assert_identical(batched, serial)
    assert ok.any() and not ok.all()                             # the grid really reaches past the mechanism's limits
    assert (serial[1]["nfev"] > 6).any()                         # ... and some solves really needed rejected steps


def test_pair_mode_axle_grid():
    from open_kinematics_amd.workloads import axle_grid_problem

    program, targets = axle_grid_problem(8, 8)                   # (half program: 29 chains, remainder 1)
    both = _BothTexts(program)
    try:
        for chain_len in (1, 4):
            assert _assert_identical(*both.solve(targets, chain_len=chain_len)).all()
    finally:
        both.close()


def test_macpherson_grid():
    """A derived point with a norm chain of its own (the strut axis), which stays serial beside the batched rows."""
    from open_kinematics_amd.workloads import macpherson_grid_problem

    program, targets = macpherson_grid_problem(8, 4)             # 32 problems
    assert _chain_rows(program) % 4 == 0
    both = _BothTexts(program)
    try:
        for chain_len in (1, 4):
            assert _assert_identical(*both.solve(targets, chain_len=chain_len)).all()
    finally:
        both.close()


@pytest.mark.parametrize("fixture,remainder", [("c1_dw_corner", 0), ("t_corner_strut_rocker", 2), ("t_corner_rocker", 3)])
def test_every_remainder_of_the_last_batch(golden, fixture, remainder):
    """(remainder 1: test_pair_mode_axle_grid)"""
    arrays, program = golden(fixture)
    program = program.with_line_mode("pinned")
    assert _chain_rows(program) % 4 == remainder
    targets = arrays["targets_abs"].reshape(-1, program.n_targets)[:64]
    both = _BothTexts(program)
    try:
        for chain_len in (1, 4):
            assert _assert_identical(*both.solve(targets, chain_len=chain_len)).all()
    finally:
        both.close()


def test_every_row_class_through_the_evaluation_hook(golden):
    """okx_quad_eval on one row of each constraint class: residuals, J^T J, J^T r and the step are bit-equal between the
    two texts, and the residuals / normal equations stay within tests/test_gpu_quad.py's tolerance of the oracle."""
    from oracle.oracle import Oracle

    arrays, program = golden("rows_all_classes")
    assert _chain_rows(program) % 4 == 3
    x, t = arrays["eval_x"], arrays["eval_targets"]
    r_o, jac_o = Oracle(program).eval(x, t)
    ata_o = np.einsum("bij,bik->bjk", jac_o, jac_o)
    atr_o = np.einsum("bij,bi->bj", jac_o, r_o)
    lam = 1e-6 * float(np.max(np.diagonal(ata_o, axis1=1, axis2=2)))
    both = _BothTexts(program)
    try:
        batched = [v.cpu().numpy() for v in both.batched.quad_eval(x, t, lam)]
        serial = [v.cpu().numpy() for v in both.serial.quad_eval(x, t, lam)]
    finally:
        both.close()
    for b, s in zip(batched, serial):
        assert np.array_equal(b, s)
    r, ata, atr, _ = batched
    assert np.all(np.abs(r - r_o) <= 2.5e-13 + 1e-13 * np.abs(r_o))
    assert np.max(np.abs(ata - ata_o)) <= 1e-11 * max(1.0, np.abs(ata_o).max())
    assert np.max(np.abs(atr - atr_o)) <= 1e-11 * max(1.0, np.abs(atr_o).max())
