"""
lean_atan2_pos of the quad kernels (``csrc/okx_quadgen.cpp``) as one instruction stream: the five ranges of its argument
reduction select their constants instead of branching (the default text; ``OKX_DEV=quad_atan_branches`` restores the
if / else chain).  64 states of the all-row-classes program put ``t = y / |x|`` of BOTH angle rows (the four-point angle row
3 and the three-point angle row 4) into each of the five ranges, just below and just above each boundary (0.4375, 0.6875,
1.1875, 2.4375), with both signs of ``x``, and onto the early returns (``y <= 0`` with ``x > 0`` and ``x < 0``; ``x = 0``).

* the oracle alone, on the CPU, shows that the states cover all of that (no GPU);
* ``okx_quad_eval``: residuals against the oracle at tests/test_gpu_parity.py's tolerance for residuals, the normal equations
  (the hook returns J^T J and J^T r, not J) at tests/test_gpu_quad.py's, and everything bit for bit between the two texts;
* a 64-problem cold solve of the program: positions and every info field bit for bit between the two texts.
"""

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

BRANCHES = "quad_atan_branches"
BOUNDS = (0.4375, 0.6875, 1.1875, 2.4375)
# one value inside each range, one on either side of each boundary (a part in a thousand away: the rows' t differs from
# tan(angle) by EPS / |v1 x v2| ~ 1e-9 relative, the oracle's from the device's by rounding)
T_VALUES = [0.2, 0.55, 0.9, 1.8, 5.0, 50.0] + [b * (1.0 + s * 1e-3) for b in BOUNDS for s in (-1.0, 1.0)]
ANGLE_ROWS = (3, 4)  # OKX_ROW_ANGLE on points (0, 3, 4, 7); OKX_ROW_THREE_POINT_ANGLE on points (3, 4, 1)
INFO = [("max_residual", "f8"), ("cost", "f8"), ("last_step", "f8"), ("iterations", "i4"), ("nfev", "i4"), ("flags", "i4"), ("reserved", "i4")]
FIELDS = ("flags", "nfev", "iterations", "cost", "max_residual", "last_step")


def _unit(v):
    return v / np.linalg.norm(v)


def _perp(u, rng):
    w = rng.standard_normal(3)
    return _unit(w - np.dot(w, u) * u)


def angle_states(program):
    """``x [64, 15]``: the free points (3, 4, 5, 6, 7) of 64 states.  Row 3's angle is between p3 - p0 and p7 - p4, row 4's
    between p3 - p4 and p1 - p4 (p0, p1 fixed): p3 is placed around p4 for row 4's angle, then p7 around p4 for row 3's."""
    assert list(program.free_point) == [3, 4, 5, 6, 7]
    assert [int(program.row_type[i]) for i in ANGLE_ROWS] == [2, 3]
    assert [list(program.row_pts[3]), list(program.row_pts[4][:3])] == [[0, 3, 4, 7], [3, 4, 1]]
    rng = np.random.default_rng(20240607)
    design = np.asarray(program.design_pos, dtype=np.float64)
    angles = [np.arctan(t) if sign > 0 else np.pi - np.arctan(t) for t in T_VALUES for sign in (1, -1)]  # 28
    states = []

    def state(p3, p4, p7):
        pos = design.copy()
        pos[3], pos[4], pos[7] = p3, p4, p7
        states.append(pos[[3, 4, 5, 6, 7]].ravel())

    for rnd in range(2):  # 56 states: row 3 walks the list forwards, row 4 backwards; two frames and sets of lengths
        for k, theta in enumerate(angles):
            phi = angles[len(angles) - 1 - k]
            p4 = design[4] + rng.uniform(-20.0, 20.0, 3)
            a = _unit(design[1] - p4)
            p3 = p4 + rng.uniform(80.0, 160.0) * (np.cos(phi) * a + np.sin(phi) * _perp(a, rng))
            u = _unit(p3 - design[0])
            state(p3, p4, p4 + rng.uniform(80.0, 160.0) * (np.cos(theta) * u + np.sin(theta) * _perp(u, rng)))
    # the early returns, with exact zeros: vectors along coordinate axes (a difference of equal coordinates is 0)
    p4 = np.array([-140.0, -30.0, 10.0])
    # row 3: v1 = p3 - p0 = (length', 0, 0); v2 parallel, antiparallel (y <= 0), perpendicular (x = 0)
    for length, v2 in ((100.0, [80.0, 0.0, 0.0]), (100.0, [-80.0, 0.0, 0.0]), (100.0, [0.0, 80.0, 0.0]), (37.0, [3.0, 0.0, 0.0]), (37.0, [-250.0, 0.0, 0.0])):
        state(design[0] + np.array([length, 0.0, 0.0]), p4, p4 + np.array(v2))
    for v1 in ([0.0, 0.0, 50.0], [0.0, 0.0, -50.0], [60.0, 0.0, 0.0]):  # row 4: v2 = p1 - p4 = (0, 0, 70')
        p4 = design[1] - np.array([0.0, 0.0, 70.0])
        state(p4 + np.array(v1), p4, design[7])
    x = np.ascontiguousarray(np.stack(states))
    assert x.shape == (64, program.n_vars)
    return x


def covered(program, x, targets):
    """{row: set of (range 0..4, sign of x) and of 'zero+' / 'zero-' / 'right'} from the ORACLE's residuals alone."""
    from oracle.oracle import Oracle

    r_o, _ = Oracle(program).eval(x, targets)
    seen = {}
    for row in ANGLE_ROWS:
        angle = r_o[:, row] + float(program.row_param[row][0])
        cases = set()
        for a in angle:
            if abs(a) < 1e-12:
                cases.add("zero+")
            elif abs(a - np.pi) < 1e-12:
                cases.add("zero-")
            elif abs(a - 0.5 * np.pi) < 1e-12:  # (the nearest range state is atan(50): 0.02 away)
                cases.add("right")
            else:
                t = abs(np.tan(a))
                below = [t < b for b in BOUNDS]
                cases.add((below.index(True) if any(below) else 4, 1 if a < 0.5 * np.pi else -1))
                for b in BOUNDS:  # either side of a boundary, closer than 0.2 %
                    if abs(t / b - 1.0) < 2e-3:
                        cases.add(("near", b, t < b, 1 if a < 0.5 * np.pi else -1))
        seen[row] = cases
    return seen


def test_the_states_cover_every_range_boundary_sign_and_early_return(golden):
    """CPU only, the oracle alone."""
    arrays, program = golden("rows_all_classes")
    x = angle_states(program)
    seen = covered(program, x, np.repeat(arrays["eval_targets"][:1], len(x), axis=0))
    want = {(k, s) for k in range(5) for s in (1, -1)} | {("near", b, side, s) for b in BOUNDS for side in (True, False) for s in (1, -1)}
    want |= {"zero+", "zero-", "right"}
    for row in ANGLE_ROWS:
        assert want <= seen[row], (row, sorted(map(str, want - seen[row])))


class _BothTexts:
    def __init__(self, program):
        from open_kinematics_amd.batch import DeviceProgram

        kept = os.environ.pop("OKX_DEV", None)
        try:
            self.selects = DeviceProgram(program, "cuda:0")
            os.environ["OKX_DEV"] = BRANCHES
            self.branches = DeviceProgram(program, "cuda:0")
        finally:
            os.environ.pop("OKX_DEV", None)
            if kept is not None:
                os.environ["OKX_DEV"] = kept
        for dp in (self.selects, self.branches):
            assert dp.kernel == "quad", dp.kernel_note

    def close(self):
        self.selects.close()
        self.branches.close()


@pytest.fixture(scope="module")
def both(golden):
    _, program = golden("rows_all_classes")
    texts = _BothTexts(program)
    yield texts
    texts.close()


@pytest.mark.gpu
def test_rows_and_normal_equations_in_every_range(golden, both):
    from oracle.oracle import Oracle

    arrays, program = golden("rows_all_classes")
    x = angle_states(program)
    t = np.repeat(arrays["eval_targets"][:1], len(x), axis=0)
    r_o, jac_o = Oracle(program).eval(x, t)
    ata_o = np.einsum("bij,bik->bjk", jac_o, jac_o)
    atr_o = np.einsum("bij,bi->bj", jac_o, r_o)
    lam = 1e-6 * float(np.max(np.diagonal(ata_o, axis1=1, axis2=2)))
    selects = [v.cpu().numpy() for v in both.selects.quad_eval(x, t, lam)]
    branches = [v.cpu().numpy() for v in both.branches.quad_eval(x, t, lam)]
    r, ata, atr, _ = selects
    err = np.abs(r - r_o)
    print("angle rows: max |r - oracle| =", err[:, list(ANGLE_ROWS)].max(axis=0), " all rows:", err.max(),
          " J^T J:", np.max(np.abs(ata - ata_o)) / max(1.0, np.abs(ata_o).max()), " J^T r:", np.max(np.abs(atr - atr_o)) / max(1.0, np.abs(atr_o).max()))
    for s, b in zip(selects, branches):
        assert np.array_equal(s, b, equal_nan=True)
    assert np.all(err <= 2.5e-13 + 1e-13 * np.abs(r_o))
    assert np.max(np.abs(ata - ata_o)) <= 1e-11 * max(1.0, np.abs(ata_o).max())
    assert np.max(np.abs(atr - atr_o)) <= 1e-11 * max(1.0, np.abs(atr_o).max())


@pytest.mark.gpu
def test_cold_solves_are_bit_identical_between_the_two_texts(golden, both):
    arrays, _ = golden("rows_all_classes")
    base = np.asarray(arrays["eval_targets"][0], dtype=np.float64)
    grid = np.stack(np.meshgrid(np.linspace(-12.0, 12.0, 8), np.linspace(-12.0, 12.0, 8), indexing="ij"), axis=-1).reshape(64, 2)
    targets = torch.as_tensor(np.ascontiguousarray(base + grid), device="cuda:0")
    results = []
    for dp in (both.selects, both.branches):
        res = dp.solve(targets, predictor=False, kernel="quad", chain_len=1)
        torch.cuda.synchronize()
        results.append((res.positions.cpu().numpy(), np.frombuffer(res.info_raw.cpu().numpy().tobytes(), dtype=INFO).copy()))
    (ps, infos), (pb, infob) = results
    for field in FIELDS:
        assert np.array_equal(infos[field], infob[field], equal_nan=True), field
    assert np.array_equal(ps, pb, equal_nan=True)
    print("converged:", int(((infos["flags"] & 7) == 1).sum()), "of 64; nfev", infos["nfev"].min(), "...", infos["nfev"].max())
    assert (infos["nfev"] >= 1).all()
