"""
GPU: EVERY derivative column of the metric catalogs - 19 per corner from the stand-alone kernel
(okx_corner_metrics_batch) and from both forms of the evaluated module (okx_evaluate_batch, quad and lane), the 7
axle-scope rates and the rotation / hardware role rates of the evaluated axle module - against the oracle's duals (oracle/metrics_oracle.py, pinned on the CPU by
differences of its values-only path, tests/test_metrics_oracle.py), along the device's own tangents and along seeded random
velocity fields; and role sets no real corner has, which take the evaluated modules' atan2 through all of its reduction
intervals and quadrants.

Tolerances.  Values: 1e-9 relative to max(1, |ref|), the suite's.  Derivative columns: NOISE / AXLE_NOISE / ROLE_NOISE below is, per
column, the largest |float64 - 50-digit| of the ORACLE's duals relative to max(1, |d|) over the states, directions and
role sets of this module (the rounding noise of the formula itself at these states).  The stand-alone kernel (IEEE
division, libm) gets 16 x that, the evaluated modules (Newton-refined reciprocals and roots, some thirty of them chained
in an instant-centre column) 64 x; floor 1e-12, and never more than the 1e-7 the reference's own derivative columns get.
Measured on an MI355X, both implementations and both forms: at most 3e-14 on the columns held to the floor, 3.0e-12 on
fvic_z (bound 2.1e-11), 2.3e-12 on svic_z (4.2e-11), 4.9e-13 on the roll centre (4.8e-11).

Not reached: a contact patch at y < 0 in a CORNER's evaluated module (the mirrored set runs on the stand-alone kernel only:
a module reads its fixed points from the program, which cannot be mirrored with the table; the right-hand corners of the
axle fixtures reach that branch in the axle module), and y = -0.0 with x < 0, where libm's atan2 says -180 degrees and the
modules' +180.
"""

import numpy as np
import pytest
import torch

from conftest import gpu_available
from test_metrics_oracle import (
    ANTI_FIXTURES,
    AXLE_GOLDENS,
    close,
    load_metrics_golden,
    oracle_axle_rows,
    oracle_catalog_rows,
    out_names,
    spec_of_roles,
)

from oracle.metrics_oracle import (
    AXLE_METRIC_NAMES,
    C1_ROLE_SETS,
    METRIC_NAMES,
    ROLE_KINDS,
    angle_arguments,
    corner_roles_from_spec,
    role_dual,
)

pytestmark = pytest.mark.gpu

# measured by ``python -m oracle.measure_metric_noise`` (see the module docstring)
NOISE = {
    "camber": 3.3e-16, "caster": 2.2e-16, "kpi": 1.7e-16, "roadwheel_angle": 3.4e-16, "wheel_travel": 0.0, "half_track": 0.0,
    "scrub_radius": 1.7e-15, "mechanical_trail": 4.4e-16, "svic_x": 6.2e-14, "svic_z": 2.6e-12, "svsa_length": 5.5e-14,
    "fvic_y": 1.5e-14, "fvic_z": 1.3e-12, "fvsa_length": 1.5e-14, "damper_length": 4.4e-16, "svsa_angle": 1.2e-15,
    "anti_dive": 2.2e-15, "anti_lift": 5.8e-16, "anti_squat": 1.0e-14,
}
AXLE_NOISE = {"heave": 0.0, "roll": 1.0e-17, "ride_height_change": 0.0, "track": 0.0, "roll_center_y": 7.8e-13,
              "roll_center_z": 7.8e-13, "rack_displacement": 0.0}
ROLE_NOISE = {"axis_rotation": 2.2e-16, "midpoint_rotation": 1.4e-17, "stem_twist": 2.1e-17, "distance": 0.0,
              "midpoint_coordinate": 2.8e-17}
STANDALONE, EVALUATED = 16.0, 64.0
CORNER_CASES = {"c1_dw_corner": "c1_dw_corner", "c4_macpherson_grid": "c4_macpherson_grid", **ANTI_FIXTURES}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def column_bound(noise: float, factor: float) -> float:
    return min(1e-7, max(factor * noise, 1e-12))


def assert_derivative_columns(got, ref, factor, label, names=METRIC_NAMES, noise=NOISE):
    """``got`` / ``ref`` = ``[B, T, columns]``: NaN pattern equal, every column within its bound."""
    assert got.shape == ref.shape, label
    assert np.array_equal(np.isnan(got), np.isnan(ref)), label
    missed = []
    for k, name in enumerate(names):
        g, r = got[..., k], ref[..., k]
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        err = float(np.max(np.abs(g[ok] - r[ok]) / np.maximum(1.0, np.abs(r[ok]))))
        bound = column_bound(noise[name], factor)
        print(f"{label} {name}: {err:.2e} (bound {bound:.1e})")
        if not err <= bound:
            missed.append((name, err, bound))
    assert not missed, (label, missed)


def random_velocities(shape, seed):
    """A seeded velocity field ``[B, T, n_out, 3]``: no direction of it is a tangent of the mechanism."""
    return np.random.default_rng(seed).normal(0.0, 1.0, size=shape)


_cache = {}


def corner_case(golden, name):
    """(pinned program, roles, spec, states) of a corner metrics golden; the program's DeviceProgram is made per test."""
    from open_kinematics_amd.metrics import roles_from_arrays

    if name not in _cache:
        _, program = golden(CORNER_CASES[name])
        program = program.with_line_mode("pinned")
        mg = load_metrics_golden(name)
        roles, _ = roles_from_arrays(out_names(program), program.design_pos[program.out_point], mg)
        _cache[name] = (program, roles, spec_of_roles(roles), mg["pos"])
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CORNER_CASES))
def test_standalone_kernel_derivative_columns_match_the_oracle(golden, name):
    """okx_corner_metrics_batch (the tiled kernel: records of 15 points), all 19 columns, every target: along the device's
    tangents, at batch sizes around the 64-state tile, and along a random velocity field."""
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.metrics import corner_state_metrics

    program, roles, spec, states = corner_case(golden, name)
    dp = DeviceProgram(program, "cuda:0")
    pos = torch.as_tensor(states, device="cuda:0")
    tan, tinfo = dp.tangents(pos)
    res = corner_state_metrics(roles, pos, tan)
    torch.cuda.synchronize()
    assert np.all(dp.tangent_info(tinfo)["flags"] == 1)
    tan_h = tan.cpu().numpy()
    ref_v, ref_d = oracle_catalog_rows(spec, states, tan_h)
    assert close(res.values.cpu().numpy(), ref_v, 1e-9)
    assert_derivative_columns(res.derivatives.cpu().numpy(), ref_d, STANDALONE, name)
    for b in (1, 63, 64, 65):
        if b <= states.shape[0]:
            lo = states.shape[0] - b  # (the last `b` states: bases that are not tile-aligned)
            part = corner_state_metrics(roles, pos[lo:], tan[lo:])
            assert close(part.values.cpu().numpy(), ref_v[lo:], 1e-9), b
            assert_derivative_columns(part.derivatives.cpu().numpy(), ref_d[lo:], STANDALONE, (name, b))
    n = min(states.shape[0], 65)
    field = random_velocities((n,) + tan_h.shape[1:], 20)
    got = corner_state_metrics(roles, pos[:n], torch.as_tensor(field, device="cuda:0"))
    _, rnd_d = oracle_catalog_rows(spec, states[:n], field)
    assert_derivative_columns(got.derivatives.cpu().numpy(), rnd_d, STANDALONE, (name, "random field"))


def axle_case(golden, name):
    """(axle, program, dp with the axle evaluation, AxleRoles, states of the metrics golden)."""
    from test_gpu_axle_evaluated import _axle

    axle, _, program, _, dp, roles, _, _ = _axle(golden, AXLE_GOLDENS[name])
    _, fixture = golden(AXLE_GOLDENS[name])
    assert list(program.out_point) == list(fixture.out_point)
    return axle, program, dp, roles, load_metrics_golden(name)["pos"]


def test_one_thread_per_state_kernel_on_an_axle_corner(golden):
    """Records of 38 points (rec > 63 doubles): okx_corner_metrics_kernel, both corners of the rocker axle, T = 3."""
    from open_kinematics_amd.metrics import corner_state_metrics

    _, program, dp, roles, states = axle_case(golden, "axle_c3")
    assert 3 * program.n_out > 63
    pos = torch.as_tensor(states, device="cuda:0")
    tan, _ = dp.tangents(pos)
    tan_h = tan.cpu().numpy()
    field = random_velocities(tan_h.shape, 21)
    for tag, corner in (("left", roles.left), ("right", roles.right)):
        spec = spec_of_roles(corner)
        res = corner_state_metrics(corner, pos, tan)
        ref_v, ref_d = oracle_catalog_rows(spec, states, tan_h)
        assert close(res.values.cpu().numpy(), ref_v, 1e-9), tag
        assert_derivative_columns(res.derivatives.cpu().numpy(), ref_d, STANDALONE, tag)
        got = corner_state_metrics(corner, pos, torch.as_tensor(field, device="cuda:0"))
        assert_derivative_columns(got.derivatives.cpu().numpy(), oracle_catalog_rows(spec, states, field)[1], STANDALONE,
                                  (tag, "random field"))


@pytest.mark.parametrize("form", ["quad", "lane"])
@pytest.mark.parametrize("name", sorted(CORNER_CASES))
def test_evaluated_module_derivative_columns_match_the_oracle(golden, name, form, monkeypatch):
    """okx_evaluate_batch in both forms: every derivative row of the block against the oracle along the block's tangents."""
    from open_kinematics_amd.batch import DeviceProgram

    program, roles, spec, states = corner_case(golden, name)
    dp = DeviceProgram(program, "cuda:0")
    dp.enable_evaluation(roles)
    assert dp.evaluation & (1 if form == "quad" else 2), dp.evaluation_note
    monkeypatch.setenv("OKX_DEV", f"evaluate_{form}")
    res = dp.evaluate(states, tangents=True)
    torch.cuda.synchronize()
    assert np.all(res.tangent_info()["flags"] == 1)
    ref_v, ref_d = oracle_catalog_rows(spec, states, res.tangents.cpu().numpy())
    assert close(res.metrics.cpu().numpy(), ref_v, 1e-9)
    assert_derivative_columns(res.derivatives.cpu().numpy(), ref_d, EVALUATED, (name, form))


def assert_axle_scope_matches_the_oracle(res, roles, states):
    """The 7 axle-scope metrics of an evaluated axle block with their rates (``eval[:, 1:, EVAL_AXLE_METRICS:+7]``) against
    the oracle along the block's own tangents, NaN pattern included.  -> the oracle's two corner specs and the tangents."""
    from open_kinematics_amd._abi import EVAL_AXLE_METRICS

    block = res.eval.cpu().numpy()
    tan = res.tangents.cpu().numpy()
    left, right = spec_of_roles(roles.left), spec_of_roles(roles.right)
    ref_v, ref_d = oracle_axle_rows(left, right, states, tan)
    assert close(block[:, 0, EVAL_AXLE_METRICS:EVAL_AXLE_METRICS + 7], ref_v, 1e-9)
    assert_derivative_columns(block[:, 1:, EVAL_AXLE_METRICS:EVAL_AXLE_METRICS + 7], ref_d, EVALUATED, "axle scope",
                              AXLE_METRIC_NAMES, AXLE_NOISE)
    return left, right, tan


def oracle_role_rows(role, states, tan):
    """``role_dual`` of one ``okx_rotation_role`` over states x targets -> ``(values [B], derivatives [B, T])``."""
    a, b = role.point, role.point_b
    rest = (tuple(role.design), tuple(role.axis_point), tuple(role.axis_dir), role.scale)
    values, derivs = np.empty(states.shape[0]), np.empty(tan.shape[:2])
    for s in range(states.shape[0]):
        for t in range(tan.shape[1]):
            values[s], derivs[s, t] = role_dual(ROLE_KINDS[role.kind], states[s][a], tan[s, t][a], states[s][b], tan[s, t][b], *rest)
    return values, derivs


def assert_axle_block_matches_the_oracle(res, roles, states):
    """... and both corners' 19 columns of the block, and its rotation / hardware role columns."""
    from open_kinematics_amd._abi import EVAL_AXLE_ROLES

    states = np.asarray(states, dtype=np.float64)
    left, right, tan = assert_axle_scope_matches_the_oracle(res, roles, states)
    block = res.eval.cpu().numpy()
    for k in range(roles.n_roles):
        kind = ROLE_KINDS[roles.roles[k].kind]
        ref_v, ref_d = oracle_role_rows(roles.roles[k], states, tan)
        assert close(block[:, 0, EVAL_AXLE_ROLES + k], ref_v, 1e-9), (k, kind)
        assert_derivative_columns(block[:, 1:, EVAL_AXLE_ROLES + k, None], ref_d[..., None], EVALUATED, ("role", k), [kind],
                                  ROLE_NOISE)
    for s, spec in enumerate((left, right)):
        corner = res.corner(s)
        ref_v, ref_d = oracle_catalog_rows(spec, states, tan)
        assert close(corner.metrics.cpu().numpy(), ref_v, 1e-9), s
        assert_derivative_columns(corner.derivatives.cpu().numpy(), ref_d, EVALUATED, ("corner", s))


@pytest.mark.parametrize("name", ["axle_c3", "axle_t_bar_roll"])
def test_axle_scope_rates_match_the_oracle(golden, name):
    """heave, roll, ride-height change, track, roll-centre y / z and rack displacement along every target's tangent."""
    _, _, dp, roles, states = axle_case(golden, name)
    res = dp.evaluate(states, tangents=True)
    torch.cuda.synchronize()
    assert np.all(res.tangent_info()["flags"] == 1)
    assert_axle_block_matches_the_oracle(res, roles, states)


# ---- roles chosen by the test ----


def c1_role_sets(golden):
    """name -> (spec, states, velocity transform): the sets of ``C1_ROLE_SETS`` on the fixture's solved states, and the
    fixture's own roles on the MIRRORED states (y -> -y: a right-hand corner, contact patch at negative y)."""
    program, roles, spec, states = corner_case(golden, "c1_dw_corner")
    design_z = float(program.design_pos[program.out_point][spec["wheel_center"]][2])
    sets = {k: ({**v, "design_wheel_center_z": design_z}, states) for k, v in C1_ROLE_SETS.items()}
    mirror = np.array([1.0, -1.0, 1.0])
    sets["mirrored"] = ({**spec, "side": -1.0, "front_brake_bias": 0.4, "axle_position": "rear", "driven_axle": "rear"},
                        states * mirror)
    return sets


def test_role_sets_reach_every_atan2_interval_and_quadrant(golden):
    """CPU part, asserted before anything runs on the device: together the sets put the (y, x) of the four angle metrics in
    each reduction interval of the evaluated modules' atan2 (|y| / |x| < 0.4375, < 0.6875, < 1.1875, < 2.4375, beyond), in
    both signs of x and of y; one set has no instant axis, one no brake bias; both side signs; a contact patch at y < 0."""
    sets = c1_role_sets(golden)
    assert len(sets) <= 6
    intervals, x_signs, y_signs = set(), set(), set()
    for name, (spec, states) in sets.items():
        if name == "mirrored":  # (the stand-alone kernel only: libm's atan2 there)
            continue
        for row in states:
            for y, x in angle_arguments(spec, row).values():
                intervals.add(int(np.digitize(abs(y) / abs(x), [0.4375, 0.6875, 1.1875, 2.4375])))
                x_signs.add(np.sign(x))
                y_signs.add(np.sign(y))
    assert intervals == {0, 1, 2, 3, 4} and x_signs == {-1.0, 1.0} and y_signs >= {-1.0, 1.0}
    assert {spec["side"] for spec, _ in sets.values()} == {-1.0, 1.0}
    assert any(spec["front_brake_bias"] is None for spec, _ in sets.values())
    spec, states = sets["mirrored"]
    assert np.all(states[:, spec["contact_patch"], 1] < 0.0)


@pytest.mark.parametrize("name", sorted(C1_ROLE_SETS) + ["mirrored"])
def test_role_set_values_and_derivatives_match_the_oracle(golden, name, monkeypatch):
    """Stand-alone kernel and both forms of the evaluated module on one role set, values and every derivative row."""
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.metrics import corner_state_metrics

    program, _, _, solved = corner_case(golden, "c1_dw_corner")
    spec, states = c1_role_sets(golden)[name]
    roles = corner_roles_from_spec(spec)
    dp = DeviceProgram(program, "cuda:0")
    tan, _ = dp.tangents(torch.as_tensor(solved, device="cuda:0"))
    sign = states[0, spec["contact_patch"], 1] / solved[0, spec["contact_patch"], 1]  # -1: the mirrored set
    tan_h = tan.cpu().numpy() * np.array([1.0, sign, 1.0])
    ref_v, ref_d = oracle_catalog_rows(spec, states, tan_h)
    nan_columns = np.isnan(ref_v).all(axis=0)
    if name == "degenerate_plane":  # no instant axis: every instant-centre and anti column NaN, the first eight finite
        assert nan_columns[8:14].all() and nan_columns[15:].all() and np.isfinite(ref_v[:, :8]).all()
        assert np.isnan(ref_d[:, :, 8:14]).all() and np.isnan(ref_d[:, :, 15:]).all() and np.isfinite(ref_d[:, :, :8]).all()
    if name == "no_brake_bias":
        assert nan_columns[16] and nan_columns[17] and not nan_columns[18]
    res = corner_state_metrics(roles, torch.as_tensor(states, device="cuda:0"), torch.as_tensor(tan_h, device="cuda:0"))
    assert close(res.values.cpu().numpy(), ref_v, 1e-9)
    assert_derivative_columns(res.derivatives.cpu().numpy(), ref_d, STANDALONE, (name, "stand-alone"))
    if name == "mirrored":  # (the evaluated modules take their tangents from the program: its states only)
        return
    dp.enable_evaluation(roles)
    for form, bit in (("quad", 1), ("lane", 2)):
        assert dp.evaluation & bit, dp.evaluation_note
        monkeypatch.setenv("OKX_DEV", f"evaluate_{form}")
        got = dp.evaluate(states, tangents=True)
        torch.cuda.synchronize()
        ref_v, ref_d = oracle_catalog_rows(spec, states, got.tangents.cpu().numpy())
        assert close(got.metrics.cpu().numpy(), ref_v, 1e-9), form
        assert_derivative_columns(got.derivatives.cpu().numpy(), ref_d, EVALUATED, (name, form))


@pytest.mark.parametrize("form", ["quad", "lane"])
def test_exact_zero_arguments_of_atan2_from_a_hand_made_table(golden, form, monkeypatch):
    """The y == 0 and x == 0 returns of the evaluated modules' atan2: okx_evaluate_batch takes states off the constraint
    manifold, so rows of the fixture with a wheel-axis or steering-axis component set to exactly zero reach them (values;
    the moving points only - a module reads its fixed points from the program).  y = +-0 with x < 0 is taken through the
    roadwheel angle, whose y is axle.x itself: a -0.0 there would read -180 in libm and +180 in the module."""
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.metrics import corner_state_metrics

    program, roles, spec, states = corner_case(golden, "c1_dw_corner")
    ai, ao, sl, su = spec["axle_inboard"], spec["axle_outboard"], spec["steer_lower"], spec["steer_upper"]
    table = states[:6].copy()
    table[0, ao, 2] = table[0, ai, 2]        # camber: y == 0, x > 0
    table[1, ao, 1] = table[1, ai, 1]        # camber and roadwheel angle: x == 0
    table[2, su, 0] = table[2, sl, 0]        # caster: y == 0
    table[3, su, 1] = table[3, sl, 1]        # KPI: y == 0
    table[4, ao, 0] = table[4, ai, 0]        # roadwheel angle: y == 0, x > 0
    table[5, [ai, ao]] = table[5, [ao, ai]]  # the wheel axis turned round: x < 0 ...
    table[5, ao, 0] = table[5, ai, 0]        # ... and y == 0: 180 degrees
    ref_v, _ = oracle_catalog_rows(spec, table, np.zeros((6, 1, program.n_out, 3)))
    assert ref_v[0, 0] == 0.0 and abs(ref_v[1, 0]) == 90.0 and abs(ref_v[1, 3]) == 90.0 and ref_v[2, 1] == 0.0
    assert ref_v[3, 2] == 0.0 and ref_v[4, 3] == 0.0 and ref_v[5, 3] == 180.0
    dp = DeviceProgram(program, "cuda:0")
    dp.enable_evaluation(roles)
    assert dp.evaluation & (1 if form == "quad" else 2), dp.evaluation_note
    monkeypatch.setenv("OKX_DEV", f"evaluate_{form}")
    got = dp.evaluate(table, tangents=False).metrics.cpu().numpy()
    # (the four angles: a module works out the wheel centre and the contact patch from the wheel axis it is given, so the
    #  columns that use them describe another table than this one)
    assert close(got[:, :4], ref_v[:, :4], 1e-9), got[:, :4]
    alone = corner_state_metrics(roles, torch.as_tensor(table, device="cuda:0")).values.cpu().numpy()
    assert close(alone, ref_v, 1e-9)
