"""
CPU: the numpy restatement of compute_state_tangents (oracle) against the reference's own outputs - on every fixture the
reference's tangents are recorded for (oracle/gen_golden_tangents.py): the five baseline programs, the ten topologies of
conftest.TOPOLOGIES and the perturbed geometries of every ``rebind_<name>.npz``.
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN, TOPOLOGIES
from oracle.oracle import Oracle
from rebind_reference import FREE_CLAMP, G, LINE_MODES, MACPHERSON, NAMES, S, fixture, geometries, reference_program

FIXTURES = ["c1_dw_corner", "c4_macpherson_grid", "u_dw_corner", "u_macpherson", "c3_axle_grid"] + TOPOLOGIES


def load_tangent_golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"tangents_{name}.npz"), allow_pickle=False))


def free_outputs(program) -> list:
    """Index of every free point in the program's output list: a fixture's ``pos`` rows that make the free vector."""
    return [list(program.out_point).index(int(p)) for p in program.free_point]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", ["softnorm", "pinned"])
def test_oracle_tangents_match_the_reference(golden, name, mode):
    """
    softnorm = the reference's formulation (zero-gradient line row + two smooth pins,
    sensitivity.py:83-87); pinned = this build's line rows.  Both give the reference's
    velocities: the pins span the same plane with the same Gram matrix.
    """
    _, program = golden(name)
    program = program.with_line_mode(mode)
    tg = load_tangent_golden(name)
    orc = Oracle(program)
    free_out = free_outputs(program)
    assert tg["vel"].shape == (len(tg["step_index"]), program.n_targets, len(program.out_point), 3)
    worst = 0.0
    for k in range(len(tg["step_index"])):
        vel, rank, sv = orc.tangents(tg["pos"][k][free_out].reshape(-1))
        worst = max(worst, float(np.max(np.abs(vel[:, program.out_point] - tg["vel"][k]))))
        if mode == "softnorm":
            assert rank == tg["rank"][k] == program.n_vars
            assert sv[-1] == pytest.approx(tg["smallest_sv"][k], rel=1e-9)
    print(f"oracle tangents {name} {mode}: {worst:.2e} (<= 1e-12)")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", LINE_MODES)
def test_oracle_tangents_match_the_reference_on_perturbed_geometries(name, mode):
    """Every geometry of ``rebind_<name>.npz`` the program's constants can express, with that geometry's own flattened
    problem (the reference's positions and row parameters), at the states the reference's tangents were taken at."""
    arrays, base = fixture(name)
    tg = load_tangent_golden(f"rebind_{name}")
    assert tg["pos"].shape == (G, S, len(base.out_point), 3) and tg["vel"].shape == (G, S, base.n_targets, len(base.out_point), 3)
    assert np.array_equal(tg["step_index"], arrays["step_index"])
    free_out = free_outputs(base)
    worst = 0.0
    for g in geometries(name):
        orc = Oracle(reference_program(name, g, mode))
        for s in range(S):
            vel, rank, sv = orc.tangents(tg["pos"][g, s][free_out].reshape(-1))
            worst = max(worst, float(np.max(np.abs(vel[:, base.out_point] - tg["vel"][g, s]))))
            if mode == "softnorm":
                assert rank == tg["rank"][g, s] == base.n_vars
                assert sv[-1] == pytest.approx(tg["smallest_sv"][g, s], rel=1e-9)
    print(f"oracle tangents rebind_{name} {mode}: {worst:.2e} (<= 1e-12)")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", MACPHERSON)
def test_the_freely_moved_clamp_is_another_mechanism(name):
    """Geometry FREE_CLAMP moved the authored strut clamp off the program's offset d0: the reference recomputes the offset,
    the program keeps its constant (the documented contract, okx.h), so the tangents differ - by far more than rounding.
    This is why that geometry is excluded above; the assertion keeps the exclusion from hiding a fixture that silently
    stopped moving the clamp."""
    _, base = fixture(name)
    tg = load_tangent_golden(f"rebind_{name}")
    orc = Oracle(reference_program(name, FREE_CLAMP, "pinned"))
    free_out = free_outputs(base)
    gap = 0.0
    for s in range(S):
        vel, _, _ = orc.tangents(tg["pos"][FREE_CLAMP, s][free_out].reshape(-1))
        gap = max(gap, float(np.max(np.abs(vel[:, base.out_point] - tg["vel"][FREE_CLAMP, s]))))
    print(f"free clamp {name}: tangents differ by {gap:.2e} (> 1e-8)")
    assert gap > 1e-8


def test_bump_tangent_moves_the_wheel_centre_at_unit_rate(golden):
    """tests/test_sensitivity.py:86: d wheel_center.z / d bump target = 1."""
    _, program = golden("c1_dw_corner")
    tg = load_tangent_golden("c1_dw_corner")
    wc = [i for i, k in enumerate(program.out_point) if program.point_keys[k].lower_name == "wheel_center"][0]
    assert np.max(np.abs(tg["vel"][:, 1, wc, 2] - 1.0)) <= 1e-12
    assert np.max(np.abs(tg["vel"][:, 0, wc, 2])) <= 1e-12
