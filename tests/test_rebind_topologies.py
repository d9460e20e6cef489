"""
Per-geometry problem emission of the ORACLE (``okx_oracle_rebind``) against the real reference on every topology: the
``rebind_<name>.npz`` fixtures hold, for four perturbed geometries of each, the table a caller would pass (derived entries
poisoned with a sentinel) and what the reference's own ``constraints()`` / ``derived_spec()`` emit at that geometry
(oracle/gen_golden_rebind.py).  tests/test_gpu_rebind_topologies.py holds the device to the same data.
"""

import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN, TOPOLOGIES
from rebind_reference import (FREE_CLAMP, G, LINE_MODES, MACPHERSON, NAMES, PARAM_REL, POS_TOL, S, TARGET_TOL,
                              all_classes_table, clamp_contract, fixture, geometries, host_targets, numpy_row_targets,
                              param_error, reference_program, sentinel_mask, table)

from oracle.oracle import Oracle


def test_fixtures_cover_every_topology():
    found = sorted(f[len("rebind_"):-len(".npz")] for f in os.listdir(GOLDEN) if f.startswith("rebind_"))
    assert found == sorted(NAMES) and set(TOPOLOGIES) <= set(NAMES)
    row_types = set()
    for name in NAMES:
        arrays, program = fixture(name)
        p, mc, t = program.n_points, program.n_rows, program.n_targets
        assert arrays["hardpoints"].shape == arrays["design_pos"].shape == (G, p, 3)
        assert arrays["row_param"].shape == (G, mc, 8) and arrays["dop_param"].shape == (G, program.n_derived)
        assert arrays["targets_abs"].shape == (G, S, t) and arrays["targets_rel"].shape == (S, t)
        assert arrays["ref_tight_pos"].shape == (G, S, program.n_out, 3) and arrays["ref_tight_maxres"].shape == (G, S)
        assert float(arrays["sigma"]) == 0.5   # no topology needed a smaller perturbation
        # the base program is the one of <name>.npz, array for array: the same generated kernels, the same kernel cache entries
        base = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
        assert all(np.array_equal(arrays[k], base[k]) for k in arrays if k.startswith("prog_"))
        # geometry 0 is the program's own; the others moved, by a perturbation of the recorded size
        assert np.array_equal(arrays["design_pos"][0], program.design_pos)
        assert np.array_equal(arrays["row_param"][0], program.row_param)
        moved = np.abs(arrays["design_pos"][1:] - program.design_pos).max(axis=(1, 2))
        assert np.all(moved > 0.5) and np.all(moved < 6 * 0.5 * 2)
        # the table: authored coordinates where the reference has them, the sentinel at every other derived entry
        mask = sentinel_mask(name)
        assert mask.any() and np.all(arrays["hardpoints"][mask] == float(arrays["sentinel"]))
        assert np.array_equal(arrays["hardpoints"][:, program.role != 2], arrays["design_pos"][:, program.role != 2])
        row_types |= set(int(v) for v in program.row_type)
    assert row_types >= {0, 2, 8, 10, 12}   # distance, angle, point on line, midpoint on plane, triple product


@pytest.mark.parametrize("line_mode", LINE_MODES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_rebind_matches_reference_emission(name, line_mode):
    arrays, program = fixture(name)
    orc = Oracle(program.with_line_mode(line_mode))
    worst_pos, worst_param = 0.0, 0.0
    for g in geometries(name):
        pos, rp = orc.rebind(arrays["hardpoints"][g])
        ref = reference_program(name, g, line_mode)
        worst_pos = max(worst_pos, float(np.max(np.abs(pos - ref.design_pos))))
        worst_param = max(worst_param, param_error(rp, ref.row_param))
    print(f"rebind {name} {line_mode}: positions {worst_pos:.2e} (<= {POS_TOL}), row parameters {worst_param:.2e} (<= {PARAM_REL})")
    assert worst_pos <= POS_TOL
    assert worst_param <= PARAM_REL


@pytest.mark.parametrize("line_mode", LINE_MODES)
@pytest.mark.parametrize("name", NAMES)
def test_sentinel_does_not_leak(name, line_mode):
    """Derived entries of the table are ignored: finite outputs, the same bits whatever stands there."""
    _, program = fixture(name)
    orc = Oracle(program.with_line_mode(line_mode))
    first, second = table(name), table(name, sentinel=-3.0e5)
    assert not np.array_equal(first, second)
    for g in range(G):
        pos_a, rp_a = orc.rebind(first[g])
        pos_b, rp_b = orc.rebind(second[g])
        assert np.all(np.isfinite(pos_a)) and np.all(np.isfinite(rp_a))
        assert np.abs(pos_a).max() < 1e4, "the sentinel reached an output"
        assert pos_a.tobytes() == pos_b.tobytes() and rp_a.tobytes() == rp_b.tobytes()


@pytest.mark.parametrize("line_mode", LINE_MODES)
@pytest.mark.parametrize("name", NAMES)
def test_tight_sweep_of_the_rebound_program_matches_reference(name, line_mode):
    arrays, program = fixture(name)
    program = program.with_line_mode(line_mode)
    orc = Oracle(program)
    bound = 1e-9 if name.startswith("u_") else 1e-7
    worst = 0.0
    for g in geometries(name):
        pos, rp = orc.rebind(arrays["hardpoints"][g])
        rebound = dataclasses.replace(program, design_pos=pos, row_param=rp)
        res = Oracle(rebound).sweep(arrays["targets_abs"][g], 1e-15, 1e-15, 1e-15)
        assert res.first_failed_step == -1
        worst = max(worst, float(np.max(np.abs(res.positions - arrays["ref_tight_pos"][g]))))
    print(f"oracle sweep {name} {line_mode}: {worst:.2e} (<= {bound})")
    assert worst <= bound


@pytest.mark.parametrize("name", NAMES)
def test_absolute_targets_from_rebound_positions(name):
    """convert_targets_to_absolute of the perturbed suspension = the geometry's own design coordinate + the displacement."""
    arrays, program = fixture(name)
    orc = Oracle(program)
    worst = 0.0
    for g in range(G):   # the target points do not hang off the strut clamp: every geometry
        pos, _ = orc.rebind(arrays["hardpoints"][g])
        worst = max(worst, float(np.max(np.abs(host_targets(program, pos, arrays["targets_rel"]) - arrays["targets_abs"][g]))))
    assert worst <= TARGET_TOL


@pytest.mark.parametrize("name", MACPHERSON)
def test_macpherson_clamp_offset_is_a_program_constant(name):
    """
    The reference reads the clamp offset d off the AUTHORED clamp; rebind keeps the program's d0 and ignores the entry.
    Geometry 3 moved the clamp freely: the rebound clamp is at LBJ + axis d0 and |d_ref - d0| along the axis from the
    reference's, every point that does not hang off it agrees with the reference, and ``strict`` says so.
    """
    arrays, program = fixture(name)
    pos, rp = Oracle(program).rebind(arrays["hardpoints"][FREE_CLAMP])
    contract = clamp_contract(name, pos)
    print(f"clamp {name}: |d_ref - d0| = {contract['offset_difference']}, rebound clamp against LBJ + axis d0 "
          f"{contract['on_axis']:.2e}, against reference + axis (d0 - d_ref) {contract['from_reference']:.2e}")
    assert min(contract["offset_difference"]) > 1e-3, "the fixture's free clamp does not leave the program's offset"
    assert contract["on_axis"] <= 1e-12
    assert contract["from_reference"] <= 1e-12
    clamps = [int(k) for k in arrays["clamp_points"]]
    assert program.authored_derived_points() == clamps
    others = np.setdiff1d(np.arange(program.n_points), clamps)
    assert np.max(np.abs(pos[others] - arrays["design_pos"][FREE_CLAMP][others])) <= POS_TOL
    clear = ~np.isin(program.row_pts, clamps).any(axis=1)
    assert clear.sum() < program.n_rows and param_error(rp[clear], arrays["row_param"][FREE_CLAMP][clear]) <= PARAM_REL
    assert param_error(rp[~clear], arrays["row_param"][FREE_CLAMP][~clear]) > 1e-6   # the rows on the clamp do differ
    # strict: the freely moved clamp is refused, the re-placed ones (and a table of any other topology) pass
    with pytest.raises(ValueError, match="strut_bottom"):
        program.check_authored_derived(arrays["hardpoints"][FREE_CLAMP], pos)
    for g in geometries(name):
        program.check_authored_derived(arrays["hardpoints"][g], Oracle(program).rebind(arrays["hardpoints"][g])[0])


def test_strict_check_has_nothing_to_say_without_authored_derived_points():
    arrays, program = fixture("t_corner_rocker")
    assert program.authored_derived_points() == []
    program.check_authored_derived(arrays["hardpoints"], arrays["design_pos"])


@pytest.mark.parametrize("line_mode", ["softnorm", "pinned"])
def test_every_row_class_rebinds_to_its_definition(golden, line_mode):
    """No reference topology emits a three-point angle row: the synthetic program with one row of every class, against the
    reference's definitions written out in extended precision."""
    _, program = golden("rows_all_classes")
    program = program.with_line_mode(line_mode)
    assert 3 in program.row_type and program.n_derived == 0
    for hard in all_classes_table():
        pos, rp = Oracle(program).rebind(hard)
        assert np.array_equal(pos, hard)
        assert param_error(rp, numpy_row_targets(program, hard)) <= PARAM_REL
