"""
tests/info_reference.py against the reference's own records: at the states the reference returned (tight and default
settings) the helper's max_residual must be the value the reference wrote down, within the row error model - on every
committed fixture that carries both.  (The reference minimises the softnorm rows; its cost is not in the fixtures.)
"""

import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from info_reference import ROW_FLOOR, ROW_REL, free_vectors, geometry_programs, reference_record, reference_records

KEYS = ("ref_tight_pos", "ref_tight_maxres", "ref_default_pos", "ref_default_maxres", "targets_abs", "prog_row_type")


def _fixtures():
    names = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(path, allow_pickle=False) as arrays:
            if all(k in arrays.files for k in KEYS):
                names.append(os.path.basename(path)[:-4])
    return names


FIXTURES = _fixtures()


def test_the_fixtures_are_found():
    assert {"c1_dw_corner", "c3_axle_grid", "c4_macpherson_grid"} <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_max_residual_at_the_references_states_is_the_references(golden, name):
    arrays, program = golden(name)
    targets = arrays["targets_abs"]
    worst = 0.0
    for setting in ("tight", "default"):
        pos, recorded = arrays[f"ref_{setting}_pos"], arrays[f"ref_{setting}_maxres"].reshape(-1)
        if "hardpoints" in arrays and pos.ndim == 4:   # geometry-major ensemble: every geometry on its own program
            g, s = pos.shape[:2]
            ref = reference_records(geometry_programs(program, arrays["hardpoints"]), s,
                                    free_vectors(program, pos.reshape(g * s, -1, 3)), targets.reshape(g * s, -1))
        else:
            ref = reference_record(program, free_vectors(program, pos), targets)
        diff = np.abs(ref.maxres - recorded)
        worst = max(worst, float(diff.max()))
        assert np.all(diff <= ROW_FLOOR + ROW_REL * recorded), (setting, float(diff.max()))
        assert np.all(ref.maxres_bound == ROW_FLOOR + ROW_REL * ref.maxres)
    print(f"{name}: worst |maxres_o - reference's| = {worst:.2e}")


def test_the_cost_bound_is_the_row_model_through_the_sum_of_squares(golden):
    """Rows moved by exactly their e_i move the cost by no more than the bound, and by most of it (the bound is not slack)."""
    arrays, program = golden("c1_dw_corner")
    pinned = program.with_line_mode("pinned")
    x = np.repeat(pinned.design_free_array()[None], 4, axis=0)
    ref = reference_record(pinned, x, arrays["targets_abs"][[0, 25, 75, 100]])
    r = ref.rows
    assert np.max(np.abs(r)) > 1.0                      # design state against swept targets: rows of tens of mm
    e = ROW_FLOOR + ROW_REL * np.abs(r)
    moved = 0.5 * np.sum((np.abs(r) + e) ** 2, axis=1)
    assert np.all(moved - ref.cost <= ref.cost_bound)
    assert np.all(moved - ref.cost >= 0.5 * ref.cost_bound)
    assert np.all(ref.cost_bound <= 1e-11 * ref.cost)   # a relative check of ~1e-12 where the rows are not small
    wide = reference_record(pinned, x, arrays["targets_abs"][[0, 25, 75, 100]], widen=np.full(4, 1e-6))
    assert np.all(wide.cost_bound > ref.cost_bound) and np.all(wide.maxres_bound == ref.maxres_bound + 1e-6)
    assert np.array_equal(wide.cost, ref.cost)
