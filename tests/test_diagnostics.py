"""Sweep diagnostics without a GPU: the NumPy path against the reference's own ``diagnose_sweep`` (fixtures
``tests/golden/diagnostics_*.npz``, written by ``tools/gen_golden_diagnostics.py``), the boundary types, the drop-in flag."""

import dataclasses
import glob
import os

import numpy as np
import pytest

from conftest import REPO
from open_kinematics_amd import diagnostics as dg

FIXTURES = sorted(os.path.basename(p)[len("diagnostics_"):-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "diagnostics_*.npz")))


def load_case(name):
    with np.load(os.path.join(REPO, "tests", "golden", f"diagnostics_{name}.npz"), allow_pickle=False) as data:
        return {k: data[k] for k in data.files}


def case_roles(case, index=None) -> dg.DiagRoles:
    """The roles of a fixture over its own point order (or over ``index``: name -> point index)."""
    names = [str(n) for n in case["point_names"]]
    index = index or {n: i for i, n in enumerate(names)}
    free = [str(n) for n in case["free_names"]]
    roles = dg.DiagRoles([index[n] for n in free], [n.upper() for n in free])
    if "center_arb_u_bar_axis_a" in index:
        for side in ("left", "right"):
            entry = {"droplink_rocker": index[f"{side}_droplink_rocker"], "droplink_u_bar": index[f"{side}_droplink_u_bar"]}
            group = ("rocker_axis_a", "rocker_axis_b", "pushrod_inboard", "pushrod_outboard")
            if all(f"{side}_{g}" in index for g in group):
                entry.update({g: index[f"{side}_{g}"] for g in group})
            roles.sides.append(entry)
        roles.bar_axis_a, roles.bar_axis_b = index["center_arb_u_bar_axis_a"], index["center_arb_u_bar_axis_b"]
    return roles


def assert_issues_match(issues, case):
    """Same count, order, (step, category, severity), message text; values to relative 1e-12."""
    assert len(issues) == len(case["issue_step"])
    for k, issue in enumerate(issues):
        assert (issue.step, issue.category, issue.severity) == (int(case["issue_step"][k]), str(case["issue_category"][k]),
                                                                str(case["issue_severity"][k])), k
        assert issue.message == str(case["issue_message"][k]), k
        want = float(case["issue_value"][k])
        if np.isnan(want):
            assert issue.value is None
        else:
            assert abs(issue.value - want) <= 1e-12 * abs(want), (k, issue.value, want)


def test_fixture_inventory():
    assert len(FIXTURES) >= 16
    counts = {name: len(load_case(name)["issue_step"]) for name in ("c4_macpherson_grid", "c3_axle_grid", "c1_dw_corner")}
    assert counts == {"c4_macpherson_grid": 66, "c3_axle_grid": 270, "c1_dw_corner": 0}


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_path_reports_the_reference_issues(name):
    case = load_case(name)
    roles = case_roles(case)
    summary, records = dg.diagnose_arrays(case["positions"], roles, case["design"], converged=case["converged"],
                                          max_residual=case["max_residual"])
    assert_issues_match(dg.issues_from_records(records, roles), case)
    cats = list(dg.DIAG_CATEGORIES)
    for c, category in enumerate(cats):
        steps = [int(s) for s, k in zip(case["issue_step"], case["issue_category"]) if str(k) == category.value]
        assert summary["n_issues"][0, c] == len(steps)
        assert summary["first_step"][0, c] == (min(steps) if steps else -1)


def test_exact_median_of_positive_displacements():
    import statistics

    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 8, 9, 64, 255):
        d = rng.uniform(0.0, 3.0, size=(7, n))
        d[rng.uniform(size=d.shape) < 0.3] = 0.0
        d[0] = 0.0
        d[1, : n // 2] = d[1, 0]  # ties
        got = dg.positive_median(d)
        for row, value in zip(d, got):
            positive = [float(v) for v in row if v > 0]
            assert value == (statistics.median(positive) if positive else 0.0)


def test_boundary_types():
    assert dg.DiagnosticCategory.JUMP == "jump" and dg.DiagnosticCategory.CHIRALITY == "chirality"
    assert [c.value for c in dg.DiagnosticCategory] == ["convergence", "residual", "jump", "derivatives", "diagnostics", "reference",
                                                        "chirality", "transmission"]
    assert dg.DiagnosticSeverity.WARNING == "warning" and dg.DiagnosticSeverity.ERROR == "error"
    warn = dg.DiagnosticIssue(3, dg.DiagnosticCategory.JUMP, dg.DiagnosticSeverity.WARNING, "w", 1.0)
    err = dg.DiagnosticIssue(None, dg.DiagnosticCategory.RESIDUAL, dg.DiagnosticSeverity.ERROR, "e", None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        warn.step = 4
    report = dg.SweepDiagnostics([warn, err])
    assert report.warnings == [warn] and report.errors == [err] and not report.ok
    assert dg.SweepDiagnostics([warn]).ok


def _suspension_and_states(case_name, golden):
    import yaml

    from open_kinematics_amd.input import build_suspension, build_sweep
    from open_kinematics_amd.state import Point3, SuspensionState
    from types import SimpleNamespace

    case = load_case(case_name)
    arrays, _ = golden(str(case["base"]))
    sus = build_suspension(yaml.safe_load(str(arrays["geometry_yaml"])))
    design = sus.initial_state()
    from open_kinematics_amd.program import key_name

    keys = {key_name(k): k for k in design.positions}
    states = [SuspensionState({keys[str(n)]: Point3(row[i]) for i, n in enumerate(case["point_names"])}, set(design.free_points))
              for row in case["positions"]]
    stats = [SimpleNamespace(converged=bool(c), nfev=1, max_residual=float(r)) for c, r in zip(case["converged"], case["max_residual"])]
    return case, sus, states, stats


@pytest.mark.parametrize("name", ["axle_transmission", "axle_snap", "stats", "corner_even", "one_state"])
def test_diagnose_sweep_on_states(golden, name):
    case, sus, states, stats = _suspension_and_states(name, golden)
    assert_issues_match(dg.diagnose_sweep(sus, states, stats, device="cpu").issues, case)


def test_evaluated_sweep_orders_and_swallows(golden, monkeypatch):
    from open_kinematics_amd import sweep as sw

    case, sus, states, stats = _suspension_and_states("stats", golden)
    advisory = sw.DerivativeIssue(None, "advisory")
    metrics = sw.SweepMetricsResult([{} for _ in states])
    monkeypatch.setattr(sw, "_derivative_issues", lambda result: [advisory])
    monkeypatch.setattr(sw, "compute_sweep_metrics", lambda *a, **k: metrics)
    plain = sw.evaluate_solved_sweep(sus, None, states, stats, device="cpu")
    assert plain.diagnostics == [advisory]  # the default: what it returned before
    full = sw.evaluate_solved_sweep(sus, None, states, stats, device="cpu", diagnose=True)
    assert full.diagnostics[-1] is advisory
    assert_issues_match(full.diagnostics[:-1], case)

    def boom(*a, **k):
        raise RuntimeError("no luck")

    monkeypatch.setattr(dg, "diagnose_sweep", boom)
    failed = sw.evaluate_solved_sweep(sus, None, states, stats, device="cpu", diagnose=True)
    assert len(failed.diagnostics) == 2 and failed.diagnostics[1] is advisory
    first = failed.diagnostics[0]
    assert (first.step, first.category, first.severity, first.value) == (None, "diagnostics", "warning", None)
    assert first.message == "Sweep diagnostics unavailable: diagnostic evaluation failed (RuntimeError: no luck)."
