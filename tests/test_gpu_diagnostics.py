"""Sweep diagnostics on the device (``okx_diagnose_sweeps_batch``) against the reference's fixtures and the NumPy path."""

import numpy as np
import pytest

from conftest import load_golden
from test_diagnostics import FIXTURES, assert_issues_match, case_roles, load_case

pytestmark = pytest.mark.gpu


def _program_case(name):
    """(case, DeviceProgram, roles in program indices, records [S, n_out, 3], free [S, n_free, 3], design [P, 3])."""
    import torch

    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.program import key_name

    case = load_case(name)
    _, program = load_golden(str(case["base"]))
    names = [k if isinstance(k, str) else key_name(k) for k in program.point_keys]
    index = {n: i for i, n in enumerate(names)}
    column = {str(n): i for i, n in enumerate(case["point_names"])}
    full = np.stack([case["positions"][:, column[n]] for n in names], axis=1)  # [S, P, 3] in program point order
    design = np.stack([case["design"][column[n]] for n in names], axis=0)
    dp = DeviceProgram(program.with_line_mode("pinned"), "cuda:0", wait_for_kernels=False)
    return (case, dp, case_roles(case, index), np.ascontiguousarray(full[:, np.asarray(program.out_point)]),
            np.ascontiguousarray(full[:, np.asarray(program.free_point)]), full, design, torch)


def _info(case, torch):
    from open_kinematics_amd._abi import INFO_CONVERGED, INFO_DTYPE

    rec = np.zeros(len(case["converged"]), dtype=INFO_DTYPE)
    rec["max_residual"], rec["flags"] = case["max_residual"], np.where(case["converged"], INFO_CONVERGED, 0)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 40).copy()).cuda()


def _assert_same(dev, host):
    """Device and NumPy results: summaries equal, the same records, values to 1e-12."""
    (ds, dr), (hs, hr) = dev, host
    assert np.array_equal(ds["n_issues"], hs["n_issues"]) and np.array_equal(ds["first_step"], hs["first_step"])
    assert np.allclose(ds["worst"], hs["worst"], rtol=1e-12, atol=0, equal_nan=True)
    for f in ("sweep", "step", "category", "subject"):
        assert np.array_equal(dr[f], hr[f]), f
    assert np.allclose(dr["value"], hr["value"], rtol=1e-12, atol=0) and np.allclose(dr["threshold"], hr["threshold"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_in_both_layouts(name):
    from open_kinematics_amd import diagnostics as dg

    case, dp, roles, records, free, full, design, torch = _program_case(name)
    info = _info(case, torch)
    for layout, pos in (("records", records), ("free", free)):
        summary, recs = dp.diagnose_host(torch.from_numpy(pos).cuda(), info, steps_per_sweep=len(pos), layout=layout, roles=roles,
                                         capacity=16)
        assert_issues_match(dg.issues_from_records(recs, roles), case)
        for c in range(5):
            mine = recs[recs["category"] == c]
            assert summary["n_issues"][0, c] == len(mine)
            assert summary["first_step"][0, c] == (mine["step"].min() if len(mine) else -1)
    _assert_same((summary, recs), dg.diagnose_arrays(full, roles, design, converged=case["converged"], max_residual=case["max_residual"]))


def test_mixed_batch_matches_numpy_and_is_independent_of_batch_size():
    from open_kinematics_amd import diagnostics as dg

    parts = [_program_case(n) for n in ("axle_rocker", "axle_mirrored", "axle_boundary", "axle_snap", "axle_transmission")]
    _, dp, roles, _, _, _, design, torch = parts[0]
    rng = np.random.default_rng(11)
    pick = rng.integers(0, len(parts), size=4100)
    records = np.concatenate([parts[k][3] for k in pick])
    full = np.concatenate([parts[k][5] for k in pick])
    steps = len(parts[0][3])
    d = torch.from_numpy(records).cuda()
    whole = dp.diagnose_host(d, steps_per_sweep=steps, roles=roles)
    _assert_same(whole, dg.diagnose_arrays(full, roles, design, steps_per_sweep=steps))
    again = dp.diagnose_host(d, steps_per_sweep=steps, roles=roles)
    assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes()
    cut = 1777 * steps
    lo, hi = dp.diagnose_host(d[:cut], steps_per_sweep=steps, roles=roles), dp.diagnose_host(d[cut:], steps_per_sweep=steps, roles=roles)
    hi[1]["sweep"] += 1777
    assert np.concatenate([lo[0], hi[0]]).tobytes() == whole[0].tobytes()
    assert np.concatenate([lo[1], hi[1]]).tobytes() == whole[1].tobytes()


def test_long_sweep_with_one_spliced_snap():
    """16384 steps: the path that stages displacements in global memory; same answer as the one-workgroup path's code."""
    from open_kinematics_amd import diagnostics as dg

    case, dp, roles, records, _, full, design, torch = _program_case("c1_dw_corner")
    n = 16384
    x = np.linspace(0, len(full) - 1, n)
    lo = np.floor(x).astype(int).clip(0, len(full) - 2)
    w = (x - lo)[:, None, None]
    long_full = full[lo] * (1 - w) + full[lo + 1] * w
    p = roles.points[2]
    long_full[9000:9040, p, 1] += 12.0  # a block on another branch: a jump in, a jump out
    out_point = np.asarray(dp.program.out_point)
    got = dp.diagnose_host(torch.from_numpy(np.ascontiguousarray(long_full[:, out_point])).cuda(), steps_per_sweep=n, roles=roles)
    _assert_same(got, dg.diagnose_arrays(long_full, roles, design))
    assert [(int(r["step"]), int(r["subject"])) for r in got[1]] == [(9000, 2), (9040, 2)]


def test_capacity_smaller_than_findings_keeps_count_and_guard():
    case, dp, roles, records, _, _, _, torch = _program_case("c3_axle_grid")
    pos = torch.from_numpy(records).cuda()
    full_summary, full_records = dp.diagnose_host(pos, steps_per_sweep=len(records), roles=roles, capacity=1024)
    assert len(full_records) == 270
    buffer = torch.full((10 + 4, 40), 0xA5, dtype=torch.uint8, device="cuda")
    out = (torch.empty((1, 80), dtype=torch.uint8, device="cuda"), buffer[:10], torch.empty(1, dtype=torch.int64, device="cuda"))
    summary, issues, count = dp.diagnose(pos, steps_per_sweep=len(records), roles=roles, out=out)
    assert int(count.item()) == 270
    assert bool((buffer[10:] == 0xA5).all())
    assert summary.cpu().numpy().tobytes() == full_summary.tobytes()


def test_moving_point_outside_the_layout_is_an_error():
    import copy

    case, dp, roles, records, free, _, _, torch = _program_case("c3_axle_grid")
    moving = set(int(q) for q in dp.program.dop_out) - set(int(q) for q in dp.program.free_point)
    assert moving, "the rocker axle has derived points that are no free points"
    bad = copy.deepcopy(roles)
    bad.points[0] = sorted(moving)[0]
    with pytest.raises(ValueError, match="not part of the"):
        dp.diagnose(torch.from_numpy(free).cuda(), steps_per_sweep=len(free), layout="free", roles=bad)


def test_per_geometry_tables_give_each_geometry_its_design_sign():
    from open_kinematics_amd import diagnostics as dg

    case, dp, roles, records, _, full, design, torch = _program_case("axle_rocker")
    g, steps = 6, len(records)
    tables = np.repeat(design[None], g, axis=0).copy()
    arm = roles.sides[0]["droplink_u_bar"]
    a, b = design[roles.bar_axis_a], design[roles.bar_axis_b]
    normal = np.cross(b - a, design[roles.sides[0]["droplink_rocker"]] - a)
    normal /= np.linalg.norm(normal)
    for k in (1, 4):  # these geometries are authored on the other branch: every step of the unchanged sweep is inverted
        tables[k, arm] = design[arm] - 2.0 * float(np.dot(design[arm] - a, normal)) * normal
    pos = torch.from_numpy(np.tile(records, (g, 1, 1))).cuda()
    got = dp.diagnose_host(pos, steps_per_sweep=steps, roles=roles, geom_pos=torch.from_numpy(tables).cuda())
    _assert_same(got, dg.diagnose_arrays(np.tile(full, (g, 1, 1)), roles, tables, steps_per_sweep=steps))
    assert got[0]["n_issues"][:, dg.DIAG_CHIRALITY].tolist() == [0, steps, 0, 0, steps, 0]


def test_replays_inside_a_graph_capture():
    case, dp, roles, records, _, _, _, torch = _program_case("c4_macpherson_grid")
    pos = torch.from_numpy(records).cuda()
    eager = dp.diagnose_host(pos, steps_per_sweep=len(records), roles=roles, capacity=128)
    out = (torch.empty((1, 80), dtype=torch.uint8, device="cuda"), torch.zeros((128, 40), dtype=torch.uint8, device="cuda"),
           torch.empty(1, dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dp.diagnose(pos, steps_per_sweep=len(records), roles=roles, out=out)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dp.diagnose(pos, steps_per_sweep=len(records), roles=roles, out=out)
    from open_kinematics_amd.diagnostics import ISSUE_DTYPE, sort_records

    for _ in range(2):
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert int(out[2].item()) == 66
        assert out[0].cpu().numpy().tobytes() == eager[0].tobytes()
        assert sort_records(out[1][:66].cpu().numpy().reshape(-1).view(ISSUE_DTYPE)).tobytes() == eager[1].tobytes()


def test_drop_in_reports_the_reference_list_for_the_rocker_axle():
    import os

    import yaml

    from conftest import REPO
    from open_kinematics_amd.input import build_suspension, build_sweep
    from open_kinematics_amd.sweep import solve_evaluated_sweep

    arrays, _ = load_golden("c3_axle_grid")
    sus = build_suspension(yaml.safe_load(str(arrays["geometry_yaml"])))
    with open(os.path.join(REPO, "tests", "golden", "geometry", "axle_rocker_sweep.yaml"), "r", encoding="utf-8") as fh:
        sweep = build_sweep(yaml.safe_load(fh), sus)
    assert solve_evaluated_sweep(sus, sweep).diagnostics == []
    ev = solve_evaluated_sweep(sus, sweep, diagnose=True)
    assert_issues_match(ev.diagnostics, load_case("axle_rocker"))


def test_two_long_axle_sweeps_with_info_take_the_staged_path():
    """Several long sweeps with U-bar sides and solver records: tile -> sweep mapping, per-sweep scratch offsets, the side and
    info lanes of the path that stages displacements in global memory (20 tracked points x 999 steps do not fit LDS)."""
    from open_kinematics_amd import diagnostics as dg
    from open_kinematics_amd._abi import INFO_CONVERGED, INFO_DTYPE

    case, dp, roles, _, _, full, design, torch = _program_case("c3_axle_grid")
    n = 1000
    x = np.linspace(0, 15, n)  # the first grid row: a smooth roll sweep
    lo = np.floor(x).astype(int).clip(0, 14)
    w = (x - lo)[:, None, None]
    smooth = full[lo] * (1 - w) + full[lo + 1] * w
    second = smooth[::-1].copy()
    arm = roles.sides[1]["droplink_u_bar"]
    a, b = design[roles.bar_axis_a], design[roles.bar_axis_b]
    for s in range(700, 731):  # the right arm on its mirror branch for a block of states
        normal = np.cross(b - a, second[s, roles.sides[1]["droplink_rocker"]] - a)
        normal /= np.linalg.norm(normal)
        second[s, arm] = second[s, arm] - 2.0 * float(np.dot(second[s, arm] - a, normal)) * normal
    both = np.concatenate([smooth, second])
    rng = np.random.default_rng(3)
    converged = rng.uniform(size=2 * n) > 0.01
    residual = np.where(rng.uniform(size=2 * n) < 0.01, 5e-3, 1e-7)
    rec = np.zeros(2 * n, dtype=INFO_DTYPE)
    rec["max_residual"], rec["flags"] = residual, np.where(converged, INFO_CONVERGED, 0)
    info = torch.from_numpy(rec.view(np.uint8).reshape(-1, 40).copy()).cuda()
    want = dg.diagnose_arrays(both, roles, design, steps_per_sweep=n, converged=converged, max_residual=residual)
    assert want[0]["n_issues"][1, dg.DIAG_CHIRALITY] == 31 and want[0]["n_issues"][0, dg.DIAG_CHIRALITY] == 0
    for layout, rows in (("records", dp.program.out_point), ("free", dp.program.free_point)):
        pos = torch.from_numpy(np.ascontiguousarray(both[:, np.asarray(rows)])).cuda()
        _assert_same(dp.diagnose_host(pos, info, steps_per_sweep=n, layout=layout, roles=roles), want)


def test_c5_solved_ensemble_with_seeded_tampering():
    """BASELINE config 5: 4096 perturbed geometries x 256 steps from a real solve, with its okx_info, and a seeded set of
    (geometry, step, point) moved 20 mm: device == NumPy path on the set of records, values to 1e-12, summaries equal; every
    tampered entry is found; the launch cut in two gives the same records; both layouts agree."""
    import torch

    from open_kinematics_amd import diagnostics as dg
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.workloads import ensemble_problem, geometry_path

    g_count, steps = 4096, 256
    program, table, rel = ensemble_problem(g_count, steps)
    dp = DeviceProgram(program, "cuda:0")
    gpos, gparam = dp.rebind(torch.as_tensor(table, device="cuda:0"))
    targets = dp.ensemble_targets(gpos, torch.as_tensor(rel, device="cuda:0"))
    res = dp.solve(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=steps, chain_len=-1)
    roles = dg.diag_roles(load_geometry(geometry_path("geometry.yaml")), program)
    out = [int(k) for k in program.out_point]
    rows_np = dg.DiagRoles([out.index(int(p)) for p in roles.points], roles.names)  # the same roles over record rows
    positions = res.positions.clone()
    rng = np.random.default_rng(2713)
    flat = rng.choice(g_count * (steps - 2), size=300, replace=False)
    tampered = [(int(f // (steps - 2)), int(f % (steps - 2)) + 1, int(rng.integers(len(roles.points)))) for f in flat]
    for g, s, k in tampered:
        positions[g * steps + s, rows_np.points[k], 1] += 20.0
    info_host = res.info()
    host = dg.diagnose_arrays(positions.cpu().numpy(), rows_np, np.zeros((program.n_out, 3)), steps_per_sweep=steps,
                              converged=res.converged(info_host), max_residual=info_host["max_residual"])
    dev = dp.diagnose_host(positions, res.info_raw, steps_per_sweep=steps, roles=roles, geom_pos=gpos, capacity=2048)
    _assert_same(dev, host)
    found = set(zip(dev[1]["sweep"].tolist(), dev[1]["step"].tolist(), dev[1]["subject"].tolist()))
    assert all((g, s, k) in found for g, s, k in tampered)
    assert dev[0]["n_issues"][:, dg.DIAG_JUMP].sum() >= 2 * len(tampered) - 8  # in and out (two picks may touch)
    free = positions[:, dp.free_out_index].contiguous()
    other = dp.diagnose_host(free, res.info_raw, steps_per_sweep=steps, layout="free", roles=roles, geom_pos=gpos, capacity=2048)
    assert other[0].tobytes() == dev[0].tobytes() and other[1].tobytes() == dev[1].tobytes()
    cut = 1777
    lo = dp.diagnose_host(positions[: cut * steps], res.info_raw[: cut * steps], steps_per_sweep=steps, roles=roles, geom_pos=gpos[:cut])
    hi = dp.diagnose_host(positions[cut * steps:], res.info_raw[cut * steps:], steps_per_sweep=steps, roles=roles, geom_pos=gpos[cut:])
    hi[1]["sweep"] += cut
    assert np.concatenate([lo[0], hi[0]]).tobytes() == dev[0].tobytes()
    assert np.concatenate([lo[1], hi[1]]).tobytes() == dev[1].tobytes()


def test_sharded_ensemble_diagnoses_its_shard():
    """``ShardedEnsemble.diagnose`` (one rank): the pass on the shard's own buffers - free coordinates, or the records of a
    direct ensemble - equals ``DeviceProgram.diagnose`` on the same states."""
    import torch

    from open_kinematics_amd import diagnostics as dg
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.workloads import ensemble_problem, geometry_path

    program, table, rel = ensemble_problem(96, 64)
    dp = DeviceProgram(program, "cuda:0")
    roles = dg.diag_roles(load_geometry(geometry_path("geometry.yaml")), program)
    table_d, rel_d = torch.as_tensor(table, device="cuda:0"), torch.as_tensor(rel, device="cuda:0")
    results = []
    for records in (False, True):
        ensemble = ShardedEnsemble(dp, table_d, rel_d, 64, records=records)
        ensemble.step()
        if records:
            ensemble.positions[17 * 64 + 30, :, 1] += 25.0  # geometry 17 snaps at step 30 and back at 31
        else:
            ensemble.free_full[17 * 64 + 30, :, 1] += 25.0
        summary, issues, count = ensemble.diagnose(roles)
        torch.cuda.synchronize()
        assert tuple(summary.shape) == (96, 80)
        view = summary.cpu().numpy().reshape(-1).view(dg.SUMMARY_DTYPE)
        buffers = (ensemble.positions, "records") if records else (ensemble.free_full, "free")
        want = dp.diagnose_host(buffers[0], ensemble.info_full, steps_per_sweep=64, layout=buffers[1], roles=roles,
                                geom_pos=ensemble.my_pos)
        assert view.tobytes() == want[0].tobytes() and int(count.item()) == len(want[1])
        jumps = view["n_issues"][:, dg.DIAG_JUMP]
        assert jumps[17] >= 2 and view["first_step"][17, dg.DIAG_JUMP] == 30 and jumps.sum() == jumps[17]
        results.append(view)
    assert np.array_equal(results[0]["n_issues"], results[1]["n_issues"]) and np.array_equal(results[0]["first_step"], results[1]["first_step"])
    with pytest.raises(ValueError, match="keeps no positions"):
        evaluated = ShardedEnsemble.__new__(ShardedEnsemble)
        evaluated.metric_index = torch.zeros(1)
        evaluated.diagnose(roles)


def test_drop_in_with_a_known_non_empty_list():
    """``diagnose=True`` has an effect and goes through the device branch of ``diagnose_sweep``: (a) the ``stats`` fixture's
    exact states and stats with the sweep's program on the GPU - the reference's list, values to 1e-12; (b)
    ``solve_evaluated_sweep(c4_macpherson_grid, diagnose=True)``: our own solve of the flattened grid, whose 66 row wraps the
    reference reports as jumps - same steps, categories and message texts (three significant digits).  The values are
    displacements between two states of two DIFFERENT default-tolerance solves (the reference's and ours), so they agree
    only as far as a default-tolerance solve pins a state: the bound is the reference's own spread, twice (two states) the
    largest distance between its default and its tight solve of this very sweep (both in the golden; 1.1e-5 mm), doubled
    again because either solve may be off by that much."""
    import yaml

    from open_kinematics_amd import diagnostics as dg
    from open_kinematics_amd.input import build_suspension, build_sweep
    from open_kinematics_amd.sweep import solve_evaluated_sweep, sweep_program
    from test_diagnostics import _suspension_and_states

    case, sus, states, stats = _suspension_and_states("stats", load_golden)
    arrays, _ = load_golden("c1_dw_corner")
    program, _ = sweep_program(sus, build_sweep(yaml.safe_load(str(arrays["sweep_yaml"])), sus))
    assert len(case["issue_step"]) == 4
    assert_issues_match(dg.diagnose_sweep(sus, states, stats, device="cuda:0", program=program).issues, case)

    arrays, _ = load_golden("c4_macpherson_grid")
    sus = build_suspension(yaml.safe_load(str(arrays["geometry_yaml"])))
    sweep = build_sweep(yaml.safe_load(str(arrays["sweep_yaml"])), sus)
    plain = solve_evaluated_sweep(sus, sweep)
    assert plain.diagnostics == []
    ev = solve_evaluated_sweep(sus, sweep, diagnose=True)
    want = load_case("c4_macpherson_grid")
    bound = 4.0 * float(np.abs(arrays["ref_default_pos"] - arrays["ref_tight_pos"]).max())
    assert 0.0 < bound < 1e-4
    assert len(ev.diagnostics) == 66 == len(want["issue_step"])
    for k, issue in enumerate(ev.diagnostics):
        assert (issue.step, issue.category, issue.severity, issue.message) == (
            int(want["issue_step"][k]), str(want["issue_category"][k]), str(want["issue_severity"][k]), str(want["issue_message"][k])), k
        assert abs(issue.value - float(want["issue_value"][k])) <= bound, k
