"""
Every field of the 40-byte okx_info record against an evaluation that shares nothing with the kernels
(tests/info_reference.py: NumPy on the C oracle's rows), on every code path that writes one - the interpreter (one wavefront
per problem, packed, two wavefronts), the quad kernel (cold and general body, single and pair mode), the lane kernel (cold,
chained, nested starts) - with the program's own geometry and with geometry tables, whole-sweep chains, both line-row forms
and the compact outputs.

At a converged state the cost is ~1e-25 and any check drowns in rounding, so the records are held to the reference where the
rows are NOT small: on a truncation ladder (max_iter = 1 .. the untruncated launch's largest iteration count; rows from
tens of mm down to rounding), at compromise points beyond the reach, and at the design-state target (a zero first step).

Per problem, at every such state (bounds: tests/info_reference.py, derived from the row tolerance of tests/test_gpu_parity.py):
  1  |max_residual - maxres_o| <= 2.5e-13 + 1e-13 maxres_o                      (reference row definitions)
  2  |cost - cost_o| <= sum |r_i| e_i + 0.5 sum e_i^2 + (m + 2) 2^-53 cost_o     (the rows the launch minimised)
  3  bit1 == (max_residual > residual_tolerance) on the device's own value; another tolerance changes bit1 alone
  4  the ladder is a prefix: iterations <= K, nfev grows with K, K >= the untruncated count gives the untruncated bits,
     K below it leaves bit0 clear and iterations == K
  5  last_step is the step between consecutive ladder states (2^-52 max|x|), or the state did not move: a rejected trial
     (cost and last_step unchanged) or a correction below step_tol that is not applied (bit0 newly set)
  6  lane kernel, nested starts without the confirming pass: 1 - 2 widened by max_i |J_i|_1 * last_step (the documented
     record of the point the last step started from); with confirm_full_pass the plain bounds
  7  bit3 clear at converged feasible states of single-corner programs with cond(J) <= 1e5
Non-finite targets and geometry entries: the problem is not accepted (bit2 set, bit0 clear), every other problem keeps its
bits, a chain goes on after it.

``pytest -s`` prints the worst difference met per path, as a fraction of its bound.
"""

import types

import numpy as np
import pytest

from conftest import gpu_available
from info_reference import free_vectors, geometry_programs, reference_record, reference_records

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STEP_TOL = 1e-11          # okx_default_opts
RESIDUAL_TOLERANCE = 1e-3
REJECTED_RUNGS = {}       # path -> ladder rungs that ended on a rejected trial point (record = the accepted point's)
WORST = {}                # path -> {"max_residual" | "cost" | "last_step": (difference, difference / bound)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    yield
    for path in sorted(WORST):
        print(f"\n[info record] {path}: " + ", ".join(f"{k} {d:.2e} ({f:.2f} of its bound)" for k, (d, f) in sorted(WORST[path].items())), end="")
    print()


@pytest.fixture(scope="module")
def device_program(golden):
    """(DeviceProgram, program, fixture arrays) per (fixture, line mode): created once for the module."""
    from open_kinematics_amd.batch import DeviceProgram

    cache = {}

    def get(name, line_mode="pinned"):
        if (name, line_mode) not in cache:
            arrays, program = golden(name)
            if line_mode is not None:
                program = program.with_line_mode(line_mode)
            cache[name, line_mode] = (DeviceProgram(program, "cuda:0"), program, arrays)
        return cache[name, line_mode]

    yield get
    for dp, _, _ in cache.values():
        dp.close()


def _caps(dp):
    """What the launch planner reads of the program (okx_debug_program_caps)."""
    import ctypes as C

    from open_kinematics_amd import _lib
    from open_kinematics_amd._abi import LaunchCaps

    caps = LaunchCaps()
    assert _lib.load().okx_debug_program_caps(dp._handle, C.byref(caps)) == 0, _lib.last_error()
    return caps


def _need(dp, kernel, n_problems, path="", optional=False, **kw):
    """The program must HAVE the kernel the case is about (every fixture the cases name has: losing one is a failure, not
    a skip) and the launch must resolve to it; `optional`: skip with the library's reason instead."""
    caps = _caps(dp)
    if optional and kernel in ("quad", "lane") and not (caps.has_quad and (kernel == "quad" or caps.has_lane)):
        pytest.skip(f"no {kernel} kernel for this program: {dp.kernel_note or dp.lane_note}")
    if kernel in ("quad", "lane"):
        assert caps.has_quad and dp.kernel == "quad", f"no generated kernels: {dp.kernel_note}"
    if kernel == "lane":
        assert caps.has_lane and dp.lane_threshold > 0, f"no lane kernel: {dp.lane_note}"
    if kernel == "packed":
        assert caps.has_packed, "the program has no packed interpreter kernel"
    assert dp.plan_launch(n_problems, kernel=kernel, chain_len=kw.pop("chain_len", 1), **kw)[0] == kernel
    if "cold" in path and kernel == "quad":
        assert caps.has_cold and dp.has_cold_body, "the program has no cold body"
    if "pair" in path:
        assert caps.quad_ppw == 8, "not a pair-mode kernel (eight problems per wavefront)"
    elif kernel == "quad":
        assert caps.quad_ppw == 16, "not a single-mode quad kernel (sixteen problems per wavefront)"
    if "two-wavefront" in path:
        assert caps.nreg > 63, "the program fits one wavefront"
    elif kernel == "single":
        assert caps.nreg <= 63


def _launch(dp, targets, **kw):
    res = dp.solve(torch.as_tensor(np.ascontiguousarray(targets), device="cuda:0"), **kw)
    torch.cuda.synchronize()
    pos = res.positions.cpu().numpy()
    return types.SimpleNamespace(pos=pos, x=free_vectors(dp.program, pos), info=res.info().copy(),
                                 raw=res.info_raw.cpu().numpy().copy())


def _note(path, field, diff, bound):
    k = int(np.argmax(diff / bound))
    entry = WORST.setdefault(path, {})
    if field not in entry or diff[k] / bound[k] > entry[field][1]:
        entry[field] = (float(diff[k]), float(diff[k] / bound[k]))


def _check_records(path, ref, launch, residual_tolerance=RESIDUAL_TOLERANCE):
    """Items 1 - 3 of the module docstring for one launch against its reference."""
    info = launch.info
    assert np.all(np.isfinite(info["max_residual"])) and np.all(np.isfinite(info["cost"])), path
    d_res = np.abs(info["max_residual"] - ref.maxres)
    d_cost = np.abs(info["cost"] - ref.cost)
    _note(path, "max_residual", d_res, ref.maxres_bound)
    _note(path, "cost", d_cost, ref.cost_bound)
    bad = np.flatnonzero(d_res > ref.maxres_bound)
    assert bad.size == 0, (path, "max_residual", bad[:8], info["max_residual"][bad[:8]], ref.maxres[bad[:8]])
    bad = np.flatnonzero(d_cost > ref.cost_bound)
    assert bad.size == 0, (path, "cost", bad[:8], info["cost"][bad[:8]], ref.cost[bad[:8]], ref.cost_bound[bad[:8]])
    assert np.array_equal((info["flags"] & 2) != 0, info["max_residual"] > residual_tolerance), (path, "bit1")
    assert np.all(info["reserved"] == 0)


def _check_other_tolerance(path, dp, targets, launch, **kw):
    """Item 3: residual_tolerance is informational - another value changes bit1 and nothing else."""
    other = _launch(dp, targets, residual_tolerance=1e-7, **kw)
    assert np.array_equal(other.pos, launch.pos), path
    for field in ("max_residual", "cost", "last_step", "iterations", "nfev", "reserved"):
        assert np.array_equal(other.info[field], launch.info[field]), (path, field)
    assert np.array_equal(other.info["flags"] & ~2, launch.info["flags"] & ~2), path
    assert np.array_equal((other.info["flags"] & 2) != 0, other.info["max_residual"] > 1e-7), path


def _check_bit3(path, program, launch, targets):
    """Item 7: pivots and Rayleigh quotient lie inside the spectrum of J^T J, so cond(J) <= 1e5 keeps the ratio >= 1e-10."""
    from oracle.oracle import Oracle

    ok = (launch.info["flags"] & 7) == 1
    _, jac = Oracle(program).eval(launch.x, targets)
    cond = np.array([np.linalg.cond(j) for j in jac])
    well = ok & (cond <= 1e5)
    assert well.any(), path
    assert np.all((launch.info["flags"][well] & 8) == 0), (path, "bit3", np.flatnonzero(well & ((launch.info["flags"] & 8) != 0)))


def _ladder(path, dp, program, targets, k_cap=None, **kw):
    """The truncation ladder of one launch configuration: items 1 - 5 at every rung.  Returns the untruncated launch."""
    kw = dict(chain_len=1, predictor=False, **kw)
    full = _launch(dp, targets, **kw)
    k_full = int(full.info["iterations"].max()) if k_cap is None else k_cap
    assert 1 <= k_full <= 10, (path, k_full)
    if k_cap is None:
        _check_records(path, reference_record(program, full.x, targets), full)
    b = len(targets)
    x_prev = np.repeat(program.design_free_array()[None], b, axis=0)
    prev = None
    bit1_seen = set()
    for k in range(1, k_full + 1):
        rung = _launch(dp, targets, max_iter=k, **kw)
        info = rung.info
        _check_records(f"{path}", reference_record(program, rung.x, targets), rung)
        bit1_seen |= set(((info["flags"] & 2) != 0).tolist())
        # 4: a prefix of the untruncated solve
        assert np.all(info["iterations"] <= k), (path, k)
        if prev is not None:
            assert np.all(info["nfev"] >= prev.info["nfev"]), (path, k)
        if k_cap is None:
            finished = k >= full.info["iterations"]
            assert np.array_equal(rung.pos[finished], full.pos[finished]), (path, k)
            assert np.array_equal(rung.raw[finished], full.raw[finished]), (path, k)
            assert np.all((info["flags"][~finished] & 1) == 0) and np.all(info["iterations"][~finished] == k), (path, k)
        # 5: last_step
        moved = np.any(rung.x != x_prev, axis=1)
        step = np.max(np.abs(rung.x - x_prev), axis=1)
        bound = 2.0 ** -52 * np.max(np.abs(rung.x), axis=1)
        d_step = np.abs(info["last_step"] - step)
        if moved.any():
            _note(path, "last_step", d_step[moved], bound[moved])
        assert np.all(d_step[moved] <= bound[moved]), (path, k, "last_step", np.flatnonzero(moved & (d_step > bound)),
                                                        info["last_step"][moved & (d_step > bound)], step[moved & (d_step > bound)])
        for i in np.flatnonzero(~moved):
            if prev is None:   # the first trial point: the record is still the design state's (its cost: item 2), no step yet
                rejected = info["last_step"][i] == 0.0
            else:
                rejected = info["cost"][i] == prev.info["cost"][i] and info["last_step"][i] == prev.info["last_step"][i]
            newly = (info["flags"][i] & 1) != 0 and (prev is None or (prev.info["flags"][i] & 1) == 0)
            assert rejected or (newly and info["last_step"][i] <= STEP_TOL), (path, k, int(i), info[i])
            if rejected and (info["flags"][i] & 1) == 0 and info["iterations"][i] == k:
                REJECTED_RUNGS[path] = REJECTED_RUNGS.get(path, 0) + 1   # a rung that ends on a rejected trial point
        x_prev, prev = rung.x, rung
    return full, bit1_seen


def _spread(n_rows, b):
    """`b` row numbers spread over a sweep of `n_rows`, ends included (101 rows: the design-state target, row 50, is one)."""
    return np.unique(np.round(np.linspace(0, n_rows - 1, b)).astype(int))


# ---- the truncation ladder on every family that solves independent problems ----

LADDERS = [  # (path, fixture, kernel, OKX_DEV, batch)
    ("interpreter", "c1_dw_corner", "single", None, 5),
    ("interpreter", "c4_macpherson_grid", "single", None, 5),
    ("packed", "c4_macpherson_grid", "packed", None, 5),
    ("packed", "c1_dw_corner", "packed", None, 5),
    ("two-wavefront", "t_axle_t_bar_heave", "single", None, 3),
    ("quad cold", "c1_dw_corner", "quad", None, 17),
    ("quad cold", "c4_macpherson_grid", "quad", None, 17),
    ("quad general", "c1_dw_corner", "quad", "no_cold", 17),
    ("quad general", "c4_macpherson_grid", "quad", "no_cold", 17),
    ("pair cold", "c3_axle_grid", "quad", None, 9),
    ("pair general", "c3_axle_grid", "quad", "no_cold", 9),
    ("lane cold", "c1_dw_corner", "lane", None, 65),
    ("lane cold", "c4_macpherson_grid", "lane", None, 65),
]


@pytest.mark.parametrize("shared_first_step", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("path,name,kernel,dev,batch", LADDERS, ids=[f"{p}-{n}".replace(" ", "_") for p, n, _, _, _ in LADDERS])
def test_truncation_ladder(device_program, monkeypatch, path, name, kernel, dev, batch, shared_first_step):
    """Items 1 - 5 and 7 on independent cold solves of every family.

    The lane kernel on c4_macpherson_grid is the case that found something: its max_residual at one converged state (grid
    row 231) was 3.41e-13 from the oracle's, 1.36 x the bound, on the 238.4 mm distance row to the strut's bottom end - a
    DERIVED point (base + unit vector x length) whose unit vector was formed with a reciprocal root good to ~4e-15.  The
    lane generator now refines that reciprocal (okx_lanegen.cpp, refine_inverse): 0.45 of the bound."""
    dp, program, arrays = device_program(name)
    _need(dp, kernel, batch, path)
    if dev:
        monkeypatch.setenv("OKX_DEV", dev)
    else:
        monkeypatch.delenv("OKX_DEV", raising=False)
    all_targets = arrays["targets_abs"]
    targets = all_targets[_spread(len(all_targets), batch)]
    assert len(targets) == batch
    label = f"{path} {name} {'shared' if shared_first_step else 'own'} first step"
    kw = dict(kernel=kernel, shared_first_step=shared_first_step)
    full, bit1_seen = _ladder(label, dp, program, targets, **kw)
    assert bit1_seen == {True, False}, (label, "both outcomes of bit1 occur on the ladder")
    assert np.all((full.info["flags"] & 7) == 1), label
    _check_other_tolerance(label, dp, targets, full, chain_len=1, predictor=False, **kw)
    if name in ("c1_dw_corner", "c4_macpherson_grid"):
        _check_bit3(label, program, full, targets)
    elif "pair" in path:
        print(f"\n[info record] {label}: bit3 set on {int(((full.info['flags'] & 8) != 0).sum())} of {batch} (printed only)", end="")


def test_ladder_on_every_row_class(device_program):
    """One row of each of the reference's constraint classes (synthetic; convergence is not required): K = 1 .. 3."""
    dp, program, arrays = device_program("rows_all_classes", None)
    for kernel in ("single", "quad", "lane"):   # (the program has all three: tests/test_gpu_lane.py)
        _need(dp, kernel, len(arrays["eval_targets"]))
        _ladder(f"{kernel} rows_all_classes", dp, program, arrays["eval_targets"], k_cap=3, kernel=kernel)


# ---- compromise points: targets beyond the reach ----

@pytest.mark.parametrize("kernel,dev", [("single", None), ("packed", None), ("quad", None), ("quad", "no_cold"), ("lane", None)])
def test_compromise_points(device_program, monkeypatch, kernel, dev):
    dp, program, arrays = device_program("c1_dw_corner")
    _need(dp, kernel, 16)
    if dev:
        monkeypatch.setenv("OKX_DEV", dev)
    targets = arrays["targets_abs"][:16].copy()
    targets[:, 1] += 2000.0
    launch = _launch(dp, targets, kernel=kernel, chain_len=1, predictor=False, max_iter=400)
    assert np.all(launch.info["max_residual"] > 1.0) and np.all(launch.info["flags"] & 2)
    _check_records(f"compromise {kernel}{' ' + dev if dev else ''}", reference_record(program, launch.x, targets), launch)


@pytest.mark.parametrize("kernel,dev", [("single", None), ("packed", None), ("quad", None), ("quad", "no_cold"), ("lane", None)])
def test_compromise_ladder_ends_on_rejected_trials(device_program, monkeypatch, kernel, dev):
    """The first iterations towards a target 2 m away overshoot: trial points are rejected, and a rung that ends on one
    must report the accepted point it still stands on (cost, max_residual, last_step unchanged), not the trial point."""
    dp, program, arrays = device_program("c1_dw_corner")
    _need(dp, kernel, 16)
    if dev:
        monkeypatch.setenv("OKX_DEV", dev)
    targets = arrays["targets_abs"][:16].copy()
    targets[:, 1] += 2000.0
    label = f"compromise ladder {kernel}{' ' + dev if dev else ''}"
    _ladder(label, dp, program, targets, k_cap=10, kernel=kernel, shared_first_step=False)
    print(f"\n[info record] {label}: {REJECTED_RUNGS.get(label, 0)} rungs ended on a rejected trial point", end="")
    assert REJECTED_RUNGS.get(label, 0) > 0, "the ladder no longer ends any rung on a rejected trial point: it has lost its purpose"


# ---- geometry tables, chained and nested starts ----

def _ensemble(device_program):
    dp, program, arrays = device_program("c5_ensemble")
    gpos, gparam = dp.rebind(torch.as_tensor(arrays["hardpoints"], device="cuda:0"))
    g, s = arrays["targets_abs"].shape[:2]
    targets = np.ascontiguousarray(arrays["targets_abs"]).reshape(g * s, -1)
    return dp, program, arrays, gpos, gparam, g, s, targets


@pytest.fixture(scope="module")
def ensemble_programs(golden):
    arrays, program = golden("c5_ensemble")
    return geometry_programs(program.with_line_mode("pinned"), arrays["hardpoints"])


@pytest.mark.parametrize("kernel", ["single", "quad", "lane"])
def test_geometry_tables(device_program, ensemble_programs, kernel):
    dp, program, arrays, gpos, gparam, g, s, targets = _ensemble(device_program)
    _need(dp, kernel, g * s)
    kw = dict(geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, kernel=kernel, chain_len=1, predictor=False)
    for max_iter in (1, 2, None):
        launch = _launch(dp, targets, **kw, **({} if max_iter is None else {"max_iter": max_iter}))
        ref = reference_records(ensemble_programs, s, launch.x, targets)
        _check_records(f"geometry tables {kernel}", ref, launch)
        if max_iter is None:
            assert np.all((launch.info["flags"] & 7) == 1)
        else:
            assert np.all(launch.info["iterations"] <= max_iter)
            assert max_iter > 1 or np.any(launch.info["max_residual"] > RESIDUAL_TOLERANCE)   # rows that are not small


NESTED_START = 2   # okx_debug_plan_launch: the lane kernel's nested start mode (tests/test_gpu_launch_branches.py)


@pytest.mark.parametrize("confirm", [False, True], ids=["default", "confirm_full_pass"])
def test_lane_nested_starts(monkeypatch, confirm):
    """The lane kernel's nested start (generated under its developer switch; a span of 256 steps, four per lane, solved in
    the order 0, 2, 1, 3).  Without the confirming pass a step after a lane's first may be taken as it is (okx_lanegen.cpp,
    body_lm_pass: a Gauss-Newton step of at most 1e-5 mm whose predicted successor is below a thousandth of step_tol): one
    evaluation, and a record that describes the point that step STARTED from, at most max_i |J_i|_1 * last_step from the
    rows of the returned state.  That one documented exception is bounded here, on exactly the problems that took it
    (not a lane's first step, nfev == iterations, last_step > step_tol); every other record, and every record under confirm_full_pass, the plain bounds."""
    import ctypes as C

    from open_kinematics_amd import _lib
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.workloads import macpherson_grid_problem
    from oracle.oracle import Oracle

    monkeypatch.setenv("OKX_DEV", "lane_nested,lane_refine")
    program, targets = macpherson_grid_problem(13, 20)
    targets = targets[:256]
    dp = DeviceProgram(program, "cuda:0")
    caps = _caps(dp)
    assert caps.has_lane and caps.has_nest, f"nested bodies not generated: {dp.lane_note}"
    opts = dp.default_opts()
    opts.kernel, opts.chain_len, opts.confirm_full_pass = 4, -1, int(confirm)
    plan = (C.c_int32 * 6)()
    assert _lib.load().okx_debug_plan_launch(C.byref(caps), C.byref(opts), 256, 0, 0, C.byref(plan)) == 0, _lib.last_error()
    assert (plan[0], plan[2]) == (4, NESTED_START)
    launch = _launch(dp, targets, kernel="lane", chain_len=-1, confirm_full_pass=confirm)
    dp.close()
    info = launch.info
    assert np.all((info["flags"] & 7) == 1)
    later = np.arange(256) % 4 != 0                      # not a lane's first step
    # the shortcut ends a solve right after a factorisation (as many evaluations as iterations: no confirming evaluation, no
    # trial evaluation after the last step) on a step ABOVE step_tol; a computed correction below step_tol ends it the same
    # way but is not applied, and every other ending evaluates the point it returns
    unevaluated = later & (info["nfev"] == info["iterations"]) & (info["last_step"] > STEP_TOL)
    widen = np.zeros(256)
    if confirm:
        assert not unevaluated.any()
    else:
        assert unevaluated.any(), "no step took the documented shortcut: the case has lost its purpose"
        assert np.all(info["last_step"][unevaluated] <= 1e-5)
        _, jac = Oracle(program).eval(launch.x, targets)
        widen[unevaluated] = (np.abs(jac).sum(axis=2).max(axis=1) * info["last_step"])[unevaluated]
        print(f"\n[info record] lane nested: {int(unevaluated.sum())} of 256 steps taken unevaluated, widest allowance {widen.max():.2e} mm", end="")
    _check_records(f"lane nested {'confirmed' if confirm else 'default'}", reference_record(program, launch.x, targets, widen), launch)


@pytest.mark.parametrize("confirm", [False, True], ids=["default", "confirm_full_pass"])
def test_lane_chained_starts_with_geometry_tables(device_program, ensemble_programs, confirm):
    """Warm-started chains of three on the lane kernel, never across a geometry (8 x 9): the plain bounds."""
    dp, program, arrays, gpos, gparam, g, s, targets = _ensemble(device_program)
    _need(dp, "lane", g * s, steps_per_geometry=s, geometry_tables=True, chain_len=3)
    assert dp.plan_launch(g * s, steps_per_geometry=s, geometry_tables=True, kernel="lane", chain_len=3) == ("lane", 3)
    kw = dict(geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, kernel="lane", chain_len=3, confirm_full_pass=confirm)
    cold = _launch(dp, targets, **{**kw, "chain_len": 1})
    for extra in ({}, {"max_iter": 2}):
        launch = _launch(dp, targets, **kw, **extra)
        _check_records(f"lane chains of 3 {'confirmed' if confirm else 'default'}", reference_records(ensemble_programs, s, launch.x, targets), launch)
    launch = _launch(dp, targets, **kw)
    assert np.all((launch.info["flags"] & 7) == 1)
    assert np.max(np.abs(launch.pos - cold.pos)) <= 1e-9      # (the planned launch is asserted above: lane, chains of 3)


@pytest.mark.parametrize("kernel", ["single", "quad", "lane"])
def test_whole_sweep_chain(device_program, kernel):
    dp, program, arrays = device_program("c1_dw_corner")
    _need(dp, kernel, 101)
    targets = arrays["targets_abs"]
    full = _launch(dp, targets, kernel=kernel, chain=True)
    assert np.all((full.info["flags"] & 7) == 1)
    _check_records(f"chain {kernel}", reference_record(program, full.x, targets), full)
    _check_bit3(f"chain {kernel}", program, full, targets)
    cut = _launch(dp, targets, kernel=kernel, chain=True, max_iter=2)
    assert np.all(cut.info["iterations"] <= 2) and np.any((cut.info["flags"] & 1) == 0)
    _check_records(f"chain {kernel}", reference_record(program, cut.x, targets), cut)


@pytest.mark.parametrize("kernel", ["single", "quad", "lane"])
def test_reference_line_rows(device_program, kernel):
    """The softnorm program minimises the reference's own rows: cost and max_residual are then over the same rows.
    (Skipped with the library's reason where the program with the reference's line row has no kernel of the family.)"""
    dp, program, arrays = device_program("c1_dw_corner", "softnorm")
    _need(dp, kernel, 101, optional=True)
    targets = arrays["targets_abs"]
    for extra in ({}, {"chain_len": 1, "predictor": False, "max_iter": 2}, {"chain_len": 1, "predictor": False, "max_iter": 1}):
        launch = _launch(dp, targets, kernel=kernel, step_tol=1e-8, **{"max_iter": 200, **extra})
        _check_records(f"softnorm {kernel}", reference_record(program, launch.x, targets), launch)
    assert np.any(launch.info["max_residual"] > RESIDUAL_TOLERANCE)   # (one iteration: rows that are not small)


# ---- compact outputs ----

OUTPUTS = [("quad cold", "c1_dw_corner", "quad", None, 17), ("quad general", "c1_dw_corner", "quad", "no_cold", 17),
           ("pair", "c3_axle_grid", "quad", None, 9), ("lane", "c1_dw_corner", "lane", None, 65)]


@pytest.mark.parametrize("path,name,kernel,dev,batch", OUTPUTS, ids=[p.replace(" ", "_") for p, *_ in OUTPUTS])
def test_compact_outputs_write_the_same_records(device_program, monkeypatch, path, name, kernel, dev, batch):
    dp, program, arrays = device_program(name)
    _need(dp, kernel, batch, path)
    if dev:
        monkeypatch.setenv("OKX_DEV", dev)
    targets = torch.as_tensor(arrays["targets_abs"][_spread(len(arrays["targets_abs"]), batch)], device="cuda:0")
    for extra in ({}, {"max_iter": 2}):
        kw = dict(kernel=kernel, chain_len=1, predictor=False, **extra)
        records = dp.solve(targets, **kw)
        free = dp.solve(targets, output="free", **kw)
        none = dp.solve(targets, output="none", **kw)
        torch.cuda.synchronize()
        assert torch.equal(free.info_raw, records.info_raw) and torch.equal(none.info_raw, records.info_raw), (path, extra)
        assert torch.equal(free.free, records.positions[:, dp.free_out_index]), (path, extra)


# ---- non-finite inputs ----

NON_FINITE = [  # (path, fixture, kernel, OKX_DEV, batch, problems hit: mid-wavefront and the ragged tail)
    ("interpreter", "c1_dw_corner", "single", None, 5, (2, 4)),
    ("packed", "c4_macpherson_grid", "packed", None, 5, (2, 4)),
    ("quad cold", "c1_dw_corner", "quad", None, 17, (7, 16)),
    ("quad general", "c1_dw_corner", "quad", "no_cold", 17, (7, 16)),
    ("pair", "c3_axle_grid", "quad", None, 9, (3, 8)),
    ("lane", "c1_dw_corner", "lane", None, 65, (30, 64)),
]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("path,name,kernel,dev,batch,hit", NON_FINITE, ids=[p.replace(" ", "_") for p, *_ in NON_FINITE])
def test_non_finite_targets_are_not_accepted(device_program, monkeypatch, path, name, kernel, dev, batch, hit, value):
    from open_kinematics_amd.batch import BatchResult

    dp, program, arrays = device_program(name)
    _need(dp, kernel, batch, path)
    if dev:
        monkeypatch.setenv("OKX_DEV", dev)
    targets = arrays["targets_abs"][_spread(len(arrays["targets_abs"]), batch)].copy()
    for shared in (True, False):
        kw = dict(kernel=kernel, chain_len=1, predictor=False, shared_first_step=shared)
        clean = _launch(dp, targets, **kw)
        assert np.all(BatchResult.accepted(clean.info))
        bad_targets = targets.copy()
        bad_targets[list(hit)] = value
        bad = _launch(dp, bad_targets, **kw)
        flags = bad.info["flags"][list(hit)]
        assert not BatchResult.accepted(bad.info)[list(hit)].any(), (path, shared, flags)
        assert np.all((flags & 4) != 0) and np.all((flags & 1) == 0), (path, shared, flags)
        others = np.setdiff1d(np.arange(batch), hit)
        assert np.array_equal(bad.pos[others], clean.pos[others]) and np.array_equal(bad.raw[others], clean.raw[others]), (path, shared)
        # a launch cut off before the non-finite cost has been met at an ACCEPTED point (generated kernels, shared first step,
        # infinite target: the head's trial point is rejected first) may end without bit2 - never with bit0 (okx.h)
        cut_clean = _launch(dp, targets, max_iter=1, **kw)
        cut = _launch(dp, bad_targets, max_iter=1, **kw)
        assert np.all((cut.info["flags"][list(hit)] & 1) == 0) and not BatchResult.accepted(cut.info)[list(hit)].any(), (path, shared)
        assert np.array_equal(cut.pos[others], cut_clean.pos[others]) and np.array_equal(cut.raw[others], cut_clean.raw[others]), (path, shared)


@pytest.mark.parametrize("kernel", ["single", "quad", "lane"])
def test_a_chain_goes_on_after_a_non_finite_target(device_program, kernel):
    from open_kinematics_amd.batch import BatchResult

    dp, program, arrays = device_program("c1_dw_corner")
    _need(dp, kernel, 101)
    targets = arrays["targets_abs"].copy()
    clean = _launch(dp, targets, kernel=kernel, chain=True)
    k = 37
    targets[k] = float("nan")
    bad = _launch(dp, targets, kernel=kernel, chain=True)
    assert (bad.info["flags"][k] & 5) == 4
    after = np.arange(k + 1, 101)
    assert np.all(BatchResult.accepted(bad.info)[after])
    assert np.max(np.abs(bad.pos[after] - clean.pos[after])) <= 1e-9
    assert np.array_equal(bad.pos[:k], clean.pos[:k]) and np.array_equal(bad.raw[:k], clean.raw[:k])


@pytest.mark.parametrize("kernel", ["single", "quad", "lane"])
def test_a_non_finite_geometry_entry_fails_that_geometry_alone(device_program, kernel):
    from open_kinematics_amd.batch import BatchResult

    dp, program, arrays, gpos, gparam, g, s, targets = _ensemble(device_program)
    _need(dp, kernel, g * s)
    kw = dict(geom_row_param=gparam, steps_per_geometry=s, kernel=kernel, chain_len=1, predictor=False)
    clean = _launch(dp, targets, geom_pos=gpos, **kw)
    assert np.all(BatchResult.accepted(clean.info))
    hit = 5
    poisoned = gpos.clone()
    poisoned[hit, int(program.free_point[2]), 1] = float("nan")
    bad = _launch(dp, targets, geom_pos=poisoned, **kw)
    rows = np.arange(hit * s, (hit + 1) * s)
    flags = bad.info["flags"][rows]
    assert not BatchResult.accepted(bad.info)[rows].any() and np.all((flags & 5) == 4), flags
    others = np.setdiff1d(np.arange(g * s), rows)
    assert np.array_equal(bad.pos[others], clean.pos[others]) and np.array_equal(bad.raw[others], clean.raw[others])
