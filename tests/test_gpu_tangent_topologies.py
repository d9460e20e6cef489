"""
GPU: the solution-manifold tangents of EVERY topology and every tangent path against the reference's own
``compute_state_tangents`` - ``tangents_<name>.npz`` on the design geometry, ``tangents_rebind_<name>.npz`` on the perturbed
geometries of ``rebind_<name>.npz`` (oracle/gen_golden_tangents.py) - at the fixtures' own states, pinned line rows.
The code under test never supplies an expectation: velocities come from the fixtures (<= 1e-9 mm per mm of target, the
bound of tests/test_gpu_tangents.py; these states have cond(J) <= 41), the pivot range of ``okx_tangent_info`` is held
inside the spectrum of J^T J with J from the CPU oracle, and the batch-shape tests ask for the same bits.

Paths: ``generated`` = okx_tangent_batch on the generated kernel (``_u``, with tables ``_g``), ``generic`` = the
interpreter's kernel (OKX_DEV=tangent_generic), ``evaluate_quad`` / ``evaluate_lane`` = the tangent epilogue of
okx_evaluate_batch in its two forms.  The lane form exists for corners of up to six free points; u_axle has no generated
kernel at all (no row joins its halves), the interpreter serves both of its okx_tangent_batch paths.

Measured on an MI355X when the module was written.  Worst |device - reference| per fixture and path (bound 1e-9), the
worst difference between two paths (bound 1e-10), the pivot range against the spectrum of J^T J over all paths (smallest
min_pivot / lambda_min, bound >= 1; largest max_pivot / lambda_max, bound <= 1) and what swapped tables move (bound > 1e-6):

  design geometry        generated  generic  eval quad  eval lane  paths    min piv  max piv
  t_axle_dw              1.4e-14    5.0e-15  1.4e-14    -          1.3e-14  2.353    0.563
  t_axle_dw_explicit     1.2e-14    1.1e-14  1.2e-14    -          1.4e-14  2.760    0.563
  t_axle_macpherson      3.1e-14    3.3e-14  3.1e-14    -          1.3e-14  1.992    0.592
  t_corner_rocker        1.3e-14    1.1e-14  1.3e-14    -          8.3e-15  2.642    0.478
  t_corner_strut         5.2e-15    5.0e-15  5.2e-15    -          3.9e-15  1.346    0.639
  t_corner_strut_rocker  6.4e-15    6.4e-15  6.4e-15    -          4.3e-15  2.119    0.478
  t_axle_t_bar_bump      8.9e-15    7.6e-15  8.9e-15    -          9.5e-15  2.920    0.486
  t_axle_t_bar_roll      8.9e-15    8.0e-15  8.9e-15    -          9.5e-15  3.067    0.480
  t_axle_heave_link      2.4e-14    1.6e-14  2.4e-14    -          2.1e-14  2.055    0.568
  t_axle_t_bar_heave     1.1e-14    7.7e-15  1.1e-14    -          1.1e-14  3.077    0.480

  per-geometry tables    generated  generic  eval quad  eval lane  paths    min piv  max piv  swapped
  t_axle_dw              1.2e-14    1.2e-14  1.2e-14    -          8.2e-15  2.321    0.563    1.9e-3
  t_axle_dw_explicit     1.5e-14    7.7e-15  1.5e-14    -          1.4e-14  2.692    0.563    4.5e-3
  t_axle_macpherson      2.3e-14    2.0e-14  2.2e-14    -          1.8e-14  1.992    0.593    2.5e-3
  t_corner_rocker        1.3e-14    1.1e-14  1.3e-14    -          7.3e-15  2.547    0.480    1.1e-2
  t_corner_strut         9.2e-15    6.4e-15  9.2e-15    -          1.1e-14  1.346    0.640    1.4e-3
  t_corner_strut_rocker  1.2e-14    1.1e-14  1.2e-14    -          7.2e-15  2.105    0.480    1.4e-2
  t_axle_t_bar_bump      1.1e-14    9.6e-15  1.1e-14    -          9.5e-15  2.784    0.486    6.8e-3
  t_axle_t_bar_roll      1.1e-14    8.0e-15  1.1e-14    -          1.0e-14  3.015    0.480    8.6e-3
  t_axle_heave_link      2.5e-14    3.0e-14  2.5e-14    -          3.2e-14  2.052    0.569    1.0e-2
  t_axle_t_bar_heave     1.0e-14    1.3e-14  1.0e-14    -          1.0e-14  2.913    0.480    1.5e-2
  c3_axle_grid           4.8e-14    2.5e-14  4.8e-14    -          4.3e-14  1.862    0.480    1.0e-2
  c4_macpherson_grid     1.6e-14    1.3e-14  1.6e-14    1.8e-14    2.5e-14  5.234    0.584    3.3e-3
  u_macpherson           1.0e-14    1.1e-14  1.0e-14    9.5e-15    1.9e-14  4.050    0.573    1.9e-3
  u_axle                 3.6e-14    3.6e-14  -          -          0        1.867    0.478    8.8e-3

Batch shapes (t_corner_rocker, 16 states per wavefront; t_axle_t_bar_heave, 8; with and without tables): batches of 1,
ppw - 1, ppw and ppw + 1 states and one of 256 * 32 * ppw + 3 states (above the grid cap: the stride loop) give the bits of
the fixture-sized launch, info records included; the record behind each output stays untouched.  No tangent kernel was
found wrong.
"""

import ctypes as C

import numpy as np
import pytest
import torch
import yaml

from conftest import TOPOLOGIES, gpu_available, load_golden
from rebind_reference import G, NAMES, S, fixture, geometries, reference_program, table
from test_tangents_oracle import free_outputs, load_tangent_golden

pytestmark = pytest.mark.gpu

BOUND = 1e-9      # device against the reference, mm per mm of target
AGREE = 1e-10     # one path against another
PATHS = ["generated", "generic", "evaluate_quad", "evaluate_lane"]
NO_QUAD = {"u_axle"}   # the interpreter's kernels only (tests/test_gpu_rebind_topologies.py)
SHAPE_FIXTURES = {"t_corner_rocker": 16, "t_axle_t_bar_heave": 8}   # a packed-quad corner, a pair-mode axle: states per wavefront
GUARD = -7.25
_loaded, _results, _spectra = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    yield
    for entry in _loaded.values():
        entry["dp"].close()
    _loaded.clear()
    _results.clear()


def _sync():
    """A faulted context fails every later launch for the wrong reason: the session ends at the first one."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as error:   # pragma: no cover
        pytest.exit(f"GPU error, nothing more is launched: {error}", returncode=3)


def _golden(name):
    return load_golden(name)


def _load(name: str) -> dict:
    """The program the loader makes of the fixture's own YAML (the fixture's program, array for array) on the device,
    with the evaluation of its metric roles enabled where the program has evaluated kernels."""
    if name in _loaded:
        return _loaded[name]
    from open_kinematics_amd._abi import LaunchCaps
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.input import build_suspension, build_sweep
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.sweep import sweep_program

    arrays, golden_program = _golden(name)
    suspension = build_suspension(yaml.safe_load(str(arrays["geometry_yaml"])))
    if hasattr(suspension, "corners") and name not in NO_QUAD:
        from test_gpu_axle_evaluated import _axle

        _, _, program, _, dp, _, _, _ = _axle(_golden, name)
    else:
        program, _ = sweep_program(suspension, build_sweep(yaml.safe_load(str(arrays["sweep_yaml"])), suspension))
        dp = DeviceProgram(program, "cuda:0")
        if name in NO_QUAD:
            assert dp.kernel != "quad" and dp.kernel_note
        else:
            assert dp.kernel == "quad", dp.kernel_note
            dp.enable_evaluation(corner_roles(suspension, program))
            assert dp.evaluation & 1, dp.evaluation_note
    want, got = golden_program.with_line_mode("pinned").to_arrays(), program.to_arrays()
    for key in want:   # the fixtures' states and tables are laid out for the fixture's program
        if key != "target_desc":
            assert np.array_equal(want[key], got[key]), f"{name}: the loader's program differs from the fixture's in {key}"
    caps = LaunchCaps()
    assert dp.lib.okx_debug_program_caps(dp._handle, C.byref(caps)) == 0
    _loaded[name] = dict(dp=dp, program=program, ppw=int(caps.quad_ppw), grid_cap=int(caps.n_cu) * int(caps.quad_waves_per_cu))
    return _loaded[name]


def _unavailable(name: str, path: str):
    """Why ``path`` cannot run on this program (None: it can)."""
    dp = _load(name)["dp"]
    if path.startswith("evaluate") and name in NO_QUAD:
        return f"no evaluated kernels: {dp.kernel_note}"
    if path == "evaluate_lane" and not dp.evaluation & 2:
        return f"no lane form of the evaluated kernels: {dp.evaluation_note or 'the program offers none'}"
    return None


def _unit(name: str, path: str) -> int:
    """States one wavefront takes together on ``path`` (1: one wavefront per state)."""
    if path == "generic" or name in NO_QUAD:
        return 1
    return 64 if path == "evaluate_lane" else _load(name)["ppw"]


def _run(name: str, path: str, pos, monkeypatch, **tables):
    """(tangents [B, T, n_out, 3], tangent info records) of ``pos`` on one path."""
    dp = _load(name)["dp"]
    if path == "generated":
        monkeypatch.delenv("OKX_DEV", raising=False)
    else:
        monkeypatch.setenv("OKX_DEV", "tangent_generic" if path == "generic" else path)
    if path.startswith("evaluate"):
        res = dp.evaluate(pos, tangents=True, **tables)
        _sync()
        tan, info = res.tangents, res.tangent_info()
    else:
        tan, tinfo = dp.tangents(pos, **tables)
        _sync()
        info = dp.tangent_info(tinfo)
    monkeypatch.delenv("OKX_DEV", raising=False)
    return tan.cpu().numpy(), info


def _base(name: str, path: str, monkeypatch):
    if ("base", name, path) not in _results:
        _results["base", name, path] = _run(name, path, load_tangent_golden(name)["pos"], monkeypatch)
    return _results["base", name, path]


def _tables(name: str):
    entry = _load(name)
    if "tables" not in entry:
        gpos, gparam = entry["dp"].rebind(torch.as_tensor(table(name), device="cuda:0"))
        _sync()
        entry["tables"] = (gpos, gparam)
    return entry["tables"]


def _rebound(name: str, path: str, monkeypatch):
    if ("tables", name, path) not in _results:
        gpos, gparam = _tables(name)
        pos = load_tangent_golden(f"rebind_{name}")["pos"].reshape(G * S, -1, 3)
        _results["tables", name, path] = _run(name, path, pos, monkeypatch, geom_pos=gpos, geom_row_param=gparam,
                                              steps_per_geometry=S)
    return _results["tables", name, path]


def _spectrum(key, program, pos) -> tuple:
    """(smallest, largest) eigenvalue of J^T J at every state ``pos [K, n_out, 3]``, J = the CPU oracle's Jacobian of the
    pinned rows and the target rows."""
    if key not in _spectra:
        from oracle.oracle import Oracle

        assert program.line_mode == "pinned"
        orc, free_out = Oracle(program), free_outputs(program)
        lo, hi = [], []
        for state in pos:
            _, jac = orc.eval(state[free_out].reshape(1, -1), np.zeros((1, program.n_targets)))
            ev = np.linalg.eigvalsh(jac[0].T @ jac[0])
            lo.append(ev[0])
            hi.append(ev[-1])
        _spectra[key] = (np.asarray(lo), np.asarray(hi))
    return _spectra[key]


def _assert_pivots_inside(info, lo, hi, what: str):
    """okx_tangent_info: the pivots of the LDL^T of J^T J lie inside its spectrum (okx.h)."""
    low = float(np.min(info["min_pivot"] / lo))
    high = float(np.max(info["max_pivot"] / hi))
    print(f"pivots {what}: min_pivot / lambda_min >= {low:.6f}, max_pivot / lambda_max <= {high:.6f}")
    assert np.all(info["min_pivot"] > 0)
    assert np.all(info["min_pivot"] >= lo * (1 - 1e-9)), what
    assert np.all(info["max_pivot"] <= hi * (1 + 1e-9)), what


# ---- a. the design geometry, four paths ----


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_tangents_match_the_reference(name, path, monkeypatch):
    reason = _unavailable(name, path)
    if reason:
        pytest.skip(reason)
    tg = load_tangent_golden(name)
    tan, info = _base(name, path, monkeypatch)
    worst = float(np.max(np.abs(tan - tg["vel"])))
    print(f"tangents base {name} {path}: {worst:.2e} (<= {BOUND})")
    assert np.all(info["flags"] == 1)
    assert worst <= BOUND
    lo, hi = _spectrum(("base", name), _golden(name)[1].with_line_mode("pinned"), tg["pos"])
    _assert_pivots_inside(info, lo, hi, f"base {name} {path}")


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_the_paths_agree(name, monkeypatch):
    got = {path: _base(name, path, monkeypatch) for path in PATHS if not _unavailable(name, path)}
    assert set(got) >= {"generated", "generic", "evaluate_quad"}
    _assert_agreement(got, f"base {name}")


def _assert_agreement(got: dict, what: str):
    paths = list(got)
    worst = 0.0
    for i, a in enumerate(paths):
        for b in paths[i + 1:]:
            worst = max(worst, float(np.max(np.abs(got[a][0] - got[b][0]))))
            assert np.array_equal(got[a][1]["flags"], got[b][1]["flags"]), f"{what}: flags of {a} and {b}"
    print(f"paths {what}: {paths} agree within {worst:.2e} (<= {AGREE})")
    assert worst <= AGREE


# ---- b. per-geometry tables ----


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_tangents_read_the_per_geometry_tables(name, path, monkeypatch):
    """What ``okx_rebind_design`` wrote, read back by every tangent kernel: G geometries of S states in one batch."""
    reason = _unavailable(name, path)
    if reason:
        pytest.skip(reason)
    tg = load_tangent_golden(f"rebind_{name}")
    tan, info = _rebound(name, path, monkeypatch)
    unit = _unit(name, path)
    if unit > 1:   # states of different geometries side by side in one wave unit
        assert len({k // S for k in range(min(unit, G * S))}) > 1
    keep = geometries(name)
    worst = float(np.max(np.abs(tan.reshape(tg["vel"].shape) - tg["vel"])[keep]))
    print(f"tangents tables {name} {path}: {worst:.2e} (<= {BOUND})")
    assert np.all(np.isfinite(tan)) and np.all(info["flags"] == 1)   # the freely moved clamp too
    assert worst <= BOUND
    lo, hi = [], []
    for g in range(G):
        a, b = _spectrum(("tables", name, g), reference_program(name, g, "pinned"), tg["pos"][g])
        lo.append(a)
        hi.append(b)
    _assert_pivots_inside(info, np.concatenate(lo), np.concatenate(hi), f"tables {name} {path}")
    # another geometry's table is another answer (the tables are really read)
    gpos, gparam = _tables(name)
    pos = tg["pos"].reshape(G * S, -1, 3)
    wrong, _ = _run(name, path, pos, monkeypatch, geom_pos=gpos.flip(0).contiguous(), geom_row_param=gparam.flip(0).contiguous(),
                    steps_per_geometry=S)
    moved = float(np.max(np.abs(wrong - tan)))
    print(f"tangents tables {name} {path}: swapped tables move the answer by {moved:.2e} (> 1e-6)")
    assert moved > 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_the_paths_agree_on_per_geometry_tables(name, monkeypatch):
    got = {path: _rebound(name, path, monkeypatch) for path in PATHS if not _unavailable(name, path)}
    assert set(got) >= {"generated", "generic"}
    _assert_agreement(got, f"tables {name}")


# ---- d. batch shapes: the slot in a wavefront, a ragged tail and the stride loop do not change the arithmetic ----


def _tangents_into(dp, pos, tables):
    """okx_tangent_batch into buffers one record longer than the batch: (tangents, info bytes), the guard row checked."""
    from open_kinematics_amd import _lib
    from open_kinematics_amd._abi import TANGENT_INFO_DTYPE
    from open_kinematics_amd.batch import _ptr

    p, b = dp.program, pos.shape[0]
    tan = torch.full((b + 1, p.n_targets, p.n_out, 3), GUARD, dtype=torch.float64, device="cuda:0")
    tinfo = torch.full((b + 1, TANGENT_INFO_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda:0")
    gpos, gparam, steps = tables if tables is not None else (None, None, 0)
    stream = torch.cuda.current_stream().cuda_stream
    rc = dp.lib.okx_tangent_batch(dp._handle, b, int(steps), _ptr(pos), _ptr(gpos), _ptr(gparam), _ptr(tan), _ptr(tinfo),
                                  C.c_void_p(stream))
    _lib.check(rc, "okx_tangent_batch")
    _sync()
    assert bool((tan[b] == GUARD).all()) and bool((tinfo[b] == 0xA5).all()), "the record behind the batch was written"
    return tan[:b], tinfo[:b]


@pytest.mark.parametrize("with_tables", [False, True], ids=["design", "tables"])
@pytest.mark.parametrize("name", list(SHAPE_FIXTURES))
def test_batch_shape_does_not_change_the_bits(name, with_tables, monkeypatch):
    monkeypatch.delenv("OKX_DEV", raising=False)
    entry = _load(name)
    dp, ppw = entry["dp"], entry["ppw"]
    assert ppw == SHAPE_FIXTURES[name]
    if with_tables:
        gpos, gparam = _tables(name)
        states = torch.as_tensor(load_tangent_golden(f"rebind_{name}")["pos"].reshape(G * S, -1, 3), device="cuda:0")
        base, base_info = dp.tangents(states, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=S)
    else:
        states = torch.as_tensor(load_tangent_golden(name)["pos"], device="cuda:0")
        base, base_info = dp.tangents(states)
    _sync()
    k = states.shape[0]
    assert np.all(dp.tangent_info(base_info)["flags"] == 1)

    def launch(index: torch.Tensor):
        """The states ``index`` (into the K of the fixture) as one batch; with tables, every state brings its geometry's."""
        tables = None
        if with_tables:
            geom = torch.div(index, S, rounding_mode="floor")
            tables = (gpos[geom].contiguous(), gparam[geom].contiguous(), 1)
        return _tangents_into(dp, states[index].contiguous(), tables)

    # the fixture's states, repeated where a batch needs more than K: the last b of them
    period = k * (-(-(ppw + 1) // k))
    for b in (1, ppw - 1, ppw, ppw + 1):
        index = torch.arange(period - b, period, device="cuda:0") % k
        tan, tinfo = launch(index)
        assert torch.equal(tan, base[index]), f"{b} states: tangents"
        assert torch.equal(tinfo, base_info[index]), f"{b} states: info records"
    # more wave units than the grid has wavefronts: the stride loop, with a ragged last unit
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 * ppw + 3
    assert n > entry["grid_cap"] * ppw, "the batch must not fit the grid"
    index = torch.arange(n, device="cuda:0") % k
    tan, tinfo = launch(index)
    whole = (n // k) * k
    assert bool((tan[:whole].reshape(n // k, k, -1) == base.reshape(1, k, -1)).all()), "a replica differs from its original"
    assert torch.equal(tan[whole:], base[:n - whole])
    assert bool((tinfo[:whole].reshape(n // k, k, -1) == base_info.reshape(1, k, -1)).all())
    assert torch.equal(tinfo[whole:], base_info[:n - whole])
