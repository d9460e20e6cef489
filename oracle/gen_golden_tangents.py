"""
Golden fixtures for the solution-manifold tangents by RUNNING the real reference:
``kinematics.core.sensitivity.compute_state_tangents`` at tight-tolerance solved states.

Run here (where /root/reference exists):  python -m oracle.gen_golden_tangents
Only data is written, two kinds of file:

tests/golden/tangents_<name>.npz, for the baseline fixtures and every topology of tests/conftest.py, with, for K sampled
sweep steps,
  step_index [K], pos [K, n_out, 3] (the reference's tight solved positions),
  vel [K, T, n_out, 3] (d point / d target), rank [K], smallest_sv [K], cond [K].
Inputs (programs, targets) are the ones of tests/golden/<name>.npz.

tests/golden/tangents_rebind_<name>.npz, for every name of oracle/gen_golden_rebind.py: the same quantities on the G
perturbed geometries and S steps of the committed ``rebind_<name>.npz``,
  pos [G, S, n_out, 3], vel [G, S, T, n_out, 3], rank / smallest_sv / cond [G, S], step_index [S].
The geometries are not stored again: the rebind generator's seeded draw is replayed (same stream, same redraws, the
fixture's sigma) and every geometry's flattened ``design_pos`` and ``row_param`` must equal the committed fixture's
exactly before anything is written.  ``pos`` is THIS run's tight sweep, the states the tangents were taken at: the
reference's tight sweeps wander inside their own floor (a few 1e-8 mm on the rack pickups) between runs, and a tangent
compared at the rebind fixture's ``ref_tight_pos`` would absorb that difference.

A committed file is never rewritten: its bytes stay where this run gives its arrays again (the files without a rack do,
bit for bit) or the same data inside the floor of the reference's tight sweep (FLOOR: the rack-steered axles, whose rack
pickups land 2e-8 mm apart between two runs even in the pinned environment below - the heap's history moves the buffers'
alignment - and the velocities 5e-11 with them); anything further off stops the run.  Each file holds states and tangents
of ONE run, which is what the tests compare.  New files are written with the deterministic writer of gen_golden_rebind.
"""

from __future__ import annotations

import copy
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import ref_shim  # noqa: E402

ref_shim.install()

from kinematics.core.input import build_suspension, build_sweep  # noqa: E402
from kinematics.core.points.derived.manager import DerivedPointsManager  # noqa: E402
from kinematics.core.sensitivity import compute_state_tangents  # noqa: E402
from kinematics.core.solver import SolverConfig, convert_targets_to_absolute, solve_suspension_sweep  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
TIGHT = SolverConfig(ftol=1e-15, xtol=1e-15, gtol=1e-15)
BASELINE = (("c1_dw_corner", 21), ("c4_macpherson_grid", 24), ("u_dw_corner", 8), ("u_macpherson", 8), ("c3_axle_grid", 6))
TOPOLOGIES = ("t_axle_dw", "t_axle_dw_explicit", "t_axle_macpherson", "t_corner_rocker", "t_corner_strut",
              "t_corner_strut_rocker", "t_axle_t_bar_bump", "t_axle_t_bar_roll", "t_axle_heave_link", "t_axle_t_bar_heave")
MAX_BYTES = 64 * 1024   # of a new file
# how far a second run of the reference may land from a committed file that is then left unwritten: the tight sweep's floor
# on rack pickups (mm; the bound tests/rebind_reference.py puts on a tight sweep), the tangent bound of the device tests
# (the smallest singular value follows the softnorm line row at the rack pickup: 1.6e-7 relative between two runs)
FLOOR = {"pos": 1e-7, "vel": 1e-9}
REL_FLOOR = {"smallest_sv": 1e-6, "cond": 1e-6}


def tangents_at(suspension, sweep, steps) -> dict:
    """The reference's tight sweep of ``suspension`` and its tangents at the sweep's ``steps``: pos / vel / rank / ..."""
    manager = DerivedPointsManager(suspension.derived_spec())
    states, _ = solve_suspension_sweep(suspension.initial_state(), suspension.constraints(), sweep, manager, TIGHT)
    out = suspension.output_points()
    initial = suspension.initial_state()
    pos, vel, rank, ssv, cond = [], [], [], [], []
    for i in steps:
        step_targets = convert_targets_to_absolute([s[i] for s in sweep.target_sweeps], initial)
        fields, info = compute_state_tangents(states[i], suspension.constraints(), manager, step_targets)
        pos.append([states[i].positions[k].data for k in out])
        vel.append([[f.velocity(k) for k in out] for f in fields])
        rank.append(info.rank)
        ssv.append(info.smallest_singular_value)
        cond.append(info.condition_number)
    return dict(pos=np.asarray(pos, dtype=np.float64), vel=np.asarray(vel, dtype=np.float64),
                rank=np.asarray(rank, dtype=np.int32), smallest_sv=np.asarray(ssv), cond=np.asarray(cond))


def write_or_keep(path: str, arrays: dict) -> str:
    """Leave a committed file with these very arrays alone; refuse to change one; write a new one deterministically."""
    from oracle.gen_golden_rebind import save_npz

    if os.path.exists(path):
        have = dict(np.load(path, allow_pickle=False))
        same = set(have) == set(arrays) and all(
            have[k].dtype == np.asarray(v).dtype and np.array_equal(have[k], np.asarray(v)) for k, v in arrays.items())
        if same:
            return "kept, reproduced bit for bit"
        # A rack-steered tight sweep of the reference lands anywhere inside its own floor (oracle/gen_golden_rebind.py: a
        # few 1e-8 mm on the rack pickups, with the environment), and its tangents move with the state.  The committed file
        # stays as it is - states and tangents of ONE run - if this run is the same data inside that floor.
        shapes = set(have) == set(arrays) and all(have[k].shape == np.asarray(v).shape for k, v in arrays.items())
        worst = {k: float(np.max(np.abs(have[k] - np.asarray(v)) / (np.abs(have[k]) if k in REL_FLOOR else 1.0)))
                 for k, v in arrays.items()} if shapes else {}
        if not shapes or any(worst[k] > FLOOR.get(k, REL_FLOOR.get(k, 0.0)) for k in worst):
            raise RuntimeError(f"{os.path.basename(path)}: this run does not reproduce the committed arrays ({worst})")
        return "kept, unwritten: this run differs inside the reference's floor, " + ", ".join(
            f"{k} {v:.1e}" for k, v in worst.items() if v > 0.0)
    save_npz(path, arrays)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise RuntimeError(f"{os.path.basename(path)}: {size} B, above the {MAX_BYTES} B of a tangent fixture")
    return f"written, {size} B"


def emit(name: str, n_samples: int) -> None:
    base = np.load(os.path.join(OUT, f"{name}.npz"), allow_pickle=False)
    geometry = yaml.safe_load(str(base["geometry_yaml"]))
    sweep_map = yaml.safe_load(str(base["sweep_yaml"]))
    suspension = build_suspension(copy.deepcopy(geometry))
    sweep = build_sweep(sweep_map, suspension)
    idx = np.unique(np.linspace(0, sweep.n_steps - 1, n_samples).round().astype(int))
    arrays = dict(step_index=idx, **tangents_at(suspension, sweep, idx))
    what = write_or_keep(os.path.join(OUT, f"tangents_{name}.npz"), arrays)
    print(f"tangents_{name}: {len(idx)} states, T={len(sweep.target_sweeps)}, rank {set(arrays['rank'].tolist())}, "
          f"cond max {arrays['cond'].max():.3g}, |vel| max {np.abs(arrays['vel']).max():.3g} ({what})")


def emit_rebind(name: str) -> None:
    """Tangents on the geometries of ``rebind_<name>.npz``: gen_golden_rebind.emit_file's draw, replayed."""
    from oracle.gen_golden_rebind import G, REDRAWS, emit_geometry, perturb, thin_sweep

    fixture = np.load(os.path.join(OUT, f"{name}.npz"), allow_pickle=False)
    rebind = np.load(os.path.join(OUT, f"rebind_{name}.npz"), allow_pickle=False)
    sigma = float(rebind["sigma"])
    base = yaml.safe_load(str(fixture["geometry_yaml"]))
    sweep_map, _rel, idx = thin_sweep(yaml.safe_load(str(fixture["sweep_yaml"])), build_suspension(copy.deepcopy(base)))
    assert np.array_equal(idx, rebind["step_index"])
    macpherson = base["type"] == "macpherson"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    per = {k: [] for k in ("pos", "vel", "rank", "smallest_sv", "cond")}
    for g in range(G):
        free_clamp = macpherson and g == G - 1
        for _ in range(REDRAWS):
            data = copy.deepcopy(base) if g == 0 else perturb(base, rng, sigma, free_clamp)
            try:
                suspension, sweep, program = emit_geometry(data, sweep_map)
            except ValueError:   # a validator of the reference rejects the draw: redrawn, as the rebind generator did
                continue
            break
        else:
            raise RuntimeError(f"{name}: geometry {g} rejected {REDRAWS} times at sigma = {sigma}")
        assert np.array_equal(program.design_pos, rebind["design_pos"][g]), f"{name}: geometry {g} is not the fixture's"
        assert np.array_equal(program.row_param, rebind["row_param"][g]), f"{name}: row parameters of geometry {g}"
        for key, value in tangents_at(suspension, sweep, range(sweep.n_steps)).items():
            per[key].append(value)
    arrays = {k: np.asarray(v) for k, v in per.items()}
    drift = float(np.max(np.abs(arrays["pos"] - rebind["ref_tight_pos"])))
    what = write_or_keep(os.path.join(OUT, f"tangents_rebind_{name}.npz"), dict(step_index=idx, **arrays))
    print(f"tangents_rebind_{name}: sigma={sigma} vel {arrays['vel'].shape}, rank {set(arrays['rank'].ravel().tolist())}, "
          f"cond max {arrays['cond'].max():.3g}, states off ref_tight_pos by {drift:.2e} ({what})")


def main() -> None:
    from oracle.gen_golden_rebind import NAMES

    for name, n_samples in BASELINE:
        emit(name, n_samples)
    for name in TOPOLOGIES:
        emit(name, 6)
    for name in NAMES:
        emit_rebind(name)


if __name__ == "__main__":
    # as oracle/gen_golden_rebind.py: a fresh interpreter with a fixed environment, so that two runs give the same bytes
    if os.environ.get("OKX_GEN_PINNED") != "1":
        env = {k: os.environ[k] for k in ("PATH", "OKX_REFERENCE_ROOT") if k in os.environ}
        env.update(OKX_GEN_PINNED="1", PYTHONHASHSEED="0", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        command = [sys.executable, "-m", "oracle.gen_golden_tangents"]
        if shutil.which("setarch"):
            command = ["setarch", os.uname().machine, "-R"] + command
        sys.exit(subprocess.call(command, env=env, cwd=REPO))
    main()
