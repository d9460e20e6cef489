"""
What the ``rebind_<name>.npz`` fixtures (oracle/gen_golden_rebind.py) say, in the shapes the tests of per-geometry problem
emission need: shared by tests/test_rebind_topologies.py (the oracle), tests/test_gpu_rebind_topologies.py (the device) and
the tangent tests on the same geometries (tests/test_tangents_oracle.py, tests/test_gpu_tangent_topologies.py).
Everything here is the reference's recorded data, re-arranged; nothing of the code under test computes an expectation.

Bounds (the project's existing ones, DESIGN.md section 4 and the C5 tests):

  POS_TOL     1e-12 mm   rebound design positions against the reference's flattened problem
  PARAM_REL   1e-14      rebound row parameters, relative to max(1, |ref|)
  TARGET_TOL  2.5e-13    absolute targets (rung R1: 1 ulp of a 1 m length)
  sweeps      rack-steered: the oracle's tight sweep <= 1e-7, device <= 6e-8 on rack pickups and <= 1e-8 elsewhere;
              unsteered (u_*): <= 1e-9
"""

import dataclasses
import functools

import numpy as np

from conftest import TOPOLOGIES, load_golden

NAMES = TOPOLOGIES + ["c3_axle_grid", "c4_macpherson_grid", "u_macpherson", "u_axle"]
MACPHERSON = ["t_axle_macpherson", "c4_macpherson_grid", "u_macpherson"]
LINE_MODES = ["softnorm", "pinned"]
G, S = 4, 5
FREE_CLAMP = 3          # the MacPherson geometry whose authored clamp moved freely: off the program's offset d0
POS_TOL = 1e-12
PARAM_REL = 1e-14
TARGET_TOL = 2.5e-13


@functools.lru_cache(maxsize=None)
def fixture(name: str):
    """(arrays, softnorm base program) of ``rebind_<name>.npz``."""
    return load_golden(f"rebind_{name}")


def geometries(name: str) -> list:
    """The geometries whose reference problem the program's constants can express (all but a freely moved clamp)."""
    return [g for g in range(G) if not (name in MACPHERSON and g == FREE_CLAMP)]


def reference_program(name: str, g: int, line_mode: str):
    """The reference's flattened problem of geometry ``g`` in ``line_mode``: its own positions and row parameters."""
    arrays, program = fixture(name)
    own = dataclasses.replace(program, design_pos=arrays["design_pos"][g].copy(), row_param=arrays["row_param"][g].copy())
    return own.with_line_mode(line_mode)


def table(name: str, sentinel: float | None = None) -> np.ndarray:
    """The hardpoint table ``[G, P, 3]``, optionally with another value in place of the fixture's sentinel."""
    arrays, program = fixture(name)
    out = arrays["hardpoints"].copy()
    if sentinel is not None:
        out[sentinel_mask(name)] = sentinel
    return out


def sentinel_mask(name: str) -> np.ndarray:
    """[G, P] True where the table holds the sentinel: every derived point but an authored strut clamp."""
    arrays, program = fixture(name)
    mask = np.repeat((program.role == 2)[None], G, axis=0)
    if "clamp_points" in arrays:
        mask[:, arrays["clamp_points"]] = False
    return mask


def param_error(got: np.ndarray, ref: np.ndarray) -> float:
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def host_targets(program, pos: np.ndarray, rel: np.ndarray) -> np.ndarray:
    """The host formula of ``DeviceProgram.ensemble_targets`` for one geometry: ``[S, T]``."""
    base = np.einsum("tc,tc->t", pos[program.tgt_point], program.tgt_dir)
    return base[None] + rel


def sweep_bounds(name: str, program) -> tuple:
    """(bound on rack pickups, bound on every other output point) of solved positions against ``ref_tight_pos``."""
    if name.startswith("u_"):
        return 1e-9, 1e-9
    return 6e-8, 1e-8


def rack_outputs(program) -> list:
    return [i for i, k in enumerate(program.out_point) if program.point_keys[k].lower_name.endswith("trackrod_inboard")]


def clamp_contract(name: str, rebound_pos: np.ndarray) -> dict:
    """
    The documented contract on the freely moved clamp (okx.h, ``okx_rebind_design``): derived-op parameters are program
    constants, so the rebound clamp sits at ``LBJ + axis * d0`` on the perturbed axis, ``d0 - d_ref`` along the axis from
    where the reference puts it.  Returns the two errors (mm, worst clamp) and the offset difference.
    """
    arrays, program = fixture(name)
    ref = arrays["design_pos"][FREE_CLAMP]
    on_axis, from_ref, offsets = 0.0, 0.0, []
    for k, point in enumerate(arrays["clamp_points"]):
        op = int(np.flatnonzero(program.dop_out == point)[0])
        start, end = int(program.dop_pts[op][0]), int(program.dop_pts[op][1])
        axis = (ref[end] - ref[start]) / np.linalg.norm(ref[end] - ref[start])
        d0, d_ref = float(arrays["clamp_offset_base"][k]), float(arrays["clamp_offset_ref"][k])
        assert d0 == float(program.dop_param[op])
        on_axis = max(on_axis, float(np.max(np.abs(rebound_pos[point] - (ref[start] + axis * d0)))))
        from_ref = max(from_ref, float(np.max(np.abs(rebound_pos[point] - ref[point] - axis * (d0 - d_ref)))))
        offsets.append(abs(d_ref - d0))
    return {"on_axis": on_axis, "from_reference": from_ref, "offset_difference": offsets}


def numpy_row_targets(program, pos: np.ndarray) -> np.ndarray:
    """
    Every row's design-state target at the positions ``pos [P, 3]`` in extended precision, from the reference's definitions
    (distance: geometric.py:17-28; angle between two vectors: geometric.py:71-104; three-point angle with the vertex at p2:
    constraints.py:248-285; triple product and its scale: attachments.py:45-74; line anchor: track_rod.py:92-96); rows with
    authored constants keep the program's.  For the row classes no reference topology emits (the three-point angle).
    """
    x = np.asarray(pos, dtype=np.longdouble)
    out = np.array(program.row_param, dtype=np.longdouble)

    def angle(v1, v2):
        u1, u2 = v1 / np.sqrt(v1 @ v1), v2 / np.sqrt(v2 @ v2)
        c = np.cross(u1, u2)
        return np.arctan2(np.sqrt(c @ c), u1 @ u2)

    for i, (kind, pts) in enumerate(zip(program.row_type, program.row_pts)):
        a, b, c, d = (int(k) for k in pts)
        if kind == 0:
            out[i, 0] = np.sqrt((x[b] - x[a]) @ (x[b] - x[a]))
        elif kind == 2:
            out[i, 0] = angle(x[b] - x[a], x[d] - x[c])
        elif kind == 3:
            out[i, 0] = angle(x[a] - x[b], x[c] - x[b])
        elif kind == 12:
            out[i, 0] = (x[b] - x[a]) @ np.cross(x[c] - x[a], x[d] - x[a])
            out[i, 1] = abs(out[i, 0])
        elif kind in (8, 13):
            out[i, 0:3] = x[a]
    return out.astype(np.float64)


def all_classes_table(seed: int = 7, sigma: float = 0.5) -> np.ndarray:
    """Three perturbed tables of the synthetic ``rows_all_classes`` program (one row of each constraint class)."""
    _, program = load_golden("rows_all_classes")
    rng = np.random.default_rng(seed)
    return program.design_pos[None] + rng.normal(0.0, sigma, (3,) + program.design_pos.shape)
