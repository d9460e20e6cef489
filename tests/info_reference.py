"""
An independent evaluation of what an ``okx_info`` record says about the state a solve returned: plain NumPy on top of the
C oracle's residual rows, nothing of the device code.  tests/test_gpu_info_record.py holds every kernel family's records
against it; tests/test_info_reference.py anchors it to the values the reference itself recorded.

  cost          0.5 * sum r_i^2 over the rows the launch minimised (a pinned program: its pin rows)
  max_residual  max |r_i| over the reference's row definitions (the softnorm form of the same program; okx.h)

Error model: the project's device-against-oracle row tolerance, e_i = 2.5e-13 + 1e-13 |r_i| (tests/test_gpu_parity.py),
propagated through the maximum and through the sum of squares:

  |max_residual - maxres_o| <= 2.5e-13 + 1e-13 maxres_o
  |cost - cost_o|           <= sum |r_i| e_i + 0.5 sum e_i^2 + (m + 2) 2^-53 cost_o      (m rows: the sum's own rounding)

``widen`` (per problem, mm) is added to every row's e_i: the one documented case of a record that describes the start of the
last step (lane kernel, nested starts without the confirming pass) moves every row by at most max_i |J_i|_1 * last_step.
"""

import dataclasses

import numpy as np

ROW_FLOOR = 2.5e-13
ROW_REL = 1e-13


@dataclasses.dataclass
class RecordReference:
    cost: np.ndarray          # [B]
    cost_bound: np.ndarray    # [B]
    maxres: np.ndarray        # [B]
    maxres_bound: np.ndarray  # [B]
    rows: np.ndarray          # [B, m] the minimised rows


def reference_record(program, x, targets, widen=None) -> RecordReference:
    """The record's ``cost`` and ``max_residual`` at the free vectors ``x [B, n]`` with their bounds (module docstring)."""
    from oracle.oracle import Oracle

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, program.n_vars)
    targets = np.ascontiguousarray(targets, dtype=np.float64).reshape(x.shape[0], -1)
    r, _ = Oracle(program).eval(x, targets, jac=False)
    reference_rows = program if program.line_mode == "softnorm" else program.with_line_mode("softnorm")
    rs, _ = Oracle(reference_rows).eval(x, targets, jac=False)
    w = np.zeros(x.shape[0]) if widen is None else np.asarray(widen, dtype=np.float64).reshape(-1)
    e = ROW_FLOOR + ROW_REL * np.abs(r) + w[:, None]
    cost = 0.5 * np.sum(r * r, axis=1)
    cost_bound = np.sum(np.abs(r) * e, axis=1) + 0.5 * np.sum(e * e, axis=1) + (r.shape[1] + 2) * 2.0 ** -53 * cost
    maxres = np.max(np.abs(rs), axis=1)
    return RecordReference(cost, cost_bound, maxres, ROW_FLOOR + ROW_REL * maxres + w, r)


def geometry_programs(program, hardpoints) -> list:
    """One program per geometry of a table ``hardpoints [G, P, 3]``: design positions and row parameters rebound by the oracle."""
    from oracle.oracle import Oracle

    base = Oracle(program)
    out = []
    for table in np.asarray(hardpoints, dtype=np.float64):
        pos, row_param = base.rebind(table)
        out.append(dataclasses.replace(program, design_pos=pos, row_param=row_param))
    return out


def reference_records(programs, steps_per_geometry: int, x, targets, widen=None) -> RecordReference:
    """``reference_record`` of a geometry-major batch: problems ``[g S, (g + 1) S)`` on ``programs[g]``."""
    s = steps_per_geometry
    x = np.asarray(x).reshape(len(programs) * s, -1)
    targets = np.asarray(targets).reshape(len(programs) * s, -1)
    w = np.zeros(len(x)) if widen is None else np.asarray(widen, dtype=np.float64).reshape(-1)
    parts = [reference_record(p, x[g * s:(g + 1) * s], targets[g * s:(g + 1) * s], w[g * s:(g + 1) * s])
             for g, p in enumerate(programs)]
    return RecordReference(*[np.concatenate([getattr(p, f.name) for p in parts]) for f in dataclasses.fields(RecordReference)])


def free_vectors(program, positions) -> np.ndarray:
    """``x [B, n]`` from output records ``[B, n_out, 3]`` (every free point of these programs is an output point)."""
    out = list(int(k) for k in program.out_point)
    index = [out.index(int(p)) for p in program.free_point]
    return np.ascontiguousarray(np.asarray(positions)[:, index]).reshape(len(positions), -1)
