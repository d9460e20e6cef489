"""
Post-sweep diagnostics (reference ``core/diagnostics.py`` and ``core/suspensions/axle/mechanisms.py:119-163, 432-549``):
the advisory checks of a solved sweep - non-convergence, residuals over the acceptance tolerance, free points that jump
more than ``max(5 mm, 4 x their median step)`` ("possible branch snap"), a U-bar arm whose signed volume changes sign
or reaches zero, a link within 0.15 of toggle.

Three layers, the same checks in each:

* ``diagnose_arrays``: vectorised NumPy over ``[n_sweeps * steps, points, 3]`` positions; the fallback without a GPU
  and the cross-check of the device pass;
* ``DeviceProgram.diagnose`` (``batch.py``, ``okx_diagnose_sweeps_batch``): the device pass over records in HBM;
* ``diagnose_sweep``: the reference's function of that name on ``SuspensionState`` lists, with the reference's types and
  message texts.

Both array layers return the findings as ``ISSUE_DTYPE`` records (the device form of ``DiagnosticIssue``) and one
``SUMMARY_DTYPE`` record per sweep; ``issues_from_records`` turns the records of one sweep into the reference's issue list.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from enum import Enum
from math import acos, degrees

import numpy as np

from .enums import PointID, PointRef, Side

CONTINUITY_ABS_FLOOR_MM = 5.0
CONTINUITY_MEDIAN_FACTOR = 4.0
SOLVE_ACCEPT_RESIDUAL = 1e-3
EPS_GEOMETRIC = 1e-6
TRANSMISSION_MARGIN_WARNING_THRESHOLD = 0.15

MAX_TRACKED_POINTS = 42  # OKX_MAX_VARS / 3


class _StrEnum(str, Enum):
    def __str__(self) -> str:
        return self.value


class DiagnosticCategory(_StrEnum):
    """Machine-readable class of advisory diagnostic (``core/diagnostics.py:34-46``)."""

    CONVERGENCE = "convergence"
    RESIDUAL = "residual"
    JUMP = "jump"
    DERIVATIVES = "derivatives"
    DIAGNOSTICS = "diagnostics"
    REFERENCE = "reference"
    CHIRALITY = "chirality"
    TRANSMISSION = "transmission"


class DiagnosticSeverity(_StrEnum):
    WARNING = "warning"
    ERROR = "error"


@dataclass(frozen=True)
class DiagnosticIssue:
    """A single finding about a solved sweep (``core/diagnostics.py:58-75``); ``step`` None: sweep-wide."""

    step: int | None
    category: DiagnosticCategory
    severity: DiagnosticSeverity
    message: str
    value: float | None


@dataclass
class SweepDiagnostics:
    """Collected diagnostics of one solved sweep (``core/diagnostics.py:78-111``)."""

    issues: list

    @property
    def ok(self) -> bool:
        return not self.errors

    @property
    def warnings(self) -> list:
        return [issue for issue in self.issues if issue.severity is DiagnosticSeverity.WARNING]

    @property
    def errors(self) -> list:
        return [issue for issue in self.issues if issue.severity is DiagnosticSeverity.ERROR]


# --------------------------------------------------------------------------------------
# the device form (include/okx.h: okx_diag_roles, okx_diag_summary, okx_diag_issue)
# --------------------------------------------------------------------------------------

DIAG_CONVERGENCE, DIAG_RESIDUAL, DIAG_JUMP, DIAG_CHIRALITY, DIAG_TRANSMISSION = range(5)
DIAG_CATEGORIES = (DiagnosticCategory.CONVERGENCE, DiagnosticCategory.RESIDUAL, DiagnosticCategory.JUMP,
                   DiagnosticCategory.CHIRALITY, DiagnosticCategory.TRANSMISSION)
TRANSMISSION_JOINTS = ("droplink @ DROPLINK_U_BAR", "pushrod @ PUSHROD_INBOARD", "droplink @ DROPLINK_ROCKER")

SUMMARY_DTYPE = np.dtype([("n_issues", "<i4", (5,)), ("first_step", "<i4", (5,)), ("worst", "<f8", (5,))])
ISSUE_DTYPE = np.dtype([("sweep", "<i8"), ("step", "<i4"), ("category", "<i4"), ("subject", "<i4"), ("reserved", "<i4"),
                        ("value", "<f8"), ("threshold", "<f8")])
assert SUMMARY_DTYPE.itemsize == 80 and ISSUE_DTYPE.itemsize == 40


class DiagSideC(C.Structure):
    _fields_ = [("droplink_rocker", C.c_int32), ("droplink_u_bar", C.c_int32), ("rocker_axis_a", C.c_int32),
                ("rocker_axis_b", C.c_int32), ("pushrod_inboard", C.c_int32), ("pushrod_outboard", C.c_int32)]


class DiagRolesC(C.Structure):
    """ctypes mirror of ``okx_diag_roles``."""

    _fields_ = [("n_points", C.c_int32), ("point", C.c_int32 * MAX_TRACKED_POINTS), ("n_sides", C.c_int32),
                ("side", DiagSideC * 2), ("bar_axis_a", C.c_int32), ("bar_axis_b", C.c_int32)]


assert C.sizeof(DiagRolesC) == 232

_SIDE_FIELDS = ("droplink_rocker", "droplink_u_bar", "rocker_axis_a", "rocker_axis_b", "pushrod_inboard", "pushrod_outboard")


@dataclass
class DiagRoles:
    """
    What the checks look at, as indices into the point axis of the positions they are given (for the device pass: the
    program's point indices).  ``points`` / ``names``: the tracked free points in ``suspension.free_points()`` order and
    the names the messages print.  ``sides``: empty, or the LEFT and RIGHT U-bar arms: a dict of ``droplink_rocker``,
    ``droplink_u_bar`` and the four rocker-group points (``-1``: the corner has no rocker group).  ``bar_axis_a`` /
    ``bar_axis_b``: the U-bar axis points.
    """

    points: list
    names: list
    sides: list = field(default_factory=list)
    bar_axis_a: int = -1
    bar_axis_b: int = -1
    side_names: tuple = ("left", "right")

    def to_c(self) -> DiagRolesC:
        if len(self.points) > MAX_TRACKED_POINTS:
            raise ValueError(f"at most {MAX_TRACKED_POINTS} tracked points, got {len(self.points)}")
        if len(self.sides) not in (0, 2):
            raise ValueError("sides: none, or LEFT and RIGHT")
        c = DiagRolesC()
        c.n_points = len(self.points)
        for k, p in enumerate(self.points):
            c.point[k] = int(p)
        c.n_sides = len(self.sides)
        for k, side in enumerate(self.sides):
            for name in _SIDE_FIELDS:
                setattr(c.side[k], name, int(side.get(name, -1)))
        c.bar_axis_a, c.bar_axis_b = int(self.bar_axis_a), int(self.bar_axis_b)
        return c


def _roles_from_keys(suspension, index: dict) -> DiagRoles:
    """The roles of ``suspension`` over the point numbering ``index`` (point key -> index)."""
    free = list(suspension.free_points())
    roles = DiagRoles([index[k] for k in free], [getattr(k, "name", str(k)) for k in free])
    if getattr(suspension, "arb_kind", "") == "u_bar":  # the only topology with diagnostics of its own
        for side in (Side.LEFT, Side.RIGHT):
            entry = {"droplink_rocker": index[PointRef(side, PointID.DROPLINK_ROCKER)],
                     "droplink_u_bar": index[PointRef(side, PointID.DROPLINK_U_BAR)]}
            group = {"rocker_axis_a": PointID.ROCKER_AXIS_A, "rocker_axis_b": PointID.ROCKER_AXIS_B,
                     "pushrod_inboard": PointID.PUSHROD_INBOARD, "pushrod_outboard": PointID.PUSHROD_OUTBOARD}
            if all(PointRef(side, p) in index for p in group.values()):
                entry.update({name: index[PointRef(side, p)] for name, p in group.items()})
            roles.sides.append(entry)
        roles.bar_axis_a = index[PointRef(Side.CENTER, PointID.ARB_U_BAR_AXIS_A)]
        roles.bar_axis_b = index[PointRef(Side.CENTER, PointID.ARB_U_BAR_AXIS_B)]
    return roles


def diag_roles(suspension, program) -> DiagRoles:
    """``DiagRoles`` of a suspension in the point indices of its flattened ``program``."""
    return _roles_from_keys(suspension, {key: i for i, key in enumerate(program.point_keys)})


# --------------------------------------------------------------------------------------
# NumPy path
# --------------------------------------------------------------------------------------


def _norm(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _triple(a, b, c):
    return _dot(a, np.cross(b, c))


def _transmission_margin(driven, axis_point, axis, link):
    """``calculate_transmission_margin`` (``mechanisms.py:145-163``) over leading axes; NaN where it is undefined."""
    with np.errstate(invalid="ignore", divide="ignore"):
        axis_norm, link_norm = _norm(axis), _norm(link)
        axis_unit = axis / axis_norm[..., None]
        radius = driven - axis_point
        radius = radius - axis_unit * _dot(radius, axis_unit)[..., None]
        tangent = np.cross(axis_unit, radius)
        tangent_norm = _norm(tangent)
        margin = np.abs(_dot(link / link_norm[..., None], tangent / tangent_norm[..., None]))
    undefined = (axis_norm == 0.0) | (link_norm == 0.0) | (tangent_norm == 0.0)
    return np.where(undefined, np.nan, margin)


def positive_median(displacements: np.ndarray) -> np.ndarray:
    """``statistics.median`` of the strictly positive entries along the last axis (0 where there are none): the mean of the
    two middle order statistics, which for an odd count are the same element."""
    d = np.where(displacements > 0, displacements, np.inf)
    d = np.sort(d, axis=-1)
    k = np.count_nonzero(displacements > 0, axis=-1)
    lo = np.take_along_axis(d, np.maximum(k - 1, 0)[..., None] // 2, axis=-1)[..., 0]
    hi = np.take_along_axis(d, np.minimum(k // 2, d.shape[-1] - 1)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        return np.where(k > 0, (lo + hi) / 2.0, 0.0)


def sort_records(issues: np.ndarray) -> np.ndarray:
    """Issue records in the reference's order: per sweep the per-step checks by step (convergence before residual), the
    jumps by point then step, the U-bar checks by side, then step, chirality before the transmission joints."""
    cat, subject, step = issues["category"], issues["subject"], issues["step"]
    group = np.where(cat <= DIAG_RESIDUAL, 0, np.where(cat == DIAG_JUMP, 1, 2))
    k1 = np.where(group == 0, step, np.where(group == 1, subject, subject & 1))
    k2 = np.where(group == 0, cat, step)
    k3 = np.where(group == 2, cat, 0)
    k4 = np.where(group == 2, subject >> 1, 0)
    return issues[np.lexsort((k4, k3, k2, k1, group, issues["sweep"]))]


def diagnose_arrays(positions, roles: DiagRoles, design, *, steps_per_sweep: int | None = None, converged=None,
                    max_residual=None, residual_tolerance: float = SOLVE_ACCEPT_RESIDUAL):
    """
    The checks on ``positions [n_sweeps * steps_per_sweep, P, 3]`` (sweep g is states ``[g S, (g + 1) S)``).  ``design``
    is ``[P, 3]`` or, per sweep, ``[n_sweeps, P, 3]``: where the fixed role points (bar axis, rocker axes) and the design
    sign of the U-bar volume come from.  ``converged`` / ``max_residual`` ``[n_sweeps * S]`` or None (skip those checks).
    Returns ``(summaries [n_sweeps] SUMMARY_DTYPE, issues ISSUE_DTYPE in the reference's order)``.
    """
    pos = np.asarray(positions, dtype=np.float64)
    b = pos.shape[0]
    s = b if steps_per_sweep is None else int(steps_per_sweep)
    if s < 1 or b % s:
        raise ValueError("bad steps_per_sweep")
    g = b // s
    pos = pos.reshape(g, s, pos.shape[1], 3)
    design = np.asarray(design, dtype=np.float64)
    design = np.broadcast_to(design, (g,) + design.shape[-2:])
    summary = np.zeros(g, dtype=SUMMARY_DTYPE)
    summary["first_step"] = -1
    summary["worst"][:, DIAG_CHIRALITY:] = np.inf
    found = []

    def add(cat, mask, value, subject, threshold):
        """``mask [g, s]``: one record per set entry."""
        gi, si = np.nonzero(mask)
        rec = np.zeros(gi.size, dtype=ISSUE_DTYPE)
        rec["sweep"], rec["step"], rec["category"] = gi, si, cat
        rec["subject"] = np.broadcast_to(subject, mask.shape)[gi, si]
        rec["value"] = np.broadcast_to(value, mask.shape)[gi, si]
        rec["threshold"] = np.broadcast_to(threshold, mask.shape)[gi, si]
        found.append(rec)
        summary["n_issues"][:, cat] += mask.sum(axis=1).astype(np.int32)
        first = np.where(mask.any(axis=1), mask.argmax(axis=1), -1)
        old = summary["first_step"][:, cat]
        summary["first_step"][:, cat] = np.where(old < 0, first, np.where(first < 0, old, np.minimum(old, first)))

    if converged is not None:
        conv = np.asarray(converged).reshape(g, s).astype(bool)
        res = np.asarray(max_residual, dtype=np.float64).reshape(g, s)
        add(DIAG_CONVERGENCE, ~conv, 0.0, 0, 0.0)
        add(DIAG_RESIDUAL, res > residual_tolerance, res, 0, residual_tolerance)
        summary["worst"][:, DIAG_RESIDUAL] = np.fmax(res, 0.0).max(axis=1)
    if s >= 2:
        for k, p in enumerate(roles.points):
            disp = _norm(pos[:, 1:, p] - pos[:, :-1, p])  # [g, s - 1]
            threshold = np.maximum(CONTINUITY_ABS_FLOOR_MM, CONTINUITY_MEDIAN_FACTOR * positive_median(disp))
            mask = np.zeros((g, s), dtype=bool)
            mask[:, 1:] = ~(disp <= threshold[:, None])
            value = np.zeros((g, s))
            value[:, 1:] = disp
            add(DIAG_JUMP, mask, value, k, threshold[:, None])
            summary["worst"][:, DIAG_JUMP] = np.fmax(summary["worst"][:, DIAG_JUMP], np.fmax(disp, 0.0).max(axis=1))
    for side, r in enumerate(roles.sides):
        a, bb = design[:, None, roles.bar_axis_a], design[:, None, roles.bar_axis_b]
        rocker, arm = pos[:, :, r["droplink_rocker"]], pos[:, :, r["droplink_u_bar"]]
        design_sign = np.sign(_triple(bb - a, design[:, None, r["droplink_rocker"]] - a, design[:, None, r["droplink_u_bar"]] - a))
        volume = _triple(bb - a, rocker - a, arm - a)
        scale = _norm(bb - a) * _norm(rocker - a) * _norm(arm - a)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(scale <= EPS_GEOMETRIC, 0.0, volume / scale)
        boundary = np.abs(margin) <= EPS_GEOMETRIC
        inverted = ~boundary & (np.sign(volume) != design_sign)
        add(DIAG_CHIRALITY, boundary, margin, side | 2, EPS_GEOMETRIC)
        add(DIAG_CHIRALITY, inverted, volume, side, 0.0)
        summary["worst"][:, DIAG_CHIRALITY] = np.fmin(summary["worst"][:, DIAG_CHIRALITY], np.abs(margin).min(axis=1))
        droplink = arm - rocker
        margins = [_transmission_margin(arm, a, bb - a, droplink)]
        if r.get("rocker_axis_a", -1) >= 0:
            def point(name):
                p = r[name]
                return pos[:, :, p]

            # (the rocker axis is read from the states, as the reference does: it is part of every record or, where the
            #  records leave fixed points out, equal to the design position)
            axis_a = point("rocker_axis_a")
            axis = point("rocker_axis_b") - axis_a
            pushrod = point("pushrod_outboard") - point("pushrod_inboard")
            margins.append(_transmission_margin(point("pushrod_inboard"), axis_a, axis, pushrod))
            margins.append(_transmission_margin(rocker, axis_a, axis, droplink))
        for joint, m in enumerate(margins):
            add(DIAG_TRANSMISSION, m < TRANSMISSION_MARGIN_WARNING_THRESHOLD, m, side | (joint << 1),
                TRANSMISSION_MARGIN_WARNING_THRESHOLD)
            summary["worst"][:, DIAG_TRANSMISSION] = np.fmin(summary["worst"][:, DIAG_TRANSMISSION],
                                                             np.where(np.isnan(m), np.inf, m).min(axis=1))
    issues = np.concatenate(found) if found else np.zeros(0, dtype=ISSUE_DTYPE)
    return summary, sort_records(issues)


def issues_from_records(records: np.ndarray, roles: DiagRoles, *, residual_tolerance: float = SOLVE_ACCEPT_RESIDUAL) -> list:
    """The reference's ``DiagnosticIssue`` list of ONE sweep from its issue records (any order)."""
    out = []
    for rec in sort_records(records):
        step, cat, subject, value = int(rec["step"]), int(rec["category"]), int(rec["subject"]), float(rec["value"])
        category = DIAG_CATEGORIES[cat]
        error, warning = DiagnosticSeverity.ERROR, DiagnosticSeverity.WARNING
        if cat == DIAG_CONVERGENCE:
            out.append(DiagnosticIssue(step, category, error, f"Step {step} did not converge.", None))
        elif cat == DIAG_RESIDUAL:
            out.append(DiagnosticIssue(step, category, error, f"Step {step} residual {value:.6g} exceeds the acceptance "
                                       f"tolerance {residual_tolerance:.6g}.", value))
        elif cat == DIAG_JUMP:
            out.append(DiagnosticIssue(step, category, warning, f"Point '{roles.names[subject]}' jumped {value:.3g} mm from step "
                                       f"{step - 1} to step {step} (threshold {float(rec['threshold']):.3g} mm); possible "
                                       "branch snap.", value))
        elif cat == DIAG_CHIRALITY:
            side = roles.side_names[subject & 1]
            text = (f"{side} U-bar arm reached its chirality boundary at step {step}." if subject & 2
                    else f"{side} U-bar arm inverted at step {step}.")
            out.append(DiagnosticIssue(step, category, error, text, value))
        else:
            side, joint = roles.side_names[subject & 1], TRANSMISSION_JOINTS[subject >> 1]
            angle = 90.0 - degrees(acos(min(1.0, value)))
            out.append(DiagnosticIssue(step, category, warning, f"{side} {joint} is {angle:.1f} deg from toggle at step {step} "
                                       f"(margin {value:.3g}).", value))
    return out


# --------------------------------------------------------------------------------------
# diagnose_sweep (core/diagnostics.py:114-133)
# --------------------------------------------------------------------------------------


def _state_arrays(suspension, states):
    """``(keys, positions [S, P, 3], design [P, 3])`` over the design state's points."""
    design_state = suspension.initial_state()
    keys = list(design_state.positions)
    design = np.asarray([design_state.positions[k].data for k in keys], dtype=np.float64)
    pos = np.empty((len(states), len(keys), 3))
    for s, state in enumerate(states):
        rows = getattr(state.positions, "rows_if_untouched", lambda: None)()
        if rows is not None and list(rows[1]) == keys:
            pos[s] = rows[0]
            continue
        for i, k in enumerate(keys):
            point = state.positions.get(k)
            pos[s, i] = design[i] if point is None else point.data
    return keys, pos, design


def diagnose_sweep(suspension, states, stats, *, device=None, program=None) -> SweepDiagnostics:
    """
    Drop-in for ``kinematics.core.diagnostics.diagnose_sweep``: the checks of one completed sweep, issues in the reference's
    order - as called with the reference's three arguments, on the host (the NumPy path), GPU or not.  The device pass
    ``okx_diagnose_sweeps_batch`` needs the sweep's flattened ``ConstraintProgram`` to know the records' layout, which the
    states alone do not carry: with ``program=`` (the drop-in layer passes the one it solved with) and a GPU (``device`` not
    ``"cpu"``) the checks run there on the states' records - the same records either way.  For ONE sweep of host states
    that route (host -> device -> launch -> host) is about wiring the same code path the ensembles use, not speed; the
    device pass earns its keep on records that are in HBM already (``DeviceProgram.diagnose``, ``ShardedEnsemble.diagnose``).
    """
    converged = np.asarray([bool(info.converged) for info in stats], dtype=bool)
    residual = np.asarray([float(info.max_residual) for info in stats], dtype=np.float64)
    head = []
    if len(stats) != len(states):  # the reference walks the two lists independently
        _, first = diagnose_arrays(np.zeros((len(stats), 1, 3)), DiagRoles([], []), np.zeros((1, 3)), converged=converged,
                                   max_residual=residual) if len(stats) else (None, np.zeros(0, dtype=ISSUE_DTYPE))
        head, converged, residual = issues_from_records(first, DiagRoles([], [])), None, None
    if len(states) == 0:
        return SweepDiagnostics(head)
    if program is not None and _want_device(device):
        import torch

        from ._abi import INFO_CONVERGED, INFO_DTYPE
        from .sensitivity import _positions_array
        from .solver import _device_program

        dp = _device_program(program, device)
        roles = diag_roles(suspension, program)
        pos = _positions_array(states, [program.point_keys[k] for k in program.out_point])
        info = None
        if converged is not None:
            rec = np.zeros(len(states), dtype=INFO_DTYPE)
            rec["max_residual"], rec["flags"] = residual, np.where(converged, INFO_CONVERGED, 0)
            info = torch.from_numpy(rec.view(np.uint8).reshape(len(states), 40)).to(dp.device)
        _, records = dp.diagnose_host(torch.as_tensor(pos, device=dp.device), info, steps_per_sweep=len(states), roles=roles,
                                      capacity=max(256, 4 * len(states)))
    else:
        keys, pos, design = _state_arrays(suspension, states)
        roles = _roles_from_keys(suspension, {k: i for i, k in enumerate(keys)})
        _, records = diagnose_arrays(pos, roles, design, converged=converged, max_residual=residual)
    return SweepDiagnostics(head + issues_from_records(records, roles))


def _want_device(device) -> bool:
    if device is not None and str(device).startswith("cpu"):
        return False
    try:
        import torch

        return bool(torch.cuda.is_available())
    except Exception:  # pragma: no cover - torch is part of the image
        return False
