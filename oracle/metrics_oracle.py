"""
CPU restatement (numpy + a 30-line forward-mode scalar) of the reference's corner state metrics and
their directional derivatives.  TEST INFRASTRUCTURE ONLY.

Follows ``kinematics/core/metrics/angles.py:22-132`` (camber, caster, KPI, toe = roadwheel angle),
``travel.py:19-45`` (wheel travel, half-track), ``steering_geometry.py:22-76`` and
``context.py:82-138`` (wheel axis, steering axis, steering-axis / ground-plane intersection),
``swing_arms.py:45-88``, ``anti_geometry.py:32-206``, ``travel.py:48-62`` (damper length), the instant axis of
``corner/double_wishbone.py:352-430`` / ``corner/macpherson.py:325-378`` over
``vector_utils/geometric.py:216-352``, ``axle_metrics.py:21-95`` and the rotation / hardware roles of an axle
(``metrics/kernels.py:58-76``, ``axle/mechanisms.py:718-815,903-944``).  The
derivative of a metric along a tangent field is what ``metrics/derivatives.py`` evaluates with the
reference's dual numbers (``primitives/dual.py``).

Two paths over the same formulas: a values-only one in numpy (``geometry_metrics``, ``axle_metrics``, ``role_value``,
``catalog_values``), pinned to the reference's goldens, and one on the duals ``D`` (``catalog_duals``,
``axle_metric_duals``, ``role_dual``: value and derivative along one direction, NaN in both where the value is
undefined), which tests/test_metrics_oracle.py pins to differences of the first.  The duals take any number type:
``number=mpmath.mpf`` gives the 50-digit run that ``oracle/measure_metric_noise.py`` compares the float64 run with.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

METRIC_NAMES = (
    "camber", "caster", "kpi", "roadwheel_angle", "wheel_travel", "half_track", "scrub_radius", "mechanical_trail",
    "svic_x", "svic_z", "svsa_length", "fvic_y", "fvic_z", "fvsa_length", "damper_length", "svsa_angle",
    "anti_dive", "anti_lift", "anti_squat",
)
AXLE_METRIC_NAMES = ("heave", "roll", "ride_height_change", "track", "roll_center_y", "roll_center_z",
                     "rack_displacement")
EPS_GEOMETRIC = 1e-6  # primitives/constants.py:9


@dataclass
class D:
    """value + derivative along one direction."""

    v: float
    d: float = 0.0

    def __add__(self, o):
        o = _lift(o)
        return D(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = _lift(o)
        return D(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return _lift(o) - self

    def __neg__(self):
        return D(-self.v, -self.d)

    def __mul__(self, o):
        o = _lift(o)
        return D(self.v * o.v, self.v * o.d + self.d * o.v)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _lift(o)
        q = self.v / o.v
        return D(q, (self.d - q * o.d) / o.v)

    def __rtruediv__(self, o):
        return _lift(o) / self


def _lift(x) -> D:
    if isinstance(x, D):
        return x
    return D(float(x), 0.0) if isinstance(x, (int, float)) else D(x, 0.0)


def _fn(x, name: str):
    """``math.<name>`` for floats; the same function of mpmath for its numbers (the 50-digit runs that measure the
    rounding noise of a column, tools of the CPU tests only)."""
    if isinstance(x, float):
        return getattr(math, name)
    if isinstance(x, np.floating):  # numpy's extended precision (the differences of tests/test_metrics_oracle.py)
        return getattr(np, {"atan2": "arctan2", "atan": "arctan", "sqrt": "sqrt"}[name])
    import mpmath

    return getattr(mpmath, name)


def _deg(x):
    """180 / pi in the precision of ``x``."""
    if isinstance(x, float):
        return 180.0 / math.pi
    if isinstance(x, np.floating):
        return type(x)(180) / (4 * np.arctan(type(x)(1)))
    import mpmath

    return 180 / mpmath.pi


def atan2(y: D, x: D) -> D:
    return D(_fn(y.v, "atan2")(y.v, x.v), (x.v * y.d - y.v * x.d) / (x.v * x.v + y.v * y.v))


def atan(q: D) -> D:
    return D(_fn(q.v, "atan")(q.v), q.d / (1.0 + q.v * q.v))


def sqrt(a: D) -> D:
    r = _fn(a.v, "sqrt")(a.v)
    return D(r, a.d / (2.0 * r))


def dabs(a: D) -> D:
    return -a if a.v < 0 else a


def corner_metrics(pos: dict, vel: dict | None, side: float, design_wheel_center_z: float, number=float):
    """
    ``pos`` / ``vel``: role name -> xyz for wheel_center, contact_patch, axle_inboard, axle_outboard,
    steer_lower, steer_upper (+ optionally damper_top, damper_bottom).  Returns ``(values[19], derivatives[19])``
    with the first eight entries (and damper_length when its points are given) filled, NaN elsewhere;
    ``geometry_metrics`` below supplies the values of the rest.
    """
    def point(name):
        v = vel[name] if vel is not None else (0.0, 0.0, 0.0)
        return [D(number(pos[name][k]), number(v[k])) for k in range(3)]

    wc, cp = point("wheel_center"), point("contact_patch")
    axi, axo = point("axle_inboard"), point("axle_outboard")
    lower, upper = point("steer_lower"), point("steer_upper")
    axle = [axo[k] - axi[k] for k in range(3)]
    steer = [upper[k] - lower[k] for k in range(3)]
    deg = _deg(number(1.0))
    # angles.py:22-50: wheel_up = axle x X * -side
    up_y, up_z = -side * axle[2], side * axle[1]
    angle = atan2(up_y, up_z)
    camber = deg * (angle if side > 0 else -angle)
    caster = deg * atan2(-steer[0], steer[2])
    kpi = deg * atan2(-side * steer[1], steer[2])
    toe = deg * (atan2(axle[0], axle[1]) if side > 0 else atan2(axle[0], -axle[1]))
    travel = wc[2] - design_wheel_center_z
    half_track = cp[1] if cp[1].v >= 0 else -cp[1]
    t = (cp[2] - lower[2]) / steer[2]  # context.py:119-138
    gx, gy = lower[0] + t * steer[0], lower[1] + t * steer[1]
    an = sqrt(axle[0] * axle[0] + axle[1] * axle[1])
    scrub = -(((gx - cp[0]) * axle[0] + (gy - cp[1]) * axle[1]) / an)
    trail = gx - cp[0]
    out = [camber, caster, kpi, toe, travel, half_track, scrub, trail]
    values, derivs = np.full(len(METRIC_NAMES), np.nan), np.full(len(METRIC_NAMES), np.nan)
    values[:8], derivs[:8] = [float(o.v) for o in out], [float(o.d) for o in out]
    if "damper_top" in pos:  # travel.py:48-62 (the reference's deriv_damper_length_wrt_hub_z differentiates this)
        top, bottom = point("damper_top"), point("damper_bottom")
        strut = [top[k] - bottom[k] for k in range(3)]
        length = sqrt(strut[0] * strut[0] + strut[1] * strut[1] + strut[2] * strut[2])
        k = METRIC_NAMES.index("damper_length")
        values[k], derivs[k] = float(length.v), float(length.d)
    return values, derivs


# ---- instant centres, swing arms, anti-geometry, damper length, axle metrics (values only) ----


def _plane(a, b, c):
    """geometric.py:216-252."""
    normal = np.cross(b - a, c - a)
    mag = np.sqrt(np.dot(normal, normal))
    if mag < EPS_GEOMETRIC:
        return None
    n = normal / mag
    return n, -np.dot(n, a)


def _two_planes(n1, d1, n2, d2):
    """geometric.py:255-290."""
    direction = np.cross(n1, n2)
    m2 = np.dot(direction, direction)
    if m2 < EPS_GEOMETRIC * EPS_GEOMETRIC:
        return None
    point = np.cross(d2 * n1 - d1 * n2, direction) / m2
    return point, direction / np.sqrt(m2)


def _at_coordinate(point, direction, axis: int, value: float):
    """geometric.py:316-352."""
    if abs(direction[axis]) < EPS_GEOMETRIC:
        return None
    return point + (value - point[axis]) / direction[axis] * direction


def instant_axis(kind: str | None, pts, dtype=np.float64):
    """``compute_instant_axis``: ``two_planes`` (double wishbone) or ``plane_and_strut`` (MacPherson).  ``dtype``: the
    working precision (numpy's extended precision for the differences of tests/test_metrics_oracle.py)."""
    pts = [np.asarray(p, dtype=dtype) for p in pts]
    if kind == "two_planes":
        upper, lower = _plane(*pts[0:3]), _plane(*pts[3:6])
        if upper is None or lower is None:
            return None
        return _two_planes(*upper, *lower)
    if kind == "plane_and_strut":
        arm = _plane(*pts[0:3])
        if arm is None:
            return None
        strut = pts[3] - pts[2]
        axis = strut / np.sqrt(np.dot(strut, strut))
        return _two_planes(*arm, axis, -np.dot(axis, pts[3]))
    return None


def instant_centres(kind, pts, wheel_center, dtype=np.float64):
    """(SVIC, FVIC), each a point or None."""
    line = instant_axis(kind, pts, dtype)
    if line is None:
        return None, None
    return _at_coordinate(*line, 1, wheel_center[1]), _at_coordinate(*line, 0, wheel_center[0])


def _norm(v):
    return np.sqrt(np.dot(v, v))


def geometry_metrics(pos: dict, side: float, axis_kind, axis_points, damper=None, wheelbase=float("nan"),
                     cg_z=float("nan"), front_brake_bias=None, axle_position=None, driven_axle=None, dtype=np.float64) -> np.ndarray:
    """The eleven catalog entries after mechanical trail (METRIC_NAMES[8:]); None -> NaN.  ``dtype``: the working precision."""
    nan = float("nan")
    wc, cp = np.asarray(pos["wheel_center"], dtype), np.asarray(pos["contact_patch"], dtype)
    svic, fvic = instant_centres(axis_kind, axis_points, wc, dtype)
    out = dict.fromkeys(METRIC_NAMES[8:], nan)
    if damper is not None:
        out["damper_length"] = _norm(np.asarray(damper[0], dtype) - np.asarray(damper[1], dtype))
    if fvic is not None:
        out["fvic_y"], out["fvic_z"] = fvic[1], fvic[2]
        dy, dz = fvic[1] - cp[1], (fvic[2] - cp[2])
        out["fvsa_length"] = np.sqrt(dy * dy + dz * dz) * (-side * np.sign(dy))
    if svic is not None:
        out["svic_x"], out["svic_z"] = svic[0], svic[2]
        out["svsa_length"] = svic[0] - cp[0]
        run, rise = svic[0] - cp[0], svic[2] - cp[2]
        height = cg_z - cp[2]
        height_ok = height > EPS_GEOMETRIC
        if abs(run) >= EPS_GEOMETRIC:
            out["svsa_angle"] = _deg(dtype(1)) * np.arctan(rise / run)
            if height_ok and front_brake_bias is not None and axle_position == "front":
                out["anti_dive"] = 100.0 * front_brake_bias * (wheelbase / height) * (rise / (cp[0] - svic[0]))
            if height_ok and front_brake_bias is not None and axle_position == "rear":
                out["anti_lift"] = 100.0 * (1.0 - front_brake_bias) * (wheelbase / height) * (rise / run)
        if driven_axle is not None and axle_position is not None and driven_axle == axle_position:
            drive_run = wc[0] - svic[0] if axle_position == "front" else svic[0] - wc[0]
            if abs(drive_run) >= EPS_GEOMETRIC and height_ok:
                out["anti_squat"] = 100.0 * (wheelbase / height) * ((svic[2] - wc[2]) / drive_run)
    return np.array([out[k] for k in METRIC_NAMES[8:]], dtype=dtype)


def axle_metrics(sides: dict, dtype=np.float64) -> np.ndarray:
    """
    ``sides['left'|'right']`` = dict(wheel_center, contact_patch, design_wheel_center_z, design_contact_patch_z,
    axis_kind, axis_points, rack_y (or None), design_rack_y).  -> AXLE_METRIC_NAMES order, computed in ``dtype``.
    """
    nan = float("nan")
    wdz, cdz, cy, lines = {}, {}, {}, []
    for name in ("left", "right"):
        s = sides[name]
        wc, cp = np.asarray(s["wheel_center"], dtype), np.asarray(s["contact_patch"], dtype)
        wdz[name] = wc[2] - s["design_wheel_center_z"]
        cdz[name] = cp[2] - s["design_contact_patch_z"]
        cy[name] = cp[1]
        _, fvic = instant_centres(s["axis_kind"], s["axis_points"], wc, dtype)
        lines.append(None if fvic is None else (cp[1], cp[2], fvic[1] - cp[1], fvic[2] - cp[2]))
    track = abs(cy["left"] - cy["right"])
    rcy = rcz = nan
    if lines[0] is not None and lines[1] is not None:
        left, right = lines
        den = left[2] * right[3] - left[3] * right[2]
        if abs(den) >= EPS_GEOMETRIC:
            t = ((right[0] - left[0]) * right[3] - (right[1] - left[1]) * right[2]) / den
            rcy, rcz = left[0] + t * left[2], left[1] + t * left[3]
    rack = sides["left"].get("rack_y")
    return np.array([
        0.5 * (wdz["left"] + wdz["right"]),
        _deg(dtype(1)) * np.arctan2(wdz["left"] - wdz["right"], track),
        -0.5 * (cdz["left"] + cdz["right"]),
        track, rcy, rcz,
        nan if rack is None else dtype(rack) - sides["left"]["design_rack_y"],
    ], dtype=dtype)


def _rotation_of(cur, design, axis_point, axis_dir, scale):
    """``metrics/kernels.py:58-76`` for ``cur`` = current - axis point as duals; NaN for a point on the axis
    (``geometric.py:47-51`` raises there)."""
    dr = [float(design[k]) - float(axis_point[k]) for k in range(3)]
    a = [float(x) for x in axis_dir]
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]  # noqa: E731
    dd, cd = dot(dr, a), dot(cur, a)
    dperp = [dr[k] - dd * a[k] for k in range(3)]
    cperp = [cur[k] - cd * a[k] for k in range(3)]
    if math.sqrt(dot(dperp, dperp)) < EPS_GEOMETRIC or math.sqrt(float(dot(cperp, cperp).v)) < EPS_GEOMETRIC:
        return float("nan"), float("nan")
    cross = [dr[1] * cur[2] - dr[2] * cur[1], dr[2] * cur[0] - dr[0] * cur[2], dr[0] * cur[1] - dr[1] * cur[0]]
    angle = atan2(_lift(dot(a, cross)), _lift(dot(dperp, cperp)))
    deg = _deg(angle.v)
    return float(scale * deg * angle.v), float(scale * deg * angle.d)


def rotation_about_fixed_axis_deg(current, velocity, design, axis_point, axis_dir, scale: float = 1.0, number=float):
    """
    ``metrics/kernels.py:58-76`` (value, derivative along ``velocity``): signed rotation of ``current`` from
    ``design`` about the fixed axis, degrees, times ``scale`` (``Side.lateral_sign`` for the rocker angle).
    """
    v = velocity if velocity is not None else (0.0, 0.0, 0.0)
    cur = [D(number(current[k]), number(v[k])) - float(axis_point[k]) for k in range(3)]
    return _rotation_of(cur, design, axis_point, axis_dir, scale)


# ---- the same catalog on duals: (values, derivatives along one direction); NaN in both where the value is undefined ----


def _points(pos, vel, number):
    """xyz rows -> lists of three duals (``vel`` None: the zero direction)."""
    out = []
    for i, p in enumerate(pos):
        v = vel[i] if vel is not None else (0.0, 0.0, 0.0)
        out.append([D(number(p[k]), number(v[k])) for k in range(3)])
    return out


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _plane_dual(a, b, c):
    """geometric.py:216-252 on duals."""
    normal = _cross(_sub(b, a), _sub(c, a))
    m2 = _dot(normal, normal)
    if not _fn(m2.v, "sqrt")(m2.v) >= EPS_GEOMETRIC:
        return None
    mag = sqrt(m2)
    n = [x / mag for x in normal]
    return n, -_dot(n, a)


def _two_planes_dual(n1, d1, n2, d2):
    """geometric.py:255-290 on duals."""
    direction = _cross(n1, n2)
    m2 = _dot(direction, direction)
    if not m2.v >= EPS_GEOMETRIC * EPS_GEOMETRIC:
        return None
    point = [x / m2 for x in _cross([d2 * n1[k] - d1 * n2[k] for k in range(3)], direction)]
    mag = sqrt(m2)
    return point, [x / mag for x in direction]


def _at_coordinate_dual(point, direction, axis: int, value: D):
    """geometric.py:316-352 on duals."""
    if not abs(direction[axis].v) >= EPS_GEOMETRIC:
        return None
    t = (value - point[axis]) / direction[axis]
    return [point[k] + t * direction[k] for k in range(3)]


def instant_axis_dual(kind, pts):
    if kind == "two_planes":
        upper, lower = _plane_dual(*pts[0:3]), _plane_dual(*pts[3:6])
        if upper is None or lower is None:
            return None
        return _two_planes_dual(*upper, *lower)
    if kind == "plane_and_strut":
        arm = _plane_dual(*pts[0:3])
        if arm is None:
            return None
        strut = _sub(pts[3], pts[2])
        length = sqrt(_dot(strut, strut))
        axis = [x / length for x in strut]
        return _two_planes_dual(*arm, axis, -_dot(axis, pts[3]))
    return None


def instant_centres_dual(kind, pts, wheel_center):
    line = instant_axis_dual(kind, pts)
    if line is None:
        return None, None
    return _at_coordinate_dual(*line, 1, wheel_center[1]), _at_coordinate_dual(*line, 0, wheel_center[0])


def geometry_metric_duals(wc, cp, side: float, axis_kind, axis_points, damper=None, wheelbase=float("nan"),
                          cg_z=float("nan"), front_brake_bias=None, axle_position=None, driven_axle=None):
    """
    ``geometry_metrics`` on duals: ``wc``, ``cp``, ``axis_points`` and ``damper`` are points of three ``D`` each.
    ``swing_arms.py:45-88``, ``anti_geometry.py:32-206``, ``travel.py:48-62``.  -> name -> ``D`` or None.
    """
    svic, fvic = instant_centres_dual(axis_kind, axis_points, wc)
    out = dict.fromkeys(METRIC_NAMES[8:], None)
    if damper is not None:
        strut = _sub(damper[0], damper[1])
        out["damper_length"] = sqrt(_dot(strut, strut))
    if fvic is not None:
        out["fvic_y"], out["fvic_z"] = fvic[1], fvic[2]
        dy, dz = fvic[1] - cp[1], fvic[2] - cp[2]
        sign = 1.0 if dy.v > 0 else (-1.0 if dy.v < 0 else 0.0)  # swing_arms.py:62-88: np.sign, a constant of the state
        out["fvsa_length"] = sqrt(dy * dy + dz * dz) * (-side * sign)
    if svic is not None:
        out["svic_x"], out["svic_z"] = svic[0], svic[2]
        out["svsa_length"] = svic[0] - cp[0]
        run, rise = svic[0] - cp[0], svic[2] - cp[2]
        height = cg_z - cp[2]
        height_ok = height.v > EPS_GEOMETRIC
        if abs(run.v) >= EPS_GEOMETRIC:
            out["svsa_angle"] = _deg(run.v) * atan(rise / run)
            if height_ok and front_brake_bias is not None and axle_position == "front":
                out["anti_dive"] = 100.0 * front_brake_bias * (wheelbase / height) * (rise / (cp[0] - svic[0]))
            if height_ok and front_brake_bias is not None and axle_position == "rear":
                out["anti_lift"] = 100.0 * (1.0 - front_brake_bias) * (wheelbase / height) * (rise / run)
        if driven_axle is not None and axle_position is not None and driven_axle == axle_position:
            drive_run = wc[0] - svic[0] if axle_position == "front" else svic[0] - wc[0]
            if abs(drive_run.v) >= EPS_GEOMETRIC and height_ok:
                out["anti_squat"] = 100.0 * (wheelbase / height) * ((svic[2] - wc[2]) / drive_run)
    return out


def catalog_duals(spec: dict, pos, vel=None, number=float):
    """
    The whole corner catalog of one state along one direction: ``pos`` / ``vel`` = ``[n_out, 3]`` rows of the output
    points, ``spec`` = the six role indices (``wheel_center`` ... ``steer_upper``), ``side``, ``design_wheel_center_z``,
    ``axis_kind``, ``axis_idx``, ``damper_idx`` (or None) and the vehicle numbers (``wheelbase``, ``cg_z``,
    ``front_brake_bias``, ``axle_position``, ``driven_axle``).  -> ``(values[19], derivatives[19])`` as float64.
    """
    basic = ("wheel_center", "contact_patch", "axle_inboard", "axle_outboard", "steer_lower", "steer_upper")
    zero = np.zeros(3)
    values, derivs = corner_metrics({k: pos[spec[k]] for k in basic},
                                    {k: (vel[spec[k]] if vel is not None else zero) for k in basic},
                                    spec["side"], spec["design_wheel_center_z"], number)
    pts = _points(pos, vel, number)
    damper = spec.get("damper_idx")
    rest = geometry_metric_duals(
        pts[spec["wheel_center"]], pts[spec["contact_patch"]], spec["side"], spec.get("axis_kind"),
        [pts[i] for i in spec.get("axis_idx", ())], damper=None if not damper else (pts[damper[0]], pts[damper[1]]),
        wheelbase=spec.get("wheelbase", float("nan")), cg_z=spec.get("cg_z", float("nan")),
        front_brake_bias=spec.get("front_brake_bias"), axle_position=spec.get("axle_position"),
        driven_axle=spec.get("driven_axle"))
    for k, name in enumerate(METRIC_NAMES[8:], start=8):
        d = rest[name]
        values[k], derivs[k] = (float("nan"), float("nan")) if d is None else (float(d.v), float(d.d))
    return values, derivs


def catalog_values(spec: dict, pos, dtype=np.float64) -> np.ndarray:
    """The values-only path over the same ``spec``: ``corner_metrics`` (first eight) + ``geometry_metrics`` (numpy),
    computed in ``dtype`` (float64, or numpy's extended precision for differences with less rounding noise)."""
    basic = ("wheel_center", "contact_patch", "axle_inboard", "axle_outboard", "steer_lower", "steer_upper")
    values, _ = corner_metrics({k: pos[spec[k]] for k in basic}, None, spec["side"], spec["design_wheel_center_z"])
    values = values.astype(dtype)  # (the first eight: short formulas, float64 throughout)
    damper = spec.get("damper_idx")
    values[8:] = geometry_metrics(
        {"wheel_center": pos[spec["wheel_center"]], "contact_patch": pos[spec["contact_patch"]]}, spec["side"],
        spec.get("axis_kind"), [pos[i] for i in spec.get("axis_idx", ())],
        damper=None if not damper else (pos[damper[0]], pos[damper[1]]), wheelbase=spec.get("wheelbase", float("nan")),
        cg_z=spec.get("cg_z", float("nan")), front_brake_bias=spec.get("front_brake_bias"),
        axle_position=spec.get("axle_position"), driven_axle=spec.get("driven_axle"), dtype=dtype)
    return values


def axle_metric_duals(left: dict, right: dict, pos, vel=None, number=float):
    """
    ``axle_metrics.py:21-95`` on duals.  ``left`` / ``right`` = ``catalog_duals`` specs with ``design_contact_patch_z``,
    ``rack_idx`` (or None) and ``design_rack_y`` added.  -> ``(values[7], derivatives[7])``.
    """
    pts = _points(pos, vel, number)
    wdz, cdz, cy, lines = [], [], [], []
    for s in (left, right):
        wc, cp = pts[s["wheel_center"]], pts[s["contact_patch"]]
        wdz.append(wc[2] - s["design_wheel_center_z"])
        cdz.append(cp[2] - s["design_contact_patch_z"])
        cy.append(cp[1])
        _, fvic = instant_centres_dual(s.get("axis_kind"), [pts[i] for i in s.get("axis_idx", ())], wc)
        lines.append(None if fvic is None else (cp[1], cp[2], fvic[1] - cp[1], fvic[2] - cp[2]))
    track = dabs(cy[0] - cy[1])
    rcy = rcz = None
    if lines[0] is not None and lines[1] is not None:
        a, b = lines
        den = a[2] * b[3] - a[3] * b[2]
        if abs(den.v) >= EPS_GEOMETRIC:
            t = ((b[0] - a[0]) * b[3] - (b[1] - a[1]) * b[2]) / den
            rcy, rcz = a[0] + t * a[2], a[1] + t * a[3]
    rack = left.get("rack_idx")
    out = [
        0.5 * (wdz[0] + wdz[1]),
        _deg(track.v) * atan2(wdz[0] - wdz[1], track),
        -0.5 * (cdz[0] + cdz[1]),
        track, rcy, rcz,
        None if rack is None else pts[rack][1] - left["design_rack_y"],
    ]
    nan = float("nan")
    return (np.array([nan if o is None else float(o.v) for o in out]),
            np.array([nan if o is None else float(o.d) for o in out]))


def axle_sides_from_specs(left: dict, right: dict, pos) -> dict:
    """The input of the values-only ``axle_metrics`` from the two specs of ``axle_metric_duals``."""
    sides = {}
    for tag, s in (("left", left), ("right", right)):
        rack = s.get("rack_idx")
        sides[tag] = dict(
            wheel_center=pos[s["wheel_center"]], contact_patch=pos[s["contact_patch"]],
            design_wheel_center_z=s["design_wheel_center_z"], design_contact_patch_z=s["design_contact_patch_z"],
            axis_kind=s.get("axis_kind"), axis_points=[pos[i] for i in s.get("axis_idx", ())],
            rack_y=None if rack is None else pos[rack][1], design_rack_y=s.get("design_rack_y", 0.0))
    return sides


def angle_arguments(spec: dict, pos) -> dict:
    """The ``(y, x)`` handed to atan2 by the four angle metrics of ``corner_metrics`` (angles.py:22-132), per name."""
    side = spec["side"]
    axle = np.asarray(pos[spec["axle_outboard"]], float) - np.asarray(pos[spec["axle_inboard"]], float)
    steer = np.asarray(pos[spec["steer_upper"]], float) - np.asarray(pos[spec["steer_lower"]], float)
    return {"camber": (-side * axle[2], side * axle[1]), "caster": (-steer[0], steer[2]),
            "kpi": (-side * steer[1], steer[2]), "roadwheel_angle": (axle[0], axle[1] if side > 0 else -axle[1])}


# Role sets over the fifteen output points of the double-wishbone corner fixture (tests/golden/c1_dw_corner.npz: 0-5 the
# wishbone pickups, 6/7 the track rod, 8/9 the wheel axis, 11 wheel centre, 14 contact patch), chosen so that the angle
# metrics' atan2 arguments leave the small first-quadrant angles of a real corner: wheel axis and steering axis are
# laid through other links' points.  ``okx_corner_roles`` takes any output point in any role.
_C1_PLANES = (3, 4, 5, 0, 1, 2)
_C1_VEHICLE = dict(wheelbase=2500.0, cg_z=450.0)
C1_ROLE_SETS = {
    # wheel axis track rod end -> upper ball joint, steering axis lower front pickup -> track rod end; front, driven
    "steep_axes": dict(wheel_center=11, contact_patch=14, axle_inboard=7, axle_outboard=5, steer_lower=0, steer_upper=7,
                       side=1.0, axis_kind="two_planes", axis_idx=_C1_PLANES, damper_idx=(5, 6), front_brake_bias=0.65,
                       axle_position="front", driven_axle="front", **_C1_VEHICLE),
    # right-hand signs, the steering axis pointing down (x < 0 for caster and KPI); rear, driven
    "right_hand_down": dict(wheel_center=11, contact_patch=14, axle_inboard=1, axle_outboard=5, steer_lower=5, steer_upper=0,
                            side=-1.0, axis_kind="two_planes", axis_idx=_C1_PLANES, damper_idx=None, front_brake_bias=0.65,
                            axle_position="rear", driven_axle="rear", **_C1_VEHICLE),
    # the first instant-axis plane through one point twice: no instant axis, the first eight columns stay defined
    "degenerate_plane": dict(wheel_center=11, contact_patch=14, axle_inboard=7, axle_outboard=2, steer_lower=3, steer_upper=7,
                             side=1.0, axis_kind="two_planes", axis_idx=(3, 3, 5, 0, 1, 2), damper_idx=None,
                             front_brake_bias=0.65, axle_position="front", driven_axle="front", **_C1_VEHICLE),
    # brake bias unset (anti-dive / anti-lift undefined, anti-squat defined), the two planes in the other order
    "no_brake_bias": dict(wheel_center=11, contact_patch=14, axle_inboard=0, axle_outboard=8, steer_lower=1, steer_upper=5,
                          side=-1.0, axis_kind="two_planes", axis_idx=(0, 1, 2, 3, 4, 5), damper_idx=None,
                          front_brake_bias=None, axle_position="front", driven_axle="front", **_C1_VEHICLE),
}


def corner_roles_from_spec(spec: dict):
    """``okx_corner_roles`` of a ``catalog_duals`` spec (the package's ctypes mirror; imported here on use only)."""
    from open_kinematics_amd.metrics import make_roles

    damper = spec.get("damper_idx")
    return make_roles(
        wheel_center=spec["wheel_center"], contact_patch=spec["contact_patch"], axle_inboard=spec["axle_inboard"],
        axle_outboard=spec["axle_outboard"], steer_lower=spec["steer_lower"], steer_upper=spec["steer_upper"],
        side_sign=spec["side"], design_wheel_center_z=spec["design_wheel_center_z"],
        instant_axis=None if spec.get("axis_kind") is None else (spec["axis_kind"], tuple(spec["axis_idx"])),
        damper=tuple(damper) if damper else None, rack_attachment=-1 if spec.get("rack_idx") is None else spec["rack_idx"],
        design_contact_patch_z=spec.get("design_contact_patch_z", 0.0), design_rack_y=spec.get("design_rack_y", 0.0),
        wheelbase=spec.get("wheelbase", float("nan")), cg_z=spec.get("cg_z", float("nan")),
        front_brake_bias=spec.get("front_brake_bias"), axle_position=spec.get("axle_position"),
        driven_axle=spec.get("driven_axle"))


ROLE_KINDS = ("axis_rotation", "midpoint_rotation", "stem_twist", "distance", "midpoint_coordinate")


def role_value(kind: str, a, b, design, axis_point, axis_dir, scale: float = 1.0):
    """
    Values only, numpy: a rotation / hardware role of an axle (``metrics/kernels.py:58-76``;
    ``axle/mechanisms.py:718-815,903-944``).  ``a`` (and ``b`` for the two-point kinds) = current points; ``design`` = the
    design point (rotations), ``(design twist in degrees, -, -)`` for ``stem_twist``; ``axis_point`` = a point of the fixed
    axis / the T-bar pivot; ``axis_dir`` = the unit axis / lateral reference / coordinate direction.  Computed in the
    precision of ``a`` / ``b``.
    """
    a, axis_point, u = np.asarray(a), np.asarray(axis_point, float), np.asarray(axis_dir, float)
    design = np.asarray(design, float)
    if kind != "axis_rotation":
        b = np.asarray(b)
        if kind == "distance":
            return _norm(a - b)
        mid = a + (b - a) / 2.0
        if kind == "midpoint_coordinate":
            return np.dot(u, mid - axis_point)
        if kind == "stem_twist":
            stem = mid - axis_point
            length = _norm(stem)
            if length < EPS_GEOMETRIC:
                return float("nan")
            stem = stem / length
            crossbar = (a - b) - stem * np.dot(a - b, stem)
            twist = np.arctan2(np.dot(stem, np.cross(u, crossbar)), np.dot(u, crossbar))
            return _deg(twist) * twist - design[0]
        a = mid
    dr, cr = design - axis_point, a - axis_point
    dperp, cperp = dr - np.dot(dr, u) * u, cr - np.dot(cr, u) * u
    if _norm(dperp) < EPS_GEOMETRIC or _norm(cperp) < EPS_GEOMETRIC:
        return float("nan")
    angle = np.arctan2(np.dot(u, np.cross(dr, cr)), np.dot(dperp, cperp))
    return scale * _deg(angle) * angle


def role_dual(kind: str, a, va, b, vb, design, axis_point, axis_dir, scale: float = 1.0, number=float):
    """``role_value`` on duals: ``(value, derivative)`` along the velocities ``va`` / ``vb`` of the two points."""
    zero = (0.0, 0.0, 0.0)
    if kind == "axis_rotation":
        return rotation_about_fixed_axis_deg(a, va, design, axis_point, axis_dir, scale, number)
    pa, pb = _points([a, b], [va if va is not None else zero, vb if vb is not None else zero], number)
    u = [float(x) for x in axis_dir]
    span = _sub(pa, pb)
    if kind == "distance":
        out = sqrt(_dot(span, span))
        return float(out.v), float(out.d)
    mid = [pa[k] + (pb[k] - pa[k]) / 2.0 for k in range(3)]
    rel = [mid[k] - float(axis_point[k]) for k in range(3)]
    if kind == "midpoint_coordinate":
        out = _dot(u, rel)
        return float(out.v), float(out.d)
    if kind == "stem_twist":
        m2 = _dot(rel, rel)
        if not _fn(m2.v, "sqrt")(m2.v) >= EPS_GEOMETRIC:
            return float("nan"), float("nan")
        length = sqrt(m2)
        stem = [x / length for x in rel]
        along = _dot(stem, span)
        crossbar = [span[k] - stem[k] * along for k in range(3)]
        twist = _deg(m2.v) * atan2(_lift(_dot(stem, _cross(u, crossbar))), _lift(_dot(u, crossbar)))
        return float(twist.v) - float(design[0]), float(twist.d)
    return _rotation_of(rel, design, axis_point, axis_dir, scale)


