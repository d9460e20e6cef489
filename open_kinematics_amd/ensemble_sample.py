"""
The definition of ``okx_ensemble_sample`` in NumPy: perturbed-geometry ensembles drawn by a COUNTER-BASED sampler.  Geometry
``g``'s draw is a pure function of ``(seed, g, latent index, attempt)`` - no draw depends on another - so a rank makes its
own shard, a chunk its own rows, and every split of an ensemble carries the same bits.  The device pass equals this module
bit for bit in all four outputs; every step below is IEEE add, multiply, divide or sqrt, each rounded on its own (no fused
multiply-add, no libm call), or integer arithmetic.

Bits: Philox4x32-10, key = (seed low word, seed high word), counter = (g low word, g high word, latent index z,
attempt | purpose << 8) with purpose ``PURPOSE_DRAW`` for a latent's uniform and ``PURPOSE_STRATA`` (g = 0, attempt = 0) for
the four round keys of latent z's stratum permutation.  Output words 0 and 1 of a draw give 52 bits ``k = w0 << 20 | w1 >> 12``
and ``u' = (k + 0.5) * 2^-52``, exact and never 0 or 1.

Strata (``LHS``): latent z's stratum of geometry g is ``pi_z(g)``, a keyed bijection of ``[0, n_total)``: a four-round Feistel
network on ``b`` bits - the smallest even b >= 2 with ``2^b >= n_total`` - walked until the value lies below ``n_total``;
the round function is a 32-bit integer mix of the right half plus the round key.  ``u = (pi + u') / n_total`` (one rounded
add, one rounded divide), clamped into ``[2^-53, 1 - 2^-53]``.  A redraw keeps the stratum and redraws ``u'`` only, so the
strata of a latent stay a permutation whatever the guards do.  ``IID``: ``u = u'``.

Kinds: ``UNIFORM`` is ``2 u - 1``; ``NORMAL`` is ``ppnd16(u)``, Wichura's AS241 inverse normal CDF with the tail's logarithm
written out (``log_unit``); ``TRUNCATED`` (to ``[-k, k]``) is ``ppnd16(Phi(-k) + u (Phi(k) - Phi(-k)))`` clamped into
``[-k, k]`` - the two constants come from the host's ``erfc`` once per plan (``SamplePlan.bound_table``) and travel with it.

Delta: ``delta_f = sum_z mixing[f][z] * latent_z``, ascending in z from 0.0, every product and sum rounded; without ``mixing``
``delta_f = scale_f * latent_f``.  ``hardpoints`` is ``nominal`` with ``nominal[c] + delta_f`` at ``c = coords[f]``.

Guards: a draw that fails one is drawn again with the next attempt number; the first valid attempt is kept.
``flags[g]`` bit 0: no attempt was valid and the last one stands (the sense of the screen's flag byte: 0 passes); bits 4-7:
the attempt kept.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

NORMAL, UNIFORM, TRUNCATED = 0, 1, 2
IID, LHS = 0, 1
GUARD_SIGN, GUARD_DISTINCT, GUARD_OFF_LINE = 0, 1, 2
PURPOSE_DRAW, PURPOSE_STRATA = 0, 1
PURPOSE_BOOTSTRAP = 2  # OKX_SAMPLE_PURPOSE_BOOTSTRAP: the Poisson weights of ensemble_stats.bootstrap_weights
MAX_COORDS = 288      # OKX_ENS_SAMPLE_MAX_COORDS (= 3 * OKX_MAX_POINTS)
MAX_LATENTS = 288     # OKX_ENS_SAMPLE_MAX_LATENTS
MAX_GUARDS = 16       # OKX_ENS_SAMPLE_MAX_GUARDS
MAX_ATTEMPTS = 16     # OKX_ENS_SAMPLE_MAX_ATTEMPTS
MAX_POINTS = 96       # OKX_MAX_POINTS

_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

U_MIN = 2.0 ** -53
U_MAX = 1.0 - 2.0 ** -53


def philox4x32_10(counter, key):
    """Philox4x32-10 of ``counter`` (four uint32 arrays that broadcast) under ``key`` (two): four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def _seed_key(seed: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def draw_bits(seed: int, g, z, attempt):
    """The 52 bits ``k`` of (seed, g, z, attempt), uint64; the arguments broadcast."""
    g = np.asarray(g, dtype=np.uint64)
    c3 = (np.asarray(attempt, dtype=np.uint64) & np.uint64(0xFF)) | np.uint64(PURPOSE_DRAW << 8)
    w0, w1, _, _ = philox4x32_10((g & _M32, g >> np.uint64(32), np.asarray(z, dtype=np.uint64), c3), _seed_key(seed))
    return (w0.astype(np.uint64) << np.uint64(20)) | (w1.astype(np.uint64) >> np.uint64(12))


def unit_from_bits(k):
    """``u' = (k + 0.5) * 2^-52`` of 52 bits k: exact, inside (0, 1)."""
    return (np.asarray(k, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -52


def strata_bits(n_total: int) -> int:
    """The Feistel network's width: the smallest even b >= 2 with 2^b >= n_total."""
    b = 2
    while (1 << b) < int(n_total):
        b += 2
    return b


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def strata_keys(seed: int, z):
    """The four round keys of latent z's permutation (uint64 arrays holding 32-bit words)."""
    z = np.asarray(z, dtype=np.uint64)
    zero = np.zeros_like(z)
    return tuple(w.astype(np.uint64) for w in philox4x32_10((zero, zero, z, zero + np.uint64(PURPOSE_STRATA << 8)), _seed_key(seed)))


def stratum(seed: int, n_total: int, g, z):
    """``pi_z(g)``: the stratum of geometry g (< n_total <= 2^32) under latent z, uint64; g and z broadcast."""
    n_total = int(n_total)
    half = np.uint64(strata_bits(n_total) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    keys = strata_keys(seed, z)  # (per latent; broadcast over the geometries below)
    g, z = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(z, dtype=np.uint64))
    keys = tuple(np.broadcast_to(k, g.shape) for k in keys)
    x = g.copy()
    walking = np.ones(x.shape, dtype=bool)
    while walking.any():
        v = x[walking]
        left, right = v >> half, v & mask
        for r in range(4):
            left, right = right, left ^ (_mix32(right + keys[r][walking]) & mask)
        v = (left << half) | right
        x[walking] = v
        walking[walking] = v >= np.uint64(n_total)
    return x


# ---- the inverse normal CDF: AS241 (PPND16), the tail's log written out ----

_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)
PPND_SPLIT1, PPND_CONST1, PPND_CONST2, PPND_SPLIT2 = 0.425, 0.180625, 1.6, 5.0

LN2 = 0.6931471805599453
SQRT_HALF = 0.7071067811865476
# log(m) = 2 s (1 + s^2 / 3 + s^4 / 5 + ...), s = (m - 1) / (m + 1): the coefficients 1 / (2 n + 1), n = 0 .. 10
_LOG = tuple(1.0 / (2 * n + 1) for n in range(11))


def _horner(coefficients, r):
    acc = np.full_like(r, coefficients[-1])
    for c in coefficients[-2::-1]:
        acc = acc * r + c
    return acc


def log_unit(x):
    """``log(x)`` of normal positive doubles by frexp and a polynomial in + - * / alone: x = m 2^e with m in [sqrt(1/2), sqrt(2)),
    ``log x = e ln2 + 2 s P(s^2)``, ``s = (m - 1) / (m + 1)``; |error| below 1e-14 on [2^-53, 1]."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    small = m < SQRT_HALF
    m = np.where(small, m * 2.0, m)
    e = np.where(small, e - 1, e).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    return e * LN2 + (2.0 * s) * _horner(_LOG, s * s)


def ppnd16(u):
    """``Phi^-1(u)`` for u in (0, 1): AS241's three regions, Horner sums, one divide each; within 1e-12 of the true value."""
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    with np.errstate(all="ignore"):
        central = np.abs(q) <= PPND_SPLIT1
        r0 = PPND_CONST1 - q * q
        v0 = q * _horner(_A, r0) / _horner(_B, r0)
        tail = np.where(central, 0.5, np.where(q < 0.0, u, 1.0 - u))
        r = np.sqrt(-log_unit(tail))
        r1 = r - PPND_CONST2
        v1 = _horner(_C, r1) / _horner(_D, r1)
        r2 = r - PPND_SPLIT2
        v2 = _horner(_E, r2) / _horner(_F, r2)
        v = np.where(r <= PPND_SPLIT2, v1, v2)
        v = np.where(q < 0.0, -v, v)
    return np.where(central, v0, v)


@dataclass(frozen=True)
class SamplePlan:
    """
    What an ensemble is drawn from.  ``nominal [P, 3]``; ``coords [F]`` int32, distinct flat indices ``p * 3 + axis`` of the
    perturbed coordinates; ``kind [Z]`` (``NORMAL`` / ``UNIFORM`` / ``TRUNCATED``) and ``bound [Z]`` (the k of ``TRUNCATED``, ignored
    otherwise) of the latents; ``mixing [F, Z]`` or None - then ``Z == F`` and ``scale [F]`` multiplies latent f; ``stratify``
    ``IID`` or ``LHS`` with ``n_total`` strata (the size of the WHOLE ensemble); ``seed`` a uint64; ``guards`` a tuple of at most 16
    ``(GUARD_SIGN, coordinate, sign, eps)``, ``(GUARD_DISTINCT, a, b, eps)`` or ``(GUARD_OFF_LINE, a, b, c, eps)`` over point
    indices; ``max_attempts`` 1 .. 16.  ``names``: the factor names of the latents (optional; see ``factor_names``).
    """

    nominal: np.ndarray
    coords: np.ndarray
    kind: np.ndarray
    bound: np.ndarray | None = None
    mixing: np.ndarray | None = None
    scale: np.ndarray | None = None
    stratify: int = IID
    n_total: int = 0
    seed: int = 0
    guards: tuple = ()
    max_attempts: int = 1
    names: tuple | None = field(default=None, compare=False)

    def __post_init__(self):
        who = "okx_ensemble_sample"
        put = lambda name, value: object.__setattr__(self, name, value)  # noqa: E731
        nominal = np.ascontiguousarray(np.asarray(self.nominal, dtype=np.float64))
        if nominal.ndim != 2 or nominal.shape[1] != 3 or not 1 <= nominal.shape[0] <= MAX_POINTS:
            raise ValueError(f"{who}: nominal must be [P, 3] with 1 <= P <= {MAX_POINTS}")
        coords = np.ascontiguousarray(np.asarray(self.coords, dtype=np.int32).reshape(-1))
        kind = np.asarray(self.kind, dtype=np.int32)
        if kind.ndim == 0:  # one kind for every latent
            kind = np.broadcast_to(kind, (coords.size if self.mixing is None else np.shape(self.mixing)[1],))
        kind = np.ascontiguousarray(kind.reshape(-1))
        z = kind.size
        bound = np.ones(z) if self.bound is None else np.ascontiguousarray(np.broadcast_to(np.asarray(self.bound, dtype=np.float64), (z,)))
        mixing = None if self.mixing is None else np.ascontiguousarray(np.asarray(self.mixing, dtype=np.float64))
        scale = None
        if mixing is None:
            scale = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if self.scale is None else self.scale, dtype=np.float64), (coords.size,)))
            if z != coords.size:
                raise ValueError(f"{who}: without mixing every coordinate has its own latent ({z} latents, {coords.size} coordinates)")
        elif mixing.shape != (coords.size, z):
            raise ValueError(f"{who}: mixing must be [{coords.size}, {z}], got {list(mixing.shape)}")
        elif self.scale is not None:
            raise ValueError(f"{who}: scale applies without mixing only")
        guards = tuple(_normal_guard(gd) for gd in self.guards)
        for name, value in (("nominal", nominal), ("coords", coords), ("kind", kind), ("bound", bound), ("mixing", mixing), ("scale", scale),
                            ("guards", guards), ("stratify", int(self.stratify)), ("n_total", int(self.n_total)),
                            ("seed", int(self.seed) & 0xFFFFFFFFFFFFFFFF), ("max_attempts", int(self.max_attempts))):
            put(name, value)
        for a in (nominal, coords, kind, bound, mixing, scale):
            if a is not None:
                a.setflags(write=False)
        check_plan(self)

    n_points = property(lambda self: int(self.nominal.shape[0]))
    n_coords = property(lambda self: int(self.coords.size))
    n_latents = property(lambda self: int(self.kind.size))

    def bound_table(self) -> np.ndarray:
        """``[Z, 3]``: k, ``Phi(-k)`` and ``Phi(k) - Phi(-k)`` of every latent (the table the device reads; (1, 0, 1) where the kind
        is not ``TRUNCATED``).  The two constants are the host's ``erfc``, taken once: they are part of the plan."""
        table = np.zeros((self.n_latents, 3))
        table[:, 0], table[:, 2] = 1.0, 1.0
        for i in np.flatnonzero(self.kind == TRUNCATED):
            k = float(self.bound[i])
            below = 0.5 * math.erfc(k / math.sqrt(2.0))
            table[i] = k, below, (1.0 - below) - below
        return table

    def guard_table(self):
        """``(ints [n, 4] int32: kind, a, b, c; reals [n, 2]: eps, sign)``, the form the guards travel in."""
        ints, reals = np.zeros((len(self.guards), 4), dtype=np.int32), np.zeros((len(self.guards), 2))
        for i, (kind, a, b, c, eps, sign) in enumerate(self.guards):
            ints[i], reals[i] = (kind, a, b, c), (eps, sign)
        return ints, reals

    def factor_names(self) -> list:
        """The names of the latents as factors: ``names`` when the plan carries them; else, without ``mixing``, the coordinate each
        latent moves (``"point7.x"``, as ``ensemble_stats.hardpoint_factors`` names them); else ``"latent<z>"``."""
        if self.names is not None:
            return list(self.names)
        if self.mixing is None:
            return [f"point{int(c) // 3}.{'xyz'[int(c) % 3]}" for c in self.coords]
        return [f"latent{z}" for z in range(self.n_latents)]


def _normal_guard(guard) -> tuple:
    """A guard as ``(kind, a, b, c, eps, sign)``."""
    guard = tuple(guard)
    kind = int(guard[0]) if guard else -1
    if kind == GUARD_SIGN and len(guard) == 4:
        return kind, int(guard[1]), 0, 0, float(guard[3]), float(guard[2])
    if kind == GUARD_DISTINCT and len(guard) == 4:
        return kind, int(guard[1]), int(guard[2]), 0, float(guard[3]), 1.0
    if kind == GUARD_OFF_LINE and len(guard) == 5:
        return kind, int(guard[1]), int(guard[2]), int(guard[3]), float(guard[4]), 1.0
    if len(guard) == 6:
        return kind, int(guard[1]), int(guard[2]), int(guard[3]), float(guard[4]), float(guard[5])
    raise ValueError(f"okx_ensemble_sample: a guard is (SIGN, coordinate, sign, eps), (DISTINCT, a, b, eps) or (OFF_LINE, a, b, c, eps), got {guard!r}")


def check_arguments(n_geometries, geometry_offset, n_total, n_points, coords, kind, bound, has_mixing, guards, stratify, max_attempts) -> None:
    """``okx_ensemble_sample_check`` on the host: ValueError in its words."""
    who = "okx_ensemble_sample"
    n, off, n_total, p = int(n_geometries), int(geometry_offset), int(n_total), int(n_points)
    coords, kind, bound = np.asarray(coords).reshape(-1), np.asarray(kind).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    f, z = coords.size, kind.size
    if n < 0 or off < 0 or n_total < 0:
        raise ValueError(f"{who}: negative n_geometries, geometry_offset or n_total")
    if not 1 <= p <= MAX_POINTS:
        raise ValueError(f"{who}: {p} points, 1 to {MAX_POINTS} allowed")
    if not 1 <= f <= MAX_COORDS:
        raise ValueError(f"{who}: {f} coordinates, 1 to {MAX_COORDS} allowed")
    if not 1 <= z <= MAX_LATENTS:
        raise ValueError(f"{who}: {z} latents, 1 to {MAX_LATENTS} allowed")
    if not has_mixing and z != f:
        raise ValueError(f"{who}: without mixing every coordinate has its own latent ({z} latents, {f} coordinates)")
    seen = set()
    for i, c in enumerate(coords.tolist()):
        if not 0 <= c < 3 * p:
            raise ValueError(f"{who}: coordinate {i} is {c}, outside [0, {3 * p})")
        if c in seen:
            raise ValueError(f"{who}: coordinate {i} repeats index {c}")
        seen.add(c)
    for i, (k, b) in enumerate(zip(kind.tolist(), bound.tolist())):
        if k not in (NORMAL, UNIFORM, TRUNCATED):
            raise ValueError(f"{who}: kind {i} is {k}, not 0 (normal), 1 (uniform) or 2 (truncated)")
        if k == TRUNCATED and not (math.isfinite(b) and b > 0.0):
            raise ValueError(f"{who}: bound {i} is {b:g}, not finite and greater than 0")
    if len(guards) > MAX_GUARDS:
        raise ValueError(f"{who}: {len(guards)} guards, at most {MAX_GUARDS}")
    for i, (gk, a, b, c, eps, sign) in enumerate(guards):
        if gk not in (GUARD_SIGN, GUARD_DISTINCT, GUARD_OFF_LINE):
            raise ValueError(f"{who}: guard {i} has kind {gk}, not 0 (sign), 1 (distinct) or 2 (off line)")
        limit = 3 * p if gk == GUARD_SIGN else p
        used = (a,) if gk == GUARD_SIGN else (a, b) if gk == GUARD_DISTINCT else (a, b, c)
        if any(not 0 <= v < limit for v in used):
            raise ValueError(f"{who}: guard {i} names an index outside [0, {limit})")
        if not math.isfinite(eps) or (gk == GUARD_SIGN and sign not in (1.0, -1.0)):
            raise ValueError(f"{who}: guard {i} needs a finite eps (and a sign of +1 or -1)")
    if stratify not in (IID, LHS):
        raise ValueError(f"{who}: stratify is {stratify}, not 0 (iid) or 1 (lhs)")
    if not 1 <= int(max_attempts) <= MAX_ATTEMPTS:
        raise ValueError(f"{who}: max_attempts is {max_attempts}, 1 to {MAX_ATTEMPTS} allowed")
    if stratify == LHS:
        if n_total > 1 << 32:
            raise ValueError(f"{who}: {n_total} strata, at most 2^32 under LHS")
        if off + n > n_total:
            raise ValueError(f"{who}: geometries [{off}, {off + n}) lie outside the {n_total} strata")


def check_plan(plan: SamplePlan, lo: int = 0, hi: int = 0) -> None:
    check_arguments(hi - lo, lo, plan.n_total, plan.n_points, plan.coords, plan.kind, plan.bound, plan.mixing is not None, plan.guards,
                    plan.stratify, plan.max_attempts)


def latents_from_units(plan: SamplePlan, u) -> np.ndarray:
    """The latents ``[n, Z]`` of the uniforms ``u [n, Z]`` by the plan's kinds."""
    u = np.asarray(u, dtype=np.float64)
    out = np.empty_like(u)
    table = plan.bound_table()
    for kind in (NORMAL, UNIFORM, TRUNCATED):
        cols = np.flatnonzero(plan.kind == kind)
        if not cols.size:
            continue
        v = u[:, cols]
        if kind == UNIFORM:
            out[:, cols] = 2.0 * v - 1.0
        elif kind == NORMAL:
            out[:, cols] = ppnd16(v)
        else:
            k, below, width = table[cols, 0], table[cols, 1], table[cols, 2]
            v = np.minimum(np.maximum(below + v * width, U_MIN), U_MAX)
            out[:, cols] = np.minimum(np.maximum(ppnd16(v), -k), k)
    return out


def stratified_unit(strata, up, n_total: int) -> np.ndarray:
    """``u = (pi + u') / n_total`` - one rounded add, one rounded divide - clamped into ``[2^-53, 1 - 2^-53]``: without the clamp
    ``pi = n - 1`` with ``u'`` near 1 rounds to 1 and the normal map returns infinity."""
    u = (np.asarray(strata).astype(np.float64) + np.asarray(up, dtype=np.float64)) / float(n_total)
    return np.minimum(np.maximum(u, U_MIN), U_MAX)


def units(plan: SamplePlan, g, attempt, strata=None) -> np.ndarray:
    """The uniforms ``[n, Z]`` of geometries ``g [n]`` (global indices) at ``attempt`` (a number or ``[n]``); ``strata [n, Z]``
    under ``LHS`` (None: computed)."""
    g = np.asarray(g, dtype=np.uint64).reshape(-1, 1)
    z = np.arange(plan.n_latents, dtype=np.uint64)[None]
    up = unit_from_bits(draw_bits(plan.seed, g, z, np.asarray(attempt, dtype=np.uint64).reshape(-1, 1)))
    if plan.stratify != LHS:
        return up
    if strata is None:
        strata = stratum(plan.seed, plan.n_total, g, z)
    return stratified_unit(strata, up, plan.n_total)


def contract(plan: SamplePlan, latents) -> np.ndarray:
    """``delta [n, F]`` of ``latents [n, Z]``."""
    if plan.mixing is None:
        return plan.scale[None] * latents
    acc = np.zeros((latents.shape[0], plan.n_coords))
    for z in range(plan.n_latents):
        acc = acc + plan.mixing[None, :, z] * latents[:, z, None]
    return acc


def guards_hold(plan: SamplePlan, points) -> np.ndarray:
    """``[n]`` bool: every guard of the plan holds for ``points [n, P, 3]``.  Sums of three squares are ``(x^2 + y^2) + z^2``."""
    ok = np.ones(points.shape[0], dtype=bool)
    flat = points.reshape(points.shape[0], -1)

    def norm(v):
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])

    with np.errstate(all="ignore"):
        for kind, a, b, c, eps, sign in plan.guards:
            if kind == GUARD_SIGN:
                ok &= sign * flat[:, a] > eps
            elif kind == GUARD_DISTINCT:
                ok &= norm(points[:, b] - points[:, a]) > eps
            else:
                d = points[:, b] - points[:, a]
                span = norm(d)
                t = d / span[:, None]
                w = points[:, c] - points[:, a]
                cross = np.stack([w[:, 1] * t[:, 2] - w[:, 2] * t[:, 1], w[:, 2] * t[:, 0] - w[:, 0] * t[:, 2],
                                  w[:, 0] * t[:, 1] - w[:, 1] * t[:, 0]], axis=1)
                ok &= (span > eps) & (norm(cross) > eps)
    return ok


def sample_host(plan: SamplePlan, lo: int = 0, hi: int | None = None):
    """
    Geometries ``[lo, hi)`` of the plan's ensemble (``hi`` None: ``n_total``): ``(hardpoints [n, P, 3], latents [n, Z], delta [n, F],
    flags [n] uint8)``.  The definition the device pass equals bit for bit.
    """
    lo = int(lo)
    hi = plan.n_total if hi is None else int(hi)
    check_plan(plan, lo, hi)
    n, p = hi - lo, plan.n_points
    g = np.arange(n, dtype=np.uint64) + np.uint64(lo)
    hardpoints = np.repeat(plan.nominal[None], n, axis=0)
    latents, delta = np.zeros((n, plan.n_latents)), np.zeros((n, plan.n_coords))
    flags = np.zeros(n, dtype=np.uint8)
    strata = stratum(plan.seed, plan.n_total, g[:, None], np.arange(plan.n_latents, dtype=np.uint64)[None]) if plan.stratify == LHS and n else None
    pending = np.arange(n)
    base = plan.nominal.reshape(-1)
    for attempt in range(plan.max_attempts):
        if not pending.size:
            break
        lat = latents_from_units(plan, units(plan, g[pending], attempt, None if strata is None else strata[pending]))
        dlt = contract(plan, lat)
        rows = np.repeat(base[None], pending.size, axis=0)
        rows[:, plan.coords] = base[plan.coords][None] + dlt
        points = rows.reshape(-1, p, 3)
        ok = guards_hold(plan, points)
        keep = ok | (attempt == plan.max_attempts - 1)
        idx = pending[keep]
        hardpoints[idx], latents[idx], delta[idx] = points[keep], lat[keep], dlt[keep]
        flags[idx] = (attempt << 4) | np.where(ok[keep], 0, 1)
        pending = pending[~keep]
    return hardpoints, latents, delta, flags


def hardpoint_plan(program, points, *, sigma=None, half_width=None, kind: int | None = None, bound=None, mixing=None, stratify: int = IID,
                   n_total: int = 0, seed: int = 0, guards=(), max_attempts: int = 1) -> SamplePlan:
    """
    A plan that perturbs all three coordinates of ``points`` (indices into the program's point table, or names) about the
    program's design positions: ``sigma`` (a number or ``[F]``) scales ``NORMAL`` / ``TRUNCATED`` latents, ``half_width`` ``UNIFORM`` ones -
    give exactly one; ``kind`` defaults to the one that goes with it.  With ``mixing [F, Z]`` the latents move the coordinates
    together (``kind`` / ``bound`` then describe the Z latents and ``sigma`` / ``half_width`` must be left out).
    """
    from .program import key_name

    # (a PointID is an int too: plain integers alone are indices, everything else is a key of the program's point table)
    index = [int(pt) if type(pt) is int or isinstance(pt, np.integer) else program.point_index(pt) for pt in points]
    coords = np.asarray([3 * i + axis for i in index for axis in range(3)], dtype=np.int32)
    if mixing is None:
        if (sigma is None) == (half_width is None):
            raise ValueError("hardpoint_plan takes sigma or half_width, one of them")
        kind = (UNIFORM if sigma is None else NORMAL) if kind is None else kind
        names = tuple(f"{key_name(program.point_keys[i]).lower()}.{'xyz'[axis]}" for i in index for axis in range(3))
        return SamplePlan(program.design_pos, coords, np.full(coords.size, kind, dtype=np.int32), bound, None, half_width if sigma is None else sigma,
                          stratify, n_total, seed, tuple(guards), max_attempts, names)
    if sigma is not None or half_width is not None:
        raise ValueError("with mixing the scales are its entries: leave sigma and half_width out")
    z = np.shape(mixing)[1]
    return SamplePlan(program.design_pos, coords, np.broadcast_to(np.asarray(NORMAL if kind is None else kind, dtype=np.int32), (z,)), bound, mixing, None,
                      stratify, n_total, seed, tuple(guards), max_attempts)


# ---- pick-freeze families (okx_ensemble_sample_families): the structured ensemble of a variance decomposition ----

SOBOL_MAX_GROUPS = 288  # OKX_ENS_SOBOL_MAX_GROUPS


@dataclass(frozen=True)
class FamilyPlan:
    """
    A pick-freeze (Saltelli) ensemble over a ``SamplePlan``: ``group [Z]`` int32 puts every latent into a factor group in
    ``[0, D)`` or ``-1`` (never swapped), ``n_families`` families of ``M = D + 2`` geometries each.  Geometry ``g`` is member
    ``b = g % M`` of family ``i = g // M``: member 0 is A, member 1 is B, member ``2 + j`` is A with group j's latents taken from
    B.  Latent z of g is the wrapped plan's draw of SOURCE ROW ``2 i + s`` at attempt 0 (``s = 1`` for B and for a latent of the
    member's own group); under ``LHS`` over ``2 n_families`` strata, whatever the wrapped plan's ``n_total`` says.  The wrapped plan
    has ``max_attempts == 1``: a redraw of one member would break the coordinates it shares with the others.
    ``n_total = n_families * M`` is the ensemble every consumer sees.  ``group_names``: the names of the groups (optional).
    """

    plan: SamplePlan
    group: np.ndarray
    n_families: int
    group_names: tuple | None = field(default=None, compare=False)

    def __post_init__(self):
        group = np.ascontiguousarray(np.asarray(self.group, dtype=np.int32).reshape(-1))
        group.setflags(write=False)
        object.__setattr__(self, "group", group)
        object.__setattr__(self, "n_families", int(self.n_families))
        if self.group_names is not None:
            object.__setattr__(self, "group_names", tuple(self.group_names))
        check_families(self)

    n_groups = property(lambda self: int(self.group.max()) + 1 if self.group.size else 0)
    family_size = property(lambda self: self.n_groups + 2)
    n_total = property(lambda self: self.n_families * self.family_size)
    n_points = property(lambda self: self.plan.n_points)
    n_coords = property(lambda self: self.plan.n_coords)
    n_latents = property(lambda self: self.plan.n_latents)

    def source_plan(self) -> SamplePlan:
        """The plain ensemble the families are cut from: the wrapped plan with ``n_total = 2 n_families``; members 0 and 1 of family
        i are its rows ``2 i`` and ``2 i + 1``."""
        import dataclasses

        return dataclasses.replace(self.plan, n_total=2 * self.n_families)

    def factor_names(self) -> list:
        return self.plan.factor_names()

    def names(self) -> list:
        """The names of the groups: ``group_names``, else ``"group<j>"``."""
        return list(self.group_names) if self.group_names is not None else [f"group{j}" for j in range(self.n_groups)]


def check_families(fplan: FamilyPlan, lo: int = 0, hi: int = 0) -> None:
    """``okx_ensemble_sample_families_check`` on the host: ValueError in its words."""
    who = "okx_ensemble_sample_families"
    plan, group, n, off, n_fam = fplan.plan, fplan.group, int(hi) - int(lo), int(lo), fplan.n_families
    if not isinstance(plan, SamplePlan):
        raise ValueError(f"{who}: a FamilyPlan wraps a SamplePlan")
    if n < 0 or off < 0 or n_fam < 0:
        raise ValueError(f"{who}: negative n_geometries, geometry_offset or n_families")
    d = fplan.n_groups
    if not 1 <= d <= SOBOL_MAX_GROUPS:
        raise ValueError(f"{who}: {d} groups, 1 to {SOBOL_MAX_GROUPS} allowed")
    if plan.max_attempts != 1:
        raise ValueError(f"{who}: max_attempts is {plan.max_attempts}; a family is drawn once (a redraw of one member would break the frozen coordinates)")
    if group.size != plan.n_latents:
        raise ValueError(f"{who}: {group.size} groups for {plan.n_latents} latents")
    if plan.stratify == LHS and 2 * n_fam > 1 << 32:
        raise ValueError(f"{who}: {2 * n_fam} strata, at most 2^32 under LHS")
    for z, gr in enumerate(group.tolist()):
        if not -1 <= gr < d:
            raise ValueError(f"{who}: group {z} is {gr}, outside [-1, {d})")
    for j in range(d):
        if not np.any(group == j):
            raise ValueError(f"{who}: group {j} has no latent")
    if fplan.group_names is not None and len(fplan.group_names) != d:
        raise ValueError(f"{who}: {len(fplan.group_names)} group names for {d} groups")
    m = d + 2
    if plan.stratify == LHS and -(-(off + n) // m) > n_fam:
        raise ValueError(f"{who}: geometries [{off}, {off + n}) lie outside the {n_fam} families of {m}")


def families_host(fplan: FamilyPlan, lo: int = 0, hi: int | None = None):
    """
    Geometries ``[lo, hi)`` of the pick-freeze ensemble (``hi`` None: ``n_total``): ``(hardpoints [n, P, 3], latents [n, Z], delta [n, F],
    flags [n] uint8)``.  The definition ``okx_ensemble_sample_families`` equals bit for bit; ``flags`` is 1 where a guard fails.
    """
    lo = int(lo)
    hi = fplan.n_total if hi is None else int(hi)
    check_families(fplan, lo, hi)
    plan, m, n_src = fplan.plan, fplan.family_size, 2 * fplan.n_families
    n, p = hi - lo, plan.n_points
    g = np.arange(n, dtype=np.uint64) + np.uint64(lo)
    family, member = g // np.uint64(m), (g % np.uint64(m)).astype(np.int64)
    from_b = (member[:, None] == 1) | ((member[:, None] >= 2) & (fplan.group[None].astype(np.int64) == member[:, None] - 2))
    src = (np.uint64(2) * family)[:, None] + from_b.astype(np.uint64)                                 # [n, Z]
    z = np.arange(plan.n_latents, dtype=np.uint64)[None]
    u = unit_from_bits(draw_bits(plan.seed, src, z, 0))
    if plan.stratify == LHS and n:
        u = stratified_unit(stratum(plan.seed, n_src, src, z), u, n_src)
    lat = latents_from_units(plan, u)
    dlt = contract(plan, lat)
    base = plan.nominal.reshape(-1)
    rows = np.repeat(base[None], n, axis=0)
    rows[:, plan.coords] = base[plan.coords][None] + dlt
    points = rows.reshape(-1, p, 3)
    flags = np.where(guards_hold(plan, points) if n else np.ones(0, dtype=bool), 0, 1).astype(np.uint8)
    return points, lat, dlt, flags


def group_by_point(plan: SamplePlan) -> tuple:
    """``(group [Z], names)`` of a plan without ``mixing``: one group per perturbed POINT, in the order the points first appear."""
    if plan.mixing is not None:
        raise ValueError("group_by_point needs a plan without mixing: a latent then moves one coordinate of one point")
    points = [int(c) // 3 for c in plan.coords]
    order = list(dict.fromkeys(points))
    names = plan.factor_names()
    first = {pt: names[points.index(pt)].rsplit(".", 1)[0] for pt in order}
    return np.asarray([order.index(pt) for pt in points], dtype=np.int32), tuple(first[pt] for pt in order)


# ---- tolerance what-ifs: likelihood reweighting of an ensemble that is already drawn (okx_ensemble_tilt_weights) ----

TILT_MAX_SCENARIOS = 256  # OKX_ENS_TILT_MAX_SCENARIOS
TILT_PARAMS = 5           # OKX_TILT_PARAMS: a, b, c, lo, hi per (scenario, latent)
LOG2E = 1.4426950408889634
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")  # 0x3fe62e42fee00000: its low 21 bits are zero, k * LN2_HI is exact for |k| <= 1100
LN2_LO = 1.9082149292705877e-10
EXP_UNIT_MIN, EXP_UNIT_MAX = -708.0, 708.0
_EXP = tuple(1.0 / math.factorial(n) for n in range(14))  # 1 / n!, n = 0 .. 13 (n! is exact in fp64, the quotient correctly rounded)


def exp_unit(x):
    """``exp(x)`` by ``+ - *``, ``rint`` and ``ldexp`` alone - ``log_unit``'s counterpart, written out so that host and device agree bit
    for bit (``np.exp`` is libm's): ``k = rint(x LOG2E)``, ``r = (x - k LN2_HI) - k LN2_LO`` (|r| <= 0.35), ``P`` the Horner sum of ``r^n / n!``,
    n = 0 .. 13, the result ``ldexp(P, k)``; within 1e-14 relative of ``exp`` on [-708, 708].  ``x < -708`` and a NaN give 0.0; ``x > 708``
    is taken as 708 (the callers' checks keep a log-weight far below it)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = x >= EXP_UNIT_MIN
        xs = np.where(live, np.minimum(x, EXP_UNIT_MAX), 0.0)
        k = np.rint(xs * LOG2E)
        r = (xs - k * LN2_HI) - k * LN2_LO
        return np.where(live, np.ldexp(_horner(_EXP, r), k.astype(np.int32)), 0.0)


def _phi_between(lo: float, hi: float) -> float:
    """``Phi(hi) - Phi(lo)`` of the standard normal by the host's ``erfc``, taken in the tail both bounds lie in."""
    root = math.sqrt(2.0)
    if lo >= 0.0:
        return 0.5 * (math.erfc(lo / root) - math.erfc(hi / root))
    if hi <= 0.0:
        return 0.5 * (math.erfc(-hi / root) - math.erfc(-lo / root))
    return (1.0 - 0.5 * math.erfc(hi / root)) - 0.5 * math.erfc(-lo / root)


def _tilt_peak(a: float, b: float, c: float, lo: float, hi: float) -> float:
    """The largest value of ``(c z + b) z + a`` a latent inside ``[lo, hi]`` can give (a sampled latent lies within +-9)."""
    lo, hi = max(lo, -9.0), min(hi, 9.0)
    at = [lo, hi] + ([-b / (2.0 * c)] if c < 0.0 and lo < -b / (2.0 * c) < hi else [])
    return max((c * z + b) * z + a for z in at)


def tolerance_scenarios(plan: SamplePlan, specs) -> np.ndarray:
    """
    The scenario table ``tilt [S, Z, 5]`` = ``(a, b, c, lo, hi)`` per (scenario, latent) that ``tilt_weights_host`` and
    ``okx_ensemble_tilt_weights`` read.  A scenario changes the LAW of some latents of ``plan``; ``specs`` is a sequence of dicts, one
    per scenario, ``{name: dict(ratio=t, shift=m, window=(lo, hi))}`` (every key optional: ``ratio`` 1, ``shift`` 0, ``window`` the
    kind's own).  ``name`` is one of ``plan.factor_names()``, or a point name (``"point7"``) for its three coordinates.  By kind:

    * ``NORMAL``: ``N(0, 1) -> N(m, t^2)``, ``c = (1 - 1 / t^2) / 2``, ``b = m / t^2``, ``a = -ln t - m^2 / (2 t^2)``; with a ``window`` the
      new law is truncated to it and ``a`` also takes ``-ln(Phi((hi - m) / t) - Phi((lo - m) / t))``;
    * ``TRUNCATED(k)``: the same ``a, b, c``; ``a`` also takes ``ln[(Phi(k) - Phi(-k)) / (Phi((hi - m) / t) - Phi((lo - m) / t))]``, the window
      ``[lo, hi]`` inside ``[-k, k]`` (default: ``[-k, k]``);
    * ``UNIFORM``: uniform on ``[m - t, m + t]`` inside ``[-1, 1]``: ``a = ln(1 / t)``, ``b = c = 0``, the window ``[m - t, m + t]``.

    An untouched latent is ``(0, 0, 0, -inf, +inf)``, so the empty spec is the identity scenario (every weight exactly 1).  The
    normalisers come from the host's ``erfc`` once, as ``SamplePlan.bound_table``'s: they are part of the table.  The new law must be
    dominated by the drawn one (a window inside the support) and - ``NORMAL`` / ``TRUNCATED`` without a window - ``t < sqrt(2)``: at
    ``t >= sqrt(2)`` the weights of a normal latent have infinite variance.
    """
    who = "okx_ensemble_tilt_weights"
    specs = list(specs)
    z = plan.n_latents
    if not 1 <= len(specs) <= TILT_MAX_SCENARIOS:
        raise ValueError(f"{who}: {len(specs)} scenarios, 1 to {TILT_MAX_SCENARIOS} allowed")
    if not 1 <= z <= MAX_LATENTS:
        raise ValueError(f"{who}: {z} latents, 1 to {MAX_LATENTS} allowed")
    names = plan.factor_names()
    bounds = plan.bound_table()
    tilt = np.zeros((len(specs), z, TILT_PARAMS))
    tilt[:, :, 3], tilt[:, :, 4] = -np.inf, np.inf
    for s, spec in enumerate(specs):
        for name, change in dict(spec).items():
            hit = [i for i, n in enumerate(names) if n == name] or [i for i, n in enumerate(names) if n.startswith(f"{name}.")]
            if not hit:
                raise ValueError(f"{who}: scenario {s} names {name!r}, which is no latent of the plan and no point of one")
            change = dict(change)
            unknown = set(change) - {"ratio", "shift", "window"}
            if unknown:
                raise ValueError(f"{who}: scenario {s}, {name!r}: a change takes ratio, shift and window (got {sorted(unknown)})")
            t, m, window = float(change.get("ratio", 1.0)), float(change.get("shift", 0.0)), change.get("window")
            if not (math.isfinite(t) and t > 0.0) or not math.isfinite(m):
                raise ValueError(f"{who}: scenario {s}, {name!r}: ratio {t:g} and shift {m:g} must be finite and the ratio greater than 0")
            if window is not None:
                window = (float(window[0]), float(window[1]))
                if not window[0] < window[1]:  # (also a NaN)
                    raise ValueError(f"{who}: scenario {s}, {name!r}: the window ({window[0]:g}, {window[1]:g}) must have lo < hi")
            for i in hit:
                kind = int(plan.kind[i])
                if kind == UNIFORM:
                    lo, hi = m - t, m + t
                    if window is not None:
                        raise ValueError(f"{who}: scenario {s}, {names[i]!r}: a uniform latent takes ratio and shift, its window is [shift - ratio, shift + ratio]")
                    if lo < -1.0 or hi > 1.0:
                        raise ValueError(f"{who}: scenario {s}, {names[i]!r}: the window [{lo:g}, {hi:g}] leaves the support [-1, 1] of the drawn law")
                    tilt[s, i] = math.log(1.0 / t), 0.0, 0.0, lo, hi
                    continue
                k = float(bounds[i, 0]) if kind == TRUNCATED else math.inf
                if window is None and t >= math.sqrt(2.0):
                    raise ValueError(f"{who}: scenario {s}, {names[i]!r}: ratio {t:g} >= sqrt(2) without a window - the weights of a normal latent then "
                                     f"have infinite variance")
                lo, hi = (-k, k) if window is None else window
                if lo < -k or hi > k:
                    raise ValueError(f"{who}: scenario {s}, {names[i]!r}: the window [{lo:g}, {hi:g}] leaves the support [{-k:g}, {k:g}] of the drawn law")
                a = -math.log(t) - m * m / (2.0 * t * t)
                if math.isfinite(lo) or math.isfinite(hi):
                    mass = _phi_between((lo - m) / t, (hi - m) / t)
                    if not mass > 0.0:
                        raise ValueError(f"{who}: scenario {s}, {names[i]!r}: the new law has no mass in the window [{lo:g}, {hi:g}]")
                    a += math.log((float(bounds[i, 2]) if kind == TRUNCATED else 1.0) / mass)
                tilt[s, i] = a, m / (t * t), 0.5 * (1.0 - 1.0 / (t * t)), lo, hi
        peak = sum(_tilt_peak(*tilt[s, i]) for i in range(z))  # (an untouched latent adds 0)
        if not peak <= 700.0:
            raise ValueError(f"{who}: scenario {s}: a log-weight may reach {peak:g}, beyond what exp_unit takes (700)")
    check_tilt(tilt)
    return tilt


def check_tilt(tilt) -> np.ndarray:
    """``tilt`` as a contiguous float64 ``[S, Z, 5]`` table, or ValueError in the words of ``okx_ensemble_tilt_check``."""
    who = "okx_ensemble_tilt_weights"
    table = np.ascontiguousarray(np.asarray(tilt, dtype=np.float64))
    if table.ndim != 3 or table.shape[2] != TILT_PARAMS:
        raise ValueError(f"{who}: the scenario table must be [S, Z, {TILT_PARAMS}] (a, b, c, lo, hi)")
    s, z = table.shape[:2]
    if not 1 <= s <= TILT_MAX_SCENARIOS:
        raise ValueError(f"{who}: {s} scenarios, 1 to {TILT_MAX_SCENARIOS} allowed")
    if not 1 <= z <= MAX_LATENTS:
        raise ValueError(f"{who}: {z} latents, 1 to {MAX_LATENTS} allowed")
    bad = np.argwhere(~np.isfinite(table[:, :, :3]).all(axis=2))
    if bad.size:
        raise ValueError(f"{who}: scenario {int(bad[0, 0])}, latent {int(bad[0, 1])}: a, b or c is not finite")
    with np.errstate(invalid="ignore"):
        bad = np.argwhere(~(table[:, :, 3] <= table[:, :, 4]))
    if bad.size:
        raise ValueError(f"{who}: scenario {int(bad[0, 0])}, latent {int(bad[0, 1])}: the window is NaN or has lo > hi")
    return table


def tilt_weights_host(latents, tilt) -> np.ndarray:
    """
    The definition of ``okx_ensemble_tilt_weights``: the likelihood ratios ``w [G, S]`` of ``latents [G, Z]`` (what the sampler kept,
    ``sample_host(plan)[1]``) under the scenarios ``tilt [S, Z, 5]`` (``tolerance_scenarios``).  Per (geometry, scenario), over the
    latents in ascending order::

        inside_z = lo <= z <= hi                 (comparisons: a NaN latent is outside)
        term_z   = (c * z + b) * z + a           (every operation rounded on its own, no fused multiply-add)
        logw     = 0.0 + term_0 + term_1 + ...   (every add rounded)
        w        = exp_unit(logw) if every latent is inside, else 0.0

    The device pass equals this bit for bit.  GUARDS AND REDRAWS need no special case: the drawn law is ``p`` conditioned on the
    guards, the target law is ``q`` under the same guards, and their ratio is ``q / p`` times a constant that the self-normalised
    estimates (``ensemble_stats.ReweighAccumulator.finalize`` divides every sum by the sum of the weights) divide out.  Under ``LHS``
    the geometries are not independent draws: the estimates stay consistent, but the effective sample size ``(sum w)^2 / sum w^2`` and
    the standard errors built on it are a heuristic there (on the conservative side for the strata's own latents).
    """
    x = np.asarray(latents, dtype=np.float64)
    table = check_tilt(tilt)
    if x.ndim != 2 or x.shape[1] != table.shape[1]:
        raise ValueError(f"okx_ensemble_tilt_weights: latents must be [G, {table.shape[1]}], one column per latent of the scenario table")
    g, s = x.shape[0], table.shape[0]
    logw = np.zeros((g, s))
    inside = np.ones((g, s), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(table.shape[1]):
            a, b, c, lo, hi = (table[None, :, i, j] for j in range(TILT_PARAMS))
            col = x[:, i, None]
            inside &= (lo <= col) & (col <= hi)
            logw = logw + ((c * col + b) * col + a)
        return np.where(inside, exp_unit(logw), 0.0)


__all__ = ["SamplePlan", "sample_host", "hardpoint_plan", "FamilyPlan", "families_host", "check_families", "group_by_point",
           "tolerance_scenarios", "tilt_weights_host", "check_tilt", "exp_unit", "TILT_MAX_SCENARIOS", "TILT_PARAMS",
           "SOBOL_MAX_GROUPS", "philox4x32_10", "draw_bits", "unit_from_bits", "stratum", "strata_bits", "strata_keys",
           "ppnd16", "log_unit", "units", "stratified_unit", "latents_from_units", "contract", "guards_hold", "check_arguments", "check_plan",
           "NORMAL", "UNIFORM", "TRUNCATED", "IID", "LHS", "GUARD_SIGN", "GUARD_DISTINCT", "GUARD_OFF_LINE", "PURPOSE_DRAW", "PURPOSE_STRATA", "PURPOSE_BOOTSTRAP",
           "MAX_COORDS", "MAX_LATENTS", "MAX_GUARDS", "MAX_ATTEMPTS", "U_MIN", "U_MAX"]
