"""
Statistics of an evaluated ensemble: per (sweep step, metric column), over the geometries, how many states were accepted,
mean, spread, the extremes and WHICH geometry produced them, and the least-squares slopes of the column on per-geometry
factors (hardpoint perturbations).

Three layers, the same accumulator in each (``include/okx.h``, ``okx_ensemble_reduce``):

* ``reduce_host``: NumPy over ``values [G, S, K]``; the fallback without a GPU and the cross-check of the device pass;
* ``DeviceProgram.reduce_ensemble`` (``ensemble_device.py``): the device pass over a column table in HBM;
* ``dist.ShardedEnsemble(reduce=True)``: every rank reduces its own shard chunk by chunk and the ranks exchange the
  accumulators alone.

Beside the moments: exact quantiles and per-entry spec-limit yield (``select_host``, ``okx_ensemble_select``) and the JOINT
spec-limit verdict per geometry (``screen_host`` / ``EnsembleScreen``, ``okx_ensemble_screen``), each in the same three layers;
and how the entries move TOGETHER over the geometries: covariance and correlation of selected entries over the complete cases
(``covariance_host`` / ``CovarianceAccumulator`` / ``EnsembleCovariance``, ``okx_ensemble_covariance``), in the same three.
ALONG the sweep inside one geometry: the curve characteristics of every (geometry, column) - fitted value, gradient and
curvature at an origin, departure from the fitted shape, extremes and where they occur (``curves_host`` / ``EnsembleCurves``,
``okx_ensemble_curves``); their table ``[G, K * 12]`` is again a column table for every pass above.
WHICH FACTOR GROUP explains the variance: the Sobol' accumulators of a pick-freeze ensemble (``ensemble_sample.FamilyPlan``) and
their first-order and total-order indices (``sobol_host`` / ``SobolAccumulator`` / ``EnsembleSobol``, ``okx_ensemble_sobol``), and
HOW FAR TO TRUST them: Poisson-bootstrap replicates of those accumulators, their standard deviations and percentile intervals
(``bootstrap_weights`` / ``sobol_bootstrap_host`` / ``SobolBootstrapAccumulator`` / ``EnsembleSobolBootstrap``, ``okx_ensemble_sobol_bootstrap``).
HOW an entry depends on ONE factor beyond a straight line, from the ordinary ensemble: its conditional moments over equal-probability
bins of every factor and the first-order indices they give (``effects_edges`` / ``bin_factors_host`` / ``effects_host`` /
``EffectsAccumulator`` / ``EnsembleEffects``, ``okx_ensemble_bin`` and ``okx_ensemble_effects``).
WHICH PAIRS of factors act together, and a model of the table: a polynomial response surface - orthonormal Hermite / Legendre polynomials
of the sampler's latents with pairwise products, fitted by least squares from the normal equations the device accumulates (``surface_terms`` /
``basis_host`` / ``surface_host`` / ``SurfaceAccumulator`` / ``EnsembleSurface``, ``okx_ensemble_basis`` and ``okx_ensemble_surface``).
THE MODEL IN USE AND UNDER TEST: the fitted surface evaluated as a column table, or the table's residuals against it (``predict_host``,
``okx_ensemble_predict``; ``ensemble_virtual.virtual_ensemble`` counts millions of drawn geometries through it), and its leave-one-out
error from residuals and leverages without a refit (``surface_loo_host`` / ``surface_validate_host`` / ``SurfaceValidation``).

``EnsembleAccumulator`` holds the raw tables; partial accumulators taken with THE SAME shift merge by additions and
comparisons (``merge``), ``finalize`` turns one into ``EnsembleStats``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ENS_COUNT, ENS_REJECTED, ENS_SUM, ENS_SUMSQ, ENS_MIN, ENS_MAX, ENS_ARGMIN, ENS_ARGMAX = range(8)
ENS_FIELDS = 8  # OKX_ENS_FIELDS

STATUS_ACCEPT_MASK = 7  # okx_info.flags: converged (1) set, residual exceeded (2) and failed (4) clear - BatchResult.accepted


def factor_moment_count(n_factors: int) -> int:
    """Length of the factor-moment table: ``sum f_p``, the lower triangle of ``sum f_p f_q`` row by row, the geometry count."""
    return n_factors + n_factors * (n_factors + 1) // 2 + 1 if n_factors > 0 else 0


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def _same_table(a, b) -> bool:
    """One table object on both sides (the sharded exchange) needs no comparison - on a device that would be a sync -; else by content."""
    return a is b or bool(__import__("torch").equal(a, b) if _is_tensor(a) else np.array_equal(a, b))


def _same_shape(a, b) -> bool:
    return tuple(a.shape) == tuple(b.shape)


class _Accumulator:
    """What the four accumulators share.  A class names its tables once (``TABLES``, constructor arguments; the first is never None)
    and the other constructor arguments a copy carries over (``CARRIED``; ``DEVICE_ONLY``: those a host copy drops)."""

    TABLES: tuple = ()
    CARRIED: tuple = ()
    DEVICE_ONLY: tuple = ()

    def _copy(self, convert, carried):
        return type(self)(**{name: None if getattr(self, name) is None else convert(getattr(self, name)) for name in self.TABLES},
                          **{name: getattr(self, name) for name in carried})

    def numpy(self):
        """Host NumPy copy (self when it is one already)."""
        if not _is_tensor(getattr(self, self.TABLES[0])):
            return self
        return self._copy(lambda t: t.detach().cpu().numpy(), [name for name in self.CARRIED if name not in self.DEVICE_ONLY])

    def to(self, device):
        """The tables as torch tensors on ``device``."""
        import torch

        return self._copy(lambda t: torch.as_tensor(t).to(device), self.CARRIED)


@dataclass
class EnsembleStats:
    """
    What ``EnsembleAccumulator.finalize`` returns, every table ``[S, K]`` (NumPy, host):
    ``count`` accepted finite values, ``rejected`` the others, ``mean``, ``variance`` (unbiased; NaN for ``count < 2``),
    ``std``, ``min`` / ``max`` (NaN for ``count == 0``), ``argmin`` / ``argmax`` (global geometry index, ties to the lowest;
    ``-1`` for ``count == 0``).  With factors: ``sensitivity [S, K, P]`` - the least-squares slopes of the column on the
    factors with an intercept -, ``intercept`` and ``r2`` ``[S, K]``.  The fit uses the UNMASKED factor moments, so it is
    defined where ``rejected == 0`` for that entry and NaN elsewhere (and where fewer than ``P + 2`` geometries were seen);
    ``r2`` is NaN where the column does not vary.
    """

    count: np.ndarray
    rejected: np.ndarray
    mean: np.ndarray
    variance: np.ndarray
    std: np.ndarray
    min: np.ndarray
    max: np.ndarray
    argmin: np.ndarray
    argmax: np.ndarray
    sensitivity: np.ndarray | None = None
    intercept: np.ndarray | None = None
    r2: np.ndarray | None = None
    factor_names: list | None = None


class EnsembleAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_reduce``: ``acc [S, K, ENS_FIELDS + P]`` float64, ``shift [S, K]`` and, with factors,
    ``factor_acc [P + P (P + 1) / 2 + 1]`` - NumPy arrays or torch tensors (host or device), whatever produced them.
    """

    TABLES, CARRIED = ("acc", "shift", "factor_acc"), ("factor_names",)

    def __init__(self, acc, shift, factor_acc=None, factor_names=None):
        self.acc = acc
        self.shift = shift
        self.factor_acc = factor_acc
        self.factor_names = list(factor_names) if factor_names is not None else None
        if acc.ndim != 3 or acc.shape[2] < ENS_FIELDS or tuple(shift.shape) != tuple(acc.shape[:2]):
            raise ValueError("acc must be [S, K, ENS_FIELDS + P] and shift [S, K]")
        if factor_acc is not None and factor_acc.shape[0] != factor_moment_count(self.n_factors):
            raise ValueError("factor_acc does not fit the accumulator's factor count")

    @property
    def n_factors(self) -> int:
        return int(self.acc.shape[2]) - ENS_FIELDS

    @classmethod
    def empty(cls, steps: int, n_columns: int, n_factors: int, shift, factor_names=None) -> "EnsembleAccumulator":
        """The accumulator of no geometry at all (the neutral element of ``merge``), NumPy."""
        acc = np.zeros((steps, n_columns, ENS_FIELDS + n_factors))
        acc[..., ENS_MIN], acc[..., ENS_MAX] = np.inf, -np.inf
        acc[..., ENS_ARGMIN] = acc[..., ENS_ARGMAX] = -1.0
        shift = np.asarray(shift, dtype=np.float64).reshape(steps, n_columns)
        return cls(acc, shift, np.zeros(factor_moment_count(n_factors)) if n_factors else None, factor_names)

    def merge(self, other: "EnsembleAccumulator") -> "EnsembleAccumulator":
        """
        ``self`` then ``other`` as one accumulator (a new one; both stay): sums add, an extreme that is strictly better
        wins and a tie goes to the LOWER geometry index.  Both must have been taken with the same shift - that is what
        makes a merge additions and comparisons only.  Works on NumPy arrays and on torch tensors alike.
        """
        a, b = self.acc, other.acc
        if not _same_shape(a, b):
            raise ValueError("accumulators of different shapes")
        if not _same_table(self.shift, other.shift):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        xp = __import__("torch") if _is_tensor(a) else np
        out = a + b
        for value, arg, better in ((ENS_MIN, ENS_ARGMIN, lambda x, y: x < y), (ENS_MAX, ENS_ARGMAX, lambda x, y: x > y)):
            av, ai, bv, bi = a[..., value], a[..., arg], b[..., value], b[..., arg]
            take = (bi >= 0) & ((ai < 0) | better(bv, av) | ((bv == av) & (bi < ai)))
            out[..., value] = xp.where(take, bv, av)
            out[..., arg] = xp.where(take, bi, ai)
        fa = None
        if self.factor_acc is not None and other.factor_acc is not None:
            fa = self.factor_acc + other.factor_acc
        return EnsembleAccumulator(out, self.shift, fa, self.factor_names)

    def finalize(self) -> EnsembleStats:
        """Moments, extremes and (with factors) the least-squares fit, on the host in fp64."""
        h = self.numpy()
        acc, shift = np.asarray(h.acc, dtype=np.float64), np.asarray(h.shift, dtype=np.float64)
        n = acc[..., ENS_COUNT]
        count, rejected = n.astype(np.int64), acc[..., ENS_REJECTED].astype(np.int64)
        s1, s2 = acc[..., ENS_SUM], acc[..., ENS_SUMSQ]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_d = np.where(n > 0, s1 / n, np.nan)
            mean = shift + mean_d
            # sum (d - mean_d)^2 = s2 - s1^2 / n, about a shift that lies inside the data
            variance = np.where(n > 1, np.maximum(s2 - s1 * mean_d, 0.0) / (n - 1), np.nan)
        std = np.sqrt(variance)
        some = n > 0
        stats = EnsembleStats(count, rejected, mean, variance, std, np.where(some, acc[..., ENS_MIN], np.nan),
                              np.where(some, acc[..., ENS_MAX], np.nan), acc[..., ENS_ARGMIN].astype(np.int64),
                              acc[..., ENS_ARGMAX].astype(np.int64), factor_names=self.factor_names)
        p = self.n_factors
        if p and h.factor_acc is not None:
            stats.sensitivity, stats.intercept, stats.r2 = _fit(acc, shift, np.asarray(h.factor_acc, dtype=np.float64), p)
        return stats


def _fit(acc, shift, factor_acc, p: int):
    """Slopes, intercept and R^2 of every entry from the normal equations of the accumulated moments."""
    g = factor_acc[-1]
    s_f = factor_acc[:p]
    tri = np.zeros((p, p))
    tri[np.tril_indices(p)] = factor_acc[p:-1]
    s_ff = tri + np.tril(tri, -1).T
    steps, cols = acc.shape[:2]
    nan = np.full((steps, cols), np.nan)
    if g < 1:
        return np.full((steps, cols, p), np.nan), nan, nan.copy()
    # centred: C = sum (f - fbar)(f - fbar)^T; the intercept separates exactly
    fbar = s_f / g
    c = s_ff - g * np.outer(fbar, fbar)
    scale = np.sqrt(np.maximum(np.diag(c), 0.0))
    scale[scale == 0.0] = 1.0
    rank = int(np.linalg.matrix_rank(c / np.outer(scale, scale), tol=1e-10)) if g > 1 else 0
    if rank < p:
        raise ValueError(f"the factor matrix is rank-deficient: rank {rank + 1} of {p + 1} columns [1 | factors]")
    n = acc[..., ENS_COUNT]
    s1, s2 = acc[..., ENS_SUM], acc[..., ENS_SUMSQ]
    cross = acc[..., ENS_FIELDS:]                                  # sum f_p d
    rhs = cross - fbar[None, None, :] * s1[..., None]              # sum (f_p - fbar_p) d
    slopes = np.linalg.solve(c, rhs.reshape(-1, p).T).T.reshape(steps, cols, p)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_d = s1 / g
        intercept = shift + mean_d - slopes @ fbar
        total = s2 - s1 * mean_d                                   # sum (d - mean_d)^2
        explained = np.einsum("skp,skp->sk", slopes, rhs)
        r2 = np.where(total > 0.0, explained / total, np.nan)
    defined = (acc[..., ENS_REJECTED] == 0) & (n == g) & (g >= p + 2)
    slopes = np.where(defined[..., None], slopes, np.nan)
    return slopes, np.where(defined, intercept, np.nan), np.where(defined, r2, np.nan)


def clean_shift(shift) -> np.ndarray:
    """A shift table with its undefined entries (NaN / inf: a metric the state does not have) replaced by 0."""
    shift = np.array(shift, dtype=np.float64, copy=True)
    shift[~np.isfinite(shift)] = 0.0
    return shift


def reduce_host(values, status=None, factors=None, shift=None, geometry_offset: int = 0, factor_names=None) -> EnsembleAccumulator:
    """
    The accumulator of ``okx_ensemble_reduce`` in NumPy.  ``values [G, S, K]``; ``status [G, S]`` uint8 (the low byte of
    ``okx_info.flags``) or None (every state accepted); ``factors [G, P]`` or None; ``shift [S, K]`` (None: the values of
    geometry 0, undefined entries 0).  Sums run over the geometries in ascending order, one after the other.
    """
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 3:
        raise ValueError("values must be [G, S, K]")
    g, s, k = v.shape
    if shift is None:
        shift = clean_shift(v[0]) if g else np.zeros((s, k))
    shift = np.asarray(shift, dtype=np.float64).reshape(s, k)
    if not np.all(np.isfinite(shift)):
        raise ValueError("the shift must be finite (clean_shift replaces undefined entries)")
    ok = np.isfinite(v)
    if status is not None:
        st = np.asarray(status).reshape(g, s).astype(np.uint8)
        ok &= ((st & STATUS_ACCEPT_MASK) == 1)[:, :, None]
    f = None if factors is None else np.asarray(factors, dtype=np.float64)
    if f is not None and (f.ndim != 2 or f.shape[0] != g):
        raise ValueError("factors must be [G, P]")
    p = 0 if f is None else f.shape[1]
    acc = np.zeros((s, k, ENS_FIELDS + p))
    with np.errstate(invalid="ignore"):
        d = np.where(ok, v - shift[None], 0.0)
    acc[..., ENS_COUNT] = ok.sum(axis=0)
    acc[..., ENS_REJECTED] = g - ok.sum(axis=0)
    for i in range(g):  # ascending geometry order, as the device walks a slab
        acc[..., ENS_SUM] += d[i]
        acc[..., ENS_SUMSQ] += d[i] * d[i]
        if p:
            acc[..., ENS_FIELDS:] += d[i][..., None] * f[i][None, None, :]
    some = ok.any(axis=0)
    lo = np.where(ok, v, np.inf)
    hi = np.where(ok, v, -np.inf)
    acc[..., ENS_MIN], acc[..., ENS_MAX] = lo.min(axis=0) if g else np.inf, hi.max(axis=0) if g else -np.inf
    # (argmin / argmax return the FIRST extreme: the lowest geometry index)
    acc[..., ENS_ARGMIN] = np.where(some, geometry_offset + lo.argmin(axis=0), -1.0) if g else -1.0
    acc[..., ENS_ARGMAX] = np.where(some, geometry_offset + hi.argmax(axis=0), -1.0) if g else -1.0
    factor_acc = None
    if p:
        factor_acc = np.zeros(factor_moment_count(p))
        rows, cols = np.tril_indices(p)
        for i in range(g):
            factor_acc[:p] += f[i]
            factor_acc[p:-1] += f[i][rows] * f[i][cols]
        factor_acc[-1] = g
    return EnsembleAccumulator(acc, shift, factor_acc, factor_names)


def hardpoint_factors(hardpoints, point_names=None, atol: float = 0.0):
    """
    ``factors="hardpoints"``: ``hardpoints [G, P, 3]`` minus their mean over the geometries, restricted to the
    coordinates that vary (a derived or unperturbed point's do not).  Returns ``(factors [G, F], names)`` with names like
    ``"upper_wishbone_outboard.x"`` (``"point7.x"`` without ``point_names``).
    """
    hp = np.asarray(hardpoints, dtype=np.float64)
    g = hp.shape[0]
    flat = hp.reshape(g, -1)
    varies = (flat.max(axis=0) - flat.min(axis=0)) > atol if g else np.zeros(flat.shape[1], dtype=bool)
    centred = flat[:, varies] - flat[:, varies].mean(axis=0)
    names = []
    for j in np.flatnonzero(varies):
        point = point_names[j // 3] if point_names is not None else f"point{j // 3}"
        names.append(f"{point}.{'xyz'[j % 3]}")
    return np.ascontiguousarray(centred), names


# ---- quantiles and spec-limit yield: exact order statistics by a radix select on integer keys (okx_ensemble_select) ----

SELECT_BITS = 4  # OKX_ENS_SELECT_BITS: key bits a round fixes
SELECT_BINS = 1 << SELECT_BITS
SELECT_ROUNDS = 64 // SELECT_BITS
SELECT_MAX_PROBS = 64  # OKX_ENS_SELECT_MAX_PROBS


@dataclass
class EnsembleQuantiles:
    """
    Per (step, column) entry over the states that count (NumPy, host): ``count [S, K]``; for every probability of ``probs [Q]``
    the two order statistics ``lower`` / ``upper [S, K, Q]`` = ``x[floor(h)]``, ``x[ceil(h)]`` with ``h = (count - 1) p`` of the
    sorted accepted values - bits of values in the table, NaN for ``count == 0`` - and ``quantile``, their interpolation
    ``lower + (h - floor(h)) (upper - lower)`` (``numpy.quantile(..., method="linear")``).  With limits: ``below`` / ``above
    [S, K]`` accepted values strictly under ``lo`` / over ``hi`` and ``yield_ = 1 - (below + above) / count`` (NaN for
    ``count == 0``).
    """

    probs: np.ndarray
    count: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    quantile: np.ndarray
    below: np.ndarray | None = None
    above: np.ndarray | None = None
    yield_: np.ndarray | None = None


def _host_f64(table) -> np.ndarray:
    """A float64 NumPy COPY of an array, a sequence or a torch tensor (host or device)."""
    return np.array(table.detach().cpu().numpy() if _is_tensor(table) else table, dtype=np.float64)


def broadcast_limits(limits, steps: int, n_columns: int) -> np.ndarray:
    """``limits`` given as ``[S, K, 2]``, ``[K, 2]`` or ``[2]`` = (lo, hi) as a contiguous float64 ``[S, K, 2]`` table of its own."""
    s, k = int(steps), int(n_columns)
    lim = _host_f64(limits)
    if lim.shape[-1:] != (2,) or lim.size not in (2, 2 * k, 2 * s * k):
        raise ValueError("limits must be [S, K, 2], [K, 2] or [2] (lo, hi)")
    return np.array(np.broadcast_to(lim.reshape(s, k, 2) if lim.size == 2 * s * k else lim.reshape(-1, 2), (s, k, 2)), order="C")


def broadcast_scale(scale, steps: int, n_columns: int) -> np.ndarray:
    """``scale`` given as ``[S, K]``, ``[K]`` or a scalar as a contiguous float64 ``[S, K]`` table of its own."""
    s, k = int(steps), int(n_columns)
    sc = _host_f64(scale)
    if sc.size not in (1, k, s * k):
        raise ValueError("scale must be [S, K], [K] or a scalar")
    return np.array(np.broadcast_to(sc.reshape(s, k) if sc.size == s * k else sc.reshape(-1), (s, k)), order="C")


def check_select_arguments(probs, limits=None, steps: int | None = None, n_columns: int | None = None):
    """``(probs [Q], limits [S, K, 2] or None)`` as float64 arrays, or ValueError in the words of ``okx_ensemble_select_check``."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    if not 1 <= p.size <= SELECT_MAX_PROBS:
        raise ValueError(f"okx_ensemble_select: 1 to {SELECT_MAX_PROBS} probabilities")
    bad = np.flatnonzero(~((p >= 0.0) & (p <= 1.0)))
    if bad.size:
        raise ValueError(f"okx_ensemble_select: probability {int(bad[0])} is {p[bad[0]]:g}, outside [0, 1]")
    if limits is None:
        return p, None
    lim = np.asarray(limits, dtype=np.float64) if steps is None else broadcast_limits(limits, steps, n_columns)
    flat = lim.reshape(-1, 2)
    nan = np.flatnonzero(np.isnan(flat).any(axis=1))
    if nan.size:
        raise ValueError(f"okx_ensemble_select: limit {int(nan[0])} is NaN (an open side is -inf / +inf)")
    bad = np.flatnonzero(flat[:, 0] > flat[:, 1])
    if bad.size:
        raise ValueError(f"okx_ensemble_select: limit {int(bad[0])} has lo > hi ({flat[bad[0], 0]:g} > {flat[bad[0], 1]:g})")
    return p, lim


def quantiles_from_order(probs, order, count, outside=None) -> EnsembleQuantiles:
    """The host's share of ``okx_ensemble_select``: ``order [S, K, Q, 2]``, ``count [S, K]``, ``outside [S, K, 2]`` or None."""
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    order = np.asarray(order, dtype=np.float64)
    count = np.asarray(count, dtype=np.int64)
    lower, upper = order[..., 0].copy(), order[..., 1].copy()
    h = np.maximum(count - 1, 0).astype(np.float64)[..., None] * probs
    frac = h - np.floor(h)
    with np.errstate(invalid="ignore", over="ignore"):
        quantile = np.where((frac == 0.0) | (lower == upper), lower, lower + frac * (upper - lower))
    out = EnsembleQuantiles(probs, count, lower, upper, quantile)
    if outside is not None:
        outside = np.asarray(outside, dtype=np.int64)
        out.below, out.above = outside[..., 0].copy(), outside[..., 1].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            out.yield_ = np.where(count > 0, 1.0 - (out.below + out.above) / count, np.nan)
    return out


def _accepted(values, status):
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 3:
        raise ValueError("values must be [G, S, K]")
    ok = np.isfinite(v)
    if status is not None:
        st = np.asarray(status).reshape(v.shape[0], v.shape[1]).astype(np.uint8)
        ok &= ((st & STATUS_ACCEPT_MASK) == 1)[:, :, None]
    return v, ok


def select_host(values, status=None, probs=(0.5,), limits=None) -> EnsembleQuantiles:
    """The plain answer by ``np.sort``: ``values [G, S, K]``, ``status [G, S]`` or None, ``limits [S, K, 2]`` (lo, hi) or None."""
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    p, lim = check_select_arguments(probs, limits, s, k)
    n = ok.sum(axis=0).astype(np.int64)
    order = np.full((s, k, p.size, 2), np.nan)
    if g:
        ranked = np.sort(np.where(ok, v, np.inf), axis=0)  # the accepted values are finite: they come first
        h = np.maximum(n - 1, 0).astype(np.float64)[..., None] * p
        for side, index in enumerate((np.floor(h), np.ceil(h))):
            picked = np.take_along_axis(ranked, np.moveaxis(index.astype(np.int64), 2, 0), axis=0)  # [Q, S, K]
            order[..., side] = np.where((n > 0)[..., None], np.moveaxis(picked, 0, 2), np.nan)
    outside = None
    if lim is not None:
        outside = np.stack([(ok & (v < lim[None, ..., 0])).sum(axis=0), (ok & (v > lim[None, ..., 1])).sum(axis=0)], axis=2).astype(np.int64)
    return quantiles_from_order(p, order, n, outside)


def select_keys(values) -> np.ndarray:
    """Order-preserving uint64 keys of finite doubles: ``bits ^ (sign ? ~0 : 1 << 63)``; -0.0 sorts before +0.0."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return bits ^ np.where(bits >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63))


def select_values(keys) -> np.ndarray:
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.where(keys >> np.uint64(63), keys ^ np.uint64(1 << 63), ~keys).view(np.float64)


@dataclass
class SelectState:
    """State of the select rounds, per selection ``j = 2 q + side``: ``prefix`` (key bits fixed so far) and ``rank`` (still
    wanted among the values that share them; < 0: nothing to select) ``[S, K, 2 Q]``, ``count [S, K]``, ``outside [S, K, 2]``."""

    prefix: np.ndarray
    rank: np.ndarray
    count: np.ndarray
    outside: np.ndarray


def select_begin(steps: int, n_columns: int, n_probs: int):
    """``(state, hist)`` of a select that has seen nothing: ``hist`` int64 ``[S, K, 2 Q, SELECT_BINS]`` (``okx.h``'s layout), zero."""
    j = 2 * n_probs
    state = SelectState(np.zeros((steps, n_columns, j), dtype=np.uint64), np.zeros((steps, n_columns, j), dtype=np.int64),
                        np.zeros((steps, n_columns), dtype=np.int64), np.zeros((steps, n_columns, 2), dtype=np.int64))
    return state, np.zeros((steps, n_columns, j, SELECT_BINS), dtype=np.int64)


def select_count_round(rnd: int, values, status, state: SelectState, hist, limits=None) -> None:
    """The count pass of round ``rnd`` over one chunk ``values [G, S, K]``: adds into ``hist`` (round 0: the shared histogram in
    selection 0, the limit counts in ``hist[s, k, 1, 0:2]``)."""
    v, ok = _accepted(values, status)
    if v.shape[0] == 0:
        return
    keys = select_keys(v)
    bins = np.arange(SELECT_BINS, dtype=np.uint64)
    digit = (keys >> np.uint64(64 - SELECT_BITS * (rnd + 1))) & np.uint64(SELECT_BINS - 1)
    hot = digit[..., None] == bins  # [G, S, K, bins]
    if rnd == 0:
        hist[:, :, 0, :] += (hot & ok[..., None]).sum(axis=0)
        if limits is not None:
            lim = np.asarray(limits, dtype=np.float64)
            hist[:, :, 1, 0] += (ok & (v < lim[None, ..., 0])).sum(axis=0)
            hist[:, :, 1, 1] += (ok & (v > lim[None, ..., 1])).sum(axis=0)
        return
    fixed = np.uint64(64 - SELECT_BITS * rnd)
    head = keys >> fixed
    for j in range(state.prefix.shape[2]):
        match = ok & (head == (state.prefix[None, :, :, j] >> fixed))
        hist[:, :, j, :] += (hot & match[..., None]).sum(axis=0)


def select_descend_round(rnd: int, state: SelectState, hist, probs) -> None:
    """The descend of round ``rnd``: the bin that holds every selection's rank, prefix and rank advanced, ``hist`` re-zeroed.
    Round 0 sums ``count``, takes the limit counts and turns the probabilities into ranks (``h = (n - 1) p`` in fp64)."""
    if rnd == 0:
        p = np.asarray(probs, dtype=np.float64).reshape(-1)
        n = hist[:, :, 0, :].sum(axis=-1)
        state.count[...] = n
        state.outside[...] = hist[:, :, 1, 0:2]
        h = (n - 1).astype(np.float64)[..., None] * p
        with np.errstate(invalid="ignore"):
            rank = np.stack([np.floor(h), np.ceil(h)], axis=-1)
            valid = (n > 0)[..., None] & (p >= 0.0) & (p <= 1.0)
        rank = np.where(valid[..., None], rank, -1.0).astype(np.int64)
        state.rank[...] = rank.reshape(state.rank.shape)
        state.prefix[...] = 0
        source = np.broadcast_to(hist[:, :, 0:1, :], hist.shape)
    else:
        source = hist
    above = np.cumsum(source, axis=-1)  # values in bins <= b
    holds = above > state.rank[..., None]
    pick = holds.argmax(axis=-1)
    found = holds.any(axis=-1) & (state.rank >= 0)
    below = np.take_along_axis(above - source, pick[..., None], axis=-1)[..., 0]
    shift = np.uint64(64 - SELECT_BITS * (rnd + 1))
    state.prefix[...] = np.where(found, state.prefix | (pick.astype(np.uint64) << shift), state.prefix)
    state.rank[...] = np.where(found, state.rank - below, -1)
    hist[...] = 0


def select_finish(state: SelectState, probs, with_limits: bool = False) -> EnsembleQuantiles:
    s, k, j = state.prefix.shape
    order = np.where(state.rank >= 0, select_values(state.prefix), np.nan).reshape(s, k, j // 2, 2)
    return quantiles_from_order(probs, order, state.count, state.outside if with_limits else None)


def select_rounds_host(values, status=None, probs=(0.5,), limits=None, chunks: int = 1, on_round=None) -> EnsembleQuantiles:
    """
    The device's protocol in NumPy: ``SELECT_ROUNDS`` rounds of count (the geometries cut into ``chunks`` runs, every run added
    into the round's one histogram) and descend.  ``on_round(rnd, hist)`` sees every round's histogram before its descend.
    """
    v = np.asarray(values, dtype=np.float64)
    g, s, k = v.shape
    p, lim = check_select_arguments(probs, limits, s, k)
    st = None if status is None else np.asarray(status).reshape(g, s)
    state, hist = select_begin(s, k, p.size)
    edges = [g * i // chunks for i in range(chunks + 1)]
    for rnd in range(SELECT_ROUNDS):
        for a, b in zip(edges[:-1], edges[1:]):
            select_count_round(rnd, v[a:b], None if st is None else st[a:b], state, hist, lim)
        if on_round is not None:
            on_round(rnd, hist)
        select_descend_round(rnd, state, hist, p)
    return select_finish(state, p, lim is not None)

# ---- joint spec-limit screening: the verdict of every GEOMETRY against all its limits at once (okx_ensemble_screen) ----

SCREEN_OUTSIDE = 1     # OKX_SCREEN_OUTSIDE: a looked-at entry that counts lies strictly below lo or above hi
SCREEN_UNRESOLVED = 2  # OKX_SCREEN_UNRESOLVED: a looked-at entry does not count
TALLY_SEEN, TALLY_PASSED, TALLY_OUTSIDE, TALLY_UNRESOLVED = range(4)


@dataclass
class EnsembleScreen:
    """
    The joint verdict of an ensemble against ``limits [S, K, 2]`` (NumPy, host).  An entry is LOOKED AT when at least one of
    its limits is finite and COUNTS by the rule of the reduction (``status & 7 == 1`` and a finite value).  Per geometry:
    ``flags [G]`` uint8 (``SCREEN_OUTSIDE`` | ``SCREEN_UNRESOLVED``; 0: the geometry passes), ``margin [G]`` - the minimum
    over the looked-at entries that count of ``min((v - lo) / scale, (hi - v) / scale)``, +inf when nothing qualifies,
    negative when ``SCREEN_OUTSIDE`` is set (short of an underflow of the division) - and ``entry [G]`` int32, ``s K + k`` of
    that minimum (the lowest on ties, -1 when nothing qualifies).  Per ensemble, int64: ``tally [4]`` = geometries seen,
    passed, outside, unresolved (the last two may overlap), ``blame [S, K, 2]`` - per ``SCREEN_OUTSIDE`` geometry one count
    at its ``entry``, side 0 when the value there is below ``lo``, side 1 otherwise - and ``passed``, the ascending global
    indices of the passing geometries.  ``margin`` / ``entry`` are None where only the verdicts were gathered
    (``ShardedEnsemble.screen``).
    """

    flags: np.ndarray
    margin: np.ndarray | None
    entry: np.ndarray | None
    tally: np.ndarray
    blame: np.ndarray
    passed: np.ndarray

    @property
    def joint_yield(self) -> float:
        """``passed / seen``; NaN for an ensemble of no geometry."""
        seen = int(self.tally[TALLY_SEEN])
        return float(self.tally[TALLY_PASSED]) / seen if seen else float("nan")

    def merge(self, other: "EnsembleScreen") -> "EnsembleScreen":
        """``self`` then ``other``, consecutive runs of geometries, as one screen: per-geometry tables concatenate, integers add."""
        if self.blame.shape != other.blame.shape:
            raise ValueError("screens of different shapes")
        both = lambda a, b: None if a is None or b is None else np.concatenate([a, b])  # noqa: E731
        return EnsembleScreen(both(self.flags, other.flags), both(self.margin, other.margin), both(self.entry, other.entry),
                              self.tally + other.tally, self.blame + other.blame, both(self.passed, other.passed))


def check_screen_arguments(limits, scale=None, steps: int | None = None, n_columns: int | None = None):
    """``(limits [S, K, 2], scale [S, K] or None)`` as float64 arrays, or ValueError in the words of ``okx_ensemble_screen_check``."""
    if limits is None:
        raise ValueError("okx_ensemble_screen: null limits")
    lim = np.asarray(limits, dtype=np.float64) if steps is None else broadcast_limits(limits, steps, n_columns)
    sc = None
    if scale is not None:
        sc = np.asarray(scale, dtype=np.float64) if steps is None else broadcast_scale(scale, steps, n_columns)
    flat = lim.reshape(-1, 2)
    nan = np.flatnonzero(np.isnan(flat).any(axis=1))
    if nan.size:
        raise ValueError(f"okx_ensemble_screen: limit {int(nan[0])} is NaN (an open side is -inf / +inf)")
    bad = np.flatnonzero(flat[:, 0] > flat[:, 1])
    if bad.size:
        raise ValueError(f"okx_ensemble_screen: limit {int(bad[0])} has lo > hi ({flat[bad[0], 0]:g} > {flat[bad[0], 1]:g})")
    if sc is not None:
        bad = np.flatnonzero(~(np.isfinite(sc.reshape(-1)) & (sc.reshape(-1) > 0.0)))
        if bad.size:
            raise ValueError(f"okx_ensemble_screen: scale {int(bad[0])} is {sc.reshape(-1)[bad[0]]:g}, not finite and > 0")
    return lim, sc


def screen_host(values, status=None, limits=None, scale=None, geometry_offset: int = 0) -> EnsembleScreen:
    """
    The joint screen in NumPy: ``values [G, S, K]``, ``status [G, S]`` or None, ``limits`` ``[S, K, 2]`` / ``[K, 2]`` / ``[2]``
    (lo, hi; -inf / +inf leaves a side open), ``scale`` ``[S, K]`` / ``[K]`` / a scalar (None: 1).  Every operation is
    rounded on its own, in the device's order: ``x = (v - lo) / scale``, ``y = (hi - v) / scale``, ``m = y if y < x else x``.
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    lim, sc = check_screen_arguments(limits, scale, s, k)
    n = s * k
    lo, hi = lim[..., 0].reshape(-1), lim[..., 1].reshape(-1)
    looked = np.isfinite(lo) | np.isfinite(hi)
    v, ok = v.reshape(g, n), ok.reshape(g, n)
    counts = ok & looked[None]
    below, above = counts & (v < lo[None]), counts & (v > hi[None])
    flags = np.where((below | above).any(axis=1), SCREEN_OUTSIDE, 0) | np.where((looked[None] & ~ok).any(axis=1), SCREEN_UNRESOLVED, 0)
    flags = flags.astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        x, y = v - lo[None], hi[None] - v
        if sc is not None:
            x, y = x / sc.reshape(-1)[None], y / sc.reshape(-1)[None]
        m = np.where(counts, np.where(y < x, y, x), np.inf)
    if n:
        holds = counts & (m == m.min(axis=1)[:, None])
        some = holds.any(axis=1)
        first = holds.argmax(axis=1)  # the first True: the lowest entry among the ties
    else:
        some, first = np.zeros(g, dtype=bool), np.zeros(g, dtype=np.int64)
    rows = np.arange(g)
    entry = np.where(some, first, -1).astype(np.int32)
    margin = np.where(some, m[rows, first], np.inf) if n else np.full(g, np.inf)
    blame = np.zeros((n, 2), dtype=np.int64)
    out = np.flatnonzero((flags & SCREEN_OUTSIDE) != 0)
    if out.size:
        at = first[out]
        np.add.at(blame, (at, np.where(v[out, at] < lo[at], 0, 1)), 1)
    tally = np.array([g, int((flags == 0).sum()), out.size, int(((flags & SCREEN_UNRESOLVED) != 0).sum())], dtype=np.int64)
    passed = (int(geometry_offset) + np.flatnonzero(flags == 0)).astype(np.int64)
    return EnsembleScreen(flags, margin, entry, tally, blame.reshape(s, k, 2), passed)


# ---- covariance and correlation of the selected entries over the complete cases (okx_ensemble_covariance) ----

COV_MAX_ENTRIES = 2048  # OKX_ENS_COV_MAX_ENTRIES


@dataclass
class EnsembleCovariance:
    """
    What ``CovarianceAccumulator.finalize`` returns (NumPy, host), for the ``N`` selected entries in the caller's order:
    ``entries [N]`` (``s K + k``), ``count`` the geometries used - those whose EVERY selected entry counts -, ``dropped`` the
    others, ``mean [N]``, ``covariance [N, N]`` (unbiased; NaN for ``count < 2``), ``std [N]`` the square root of its diagonal
    and ``correlation [N, N]`` (NaN where a variance is 0).  Symmetric bit for bit.
    """

    entries: np.ndarray
    count: int
    dropped: int
    mean: np.ndarray
    covariance: np.ndarray
    std: np.ndarray
    correlation: np.ndarray


def check_covariance_arguments(entries, n_table_entries: int) -> np.ndarray:
    """``entries [N]`` as int32 (None: all ``n_table_entries`` in natural order), or ValueError in the words of
    ``okx_ensemble_covariance_check``."""
    n_table = int(n_table_entries)
    if entries is None:
        e = np.arange(min(n_table, COV_MAX_ENTRIES + 1), dtype=np.int64)
        if not 1 <= n_table <= COV_MAX_ENTRIES:
            raise ValueError(f"okx_ensemble_covariance: {n_table} entries selected, 1 to {COV_MAX_ENTRIES} allowed")
        return e.astype(np.int32)
    e = np.atleast_1d(np.asarray(entries)).reshape(-1)
    if e.size and not np.issubdtype(e.dtype, np.integer):
        raise ValueError("entries must be integers s * n_columns + k")
    e = e.astype(np.int64)
    if not 1 <= e.size <= COV_MAX_ENTRIES:
        raise ValueError(f"okx_ensemble_covariance: {e.size} entries selected, 1 to {COV_MAX_ENTRIES} allowed")
    bad = np.flatnonzero((e < 0) | (e >= n_table))
    if bad.size:
        raise ValueError(f"okx_ensemble_covariance: entry {int(bad[0])} is {int(e[bad[0]])}, outside [0, {n_table})")
    _, first = np.unique(e, return_index=True)
    again = np.setdiff1d(np.arange(e.size), first)  # the positions that repeat an earlier one, ascending
    if again.size:
        at = int(again[0])
        raise ValueError(f"okx_ensemble_covariance: entry {at} repeats entry {int(np.flatnonzero(e == e[at])[0])} (index {int(e[at])})")
    return e.astype(np.int32)


class CovarianceAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_covariance``: ``gram [N, N]`` and ``sum [N]`` float64, ``counts [2]`` int64 (used,
    dropped), ``shift [S, K]`` and ``entries [N]`` int32 - NumPy arrays or torch tensors (host or device), whatever produced
    them.  ``used [G]`` uint8 (or None) is the per-geometry byte of the LAST call that filled it.
    """

    TABLES, CARRIED, DEVICE_ONLY = ("gram", "sum", "counts", "shift", "entries", "used"), ("natural",), ("natural",)

    def __init__(self, gram, sum, counts, shift, entries, used=None, *, natural: bool = False):  # noqa: A002
        self.gram, self.sum, self.counts, self.shift, self.entries, self.used = gram, sum, counts, shift, entries, used
        self.natural = bool(natural)  # (all entries in natural order: the device pass is given no entry list)
        n = int(entries.shape[0])
        if tuple(gram.shape) != (n, n) or tuple(sum.shape) != (n,) or tuple(counts.shape) != (2,) or shift.ndim != 2:
            raise ValueError("gram must be [N, N], sum [N], counts [2], shift [S, K] and entries [N]")

    @classmethod
    def empty(cls, shift, entries=None) -> "CovarianceAccumulator":
        """The accumulator of no geometry at all (the neutral element of ``merge``), NumPy."""
        shift = np.asarray(shift, dtype=np.float64)
        e = check_covariance_arguments(entries, shift.size)
        return cls(np.zeros((e.size, e.size)), np.zeros(e.size), np.zeros(2, dtype=np.int64), shift, e)

    def merge(self, other: "CovarianceAccumulator") -> "CovarianceAccumulator":
        """``self`` then ``other`` as one accumulator (a new one; both stay): additions only, which is why both must have been
        taken with the same shift and the same entries.  Works on NumPy arrays and on torch tensors alike."""
        if not (_same_shape(self.entries, other.entries) and _same_table(self.entries, other.entries)):
            raise ValueError("accumulators of different entries cannot be merged")
        if not (_same_shape(self.shift, other.shift) and _same_table(self.shift, other.shift)):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        return CovarianceAccumulator(self.gram + other.gram, self.sum + other.sum, self.counts + other.counts, self.shift, self.entries)

    def finalize(self) -> EnsembleCovariance:
        """Mean, covariance, std and correlation on the host in fp64."""
        h = self.numpy()
        gram, s1 = np.asarray(h.gram, dtype=np.float64), np.asarray(h.sum, dtype=np.float64)
        entries = np.asarray(h.entries, dtype=np.int64)
        shift = np.asarray(h.shift, dtype=np.float64).reshape(-1)[entries]
        n, dropped = int(h.counts[0]), int(h.counts[1])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = shift + s1 / n if n > 0 else np.full(s1.shape, np.nan)
            # sum (d_n - mean_n)(d_m - mean_m) = gram - s1 s1^T / n, about a shift that lies inside the data
            cov = (gram - np.outer(s1, s1) / n) / (n - 1) if n > 1 else np.full(gram.shape, np.nan)
            var = np.maximum(np.diag(cov), 0.0) if n > 1 else np.diag(cov)
            std = np.sqrt(var)
            scale = np.outer(std, std)
            corr = np.where(scale > 0.0, cov / scale, np.nan)
        return EnsembleCovariance(entries, n, dropped, mean, cov, std, corr)


def covariance_host(values, status=None, entries=None, shift=None) -> CovarianceAccumulator:
    """
    The accumulator of ``okx_ensemble_covariance`` in NumPy.  ``values [G, S, K]``; ``status [G, S]`` uint8 or None (every
    state accepted); ``entries [N]`` distinct ``s K + k`` (None: all, natural order); ``shift [S, K]`` (None: the values of
    geometry 0, undefined entries 0).  A geometry is USED when every selected entry of it counts (``status & 7 == 1`` and a
    finite value); the sums run over the used geometries in ascending order, one after the other.
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    e = check_covariance_arguments(entries, s * k)
    if shift is None:
        shift = clean_shift(v[0]) if g else np.zeros((s, k))
    shift = np.asarray(shift, dtype=np.float64).reshape(s, k)
    if not np.all(np.isfinite(shift)):
        raise ValueError("the shift must be finite (clean_shift replaces undefined entries)")
    at = e.astype(np.int64)
    used = ok.reshape(g, s * k)[:, at].all(axis=1)
    with np.errstate(invalid="ignore"):
        d = np.where(used[:, None], v.reshape(g, s * k)[:, at] - shift.reshape(-1)[at][None], 0.0)
    gram, s1 = np.zeros((e.size, e.size)), np.zeros(e.size)
    for i in np.flatnonzero(used):  # ascending geometry order, as the device walks a slab
        gram += np.outer(d[i], d[i])
        s1 += d[i]
    counts = np.array([int(used.sum()), g - int(used.sum())], dtype=np.int64)
    return CovarianceAccumulator(gram, s1, counts, shift, e, used.astype(np.uint8))



# ---- per-geometry sweep-curve characteristics: a low-degree fit ALONG the sweep inside every geometry (okx_ensemble_curves) ----

CURVE_FIELDS = 12  # OKX_CURVE_FIELDS
CURVE_C0, CURVE_C1, CURVE_C2, CURVE_C3, CURVE_RMS, CURVE_DEPARTURE, CURVE_MIN, CURVE_MAX, CURVE_X_AT_MIN, CURVE_X_AT_MAX, CURVE_X_LO, CURVE_X_HI = range(12)
CURVE_MAX_DEGREE = 3
CURVE_PIVOT = 2.0 ** -40  # a fit is refused when a Cholesky pivot of the normal matrix in u is not greater than this times its diagonal entry


@dataclass
class EnsembleCurves:
    """
    What ``curves_host`` returns (NumPy) and ``DeviceProgram.curves_ensemble`` leaves in HBM (torch tensors): ``features
    [G, K, 12]`` float64 and ``count [G, K]`` int32, the used steps of column k of geometry g.  A step is USED when its state
    counts (``status & 7 == 1``), its abscissa x is finite and inside the closed window, and the value is finite.  Fields:
    0 .. 3 ``c0 .. c3`` of the least-squares polynomial of degree D in ``u = (x - origin) / scale`` over the used steps, in x
    units about ``origin`` (``c_i = a_i / scale^i``; degrees above D are 0.0); 4 the rms of the residuals ``sqrt(sum r^2 / n)``;
    5 the largest ``abs(r)``; 6, 7 the smallest and largest used value and 8, 9 the abscissa where they are taken (the lowest
    step on ties); 10, 11 the smallest and largest used abscissa (the lowest step on ties) - 6 .. 11 exact table bits.  With no
    used step all 12 are NaN; with fewer than D + 1 used steps or a refused fit (``CURVE_PIVOT``) fields 0 .. 5 are NaN.
    ``table()`` is the ``[G, K * 12]`` column table the other ensemble passes take with ``steps_per_geometry=1``.
    """

    features: object
    count: object
    abscissa: object = None  # device: the shared abscissa [S] as uploaded, or None (a column of the table)
    arguments: tuple = ()    # (x_column, origin, scale, lo, hi, degree) the tables were made with

    def table(self):
        return self.features.reshape(self.features.shape[0], self.features.shape[1] * self.features.shape[2])

    def _field(self, f):
        return self.features[..., f]

    value_at_origin = property(lambda self: self._field(CURVE_C0), doc="``c0 [G, K]``: the fitted value at the origin.")
    gradient = property(lambda self: self._field(CURVE_C1), doc="``c1 [G, K]``: the fitted gradient at the origin.")
    curvature = property(lambda self: 2.0 * self._field(CURVE_C2), doc="``2 c2 [G, K]``: the fitted second derivative at the origin.")
    cubic = property(lambda self: self._field(CURVE_C3), doc="``c3 [G, K]``.")
    rms = property(lambda self: self._field(CURVE_RMS), doc="rms of the fit residuals.")
    departure = property(lambda self: self._field(CURVE_DEPARTURE), doc="Largest ``abs`` residual: linearity when D = 1.")
    min = property(lambda self: self._field(CURVE_MIN))
    max = property(lambda self: self._field(CURVE_MAX))
    x_at_min = property(lambda self: self._field(CURVE_X_AT_MIN))
    x_at_max = property(lambda self: self._field(CURVE_X_AT_MAX))
    x_lo = property(lambda self: self._field(CURVE_X_LO))
    x_hi = property(lambda self: self._field(CURVE_X_HI))

    def finalize(self) -> "EnsembleCurves":
        """Host NumPy copy (self when it is one already)."""
        if not _is_tensor(self.features):
            return self
        return EnsembleCurves(self.features.detach().cpu().numpy(), self.count.detach().cpu().numpy(), None, self.arguments)


def check_curve_arguments(abscissa, origin, scale, degree, window, steps: int, n_columns: int):
    """``(x [S] float64 or None, x_column, origin, scale, lo, hi, degree)``, or ValueError in the words of
    ``okx_ensemble_curves_check``.  ``abscissa``: an integer (a column of the table) or a shared ``[S]`` table."""
    s, k = int(steps), int(n_columns)
    if isinstance(degree, bool) or int(degree) != degree or not 0 <= int(degree) <= CURVE_MAX_DEGREE:
        raise ValueError(f"okx_ensemble_curves: degree {degree}, 0 to {CURVE_MAX_DEGREE} allowed")
    scale, origin = float(scale), float(origin)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"okx_ensemble_curves: scale is {scale:g}, not finite and > 0")
    if np.isnan(origin):
        raise ValueError("okx_ensemble_curves: origin is NaN")
    lo, hi = (-np.inf, np.inf) if window is None else (float(window[0]), float(window[1]))
    if np.isnan(lo) or np.isnan(hi):
        raise ValueError("okx_ensemble_curves: window is NaN (an open side is -inf / +inf)")
    if lo > hi:
        raise ValueError(f"okx_ensemble_curves: window has lo > hi ({lo:g} > {hi:g})")
    if abscissa is None:
        raise ValueError("okx_ensemble_curves: abscissa is needed: a column of the table or a shared [S] table")
    if isinstance(abscissa, (int, np.integer)) and not isinstance(abscissa, bool):
        if not 0 <= int(abscissa) < k:
            raise ValueError(f"okx_ensemble_curves: abscissa column {int(abscissa)}, outside [0, {k})")
        return None, int(abscissa), origin, scale, lo, hi, int(degree)
    x = np.ascontiguousarray(_host_f64(abscissa).reshape(-1))
    if x.size != s:
        raise ValueError(f"okx_ensemble_curves: shared abscissa of {x.size} values, {s} steps")
    return x, -1, origin, scale, lo, hi, int(degree)


def curve_normal_refused(u, degree: int) -> bool:
    """The refusal rule on the used ``u [n]``: a pivot of the Cholesky factor of ``V^T V`` (V the Vandermonde matrix of degree
    ``degree``) is not greater than ``CURVE_PIVOT`` times its diagonal entry."""
    v = np.vander(np.asarray(u, dtype=np.float64), degree + 1, increasing=True)
    a = v.T @ v
    low = np.zeros_like(a)
    for j in range(degree + 1):
        d = a[j, j] - np.dot(low[j, :j], low[j, :j])
        if not d > CURVE_PIVOT * a[j, j]:
            return True
        low[j, j] = np.sqrt(d)
        for i in range(j + 1, degree + 1):
            low[i, j] = (a[i, j] - np.dot(low[i, :j], low[j, :j])) / low[j, j]
    return False


def curves_host(values, status=None, abscissa=None, origin: float = 0.0, scale: float = 1.0, degree: int = 2, window=None) -> EnsembleCurves:
    """
    The definition of ``okx_ensemble_curves`` in NumPy: ``values [G, S, K]``, ``status [G, S]`` or None, ``abscissa`` a shared
    ``x [S]`` or an integer column ``kx`` (``x[g, s] = values[g, s, kx]``).  The fit is ``numpy.linalg.lstsq`` on the Vandermonde
    matrix in ``u = (x - origin) / scale`` over the used steps of every (geometry, column); see ``EnsembleCurves``.
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    x, kx, origin, scale, lo, hi, degree = check_curve_arguments(abscissa, origin, scale, degree, window, s, k)
    xs = np.broadcast_to(x[None], (g, s)) if x is not None else v[:, :, kx]
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(xs) & (xs >= lo) & (xs <= hi)
    used = ok & inside[:, :, None]
    features = np.full((g, k, CURVE_FIELDS), np.nan)
    count = used.sum(axis=1).astype(np.int32)
    for gi in range(g):
        for ki in range(k):
            at = np.flatnonzero(used[gi, :, ki])
            if at.size == 0:
                continue
            y, xu = v[gi, at, ki], xs[gi, at]
            f = features[gi, ki]
            # (argmin / argmax return the FIRST extreme: the lowest step)
            f[CURVE_MIN], f[CURVE_X_AT_MIN] = y[np.argmin(y)], xu[np.argmin(y)]
            f[CURVE_MAX], f[CURVE_X_AT_MAX] = y[np.argmax(y)], xu[np.argmax(y)]
            f[CURVE_X_LO], f[CURVE_X_HI] = xu[np.argmin(xu)], xu[np.argmax(xu)]
            u = (xu - origin) / scale
            if at.size < degree + 1 or curve_normal_refused(u, degree):
                continue
            vander = np.vander(u, degree + 1, increasing=True)
            a = np.linalg.lstsq(vander, y, rcond=None)[0]
            r = y - vander @ a
            f[:4] = 0.0
            f[: degree + 1] = a / scale ** np.arange(degree + 1)
            f[CURVE_RMS] = np.sqrt(np.sum(r * r) / at.size)
            f[CURVE_DEPARTURE] = np.max(np.abs(r))
    return EnsembleCurves(features, count, None, (kx, origin, scale, lo, hi, degree))


# ---- the Pareto front of the ensemble: the geometries no other geometry beats on every objective (okx_ensemble_front) ----

FRONT_MIN, FRONT_MAX, FRONT_TARGET = 0, 1, 2  # OKX_FRONT_MIN / _MAX / _TARGET
FRONT_MAX_OBJECTIVES = 8  # OKX_ENS_FRONT_MAX_OBJECTIVES
FRONT_MAX_GEOMETRIES = 65536  # OKX_ENS_FRONT_MAX_GEOMETRIES
FRONT_SEEN, FRONT_CANDIDATES, FRONT_MEMBERS = range(3)
_FRONT_SENSES = {"min": FRONT_MIN, "max": FRONT_MAX, "target": FRONT_TARGET}


def check_front_arguments(objectives, steps: int, n_columns: int, n_geometries: int = 0):
    """``(entries [M] int32, sense [M] int32, target [M] float64)`` of ``objectives`` - a sequence of ``(step, column, sense)`` or
    ``(step, column, "target", value)``, sense ``"min"`` / ``"max"`` / ``"target"`` or ``FRONT_MIN`` / ``FRONT_MAX`` / ``FRONT_TARGET`` -
    or ValueError in the words of ``okx_ensemble_front_check``.  ``entries`` are ``step * n_columns + column``; the target of an
    objective that aims at none is 0."""
    s, k, g = int(steps), int(n_columns), int(n_geometries)
    who = "okx_ensemble_front"
    if g > FRONT_MAX_GEOMETRIES:
        raise ValueError(f"{who}: {g} geometries, at most {FRONT_MAX_GEOMETRIES} in one call (chunk and merge)")
    try:
        objectives = [tuple(o) for o in objectives]
    except TypeError:
        raise ValueError(f"{who}: objectives must be a sequence of (step, column, sense) or (step, column, 'target', value)") from None
    m = len(objectives)
    if not 1 <= m <= FRONT_MAX_OBJECTIVES:
        raise ValueError(f"{who}: {m} objectives, 1 to {FRONT_MAX_OBJECTIVES} allowed")
    entries, sense, target = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.float64)
    for i, o in enumerate(objectives):
        if len(o) not in (3, 4):
            raise ValueError(f"{who}: objective {i} must be (step, column, sense) or (step, column, 'target', value)")
        step, column, kind = o[0], o[1], o[2]
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in (step, column)):
            raise ValueError(f"{who}: objective {i}: step and column must be integers")
        if not (0 <= int(step) < s and 0 <= int(column) < k):
            raise ValueError(f"{who}: entry {i} is (step {int(step)}, column {int(column)}), outside [0, {s}) x [0, {k})")
        entries[i] = int(step) * k + int(column)
        again = np.flatnonzero(entries[:i] == entries[i])
        if again.size:
            raise ValueError(f"{who}: entry {i} repeats entry {int(again[0])} (index {int(entries[i])})")
        kind = _FRONT_SENSES.get(kind.lower(), -1) if isinstance(kind, str) else kind
        if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not FRONT_MIN <= int(kind) <= FRONT_TARGET:
            raise ValueError(f"{who}: sense {i} is {o[2]!r}, not 0 (min), 1 (max) or 2 (target)")
        sense[i] = int(kind)
        if sense[i] == FRONT_TARGET:
            if len(o) != 4:
                raise ValueError(f"{who}: objective {i} aims at a target and no target is given")
            if not np.isfinite(float(o[3])):
                raise ValueError(f"{who}: target {i} is {float(o[3]):g}, not finite")
            target[i] = float(o[3])
        elif len(o) == 4:
            raise ValueError(f"{who}: objective {i} gives a target and does not aim at one")
    return entries, sense, target


def front_objectives(raw, sense, target) -> np.ndarray:
    """The objective values ``[n, M]`` of raw table values: ``v``, ``-v`` or ``abs(v - target)``, the subtraction rounded once."""
    raw = np.asarray(raw, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(sense[None] == FRONT_MAX, -raw, np.where(sense[None] == FRONT_TARGET, np.abs(raw - target[None]), raw))


def front_dominated(objective, candidate) -> np.ndarray:
    """``dominated [n]`` int32 of objective vectors ``[n, M]`` (smaller is better) and the candidate bytes ``[n]``: how many
    candidates dominate each candidate, -1 for the others.  Blocked over b: ``n = 4099`` never allocates ``n^2 M``."""
    candidate = np.asarray(candidate, dtype=bool)
    out = np.full(candidate.shape[0], -1, dtype=np.int32)
    rows = np.flatnonzero(candidate)
    c = np.ascontiguousarray(np.asarray(objective, dtype=np.float64)[rows].T)  # [M, n]
    n = rows.size
    block = max(1, (1 << 21) // max(n, 1))
    for b0 in range(0, n, block):
        b1 = min(b0 + block, n)
        le, ge = np.ones((b1 - b0, n), dtype=bool), np.ones((b1 - b0, n), dtype=bool)
        for col in c:  # a dominates b: a <= b everywhere and not a >= b everywhere (IEEE compares: -0.0 == +0.0)
            le &= col[None, :] <= col[b0:b1, None]
            ge &= col[None, :] >= col[b0:b1, None]
        out[rows[b0:b1]] = (le & ~ge).sum(axis=1)
    return out


@dataclass
class EnsembleFront:
    """
    The nondominated (Pareto) front of an ensemble on ``M`` objectives (NumPy, host).  A geometry is a CANDIDATE when its mask
    byte is 0 (or there is no mask) and every selected entry counts (``status & 7 == 1`` and a finite value); a DOMINATES b when
    a's objectives are ``<=`` b's everywhere and ``<`` somewhere.  ``dominated [G]`` int32: the number of candidates that
    dominate the geometry, -1 when it is no candidate, 0 on the front (None for a merged front); ``tally [3]`` int64:
    geometries seen, candidates, front members; ``index [F]`` int64 and ``values [F, M]``: the ids of the front members in
    ascending row order and the RAW table values of their objectives, exact bits.  ``sense [M]`` / ``target [M]`` say how a
    value column is compared, which is all ``merge`` needs.
    """

    dominated: np.ndarray | None
    tally: np.ndarray
    index: np.ndarray
    values: np.ndarray
    sense: np.ndarray
    target: np.ndarray

    def merge(self, other: "EnsembleFront") -> "EnsembleFront":
        """The front of the union of the two fronts' rows: ``front(A u B) = front(front(A) u front(B))``.  The ids are kept,
        ``seen`` and ``candidates`` add; a merged front carries no per-geometry ``dominated``."""
        if self.values.shape[1] != other.values.shape[1] or not np.array_equal(self.sense, other.sense) \
                or not np.array_equal(self.target, other.target):
            raise ValueError("fronts of different objectives")
        values, index = np.concatenate([self.values, other.values]), np.concatenate([self.index, other.index])
        dominated = front_dominated(front_objectives(values, self.sense, self.target), np.ones(index.size, dtype=bool))
        keep = dominated == 0
        tally = np.array([self.tally[FRONT_SEEN] + other.tally[FRONT_SEEN], self.tally[FRONT_CANDIDATES] + other.tally[FRONT_CANDIDATES],
                          int(keep.sum())], dtype=np.int64)
        return EnsembleFront(None, tally, index[keep], values[keep], self.sense, self.target)


def front_host(values, status=None, objectives=None, mask=None, index=None, geometry_offset: int = 0) -> EnsembleFront:
    """
    The definition of ``okx_ensemble_front`` in NumPy: ``values [G, S, K]``, ``status [G, S]`` or None, ``objectives`` as
    ``check_front_arguments`` takes them, ``mask [G]`` (0: the geometry may be a candidate - the flag byte of ``screen_host``) or
    None, ``index [G]`` the ids of the geometries (None: ``geometry_offset + g``).
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    if objectives is None:
        raise ValueError("okx_ensemble_front: objectives are needed")
    entries, sense, target = check_front_arguments(objectives, s, k, g)
    raw = v.reshape(g, s * k)[:, entries]
    candidate = ok.reshape(g, s * k)[:, entries].all(axis=1)
    if mask is not None:
        candidate &= np.asarray(mask).reshape(g) == 0
    dominated = front_dominated(front_objectives(raw, sense, target), candidate)
    keep = dominated == 0
    ids = (int(geometry_offset) + np.arange(g, dtype=np.int64)) if index is None else np.asarray(index, dtype=np.int64).reshape(g)
    tally = np.array([g, int(candidate.sum()), int(keep.sum())], dtype=np.int64)
    return EnsembleFront(dominated, tally, ids[keep], raw[keep], sense, target)


# ---- Sobol' indices of a pick-freeze ensemble: which factor group explains the variance (okx_ensemble_sobol) ----

SOBOL_COUNT, SOBOL_DROPPED, SOBOL_SUM_A, SOBOL_SUM_B, SOBOL_SUMSQ_A, SOBOL_SUMSQ_B = range(6)
SOBOL_FIELDS = 6  # OKX_SOBOL_FIELDS; then per group j: P_j, Q_j, R_j at SOBOL_FIELDS + 3 j + 0 / 1 / 2
SOBOL_MAX_GROUPS = 288  # OKX_ENS_SOBOL_MAX_GROUPS


@dataclass
class EnsembleSobol:
    """
    What ``SobolAccumulator.finalize`` returns (NumPy, host): per (step, column) entry ``count`` the families whose every member
    counts and ``dropped`` the others ``[S, K]``, ``mean`` and ``variance`` ``[S, K]`` of the response over A and B together, and per
    factor group ``[S, K, D]``: ``first`` the first-order index (Saltelli 2010: ``(P_j / n) / V``), ``first_jansen`` the same by
    Jansen's form (``1 - (R_j / 2n) / V``) and ``total`` the total-order index (Jansen: ``(Q_j / 2n) / V``).  NaN where no family
    counts or the variance is not positive.
    """

    count: np.ndarray
    dropped: np.ndarray
    mean: np.ndarray
    variance: np.ndarray
    first: np.ndarray
    first_jansen: np.ndarray
    total: np.ndarray
    group_names: list | None = None


class SobolAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_sobol``: ``acc [S, K, SOBOL_FIELDS + 3 D]`` float64 and ``shift [S, K]`` - NumPy arrays or torch
    tensors (host or device), whatever produced them.
    """

    TABLES, CARRIED = ("acc", "shift"), ("group_names",)

    def __init__(self, acc, shift, group_names=None):
        self.acc, self.shift = acc, shift
        self.group_names = list(group_names) if group_names is not None else None
        if acc.ndim != 3 or acc.shape[2] < SOBOL_FIELDS + 3 or (acc.shape[2] - SOBOL_FIELDS) % 3 or tuple(shift.shape) != tuple(acc.shape[:2]):
            raise ValueError("acc must be [S, K, SOBOL_FIELDS + 3 D] and shift [S, K]")

    @property
    def n_groups(self) -> int:
        return (int(self.acc.shape[2]) - SOBOL_FIELDS) // 3

    @classmethod
    def empty(cls, steps: int, n_columns: int, n_groups: int, shift, group_names=None) -> "SobolAccumulator":
        """The accumulator of no family at all (the neutral element of ``merge``), NumPy."""
        return cls(np.zeros((steps, n_columns, SOBOL_FIELDS + 3 * n_groups)), np.asarray(shift, dtype=np.float64).reshape(steps, n_columns), group_names)

    def merge(self, other: "SobolAccumulator") -> "SobolAccumulator":
        """``self`` then ``other`` as one accumulator (a new one; both stay): additions only, which is why both must have been taken
        with the same shift.  Works on NumPy arrays and on torch tensors alike."""
        if not _same_shape(self.acc, other.acc):
            raise ValueError("accumulators of different shapes")
        if not _same_table(self.shift, other.shift):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        return SobolAccumulator(self.acc + other.acc, self.shift, self.group_names)

    def finalize(self) -> EnsembleSobol:
        """Mean, variance and the indices on the host in fp64."""
        h = self.numpy()
        acc, shift = np.asarray(h.acc, dtype=np.float64), np.asarray(h.shift, dtype=np.float64)
        n = acc[..., SOBOL_COUNT]
        groups = acc[..., SOBOL_FIELDS:].reshape(acc.shape[0], acc.shape[1], self.n_groups, 3)
        p, q, r = groups[..., 0], groups[..., 1], groups[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_d = (acc[..., SOBOL_SUM_A] + acc[..., SOBOL_SUM_B]) / (2.0 * n)
            v = (acc[..., SOBOL_SUMSQ_A] + acc[..., SOBOL_SUMSQ_B]) / (2.0 * n) - mean_d * mean_d
            defined = (n > 0) & (v > 0.0)
            nn, vv = n[..., None], v[..., None]
            first = np.where(defined[..., None], (p / nn) / vv, np.nan)
            first_jansen = np.where(defined[..., None], 1.0 - (r / (2.0 * nn)) / vv, np.nan)
            total = np.where(defined[..., None], (q / (2.0 * nn)) / vv, np.nan)
            mean = np.where(n > 0, mean_d + shift, np.nan)
        return EnsembleSobol(n.astype(np.int64), acc[..., SOBOL_DROPPED].astype(np.int64), mean, np.where(defined, v, np.nan), first, first_jansen,
                             total, self.group_names)


def sobol_terms(values, status=None, mask=None, n_groups: int = 1, shift=None):
    """
    The terms ``okx_ensemble_sobol`` sums, per family: ``(counts [N, S, K] bool, terms [N, S, K, SOBOL_FIELDS + 3 D], shift [S, K])`` of
    ``values [N * M, S, K]`` (``M = D + 2``, family i's members contiguous), ``status [N * M, S]`` uint8 or None and ``mask [N * M]``
    uint8 or None (bit 0 set: the member does not count).  Every difference and product is rounded on its own; the terms of a
    family that does not count are 0 (its DROPPED term 1).
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    d = int(n_groups)
    if not 1 <= d <= SOBOL_MAX_GROUPS:
        raise ValueError(f"okx_ensemble_sobol: {d} groups, 1 to {SOBOL_MAX_GROUPS} allowed")
    m = d + 2
    if g % m:
        raise ValueError(f"okx_ensemble_sobol: {g} geometries are no whole families of {m}")
    n = g // m
    if shift is None:
        shift = clean_shift(v[0]) if g else np.zeros((s, k))
    shift = np.asarray(shift, dtype=np.float64).reshape(s, k)
    if not np.all(np.isfinite(shift)):
        raise ValueError("the shift must be finite (clean_shift replaces undefined entries)")
    if mask is not None:
        ok = ok & ((np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0)[:, None, None]
    counts = ok.reshape(n, m, s, k).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        dv = np.where(counts[:, None], v.reshape(n, m, s, k) - shift[None, None], 0.0)
        da, db, dj = dv[:, 0], dv[:, 1], np.moveaxis(dv[:, 2:], 1, -1)  # [N, S, K], [N, S, K], [N, S, K, D]
        terms = np.zeros((n, s, k, SOBOL_FIELDS + 3 * d))
        terms[..., SOBOL_COUNT], terms[..., SOBOL_DROPPED] = counts, ~counts
        terms[..., SOBOL_SUM_A], terms[..., SOBOL_SUM_B] = da, db
        terms[..., SOBOL_SUMSQ_A], terms[..., SOBOL_SUMSQ_B] = da * da, db * db
        ua, ub = da[..., None] - dj, db[..., None] - dj
        terms[..., SOBOL_FIELDS + 0 :: 3] = db[..., None] * (dj - da[..., None])
        terms[..., SOBOL_FIELDS + 1 :: 3] = ua * ua
        terms[..., SOBOL_FIELDS + 2 :: 3] = ub * ub
    return counts, terms, shift


def sobol_host(values, status=None, mask=None, n_groups: int = 1, shift=None, group_names=None) -> SobolAccumulator:
    """
    The accumulator of ``okx_ensemble_sobol`` in NumPy (arguments as ``sobol_terms`` takes them; ``shift`` None: the values of
    geometry 0, undefined entries 0).  The sums run over the families in ascending order, one after the other.
    """
    v = np.asarray(values, dtype=np.float64)
    m = int(n_groups) + 2
    _, terms, shift = sobol_terms(v[:0], None if status is None else np.asarray(status)[:0], None, n_groups,
                                  (clean_shift(v[0]) if v.shape[0] else None) if shift is None else shift)
    if v.ndim == 3 and v.shape[0] % m:
        sobol_terms(v, status, mask, n_groups, shift)  # (raises: no whole families)
    acc = np.zeros(terms.shape[1:])
    block = 64 * m  # (the terms of 64 families at a time: a C5 table's would not fit the host otherwise)
    for lo in range(0, v.shape[0], block):
        rows = slice(lo, lo + block)
        _, terms, _ = sobol_terms(v[rows], None if status is None else np.asarray(status)[rows], None if mask is None else np.asarray(mask).reshape(-1)[rows],
                                  n_groups, shift)
        for i in range(terms.shape[0]):  # ascending family order, as the device walks a slab
            acc += terms[i]
    return SobolAccumulator(acc, shift, group_names)


# ---- Poisson bootstrap of the Sobol' indices: how far to trust them (okx_ensemble_bootstrap_weights, okx_ensemble_sobol_bootstrap) ----

BOOTSTRAP_MAX_REPLICATES = 1024  # OKX_ENS_BOOTSTRAP_MAX_REPLICATES
# T[k] = floor(2^32 sum_{j <= k} e^-1 / j!), k = 0 .. 12: the weight of a 32-bit word u is the number of k with u >= T[k]
BOOTSTRAP_THRESHOLDS = np.array([0x5E2D58D8, 0xBC5AB1B1, 0xEB715E1D, 0xFB239797, 0xFF1025F5, 0xFFD90F3B, 0xFFFA8B71, 0xFFFF540C, 0xFFFFED1F, 0xFFFFFE21,
                                 0xFFFFFFD4, 0xFFFFFFFC, 0xFFFFFFFF], dtype=np.uint32)
BOOTSTRAP_MAX_WEIGHT = 13  # OKX_ENS_BOOTSTRAP_MAX_WEIGHT


def check_replicates(who: str, n_replicates) -> int:
    r = int(n_replicates)
    if not 1 <= r <= BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"{who}: {r} replicates, 1 to {BOOTSTRAP_MAX_REPLICATES} allowed")
    return r


def bootstrap_weights(seed: int, lo: int, hi: int, n_replicates: int) -> np.ndarray:
    """
    The definition of ``okx_ensemble_bootstrap_weights`` in NumPy: ``uint8 [hi - lo, R]``, the Poisson(1) weight of GLOBAL row ``i`` in
    ``[lo, hi)`` (for the Sobol' bootstrap a row is a family) in replicate ``r`` - a pure function of ``(seed, i, r)``, so any range is
    the slice of the whole and every chunk, device and rank forms the same replicates.  ``u`` is word ``r % 4`` of
    ``philox4x32_10((i & 0xffffffff, i >> 32, r // 4, PURPOSE_BOOTSTRAP << 8), key of the seed)`` and the weight the number of
    ``BOOTSTRAP_THRESHOLDS`` that ``u`` reaches: integers only, at most 13.
    """
    from .ensemble_sample import PURPOSE_BOOTSTRAP, _seed_key, philox4x32_10

    r = check_replicates("okx_ensemble_bootstrap_weights", n_replicates)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi < lo:
        raise ValueError(f"okx_ensemble_bootstrap_weights: bad range [{lo}, {hi})")
    rows = (np.uint64(lo) + np.arange(hi - lo, dtype=np.uint64))[:, None]
    quads = np.arange((r + 3) // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10((rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), quads, np.uint64(PURPOSE_BOOTSTRAP << 8)), _seed_key(seed))
    u = np.stack(np.broadcast_arrays(*words), axis=-1).reshape(hi - lo, 4 * ((r + 3) // 4))[:, :r]
    return np.searchsorted(BOOTSTRAP_THRESHOLDS, u, side="right").astype(np.uint8)


@dataclass
class EnsembleSobolBootstrap:
    """
    What ``SobolBootstrapAccumulator.finalize`` returns (NumPy, host): ``SobolAccumulator.finalize`` of every replicate - ``first``,
    ``first_jansen``, ``total`` ``[R, S, K, D]`` and ``mean``, ``variance`` ``[R, S, K]``, NaN where a replicate leaves the quantity
    undefined - with, over the replicates and NaN-aware, ``<name>_std`` (``ddof = 1``) and the percentile interval
    ``interval(name, level)``.  ``defined [S, K]``: the replicates in which the entry's indices are defined.  Families are
    resampled as independent units; under ``LHS`` they are not quite independent, so the intervals are on the conservative side.
    """

    first: np.ndarray
    first_jansen: np.ndarray
    total: np.ndarray
    mean: np.ndarray
    variance: np.ndarray
    first_std: np.ndarray
    first_jansen_std: np.ndarray
    total_std: np.ndarray
    mean_std: np.ndarray
    variance_std: np.ndarray
    defined: np.ndarray
    level: float = 0.95
    group_names: list | None = None

    NAMES = ("first", "first_jansen", "total", "mean", "variance")

    def interval(self, name: str, level: float | None = None):
        """``(lo, hi)``: ``np.nanquantile`` of the replicates of ``name`` at ``(1 - level) / 2`` and ``(1 + level) / 2`` (linear rule)."""
        if name not in self.NAMES:
            raise ValueError(f"no replicates of {name!r}: one of {self.NAMES}")
        level = self.level if level is None else float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie inside (0, 1)")
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (an entry no replicate defines: NaN)
            lo, hi = np.nanquantile(getattr(self, name), [(1.0 - level) / 2.0, (1.0 + level) / 2.0], axis=0)
        return lo, hi


class SobolBootstrapAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_sobol_bootstrap``: ``acc [R, S, K, SOBOL_FIELDS + 3 D]`` float64 - replicate ``r`` holds the fields
    of a ``SobolAccumulator`` with every family's term multiplied by the family's weight - ``shift [S, K]`` and the ``seed`` of the
    weights; NumPy arrays or torch tensors (host or device).
    """

    TABLES, CARRIED = ("acc", "shift"), ("seed", "group_names")

    def __init__(self, acc, shift, seed: int, group_names=None):
        self.acc, self.shift, self.seed = acc, shift, int(seed)
        self.group_names = list(group_names) if group_names is not None else None
        if acc.ndim != 4 or acc.shape[0] < 1 or acc.shape[3] < SOBOL_FIELDS + 3 or (acc.shape[3] - SOBOL_FIELDS) % 3 \
                or tuple(shift.shape) != tuple(acc.shape[1:3]):
            raise ValueError("acc must be [R, S, K, SOBOL_FIELDS + 3 D] and shift [S, K]")

    @property
    def n_groups(self) -> int:
        return (int(self.acc.shape[3]) - SOBOL_FIELDS) // 3

    @property
    def n_replicates(self) -> int:
        return int(self.acc.shape[0])

    def merge(self, other: "SobolBootstrapAccumulator") -> "SobolBootstrapAccumulator":
        """``self`` then ``other`` as one accumulator (a new one): additions only, which is why both must have been taken with the same
        shift and - the weights of a family are a function of the seed - the same seed."""
        if not _same_shape(self.acc, other.acc):
            raise ValueError("accumulators of different shapes")
        if self.seed != other.seed:
            raise ValueError("accumulators taken with different seeds cannot be merged")
        if not _same_table(self.shift, other.shift):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        return SobolBootstrapAccumulator(self.acc + other.acc, self.shift, self.seed, self.group_names)

    def finalize(self, level: float = 0.95) -> EnsembleSobolBootstrap:
        """``SobolAccumulator.finalize`` of every replicate (``COUNT_r`` plays the part of ``n``), their standard deviations and the
        percentile intervals at ``level``, on the host in fp64."""
        import warnings

        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie inside (0, 1)")
        h = self.numpy()
        parts = [SobolAccumulator(np.asarray(h.acc[r], dtype=np.float64), h.shift).finalize() for r in range(h.n_replicates)]
        tables = {name: np.stack([getattr(part, name) for part in parts]) for name in EnsembleSobolBootstrap.NAMES}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (fewer than two defined replicates: NaN)
            std = {f"{name}_std": np.nanstd(table, axis=0, ddof=1) for name, table in tables.items()}
        defined = np.isfinite(tables["variance"]).sum(axis=0).astype(np.int64)
        return EnsembleSobolBootstrap(**tables, **std, defined=defined, level=float(level), group_names=self.group_names)


def sobol_bootstrap_host(values, status=None, mask=None, n_groups: int = 1, shift=None, *, seed: int, n_replicates: int, family_offset: int = 0,
                         weights=None, group_names=None) -> SobolBootstrapAccumulator:
    """
    The accumulator of ``okx_ensemble_sobol_bootstrap`` in NumPy (table arguments as ``sobol_terms`` takes them): family ``i`` of the
    table is GLOBAL family ``family_offset + i`` and enters replicate ``r`` with the weight ``bootstrap_weights(seed, ...)[i, r]`` -
    families ascending, ``acc[r] += w * term`` with the product rounded, then the sum; a replicate in which the family's weight is 0
    is left alone (adding +0 changes no bit).  ``weights [N, R]``: these instead of the seed's (a test's all-ones table).
    """
    r = check_replicates("okx_ensemble_sobol_bootstrap", n_replicates)
    if int(family_offset) < 0:
        raise ValueError("okx_ensemble_sobol_bootstrap: negative family_offset")
    v = np.asarray(values, dtype=np.float64)
    m = int(n_groups) + 2
    _, terms, shift = sobol_terms(v[:0], None if status is None else np.asarray(status)[:0], None, n_groups,
                                  (clean_shift(v[0]) if v.shape[0] else None) if shift is None else shift)
    if v.ndim == 3 and v.shape[0] % m:
        sobol_terms(v, status, mask, n_groups, shift)  # (raises: no whole families)
    n = v.shape[0] // m
    if weights is None:
        weights = bootstrap_weights(seed, int(family_offset), int(family_offset) + n, r)
    weights = np.asarray(weights)
    if weights.shape != (n, r):
        raise ValueError(f"weights must be [{n}, {r}]")
    acc = np.zeros((r,) + terms.shape[1:])
    block = 64 * m
    for lo in range(0, v.shape[0], block):
        rows = slice(lo, lo + block)
        _, terms, _ = sobol_terms(v[rows], None if status is None else np.asarray(status)[rows], None if mask is None else np.asarray(mask).reshape(-1)[rows],
                                  n_groups, shift)
        for i in range(terms.shape[0]):  # ascending family order, as the device walks a slab
            w = weights[lo // m + i]
            drawn = np.flatnonzero(w)
            acc[drawn] += w[drawn].astype(np.float64)[:, None, None, None] * terms[i][None]
    return SobolBootstrapAccumulator(acc, shift, seed, group_names)


__all__ = ["EnsembleAccumulator", "EnsembleStats", "reduce_host", "hardpoint_factors", "clean_shift", "factor_moment_count",
           "ENS_FIELDS", "ENS_COUNT", "ENS_REJECTED", "ENS_SUM", "ENS_SUMSQ", "ENS_MIN", "ENS_MAX", "ENS_ARGMIN", "ENS_ARGMAX",
           "EnsembleQuantiles", "SelectState", "select_host", "select_rounds_host", "select_begin", "select_count_round", "select_descend_round",
           "select_finish", "select_keys", "select_values", "quantiles_from_order", "check_select_arguments", "broadcast_limits", "broadcast_scale", "SELECT_BITS", "SELECT_BINS",
           "SELECT_ROUNDS", "SELECT_MAX_PROBS", "EnsembleScreen", "screen_host", "check_screen_arguments", "SCREEN_OUTSIDE",
           "SCREEN_UNRESOLVED", "TALLY_SEEN", "TALLY_PASSED", "TALLY_OUTSIDE", "TALLY_UNRESOLVED", "EnsembleCovariance", "CovarianceAccumulator",
           "covariance_host", "check_covariance_arguments", "COV_MAX_ENTRIES", "EnsembleCurves", "curves_host", "check_curve_arguments",
           "curve_normal_refused", "CURVE_FIELDS", "CURVE_MAX_DEGREE", "CURVE_PIVOT", "EnsembleFront", "front_host", "front_dominated",
           "front_objectives", "check_front_arguments", "FRONT_MIN", "FRONT_MAX", "FRONT_TARGET", "FRONT_MAX_OBJECTIVES", "FRONT_MAX_GEOMETRIES",
           "FRONT_SEEN", "FRONT_CANDIDATES", "FRONT_MEMBERS", "EnsembleSobol", "SobolAccumulator", "sobol_host", "sobol_terms", "SOBOL_COUNT",
           "SOBOL_DROPPED", "SOBOL_SUM_A", "SOBOL_SUM_B", "SOBOL_SUMSQ_A", "SOBOL_SUMSQ_B", "SOBOL_FIELDS", "SOBOL_MAX_GROUPS", "EnsembleSobolBootstrap",
           "SobolBootstrapAccumulator", "sobol_bootstrap_host", "bootstrap_weights", "check_replicates", "BOOTSTRAP_MAX_REPLICATES", "BOOTSTRAP_THRESHOLDS",
           "BOOTSTRAP_MAX_WEIGHT"]


# ---- main effects from given data: conditional moments over equal-probability bins of every factor (okx_ensemble_bin, okx_ensemble_effects) ----

EFFECTS_COUNT, EFFECTS_SUM, EFFECTS_SUMSQ = range(3)
EFFECTS_FIELDS = 3  # OKX_EFFECTS_FIELDS
EFFECTS_MAX_BINS = 64  # OKX_ENS_EFFECTS_MAX_BINS
EFFECTS_MAX_FACTORS = 288  # OKX_ENS_EFFECTS_MAX_FACTORS (as OKX_ENS_SAMPLE_MAX_LATENTS)
EFFECTS_NO_BIN = 255  # OKX_ENS_EFFECTS_NO_BIN: the factor is NaN, the geometry is left out for that factor alone


def check_effects_arguments(n_bins, n_factors, edges=None, bins=None):
    """``(n_bins, edges [F, n_bins - 1] float64 or None, bins [G, F] uint8 or None)``, or ValueError in the words of
    ``okx_ensemble_bin`` / ``okx_ensemble_effects``: the caps, edges finite and non-decreasing per factor, bin bytes below ``n_bins`` or
    ``EFFECTS_NO_BIN``."""
    who = "okx_ensemble_effects"
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= int(n_bins) <= EFFECTS_MAX_BINS:
        raise ValueError(f"{who}: {n_bins} bins, 1 to {EFFECTS_MAX_BINS} allowed")
    b, f = int(n_bins), int(n_factors)
    if not 1 <= f <= EFFECTS_MAX_FACTORS:
        raise ValueError(f"{who}: {f} factors, 1 to {EFFECTS_MAX_FACTORS} allowed")
    if edges is not None:
        edges = np.ascontiguousarray(_host_f64(edges))
        if edges.shape != (f, b - 1):
            raise ValueError(f"okx_ensemble_bin: edges must be [{f}, {b - 1}] (factors, bins - 1), got {list(edges.shape)}")
        bad = np.argwhere(~np.isfinite(edges))
        if bad.size:
            j, i = (int(x) for x in bad[0])
            raise ValueError(f"okx_ensemble_bin: edge {i} of factor {j} is {edges[j, i]:g}, not finite")
        bad = np.argwhere(edges[:, 1:] < edges[:, :-1])
        if bad.size:
            j, i = (int(x) for x in bad[0])
            raise ValueError(f"okx_ensemble_bin: the edges of factor {j} decrease at edge {i + 1} ({edges[j, i + 1]:g} < {edges[j, i]:g})")
    if bins is not None:
        bins = np.asarray(bins)
        if bins.ndim != 2 or bins.shape[1] != f or bins.dtype != np.uint8:
            raise ValueError(f"{who}: bins must be uint8 [G, {f}]")
        bad = np.argwhere((bins >= b) & (bins != EFFECTS_NO_BIN))
        if bad.size:
            g, j = (int(x) for x in bad[0])
            raise ValueError(f"{who}: the bin of geometry {g} for factor {j} is {int(bins[g, j])}, neither below {b} nor {EFFECTS_NO_BIN}")
    return b, edges, bins


def effects_edges(source, n_bins: int) -> np.ndarray:
    """
    ``[F, n_bins - 1]`` ascending interior edges of ``n_bins`` equal-probability bins of every factor.  ``source`` an
    ``ensemble_sample.SamplePlan`` (the factors are its latents): the ANALYTIC edges, the plan's own inverse CDFs at ``k / n_bins``
    through ``ensemble_sample.latents_from_units`` - every rank computes the same bits without seeing a sample.  ``source`` a table
    ``[G, F]``: the exact order statistic ``sorted(column)[ceil(k G / n_bins) - 1]``, a member of the column, no interpolation.
    """
    from .ensemble_sample import SamplePlan, latents_from_units

    if isinstance(source, SamplePlan):
        b = check_effects_arguments(n_bins, source.n_latents)[0]
        u = np.repeat((np.arange(1, b, dtype=np.float64) / float(b))[:, None], source.n_latents, axis=1)  # [B - 1, Z]
        return np.ascontiguousarray(latents_from_units(source, u).T)
    table = _host_f64(source)
    if table.ndim != 2 or table.shape[0] < 1:
        raise ValueError("okx_ensemble_bin: the edges of a table need factors [G, F] with G >= 1")
    g, f = table.shape
    b = check_effects_arguments(n_bins, f)[0]
    at = np.asarray([(k * g + b - 1) // b - 1 for k in range(1, b)], dtype=np.int64)  # ceil(k G / B) - 1, in integers
    return np.ascontiguousarray(np.sort(table, axis=0)[at].T.reshape(f, b - 1))


def bin_factors_host(factors, edges) -> np.ndarray:
    """
    ``okx_ensemble_bin``'s bin bytes in NumPy: ``[G, F]`` uint8 of ``factors [G, F]`` against ``edges [F, B - 1]``.  The bin is the NUMBER
    OF EDGES ``<= x`` - comparisons only: a value on an edge goes to the upper bin, ``-inf`` / ``+inf`` land in the end bins.  NaN gives
    ``EFFECTS_NO_BIN``: the geometry is left out for that factor only.
    """
    x = np.asarray(factors, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("factors must be [G, F]")
    edges = np.asarray(edges, dtype=np.float64).reshape(x.shape[1], -1)
    _, edges, _ = check_effects_arguments(edges.shape[1] + 1, x.shape[1], edges)
    with np.errstate(invalid="ignore"):
        at = (edges[None, :, :] <= x[:, :, None]).sum(axis=2)
    return np.where(np.isnan(x), EFFECTS_NO_BIN, at).astype(np.uint8)


def bin_lists_host(bins, n_bins: int):
    """``(order [F, G] int32, offsets [F, n_bins + 1] int64)`` of ``okx_ensemble_bin`` from the bin bytes ``[G, F]``: per factor the binned
    geometries bin by bin, ascending geometry index inside a bin (the slots behind them -1), and where every bin starts."""
    bins = np.asarray(bins)
    b, _, bins = check_effects_arguments(n_bins, bins.shape[1] if bins.ndim == 2 else 0, None, bins)
    g, f = bins.shape
    order = np.full((f, g), -1, dtype=np.int32)
    offsets = np.zeros((f, b + 1), dtype=np.int64)
    for j in range(f):
        ranked = np.argsort(bins[:, j], kind="stable")  # (255 sorts last)
        n = int((bins[:, j] != EFFECTS_NO_BIN).sum())
        order[j, :n] = ranked[:n]
        offsets[j, 1:] = np.cumsum(np.bincount(bins[:, j], minlength=256)[:b])
    return order, offsets


@dataclass
class EnsembleEffects:
    """
    What ``EffectsAccumulator.finalize`` returns (NumPy, host), the main effects of every factor on every (step, column) entry from
    given data (Plischke 2010).  Per (factor, bin, entry) ``[F, B, S, K]``: ``count`` the geometries of the bin that count at the entry,
    ``mean`` the conditional mean ``E[value | factor in bin]`` (NaN for an empty bin) and ``std`` the within-bin standard deviation
    (unbiased; NaN for ``count < 2``).  Per (factor, entry) ``[F, S, K]``, from the bins' sums - a geometry whose factor is NaN is in no
    bin, so these may differ from factor to factor: ``total_count``, ``total_mean``, ``total_variance`` (unbiased; NaN for ``total_count <
    2``), ``first = SSB / SST`` with ``SSB = sum_b s_b^2 / n_b - s^2 / n`` and ``SST = q - s^2 / n``, the share of the variance the
    conditional means explain, and ``first_corrected = (SSB - (B' - 1) MSW) / SST`` with ``MSW = (SST - SSB) / (n - B')`` and ``B'`` the
    non-empty bins: ``first`` less its upward bias of about ``(B' - 1) / n`` (the one-way ANOVA correction; it may come out slightly
    negative).  Both are NaN where ``SST <= 0`` or ``n <= B'``.  ``edges [F, B - 1]`` are the bins' interior edges.

    ``first`` is the first-order Sobol' index of the factor only when the factors are INDEPENDENT.  That holds for the sampler's
    latents (``factors="sampled"``); it does not hold for the mixed coordinates of a plan with ``mixing``, where a factor's bins also
    sort the geometries by what correlates with it.
    """

    count: np.ndarray
    mean: np.ndarray
    std: np.ndarray
    total_count: np.ndarray
    total_mean: np.ndarray
    total_variance: np.ndarray
    first: np.ndarray
    first_corrected: np.ndarray
    edges: np.ndarray
    factor_names: list | None = None


class EffectsAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_effects``: ``acc [F, B, EFFECTS_FIELDS, S, K]`` float64 (``COUNT``, ``SUM d``, ``SUMSQ d d`` of every
    bin of every factor), ``shift [S, K]`` and ``edges [F, B - 1]`` - NumPy arrays or torch tensors (host or device), whatever produced
    them.
    """

    TABLES, CARRIED = ("acc", "shift", "edges"), ("factor_names",)

    def __init__(self, acc, shift, edges, factor_names=None):
        self.acc, self.shift, self.edges = acc, shift, edges
        self.factor_names = list(factor_names) if factor_names is not None else None
        if acc.ndim != 5 or acc.shape[2] != EFFECTS_FIELDS or tuple(shift.shape) != tuple(acc.shape[3:]) \
                or tuple(edges.shape) != (acc.shape[0], acc.shape[1] - 1):
            raise ValueError("acc must be [F, B, EFFECTS_FIELDS, S, K], shift [S, K] and edges [F, B - 1]")

    n_factors = property(lambda self: int(self.acc.shape[0]))
    n_bins = property(lambda self: int(self.acc.shape[1]))

    @classmethod
    def empty(cls, steps: int, n_columns: int, shift, edges, factor_names=None) -> "EffectsAccumulator":
        """The accumulator of no geometry at all (the neutral element of ``merge``), NumPy."""
        edges = np.asarray(edges, dtype=np.float64)
        return cls(np.zeros((edges.shape[0], edges.shape[1] + 1, EFFECTS_FIELDS, steps, n_columns)),
                   np.asarray(shift, dtype=np.float64).reshape(steps, n_columns), edges, factor_names)

    def merge(self, other: "EffectsAccumulator") -> "EffectsAccumulator":
        """``self`` then ``other`` as one accumulator (a new one; both stay): additions only, which is why both must have been taken
        with the same shift and the same edges.  Works on NumPy arrays and on torch tensors alike."""
        if not _same_shape(self.acc, other.acc):
            raise ValueError("accumulators of different shapes")
        if not _same_table(self.edges, other.edges):
            raise ValueError("accumulators binned with different edges cannot be merged")
        if not _same_table(self.shift, other.shift):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        return EffectsAccumulator(self.acc + other.acc, self.shift, self.edges, self.factor_names)

    def finalize(self) -> EnsembleEffects:
        """Conditional means, within-bin spreads and the first-order indices on the host in fp64."""
        h = self.numpy()
        acc, shift = np.asarray(h.acc, dtype=np.float64), np.asarray(h.shift, dtype=np.float64)
        nb, sb, qb = acc[:, :, EFFECTS_COUNT], acc[:, :, EFFECTS_SUM], acc[:, :, EFFECTS_SUMSQ]  # [F, B, S, K]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_b = np.where(nb > 0, sb / nb, np.nan)
            within_b = np.where(nb > 0, np.maximum(qb - sb * mean_b, 0.0), 0.0)  # sum (d - mean_b)^2 of the bin
            std = np.sqrt(np.where(nb > 1, within_b / (nb - 1), np.nan))
            n, s, q = nb.sum(axis=1), sb.sum(axis=1), qb.sum(axis=1)              # [F, S, K]
            filled = (nb > 0).sum(axis=1).astype(np.float64)
            mean_d = np.where(n > 0, s / n, np.nan)
            sst = q - s * mean_d
            ssb = np.where(nb > 0, sb * mean_b, 0.0).sum(axis=1) - s * mean_d
            defined = (sst > 0.0) & (n > filled)
            msw = (sst - ssb) / (n - filled)
            first = np.where(defined, ssb / sst, np.nan)
            corrected = np.where(defined, (ssb - (filled - 1.0) * msw) / sst, np.nan)
            variance = np.where(n > 1, np.maximum(sst, 0.0) / (n - 1), np.nan)
        return EnsembleEffects(nb.astype(np.int64), shift[None, None] + mean_b, std, n.astype(np.int64), shift[None] + mean_d, variance, first, corrected,
                               np.asarray(h.edges, dtype=np.float64), self.factor_names)


def effects_terms(values, status=None, mask=None, shift=None):
    """The terms ``okx_ensemble_effects`` sums, per geometry: ``(counts [G, S, K] bool, d [G, S, K], shift [S, K])`` of ``values [G, S, K]``,
    ``status [G, S]`` uint8 or None and ``mask [G]`` uint8 or None (bit 0 set: the geometry does not count); ``d = value - shift``, rounded,
    0 where the geometry does not count."""
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    if shift is None:
        shift = clean_shift(v[0]) if g else np.zeros((s, k))
    shift = np.asarray(shift, dtype=np.float64).reshape(s, k)
    if not np.all(np.isfinite(shift)):
        raise ValueError("the shift must be finite (clean_shift replaces undefined entries)")
    if mask is not None:
        ok = ok & ((np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0)[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(ok, v - shift[None], 0.0)
    return ok, d, shift


def effects_host(values, status=None, mask=None, bins=None, n_bins: int = 1, shift=None, edges=None, factor_names=None) -> EffectsAccumulator:
    """
    The accumulator of ``okx_ensemble_effects`` in NumPy.  ``values [G, S, K]``; ``status [G, S]`` uint8 or None (every state accepted);
    ``mask [G]`` uint8 or None (bit 0 set: the geometry does not count - the sampler's / screen's flag byte); ``bins [G, F]`` uint8 the
    bin of every geometry for every factor (``bin_factors_host``; ``EFFECTS_NO_BIN``: in none); ``shift [S, K]`` (None: the values of
    geometry 0, undefined entries 0); ``edges [F, n_bins - 1]`` what the bins were cut with (None: not recorded, NaN).  Cell (factor,
    bin, entry) covers the geometries of that bin that count at the entry; every difference and product is rounded on its own and
    the sums run over the bin's geometries in ascending order, one after the other.
    """
    ok, d, shift = effects_terms(values, status, mask, shift)
    g, s, k = d.shape
    if bins is None:
        raise ValueError("okx_ensemble_effects: bins are needed (bin_factors_host)")
    bins = np.asarray(bins)
    b, edges, bins = check_effects_arguments(n_bins, bins.shape[1] if bins.ndim == 2 else 0, edges, bins)
    if bins.shape[0] != g:
        raise ValueError(f"okx_ensemble_effects: bins must be uint8 [{g}, F], one row per geometry")
    f = bins.shape[1]
    order, offsets = bin_lists_host(bins, b)
    acc = np.zeros((f, b, EFFECTS_FIELDS, s, k))
    with np.errstate(over="ignore", invalid="ignore"):
        sq = d * d
    for j in range(f):
        lengths = np.diff(offsets[j])
        for p in range(int(lengths.max()) if b else 0):  # the p-th geometry of every bin that has one: each cell's chain in ascending order
            has = np.flatnonzero(lengths > p)
            at = order[j, offsets[j, has] + p]
            acc[j, has, EFFECTS_COUNT] += ok[at]
            acc[j, has, EFFECTS_SUM] += d[at]
            acc[j, has, EFFECTS_SUMSQ] += sq[at]
    if edges is None:
        edges = np.full((f, b - 1), np.nan)
    return EffectsAccumulator(acc, shift, edges, factor_names)


# ---- tolerance what-ifs: the evaluated table under likelihood weights, scenario by scenario (okx_ensemble_reweigh) ----

(REWEIGH_COUNT, REWEIGH_W, REWEIGH_WW, REWEIGH_WD, REWEIGH_WDD, REWEIGH_WWD, REWEIGH_WWDD, REWEIGH_OUT_LO, REWEIGH_OUT_HI,
 REWEIGH_WW_OUT) = range(10)
REWEIGH_FIELDS = 10  # OKX_REWEIGH_FIELDS
(REWEIGH_JOINT_SEEN, REWEIGH_JOINT_SEEN_WW, REWEIGH_JOINT_PASS, REWEIGH_JOINT_PASS_WW, REWEIGH_JOINT_OUTSIDE, REWEIGH_JOINT_UNRESOLVED,
 REWEIGH_JOINT_GEOMETRIES) = range(7)
REWEIGH_JOINT_FIELDS = 7  # OKX_REWEIGH_JOINT_FIELDS
REWEIGH_MAX_SCENARIOS = 256  # OKX_ENS_TILT_MAX_SCENARIOS


def check_reweigh_limits(limits, steps: int, n_columns: int) -> np.ndarray:
    """``limits`` as a contiguous float64 ``[S, K, 2]`` table without NaN and with ``lo <= hi``, or ValueError."""
    who = "okx_ensemble_reweigh"
    limits = broadcast_limits(limits, steps, n_columns)
    if np.isnan(limits).any():
        raise ValueError(f"{who}: a limit is NaN (an open side is -inf / +inf)")
    if np.any(limits[..., 0] > limits[..., 1]):
        raise ValueError(f"{who}: a limit has lo > hi")
    return limits


def check_reweigh_arguments(weights, n_geometries: int, limits=None, verdict=None, steps: int | None = None, n_columns: int | None = None):
    """``(weights [G, S] float64, limits [S, K, 2] or None, verdict [G] uint8 or None)``, or ValueError in the words of
    ``okx_ensemble_reweigh``: the scenario cap, one weight row and one verdict byte per geometry, limits without NaN and with lo <= hi."""
    who = "okx_ensemble_reweigh"
    w = np.asarray(weights.detach().cpu().numpy() if _is_tensor(weights) else weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[0] != n_geometries:
        raise ValueError(f"{who}: weights must be [{n_geometries}, S], one row per geometry")
    if not 1 <= w.shape[1] <= REWEIGH_MAX_SCENARIOS:
        raise ValueError(f"{who}: {w.shape[1]} scenarios, 1 to {REWEIGH_MAX_SCENARIOS} allowed")
    if limits is not None:
        limits = check_reweigh_limits(limits, steps, n_columns)
    if verdict is not None:
        verdict = np.asarray(verdict.detach().cpu().numpy() if _is_tensor(verdict) else verdict)
        if verdict.shape != (n_geometries,) or verdict.dtype != np.uint8:
            raise ValueError(f"{who}: verdict must be uint8 [{n_geometries}], the screen's flag byte of every geometry")
    return w, limits, verdict


@dataclass
class EnsembleWhatIf:
    """
    What ``ReweighAccumulator.finalize`` returns (NumPy, host): what the scatter and the yield of every (step, column) entry BECOME
    under every scenario, from the ensemble as it was drawn.  Per (scenario, entry) ``[N, S, K]``, self-normalised (every sum divided
    by the sum of the weights, so a constant factor of the weights - the guards' acceptance rate - drops out): ``count`` the states
    that count with a weight above 0, ``mean = shift + WD / W``, ``variance = WDD / W - (WD / W)^2`` (not below 0), ``std``,
    ``ess = W^2 / WW`` the effective sample size, ``mean_se = sqrt(WWDD - 2 mu WWD + mu^2 WW) / W`` with ``mu = WD / W`` the standard
    error of the mean (the delta method of a ratio estimator), ``yield_ = 1 - (OUT_LO + OUT_HI) / W`` and ``yield_se`` by the same pattern
    from ``WW_OUT`` (both None without limits), ``below`` / ``above`` the weighted shares under ``lo`` / over ``hi``.  Per scenario ``[N]``,
    over the geometries the mask leaves: ``joint_yield = PASS / SEEN`` with ``joint_yield_se`` (the verdict is the screen's flag byte; without
    one every geometry passes), ``outside`` / ``unresolved`` the weighted shares of those flags, ``ess_all = SEEN^2 / SEEN_WW`` and
    ``mean_weight = SEEN / geometries`` - NEAR 1 when the draw supports the scenario; far from 1 the scenario asks for geometries the
    ensemble does not hold, and none of the above is to be trusted.  Entries and scenarios without weight are NaN.

    Under ``LHS`` the geometries are not independent: ``ess`` and the standard errors are a heuristic there.
    """

    count: np.ndarray
    mean: np.ndarray
    variance: np.ndarray
    std: np.ndarray
    ess: np.ndarray
    mean_se: np.ndarray
    yield_: np.ndarray | None
    yield_se: np.ndarray | None
    below: np.ndarray | None
    above: np.ndarray | None
    joint_yield: np.ndarray
    joint_yield_se: np.ndarray
    outside: np.ndarray
    unresolved: np.ndarray
    ess_all: np.ndarray
    mean_weight: np.ndarray
    geometries: int = 0
    scenario_names: list | None = None


class ReweighAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_reweigh``: ``acc [N, REWEIGH_FIELDS, S, K]`` float64 (scenario, field, entry), ``joint [N,
    REWEIGH_JOINT_FIELDS]``, ``shift [S, K]`` and ``limits [S, K, 2]`` or None - NumPy arrays or torch tensors (host or device), whatever
    produced them.  Accumulators of disjoint geometries merge by addition.
    """

    TABLES, CARRIED = ("acc", "joint", "shift", "limits"), ("scenario_names",)

    def __init__(self, acc, joint, shift, limits=None, scenario_names=None):
        self.acc, self.joint, self.shift, self.limits = acc, joint, shift, limits
        self.scenario_names = list(scenario_names) if scenario_names is not None else None
        if acc.ndim != 4 or acc.shape[1] != REWEIGH_FIELDS or tuple(shift.shape) != tuple(acc.shape[2:]) \
                or tuple(joint.shape) != (acc.shape[0], REWEIGH_JOINT_FIELDS) or (limits is not None and tuple(limits.shape) != tuple(acc.shape[2:]) + (2,)):
            raise ValueError("acc must be [N, REWEIGH_FIELDS, S, K], joint [N, REWEIGH_JOINT_FIELDS], shift [S, K] and limits [S, K, 2]")

    n_scenarios = property(lambda self: int(self.acc.shape[0]))

    @classmethod
    def empty(cls, n_scenarios: int, steps: int, n_columns: int, shift, limits=None, scenario_names=None) -> "ReweighAccumulator":
        """The accumulator of no geometry at all (the neutral element of ``merge``), NumPy."""
        return cls(np.zeros((n_scenarios, REWEIGH_FIELDS, steps, n_columns)), np.zeros((n_scenarios, REWEIGH_JOINT_FIELDS)),
                   np.asarray(shift, dtype=np.float64).reshape(steps, n_columns), limits, scenario_names)

    def merge(self, other: "ReweighAccumulator") -> "ReweighAccumulator":
        """``self`` then ``other`` as one accumulator (a new one; both stay): additions only, which is why both must have been taken
        with the same shift and the same limits.  Works on NumPy arrays and on torch tensors alike."""
        if not _same_shape(self.acc, other.acc):
            raise ValueError("accumulators of different shapes")
        if not _same_table(self.shift, other.shift):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        if (self.limits is None) != (other.limits is None) or (self.limits is not None and not _same_table(self.limits, other.limits)):
            raise ValueError("accumulators taken with different limits cannot be merged")
        return ReweighAccumulator(self.acc + other.acc, self.joint + other.joint, self.shift, self.limits, self.scenario_names)

    def finalize(self) -> EnsembleWhatIf:
        """The self-normalised estimates on the host in fp64."""
        h = self.numpy()
        acc, joint, shift = (np.asarray(t, dtype=np.float64) for t in (h.acc, h.joint, h.shift))
        w, ww = acc[:, REWEIGH_W], acc[:, REWEIGH_WW]
        with np.errstate(invalid="ignore", divide="ignore"):
            some = w > 0.0
            mu = np.where(some, acc[:, REWEIGH_WD] / w, np.nan)
            variance = np.maximum(acc[:, REWEIGH_WDD] / w - mu * mu, 0.0)
            variance = np.where(some, variance, np.nan)
            ess = np.where(some, w * w / ww, np.nan)
            mean_se = np.sqrt(np.maximum(acc[:, REWEIGH_WWDD] - 2.0 * mu * acc[:, REWEIGH_WWD] + mu * mu * ww, 0.0)) / w
            yield_ = yield_se = below = above = None
            if h.limits is not None:
                below, above = np.where(some, acc[:, REWEIGH_OUT_LO] / w, np.nan), np.where(some, acc[:, REWEIGH_OUT_HI] / w, np.nan)
                out = below + above
                yield_ = 1.0 - out
                yield_se = np.sqrt(np.maximum(acc[:, REWEIGH_WW_OUT] - 2.0 * out * acc[:, REWEIGH_WW_OUT] + out * out * ww, 0.0)) / w
            seen, seen_ww = joint[:, REWEIGH_JOINT_SEEN], joint[:, REWEIGH_JOINT_SEEN_WW]
            any_seen = seen > 0.0
            p = np.where(any_seen, joint[:, REWEIGH_JOINT_PASS] / seen, np.nan)
            p_ww = joint[:, REWEIGH_JOINT_PASS_WW]
            p_se = np.sqrt(np.maximum(p_ww - 2.0 * p * p_ww + p * p * seen_ww, 0.0)) / seen
            geometries = joint[:, REWEIGH_JOINT_GEOMETRIES]
            return EnsembleWhatIf(acc[:, REWEIGH_COUNT].astype(np.int64), shift[None] + mu, variance, np.sqrt(variance), ess, np.where(some, mean_se, np.nan),
                                  yield_, yield_se, below, above, p, np.where(any_seen, p_se, np.nan),
                                  np.where(any_seen, joint[:, REWEIGH_JOINT_OUTSIDE] / seen, np.nan),
                                  np.where(any_seen, joint[:, REWEIGH_JOINT_UNRESOLVED] / seen, np.nan),
                                  np.where(any_seen, seen * seen / seen_ww, np.nan), np.where(geometries > 0, seen / geometries, np.nan),
                                  int(geometries.max()) if geometries.size else 0, self.scenario_names)


def reweigh_terms(values, status=None, mask=None, shift=None, limits=None):
    """What ``okx_ensemble_reweigh`` forms per geometry before a weight comes in: ``(counts [G, S, K] bool, d [G, S, K], below, above
    [G, S, K] bool, shift [S, K])`` of ``values [G, S, K]``, ``status [G, S]`` uint8 or None, ``mask [G]`` uint8 or None (bit 0 set: the
    geometry does not count) and ``limits [S, K, 2]`` or None; ``d = value - shift``, rounded, 0 where the state does not count;
    ``below`` / ``above``: the state counts and its value lies strictly under ``lo`` / over ``hi``."""
    ok, d, shift = effects_terms(values, status, mask, shift)
    v = np.asarray(values, dtype=np.float64)
    if limits is None:
        below = above = np.zeros(v.shape, dtype=bool)
    else:
        with np.errstate(invalid="ignore"):
            below, above = ok & (v < limits[None, ..., 0]), ok & (v > limits[None, ..., 1])
    return ok, d, below, above, shift


def reweigh_scenario_terms(ok, d, below, above, w):
    """The ten terms ``[REWEIGH_FIELDS, G', S, K]`` of ONE scenario with the weights ``w [G']``: every product rounded on its own, in the
    order the device forms them - ``wl = w`` where the state counts else 0, ``wwl = w w`` likewise, ``wl d``, ``(wl d) d``, ``wwl d``,
    ``(wwl d) d``, and ``wl`` / ``wwl`` where the value is outside."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.asarray(w, dtype=np.float64)[:, None, None]
        wl, wwl = np.where(ok, w, 0.0), np.where(ok, w * w, 0.0)
        wd, wwd = wl * d, wwl * d
        return np.stack([(ok & (w > 0.0)).astype(np.float64), wl, wwl, wd, wd * d, wwd, wwd * d, np.where(below, wl, 0.0), np.where(above, wl, 0.0),
                         np.where(below | above, wwl, 0.0)])


def reweigh_host(values, status=None, mask=None, weights=None, shift=None, limits=None, verdict=None, scenario_names=None) -> ReweighAccumulator:
    """
    The accumulator of ``okx_ensemble_reweigh`` in NumPy.  ``values [G, S, K]``; ``status [G, S]`` uint8 or None (every state accepted);
    ``mask [G]`` uint8 or None (bit 0 set: the geometry does not count - the sampler's flag byte); ``weights [G, N]`` the likelihood
    ratios of N scenarios (``ensemble_sample.tilt_weights_host``, or any table of doubles); ``shift [S, K]`` (None: the values of
    geometry 0, undefined entries 0); ``limits`` ``[S, K, 2]``, ``[K, 2]`` or ``[2]`` = (lo, hi) or None (nothing is outside); ``verdict [G]``
    uint8 the screen's flag byte of every geometry (0 passes) or None (every geometry passes).  With ``d = value - shift`` and
    ``ww = w w``, per (scenario, entry) over the states that count: ``COUNT`` those with ``w > 0``, ``W``, ``WW``, ``WD = sum w d``,
    ``WDD = sum (w d) d``, ``WWD``, ``WWDD``, ``OUT_LO = sum w [v < lo]``, ``OUT_HI = sum w [v > hi]``, ``WW_OUT``; per scenario over the geometries
    whose mask bit is clear: ``SEEN = sum w``, ``SEEN_WW``, ``PASS = sum w [verdict == 0]``, ``PASS_WW``, ``OUTSIDE = sum w [verdict & 1]``,
    ``UNRESOLVED = sum w [verdict & 2]`` and ``GEOMETRIES``, their number.  A geometry whose weight is 0 adds nothing.
    """
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 3:
        raise ValueError("values must be [G, S, K]")
    g, s, k = v.shape
    if weights is None:
        raise ValueError("okx_ensemble_reweigh: weights are needed (tilt_weights_host)")
    w, limits, verdict = check_reweigh_arguments(weights, g, limits, verdict, s, k)
    ok, d, below, above, shift = reweigh_terms(v, status, mask, shift, limits)
    n = w.shape[1]
    acc = np.zeros((n, REWEIGH_FIELDS, s, k))
    rows = max(1, (1 << 21) // max(1, s * k))  # geometries per block: the ten term tables of a block stay near 160 MB
    for i in range(n):
        for a in range(0, g, rows):
            live = np.flatnonzero(w[a : a + rows, i] != 0.0) + a  # (a weight of 0 adds nothing, and the device skips it)
            if live.size:
                acc[i] += reweigh_scenario_terms(ok[live], d[live], below[live], above[live], w[live, i]).sum(axis=1)
    seen = np.ones(g, dtype=bool) if mask is None else (np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0
    flag = np.zeros(g, dtype=np.uint8) if verdict is None else verdict
    joint = np.zeros((n, REWEIGH_JOINT_FIELDS))
    with np.errstate(invalid="ignore", over="ignore"):
        wl = np.where(seen[:, None], w, 0.0)
        wwl = np.where(seen[:, None], w * w, 0.0)
        passed = (flag == 0)[:, None]
        joint[:, REWEIGH_JOINT_SEEN], joint[:, REWEIGH_JOINT_SEEN_WW] = wl.sum(axis=0), wwl.sum(axis=0)
        joint[:, REWEIGH_JOINT_PASS], joint[:, REWEIGH_JOINT_PASS_WW] = np.where(passed, wl, 0.0).sum(axis=0), np.where(passed, wwl, 0.0).sum(axis=0)
        joint[:, REWEIGH_JOINT_OUTSIDE] = np.where((flag & SCREEN_OUTSIDE != 0)[:, None], wl, 0.0).sum(axis=0)
        joint[:, REWEIGH_JOINT_UNRESOLVED] = np.where((flag & SCREEN_UNRESOLVED != 0)[:, None], wl, 0.0).sum(axis=0)
    joint[:, REWEIGH_JOINT_GEOMETRIES] = float(seen.sum())
    return ReweighAccumulator(acc, joint, shift, limits, scenario_names)


# ---- polynomial response surface with pairwise interactions: a regression on orthonormal polynomials of the factors (okx_ensemble_basis, okx_ensemble_surface) ----

SURFACE_MONOMIAL, SURFACE_HERMITE, SURFACE_LEGENDRE = 0, 1, 2  # OKX_SURFACE_*
SURFACE_MAX_TERMS = 1024    # OKX_ENS_SURFACE_MAX_TERMS: 1024 terms with 2048 entries keep every table below 16 MB
SURFACE_MAX_ENTRIES = 2048  # OKX_ENS_SURFACE_MAX_ENTRIES
SURFACE_MAX_DEGREE = 3      # OKX_ENS_SURFACE_MAX_DEGREE
SURFACE_MAX_FACTORS = 288   # OKX_ENS_SAMPLE_MAX_LATENTS
SURFACE_PIVOT = CURVE_PIVOT  # a fit is refused when a Cholesky pivot of the Gram matrix scaled to a unit diagonal is not greater than this
_SURFACE_KINDS = ("monomial", "Hermite", "Legendre")


@dataclass
class SurfaceBasis:
    """
    The terms of a response surface (``surface_terms``): ``law [P, 3]`` float64 = (kind, centre, scale) per factor, kind ``SURFACE_MONOMIAL`` /
    ``SURFACE_HERMITE`` / ``SURFACE_LEGENDRE``; ``terms [T, 4]`` int32 = (a, da, b, db): the term is ``psi_da(u_a) psi_db(u_b)`` with
    ``u = (x - centre) * scale``, ``b = -1, db = 0`` without a second factor; term 0 is the constant ``(-1, 0, -1, 0)``.  ``orthonormal``: the
    terms are orthonormal under the law the factors were drawn from, so the squared coefficients are variance shares (the indices of
    ``SurfaceAccumulator.finalize``).  ``factor_names``: one per factor, or None.
    """

    law: np.ndarray
    terms: np.ndarray
    orthonormal: bool = False
    factor_names: tuple | None = None

    n_factors = property(lambda self: int(self.law.shape[0]))
    n_terms = property(lambda self: int(self.terms.shape[0]))

    def same(self, other: "SurfaceBasis") -> bool:
        return self is other or (np.array_equal(self.law, other.law) and np.array_equal(self.terms, other.terms) and self.orthonormal == other.orthonormal)

    def term_name(self, t: int) -> str:
        """Term ``t`` in words: ``"1"``, ``"psi2(point3.z)"``, ``"psi1(point3.z) psi1(point4.z)"``."""
        name = (lambda p: self.factor_names[p] if self.factor_names is not None else f"factor{p}")
        a, da, b, db = (int(x) for x in self.terms[t])
        parts = [f"psi{d}({name(p)})" for p, d in ((a, da), (b, db)) if p >= 0]
        return " ".join(parts) if parts else "1"


def check_surface_basis(law, terms) -> tuple:
    """``(law [P, 3] float64, terms [T, 4] int32)``, contiguous, or ValueError in the words of ``okx_ensemble_basis_check``."""
    who = "okx_ensemble_basis"
    law, raw = np.asarray(law, dtype=np.float64), np.asarray(terms)
    if law.ndim != 2 or law.shape[1] != 3 or raw.ndim != 2 or raw.shape[1] != 4:
        raise ValueError("law must be [P, 3] = (kind, centre, scale) and terms [T, 4] = (a, da, b, db)")
    if raw.size and not np.issubdtype(raw.dtype, np.integer):
        raise ValueError("terms must be integers (a, da, b, db)")
    p, t = law.shape[0], raw.shape[0]
    if not 1 <= t <= SURFACE_MAX_TERMS:
        raise ValueError(f"{who}: {t} terms, 1 to {SURFACE_MAX_TERMS} allowed")
    if not 1 <= p <= SURFACE_MAX_FACTORS:
        raise ValueError(f"{who}: {p} factors, 1 to {SURFACE_MAX_FACTORS} allowed")
    for i in range(p):
        if law[i, 0] not in (SURFACE_MONOMIAL, SURFACE_HERMITE, SURFACE_LEGENDRE):
            raise ValueError(f"{who}: factor {i} has kind {law[i, 0]:g}, not 0 (monomial), 1 (Hermite) or 2 (Legendre)")
        if not np.all(np.isfinite(law[i, 1:])):
            raise ValueError(f"{who}: factor {i} has a centre or scale that is not finite")
    raw = raw.astype(np.int64)
    if tuple(raw[0]) != (-1, 0, -1, 0):
        raise ValueError(f"{who}: term 0 must be the constant (-1, 0, -1, 0)")
    for i in range(t):
        for f, d in ((raw[i, 0], raw[i, 1]), (raw[i, 2], raw[i, 3])):
            if f < -1 or f >= p:
                raise ValueError(f"{who}: term {i} names factor {int(f)}, outside [-1, {p})")
            if (d != 0) if f < 0 else not 1 <= d <= SURFACE_MAX_DEGREE:
                raise ValueError(f"{who}: term {i} has degree {int(d)} of factor {int(f)} (0 without a factor, else 1 to {SURFACE_MAX_DEGREE})")
    return np.ascontiguousarray(law), np.ascontiguousarray(raw.astype(np.int32))


def surface_terms(source, degree: int = 2, interactions: bool = True, factors=None) -> SurfaceBasis:
    """
    The basis of a response surface of total degree ``degree`` (1 to 3) over the factors of ``source``:

    * an ``ensemble_sample.SamplePlan``: its LATENTS are the factors (also with ``mixing``).  An untruncated normal latent gives Hermite with
      (0, 1), a uniform latent on ``[lo, hi] = [-1, 1]`` Legendre with centre ``(lo + hi) / 2`` and scale ``2 / (hi - lo)``, a truncated normal
      Hermite with (0, 1) - its polynomials are then not orthonormal under the law, which clears ``orthonormal``;
    * a factor table ``[G, P]`` of ALL geometries (every rank then gets the same bits): monomials of the standardised column, centre = the
      column mean, scale = 1 / the column standard deviation (1 where that is 0), over the finite values; ``orthonormal`` is cleared.

    Term 0 is the constant; then every factor's degree 1, then every factor's degree 2 (and 3), then with ``interactions`` the products
    ``psi_1(u_a) psi_1(u_b)`` for ``a > b``.  ``factors``: the indices of the factors to take (None: all), in the order wanted.
    """
    degree = int(degree)
    if not 1 <= degree <= SURFACE_MAX_DEGREE:
        raise ValueError(f"the degree of a response surface is 1 to {SURFACE_MAX_DEGREE}, not {degree}")
    orthonormal, names = True, None
    if hasattr(source, "kind") and hasattr(source, "n_latents"):
        from .ensemble_sample import NORMAL, TRUNCATED, UNIFORM

        p = source.n_latents
        law = np.zeros((p, 3))
        for i, kind in enumerate(source.kind):
            if kind == UNIFORM:
                lo, hi = -1.0, 1.0  # ensemble_sample.latents_from_units: 2 u - 1
                law[i] = SURFACE_LEGENDRE, (lo + hi) / 2.0, 2.0 / (hi - lo)
            elif kind in (NORMAL, TRUNCATED):
                law[i] = SURFACE_HERMITE, 0.0, 1.0
                orthonormal = orthonormal and kind == NORMAL
            else:
                raise ValueError(f"latent {i} has kind {int(kind)}: no polynomial family is known for it")
        names = tuple(source.factor_names())
    else:
        table = np.asarray(source, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] < 1:
            raise ValueError("the source of a basis is a SamplePlan or a factor table [G, P]")
        p = table.shape[1]
        law = np.zeros((p, 3))
        law[:, 0], law[:, 2] = SURFACE_MONOMIAL, 1.0
        for i in range(p):
            x = table[:, i][np.isfinite(table[:, i])]
            if x.size:
                law[i, 1] = np.mean(x)
                sd = float(np.std(x))
                law[i, 2] = 1.0 / sd if sd > 0.0 and np.isfinite(1.0 / sd) else 1.0
        orthonormal = False
    take = np.arange(p) if factors is None else np.atleast_1d(np.asarray(factors)).reshape(-1)
    if take.size and not np.issubdtype(take.dtype, np.integer):
        raise ValueError("factors= takes factor indices")
    take = take.astype(np.int64)
    if take.size < 1 or np.any(take < 0) or np.any(take >= p) or np.unique(take).size != take.size:
        raise ValueError(f"factors= must be distinct indices in [0, {p})")
    f = take.size
    t = 1 + degree * f + (f * (f - 1) // 2 if interactions and degree >= 2 else 0)
    if t > SURFACE_MAX_TERMS:
        raise ValueError(f"okx_ensemble_basis: {t} terms, 1 to {SURFACE_MAX_TERMS} allowed")
    rows = [(-1, 0, -1, 0)]
    for d in range(1, degree + 1):
        rows += [(int(a), d, -1, 0) for a in take]
    if interactions and degree >= 2:
        rows += [(int(take[i]), 1, int(take[j]), 1) for i in range(f) for j in range(i)]
    law, terms = check_surface_basis(law, np.array(rows, dtype=np.int32))
    return SurfaceBasis(law, terms, orthonormal, names)


def _surface_psi(kind, u):
    """``[4, G]``: psi_0 .. psi_3 of ``u [G]`` for one factor; every operation rounded on its own, as the device does them."""
    uu = u * u
    if kind == SURFACE_HERMITE:
        return np.stack([np.ones_like(u), u, (uu - 1.0) * 0.7071067811865476, ((uu - 3.0) * u) * 0.408248290463863])
    if kind == SURFACE_LEGENDRE:
        return np.stack([np.ones_like(u), u * 1.7320508075688772, (3.0 * uu - 1.0) * 1.118033988749895, ((5.0 * uu - 3.0) * u) * 1.3228756555322954])
    return np.stack([np.ones_like(u), u, uu, uu * u])


def basis_host(factors, basis: SurfaceBasis):
    """
    ``okx_ensemble_basis`` in NumPy: ``(phi [G, T] float64, valid [G] uint8)`` of ``factors [G, P]``.  ``valid`` is 0 where any factor of the
    row is not finite, and that row of ``phi`` is then 0.  No fused multiply-add anywhere: the device gives the same bits.
    """
    x = np.asarray(factors, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != basis.n_factors:
        raise ValueError(f"factors must be [G, {basis.n_factors}], one column per factor of the basis")
    g = x.shape[0]
    valid = np.isfinite(x).all(axis=1)
    one = np.ones((4, g))
    with np.errstate(invalid="ignore", over="ignore"):
        psi = {}
        for p in np.unique(basis.terms[:, (0, 2)]):
            if p >= 0:
                psi[int(p)] = _surface_psi(int(basis.law[p, 0]), (x[:, p] - basis.law[p, 1]) * basis.law[p, 2])
        phi = np.empty((g, basis.n_terms))
        for t, (a, da, b, db) in enumerate(basis.terms):
            phi[:, t] = (psi[int(a)] if a >= 0 else one)[da] * (psi[int(b)] if b >= 0 else one)[db]
    phi[~valid] = 0.0
    return phi, valid.astype(np.uint8)


def check_surface_arguments(entries, n_table_entries: int, n_terms: int | None = None) -> np.ndarray:
    """``entries [N]`` as int32 (None: all ``n_table_entries`` in natural order) by ``check_covariance_arguments``' rules with the surface pass's
    own limit, or ValueError in the words of ``okx_ensemble_surface_check``."""
    who = "okx_ensemble_surface"
    if n_terms is not None and not 1 <= int(n_terms) <= SURFACE_MAX_TERMS:
        raise ValueError(f"{who}: {int(n_terms)} terms, 1 to {SURFACE_MAX_TERMS} allowed")
    n_table = int(n_table_entries)
    n = n_table if entries is None else np.atleast_1d(np.asarray(entries)).size
    if not 1 <= n <= SURFACE_MAX_ENTRIES:
        raise ValueError(f"{who}: {n} entries selected, 1 to {SURFACE_MAX_ENTRIES} allowed")
    try:  # (SURFACE_MAX_ENTRIES <= COV_MAX_ENTRIES: the count has passed, the other rules are the covariance pass's)
        return check_covariance_arguments(entries, n_table)
    except ValueError as err:
        raise ValueError(str(err).replace("okx_ensemble_covariance", who)) from None


@dataclass
class EnsembleSurface:
    """
    What ``SurfaceAccumulator.finalize`` returns (NumPy, host), for the ``N`` selected entries in the caller's order and the ``T`` terms of
    ``basis``: ``entries [N]``, ``count`` the geometries used and ``dropped`` the others, ``shift [N]`` (of the entries), ``coefficients [T, N]``
    so that ``value ~ shift + sum_t c_t psi_t``, ``r2 [N]`` (NaN where the entry does not vary), ``residual_std [N]`` (``count - T`` degrees of
    freedom).  With an orthonormal basis the variance shares of the fit: ``variance [N] = sum_{t > 0} c_t^2``, ``first [P, N]`` from the terms
    of factor p alone, ``interaction [P, P, N]`` (symmetric, zero diagonal) from the product terms, ``total [P, N]`` from every term that contains
    p - each divided by ``variance`` (NaN where that is 0); otherwise None.  For ``surface_validate_host`` / ``DeviceProgram.validate_surface``
    the fit also carries ``whitener [T, T]`` = ``S L^-T`` of its own scaled Cholesky factor (``Phi @ whitener`` has orthonormal columns over the
    used geometries, so a row's squared norm there is its leverage) and ``total_ss [N]``, the centred sum of squares of the entries.
    """

    entries: np.ndarray
    count: int
    dropped: int
    basis: SurfaceBasis
    shift: np.ndarray
    coefficients: np.ndarray
    r2: np.ndarray
    residual_std: np.ndarray
    variance: np.ndarray | None = None
    first: np.ndarray | None = None
    interaction: np.ndarray | None = None
    total: np.ndarray | None = None
    whitener: np.ndarray | None = None
    total_ss: np.ndarray | None = None

    def predict(self, factors) -> np.ndarray:
        """``[G, N]``: the fitted entries at ``factors [G, P]`` - ``shift + basis_host(factors) @ coefficients``; NaN where a factor is not finite."""
        phi, valid = basis_host(factors, self.basis)
        out = self.shift[None, :] + phi @ self.coefficients
        out[valid == 0] = np.nan
        return out


class SurfaceAccumulator(_Accumulator):
    """
    The raw tables of ``okx_ensemble_surface``: ``gram [T, T]``, ``cross [T, N]`` and ``sumsq [N]`` float64, ``counts [2]`` int64 (used, dropped),
    ``shift [S, K]`` and ``entries [N]`` int32 - NumPy arrays or torch tensors (host or device), whatever produced them -, and the
    ``SurfaceBasis`` the rows of Phi were made with.  ``used [G]`` uint8 (or None) is the per-geometry byte of the LAST call that filled it.
    """

    TABLES, CARRIED, DEVICE_ONLY = ("gram", "cross", "sumsq", "counts", "shift", "entries", "used"), ("basis", "natural"), ("natural",)

    def __init__(self, gram, cross, sumsq, counts, shift, entries, used=None, *, basis: SurfaceBasis, natural: bool = False):
        self.gram, self.cross, self.sumsq, self.counts, self.shift, self.entries, self.used = gram, cross, sumsq, counts, shift, entries, used
        self.basis, self.natural = basis, bool(natural)
        t, n = basis.n_terms, int(entries.shape[0])
        if tuple(gram.shape) != (t, t) or tuple(cross.shape) != (t, n) or tuple(sumsq.shape) != (n,) or tuple(counts.shape) != (2,) or shift.ndim != 2:
            raise ValueError("gram must be [T, T], cross [T, N], sumsq [N], counts [2], shift [S, K] and entries [N]")

    @classmethod
    def empty(cls, shift, basis: SurfaceBasis, entries=None) -> "SurfaceAccumulator":
        """The accumulator of no geometry at all (the neutral element of ``merge``), NumPy."""
        shift = np.asarray(shift, dtype=np.float64)
        e = check_surface_arguments(entries, shift.size, basis.n_terms)
        t = basis.n_terms
        return cls(np.zeros((t, t)), np.zeros((t, e.size)), np.zeros(e.size), np.zeros(2, dtype=np.int64), shift, e, basis=basis)

    def merge(self, other: "SurfaceAccumulator") -> "SurfaceAccumulator":
        """``self`` then ``other`` as one accumulator (a new one; both stay): additions only, which is why both must have been taken with the
        same shift, entries and basis.  Works on NumPy arrays and on torch tensors alike."""
        if not self.basis.same(other.basis):
            raise ValueError("accumulators of different bases cannot be merged")
        if not (_same_shape(self.entries, other.entries) and _same_table(self.entries, other.entries)):
            raise ValueError("accumulators of different entries cannot be merged")
        if not (_same_shape(self.shift, other.shift) and _same_table(self.shift, other.shift)):
            raise ValueError("accumulators taken with different shifts cannot be merged")
        return SurfaceAccumulator(self.gram + other.gram, self.cross + other.cross, self.sumsq + other.sumsq, self.counts + other.counts, self.shift,
                                  self.entries, basis=self.basis)

    def finalize(self) -> EnsembleSurface:
        """The least-squares fit on the host in fp64: the Gram matrix scaled to a unit diagonal, Cholesky, two triangular solves.  ValueError
        when fewer than ``T + 2`` geometries were used, or naming the first term whose pivot is ``<= 2^-40`` (it is not independent of the
        terms before it)."""
        h = self.numpy()
        basis = h.basis
        gram, cross, sumsq = (np.asarray(x, dtype=np.float64) for x in (h.gram, h.cross, h.sumsq))
        entries = np.asarray(h.entries, dtype=np.int64)
        shift = np.asarray(h.shift, dtype=np.float64).reshape(-1)[entries]
        n, dropped = int(h.counts[0]), int(h.counts[1])
        t = basis.n_terms
        if n < t + 2:
            raise ValueError(f"the response surface is refused: {n} geometries used, a fit of {t} terms needs at least T + 2 = {t + 2}")
        diag = np.diag(gram)
        s = 1.0 / np.sqrt(np.where(diag > 0.0, diag, 1.0))  # (a term that is 0 in every used geometry keeps its 0 diagonal: refused below)
        a = gram * np.outer(s, s)
        lower = np.zeros((t, t))
        for j in range(t):
            pivot = a[j, j] - lower[j, :j] @ lower[j, :j]
            if not pivot > SURFACE_PIVOT:
                raise ValueError(f"the response surface is refused: term {j} ({basis.term_name(j)}) is rank-deficient - not independent of the terms "
                                 f"before it (pivot {pivot:.3g} <= 2^-40 of its diagonal entry)")
            lower[j, j] = np.sqrt(pivot)
            lower[j + 1:, j] = (a[j + 1:, j] - lower[j + 1:, :j] @ lower[j, :j]) / lower[j, j]
        y = cross * s[:, None]
        for j in range(t):  # L z = y
            y[j] = (y[j] - lower[j, :j] @ y[:j]) / lower[j, j]
        for j in range(t - 1, -1, -1):  # L^T c' = z
            y[j] = (y[j] - lower[j + 1:, j] @ y[j + 1:]) / lower[j, j]
        c = y * s[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            # term 0 separates as _fit separates the intercept: sum (phi_t - mean phi_t) d = cross_t - gram[t][0] cross_0 / n
            centred = cross[1:] - np.outer(gram[1:, 0], cross[0]) / n
            total_ss = sumsq - cross[0] * cross[0] / n
            explained = np.einsum("tn,tn->n", c[1:], centred)
            r2 = np.where(total_ss > 0.0, explained / total_ss, np.nan)
            residual_std = np.sqrt(np.maximum(total_ss - explained, 0.0) / (n - t))
        out = EnsembleSurface(entries, n, dropped, basis, shift, c, r2, residual_std)
        inverse = np.zeros((t, t))  # L^-1 by forward substitution, row by row
        for j in range(t):
            inverse[j, :j] = -(lower[j, :j] @ inverse[:j, :j]) / lower[j, j]
            inverse[j, j] = 1.0 / lower[j, j]
        out.whitener, out.total_ss = s[:, None] * inverse.T, total_ss
        if basis.orthonormal:
            p, cc = basis.n_factors, c * c
            variance = cc[1:].sum(axis=0)
            first, total, inter = np.zeros((p, c.shape[1])), np.zeros((p, c.shape[1])), np.zeros((p, p, c.shape[1]))
            for i in range(1, t):
                a_, _, b_, _ = (int(x) for x in basis.terms[i])
                if b_ < 0 or a_ < 0 or a_ == b_:
                    f = a_ if a_ >= 0 else b_
                    first[f] += cc[i]
                    total[f] += cc[i]
                else:
                    inter[a_, b_] += cc[i]
                    inter[b_, a_] += cc[i]
                    total[a_] += cc[i]
                    total[b_] += cc[i]
            with np.errstate(invalid="ignore", divide="ignore"):
                share = np.where(variance > 0.0, 1.0 / variance, np.nan)
                out.variance, out.first, out.interaction, out.total = variance, first * share, inter * share, total * share
        return out


def surface_host(values, status=None, mask=None, phi=None, valid=None, entries=None, shift=None, basis: SurfaceBasis | None = None) -> SurfaceAccumulator:
    """
    The accumulator of ``okx_ensemble_surface`` in NumPy.  ``values [G, S, K]``; ``status [G, S]`` uint8 or None (every state accepted); ``mask [G]``
    uint8 or None, bit 0 set: the geometry does not count; ``phi [G, T]`` and ``valid [G]`` from ``basis_host``; ``entries [N]`` distinct ``s K + k``
    (None: all, natural order); ``shift [S, K]`` (None: the values of geometry 0, undefined entries 0); ``basis`` the ``SurfaceBasis`` of ``phi``
    (``finalize`` needs it).  COMPLETE CASES: a geometry is USED when every selected entry of it counts (``status & 7 == 1`` and a finite
    value), bit 0 of its mask byte is clear and ``valid`` is set.  The sums run over the used geometries in ascending order, one after the
    other; every product is rounded before its addition.
    """
    v, ok = _accepted(values, status)
    g, s, k = v.shape
    phi = np.asarray(phi, dtype=np.float64)
    if phi.ndim != 2 or phi.shape[0] != g:
        raise ValueError(f"phi must be [G, T] = [{g}, T], one row per geometry of the table")
    t = phi.shape[1]
    e = check_surface_arguments(entries, s * k, t)
    if basis is not None and basis.n_terms != t:
        raise ValueError(f"phi has {t} columns, the basis {basis.n_terms} terms")
    if shift is None:
        shift = clean_shift(v[0]) if g else np.zeros((s, k))
    shift = np.asarray(shift, dtype=np.float64).reshape(s, k)
    if not np.all(np.isfinite(shift)):
        raise ValueError("the shift must be finite (clean_shift replaces undefined entries)")
    at = e.astype(np.int64)
    used = ok.reshape(g, s * k)[:, at].all(axis=1)
    if mask is not None:
        used &= (np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0
    if valid is not None:
        used &= np.asarray(valid).reshape(g) != 0
    with np.errstate(invalid="ignore"):
        d = np.where(used[:, None], v.reshape(g, s * k)[:, at] - shift.reshape(-1)[at][None], 0.0)
    gram, cross, sumsq = np.zeros((t, t)), np.zeros((t, e.size)), np.zeros(e.size)
    for i in np.flatnonzero(used):  # ascending geometry order, as the device walks a slab
        gram += np.outer(phi[i], phi[i])
        cross += np.outer(phi[i], d[i])
        sumsq += d[i] * d[i]
    counts = np.array([int(used.sum()), g - int(used.sum())], dtype=np.int64)
    if basis is None:  # (a table of doubles without a law: the terms are anonymous monomials of nothing; finalize solves, names by number)
        basis = SurfaceBasis(np.array([[0.0, 0.0, 1.0]]), np.array([[-1, 0, -1, 0]] + [[0, 1, -1, 0]] * (t - 1), dtype=np.int32))
    return SurfaceAccumulator(gram, cross, sumsq, counts, shift, e, used.astype(np.uint8), basis=basis)


# ---- evaluation of a response surface: the model as a column table, and its leave-one-out error (okx_ensemble_predict) ----

PREDICT_VALUE, PREDICT_RESIDUAL = 0, 1  # OKX_PREDICT_*


def check_predict_arguments(basis: SurfaceBasis, coefficients, shift=None, entries=None, n_table_entries: int = 0):
    """``(coefficients [T, N] float64, shift [N] float64 or None, entries [N] int32 or None)`` or ValueError in the words of
    ``okx_ensemble_predict`` / ``okx_ensemble_predict_check``.  ``n_table_entries > 0``: the RESIDUAL table has that many entries."""
    who = "okx_ensemble_predict"
    c = np.asarray(coefficients, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != basis.n_terms:
        raise ValueError(f"coefficients must be [T, N] = [{basis.n_terms}, N], one row per term of the basis")
    n = c.shape[1]
    if not 1 <= n <= SURFACE_MAX_ENTRIES:
        raise ValueError(f"{who}: {n} entries, 1 to {SURFACE_MAX_ENTRIES} allowed")
    if shift is not None:
        shift = np.asarray(shift, dtype=np.float64).reshape(-1)
        if shift.size != n:
            raise ValueError(f"shift must be [N] = [{n}], one per column of the coefficients")
    e = None
    if n_table_entries > 0:
        count = int(n_table_entries) if entries is None else np.atleast_1d(np.asarray(entries)).size
        if count != n:
            raise ValueError(f"{who}: {count} entries of the table for {n} columns of the coefficients"
                             if entries is not None else f"{who}: without an entry list all {int(n_table_entries)} entries are selected, not {n}")
        try:
            e = check_covariance_arguments(entries, int(n_table_entries))
        except ValueError as err:
            raise ValueError(str(err).replace("okx_ensemble_covariance", who)) from None
    return c, shift, e


def predict_host(factors, basis: SurfaceBasis, coefficients, shift=None, mask=None, values=None, status=None, entries=None):
    """
    ``okx_ensemble_predict`` in NumPy, the definition of both modes: ``(out [G, N] float64, valid [G] uint8)``.  ``factors [G, P]``;
    ``coefficients [T, N]``; ``shift [N]`` or None (zeros); ``mask [G]`` uint8 or None, bit 0 set drops the row.  VALUE mode (``values`` None):
    ``out = shift + basis_host(factors) @ coefficients``.  RESIDUAL mode: ``values [G, S, K]`` (``status [G, S]`` uint8 or None: every state
    accepted; ``entries [N]`` distinct ``s K + k``, None: all ``S K = N`` in natural order) gives ``out = value - (shift + ...)``, NaN where the
    entry does not count (``status & 7 != 1`` or a value that is not finite).  ``valid`` is 0 where a factor of the row is not finite or its mask
    bit is set, and that row is NaN in every column.  The device sums the terms in another order (``include/okx.h``): it agrees within
    ``(T + 4) u (|shift| + sum |psi_t c_t|) + 2 u |value|`` each side, not bit for bit.
    """
    n_table = 0
    if values is not None:
        v, ok = _accepted(values, status)
        n_table = v.shape[1] * v.shape[2]
    c, shift, e = check_predict_arguments(basis, coefficients, shift, entries, n_table)
    phi, valid = basis_host(factors, basis)
    g = phi.shape[0]
    if mask is not None:
        valid = valid & ((np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0).astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        out = phi @ c
        if shift is not None:
            out = shift[None, :] + out
        if values is not None:
            if v.shape[0] != g:
                raise ValueError(f"values must be [G, S, K] with G = {g}, one geometry per factor row")
            at = e.astype(np.int64)
            out = np.where(ok.reshape(g, n_table)[:, at], v.reshape(g, n_table)[:, at] - out, np.nan)
    out[valid == 0] = np.nan
    return out, valid.astype(np.uint8)


@dataclass
class SurfaceValidation:
    """
    The leave-one-out check of a fitted surface (``surface_validate_host``, ``DeviceProgram.validate_surface``) over the ``count`` used
    geometries, per entry ``[N]``: ``loo_rms`` = sqrt(mean e_loo^2), ``q2`` = 1 - sum e_loo^2 / total_ss (NaN where the entry does not vary; the
    out-of-sample counterpart of ``r2``, never above it), ``loo_max`` = max |e_loo| and ``loo_max_geometry`` where it is; per fit
    ``max_leverage`` and ``mean_leverage`` (T / count for a fit over exactly these geometries).  ``e_loo = e / (1 - h)``: the error of the fit
    WITHOUT geometry g AT geometry g, from the residual ``e`` and the leverage ``h`` of the fit with it - no refit.
    """

    loo_rms: np.ndarray
    q2: np.ndarray
    loo_max: np.ndarray
    loo_max_geometry: np.ndarray
    max_leverage: float
    mean_leverage: float
    count: int


def surface_used_host(surface: "EnsembleSurface", factors, values, status=None, mask=None) -> np.ndarray:
    """``[G]`` bool: the complete cases of ``surface_host`` for the entries of ``surface``."""
    v, ok = _accepted(values, status)
    g = v.shape[0]
    used = ok.reshape(g, -1)[:, np.asarray(surface.entries, dtype=np.int64)].all(axis=1)
    used &= np.isfinite(np.asarray(factors, dtype=np.float64)).all(axis=1)
    if mask is not None:
        used &= (np.asarray(mask).reshape(g).astype(np.uint8) & 1) == 0
    return used


def validation_from_terms(e, h, used, total_ss) -> SurfaceValidation:
    """``SurfaceValidation`` from the residuals ``e [G, N]``, the leverages ``h [G]`` and ``used [G]`` (NumPy); rows that are not used do not count."""
    used = np.asarray(used).reshape(-1) != 0
    count = int(used.sum())
    n = e.shape[1]
    if count == 0:
        nan = np.full(n, np.nan)
        return SurfaceValidation(nan, nan.copy(), nan.copy(), np.full(n, -1, dtype=np.int64), float("nan"), float("nan"), 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        loo = np.where(used[:, None], e / (1.0 - h)[:, None], 0.0)
        ss = (loo * loo).sum(axis=0)
        q2 = np.where(np.asarray(total_ss) > 0.0, 1.0 - ss / np.asarray(total_ss), np.nan)
    at = np.abs(loo).argmax(axis=0)
    return SurfaceValidation(np.sqrt(ss / count), q2, np.abs(loo)[at, np.arange(n)], at.astype(np.int64), float(h[used].max()), float(h[used].mean()), count)


def surface_loo_host(surface: "EnsembleSurface", factors, values, status=None, mask=None, used=None) -> tuple:
    """``(e [G, N], h [G], used [G] bool)`` of ``surface_validate_host``: the residuals ``predict_host(RESIDUAL)``, the leverages
    ``|phi_g whitener|^2`` and the used geometries; ``e_loo = e / (1 - h)`` on the used rows."""
    if surface.whitener is None or surface.total_ss is None:
        raise ValueError("the surface carries no whitener (SurfaceAccumulator.finalize fills it)")
    if used is None:
        used = surface_used_host(surface, factors, values, status, mask)
    used = np.asarray(used).reshape(-1) != 0
    e, _ = predict_host(factors, surface.basis, surface.coefficients, surface.shift, mask, values, status, surface.entries)
    z, _ = predict_host(factors, surface.basis, surface.whitener)
    with np.errstate(invalid="ignore"):
        h = (z * z).sum(axis=1)
    return e, h, used


def surface_validate_host(surface: "EnsembleSurface", factors, values, status=None, mask=None, used=None) -> SurfaceValidation:
    """
    The leave-one-out error of ``surface`` (a finalized fit with its ``whitener`` and ``total_ss``) over the geometries it was fitted on:
    ``factors [G, P]``, ``values [G, S, K]``, ``status`` and ``mask`` as ``surface_host`` took them; ``used [G]`` the used bytes of the fit
    (None: the complete cases are found again).  ``e = predict_host(RESIDUAL)``, ``h = |phi_g whitener|^2``, ``e_loo = e / (1 - h)``.
    """
    e, h, used = surface_loo_host(surface, factors, values, status, mask, used)
    return validation_from_terms(e, h, used, surface.total_ss)
