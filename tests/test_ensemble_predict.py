"""
CPU: the evaluation of a fitted response surface and its leave-one-out error in NumPy (open_kinematics_amd/ensemble_stats.py: predict_host,
SurfaceAccumulator.finalize's whitener and total_ss, surface_loo_host, surface_validate_host) - the definitions the device pass
okx_ensemble_predict and DeviceProgram.validate_surface are held to (tests/test_gpu_ensemble_predict.py).

Every tolerance is derived here (u = 2^-53), never taken from an outcome.

THE PREDICT BOUND.  psi_t (the basis row) carries the same bits in every layer.  out = shift + sum_t psi_t c_t is a sum of T products in SOME
order - BLAS on the host; ascending panels of 32 terms, four at a time inside the matrix instruction, on the device - from an accumulator
that starts at 0 (padded zero terms add exactly nothing): T products rounded (none when fused) and T additions, gamma_{T+1} sum |psi_t c_t|
for every order (Higham, Accuracy and Stability, eq. 4.4); one rounded addition of the shift makes it gamma_{T+2} (|shift| + sum |psi_t c_t|);
RESIDUAL mode rounds value - that once more: gamma_{T+3} (|shift| + sum |...|) + u |value|.  gamma_k = k u / (1 - k u) <= (k + 1) u for
k (k + 1) u <= 1, so with S = |shift| + sum_t |psi_t c_t|
                              |out - exact| <= E = (T + 4) u S + 2 u |value|
and two float results are within 2 E of each other.  The bound's own sum is rounded too: a factor 1 + 4 T u.

THE LOO TOLERANCE.  A = the Gram matrix of the used rows scaled to a unit diagonal, kappa = cond_2(A).  The fit solves the normal equations
by Cholesky: the Gram sums carry a relative error of (G + 1) u, the factorisation and the two triangular solves a backward error of
gamma_{3T+1} (Higham, theorems 10.3, 10.4), so |dc| <= kappa (G + 3 T + 2) u |c| to first order; lstsq (QR / SVD on Phi itself) is better
conditioned and is inside the same expression.  A prediction phi_j . c moves by at most |phi_j| |dc| <= T max|phi c| ~ T scale, the leverage
by the same relative amount, and 1 / (1 - h) <= 2 (ASSERTED, not measured) keeps the division from magnifying either by more than 2, its
derivative by more than 4.  So with scale_n = max_g |value - shift| of the entry
                              |e_loo - refit| <= 8 kappa (G + 3 T + 2) T u scale_n
"""

import numpy as np
import pytest

from open_kinematics_amd.ensemble_stats import (basis_host, predict_host, surface_host, surface_loo_host, surface_terms,
                                                surface_validate_host)
from test_ensemble_surface import hermite_plan

U = 2.0 ** -53


def predict_bounds(phi, coefficients, shift=None, values=None):
    """E ``[G, N]`` of the module docstring: ``phi [G, T]`` the basis rows, ``coefficients [T, N]``, ``shift [N]`` or None, ``values [G, N]`` the
    table's entries in RESIDUAL mode (undefined ones count as 0)."""
    t = phi.shape[1]
    with np.errstate(invalid="ignore"):
        s = np.abs(phi) @ np.abs(coefficients)
    if shift is not None:
        s = s + np.abs(shift)[None, :]
    e = (t + 4) * U * (1.0 + 4 * t * U) * s
    if values is not None:
        e = e + 2 * U * np.abs(np.nan_to_num(values, nan=0.0, posinf=0.0, neginf=0.0))
    return e


def loo_tolerance(phi_used, g, scale):
    """``(tolerance [N], kappa)`` of the module docstring from the basis rows of the used geometries."""
    t = phi_used.shape[1]
    gram = phi_used.T @ phi_used
    s = 1.0 / np.sqrt(np.diag(gram))
    kappa = float(np.linalg.cond(gram * np.outer(s, s)))
    return 8.0 * kappa * (g + 3 * t + 2) * t * U * scale, kappa


def loo_case(g=400, s=3, k=4, p=6, seed=5, degree=2):
    """(values [G, S, K], x [G, P], basis, shift [S, K]) in the draw order of test_gpu_ensemble_surface.real_case, no row spoiled."""
    rng = np.random.default_rng(seed)
    basis = surface_terms(hermite_plan(p), degree=degree)
    x = rng.normal(size=(g, p))
    values = rng.normal(size=(s, k))[None] * 3.0 + rng.normal(size=(g, s, k)) * 0.2 + (x @ rng.normal(size=(p, s * k))).reshape(g, s, k) \
        + (x[:, 0] * x[:, 1])[:, None, None] * rng.normal(size=(s, k))[None]
    return values, x, basis, values[3].copy()


def fitted(values, x, basis, shift, entries=None, status=None, mask=None):
    phi, valid = basis_host(x, basis)
    return surface_host(values, status, mask, phi, valid, entries, shift, basis=basis).finalize()


@pytest.fixture(scope="module")
def case():
    values, x, basis, shift = loo_case()
    return values, x, basis, shift, fitted(values, x, basis, shift)


def test_value_mode_is_the_surface_prediction(case):
    values, x, basis, shift, fit = case
    at = np.random.default_rng(1).normal(size=(50, 6))
    at[4, 2], at[9, 0], at[11, 5] = np.nan, np.inf, -np.inf
    out, valid = predict_host(at, basis, fit.coefficients, fit.shift)
    want = fit.predict(at)
    rows = np.ones(50, dtype=bool)
    rows[[4, 9, 11]] = False
    assert out.shape == (50, 12) and np.array_equal(valid, rows.astype(np.uint8))
    assert np.array_equal(out[rows], want[rows]) and np.all(np.isnan(out[~rows])) and np.all(np.isnan(want[~rows]))
    # no shift: zeros
    plain, _ = predict_host(at, basis, fit.coefficients)
    assert np.array_equal(plain[rows], (basis_host(at, basis)[0] @ fit.coefficients)[rows])


def test_a_masked_row_is_dropped_whatever_its_other_bits(case):
    _, x, basis, _, fit = case
    mask = np.zeros(20, dtype=np.uint8)
    mask[[2, 7]], mask[3], mask[5] = 1, 0xF0, 0x13  # bit 0; other bits alone; bit 0 among others
    out, valid = predict_host(x[:20], basis, fit.coefficients, fit.shift, mask=mask)
    dropped = np.isin(np.arange(20), [2, 5, 7])
    assert np.array_equal(valid, (~dropped).astype(np.uint8)) and np.all(np.isnan(out[dropped])) and np.all(np.isfinite(out[~dropped]))
    assert np.array_equal(out[~dropped], predict_host(x[:20], basis, fit.coefficients, fit.shift)[0][~dropped])


def test_residual_mode(case):
    values, x, basis, shift, _ = case
    entries = np.array([7, 0, 3, 11])
    fit = fitted(values, x, basis, shift, entries)
    assert np.array_equal(fit.entries, entries)
    g = 40
    v, st = values[:g].copy(), np.ones((g, 3), dtype=np.uint8)
    v[1, 0, 3], v[2, 1, 3], v[4, 2, 2] = np.nan, np.inf, np.nan   # entries 3, 7 and 10 (10 is not selected)
    st[5, 0], st[6, 1], st[8, 2] = 3, 5, 0                        # residual exceeded: entries 0, 3; failed: entry 7; not converged: entry 11
    xs = x[:g].copy()
    xs[9, 1] = np.nan
    out, valid = predict_host(xs, basis, fit.coefficients, fit.shift, values=v, status=st, entries=entries)
    model = predict_host(xs, basis, fit.coefficients, fit.shift)[0]
    want = v.reshape(g, 12)[:, entries] - model
    nan = np.zeros((g, 4), dtype=bool)
    nan[1, 2], nan[2, 0], nan[5, 1], nan[5, 2], nan[6, 0], nan[8, 3], nan[9, :] = True, True, True, True, True, True, True
    assert np.array_equal(np.isnan(out), nan) and valid[9] == 0 and valid.sum() == g - 1
    assert np.array_equal(out[~nan], want[~nan])
    # natural order needs N = S K; the words of the library
    with pytest.raises(ValueError, match="without an entry list all 12 entries are selected, not 4"):
        predict_host(xs, basis, fit.coefficients, fit.shift, values=v)
    with pytest.raises(ValueError, match=r"okx_ensemble_predict: entry 1 repeats entry 0 \(index 4\)"):
        predict_host(xs, basis, fit.coefficients[:, :2], fit.shift[:2], values=v, entries=[4, 4])
    with pytest.raises(ValueError, match="one row per term of the basis"):
        predict_host(xs, basis, fit.coefficients[1:], fit.shift)
    with pytest.raises(ValueError, match="one geometry per factor row"):
        predict_host(xs[:5], basis, fit.coefficients, fit.shift, values=v, entries=entries)
    full = fitted(values, x, basis, shift)
    whole, _ = predict_host(xs, basis, full.coefficients, full.shift, values=v, status=st)  # natural order
    model = predict_host(xs, basis, full.coefficients, full.shift)[0]
    assert whole.shape == (g, 12) and np.array_equal(np.isnan(whole[:, entries]), nan) and np.isnan(whole[4, 10])
    defined = ~np.isnan(whole)
    assert np.array_equal(whole[defined], (v.reshape(g, 12) - model)[defined])


def test_the_bound_holds_between_two_summation_orders(case):
    """predict_host against a term-by-term sum in DESCENDING order, in both modes: inside 2 E - the bound is not vacuous either (it is below
    1e-12 of the entry's scale)."""
    values, x, basis, shift, fit = case
    phi, _ = basis_host(x, basis)
    table = values.reshape(400, 12)
    for v in (None, values):
        got, _ = predict_host(x, basis, fit.coefficients, fit.shift, values=v)
        other = np.zeros((400, 12))
        for t in range(basis.n_terms - 1, -1, -1):
            other += phi[:, t, None] * fit.coefficients[t][None, :]
        other = fit.shift[None, :] + other
        if v is not None:
            other = table - other
        bound = predict_bounds(phi, fit.coefficients, fit.shift, None if v is None else table)
        assert np.all(np.abs(got - other) <= 2 * bound) and np.all(bound <= 1e-12 * np.abs(table).max(axis=0))


def test_whitener_and_total_ss(case):
    values, x, basis, shift, fit = case
    phi, _ = basis_host(x, basis)
    g, t = phi.shape
    d = values.reshape(g, 12) - fit.shift[None, :]
    tolerance, kappa = loo_tolerance(phi, g, 1.0)
    z = phi @ fit.whitener
    gap = np.abs(z.T @ z - np.eye(t)).max()
    print(f"whitener: |Z^T Z - I| = {gap:.2e}, tolerance {tolerance:.2e}, kappa {kappa:.2f}")
    assert fit.whitener.shape == (t, t) and gap <= tolerance
    centred = ((d - d.mean(axis=0)) ** 2).sum(axis=0)
    assert np.all(np.abs(fit.total_ss - centred) <= 8 * (g + 2) * U * (d * d).sum(axis=0))  # sumsq - cross_0^2 / n: both sums within (G + 1) u of theirs
    # a fit over complete cases only: the dropped rows take no part
    st = np.ones((g, 3), dtype=np.uint8)
    st[[5, 17], 1] = 2
    mask = np.zeros(g, dtype=np.uint8)
    mask[40] = 1
    part = fitted(values, x, basis, shift, status=st, mask=mask)
    keep = np.ones(g, dtype=bool)
    keep[[5, 17, 40]] = False
    assert part.count == g - 3
    zp = phi[keep] @ part.whitener
    assert np.abs(zp.T @ zp - np.eye(t)).max() <= tolerance
    dk = d[keep]
    assert np.all(np.abs(part.total_ss - ((dk - dk.mean(axis=0)) ** 2).sum(axis=0)) <= 8 * (g + 2) * U * (dk * dk).sum(axis=0))


def test_loo_against_brute_force_refits(case):
    values, x, basis, shift, fit = case
    g = 400
    phi, _ = basis_host(x, basis)
    assert basis.n_terms == 28
    d = values.reshape(g, 12) - fit.shift[None, :]
    e, h, used = surface_loo_host(fit, x, values)
    assert used.all() and e.shape == (g, 12)
    check = surface_validate_host(fit, x, values)
    # the CONDITION of the comparison, before anything is compared: 1 / (1 - h) <= 2
    assert check.max_leverage <= 0.5, check.max_leverage
    assert check.count == g and abs(check.mean_leverage - 28 / g) <= 1e-9 and check.max_leverage == h.max()
    loo = e / (1.0 - h)[:, None]
    order = np.argsort(h)
    tolerance, kappa = loo_tolerance(phi, g, np.abs(d).max(axis=0))
    worst = 0.0
    for j in list(order[-3:]) + [int(order[0]), int(order[g // 2])]:
        others = np.arange(g) != j
        refit, *_ = np.linalg.lstsq(phi[others], d[others], rcond=None)
        actual = d[j] - phi[j] @ refit
        gap = np.abs(loo[j] - actual)
        worst = max(worst, float((gap / np.abs(d).max(axis=0)).max()))
        assert np.all(gap <= tolerance), (j, h[j], gap.max())
    print(f"LOO against refits: gap {worst:.2e} of the entry's scale, tolerance {float((tolerance / np.abs(d).max(axis=0)).max()):.2e}, "
          f"kappa {kappa:.2f}, max leverage {check.max_leverage:.3f}")
    # the summary is the summary of these terms
    assert np.allclose(check.loo_rms, np.sqrt((loo * loo).mean(axis=0)), rtol=1e-13, atol=0.0)
    at = np.abs(loo).argmax(axis=0)
    assert np.array_equal(check.loo_max_geometry, at) and np.array_equal(check.loo_max, np.abs(loo)[at, np.arange(12)])
    assert np.all(check.q2 <= fit.r2) and np.all(check.q2 > 0.9)
    assert np.allclose(check.q2, 1.0 - (loo * loo).sum(axis=0) / fit.total_ss, rtol=1e-13, atol=0.0)


def test_validation_over_complete_cases(case):
    """Rows that the fit dropped do not count, whether the caller passes the fit's used bytes or lets them be found again."""
    values, x, basis, shift, _ = case
    g = 400
    v, st, xs = values.copy(), np.ones((g, 3), dtype=np.uint8), x.copy()
    mask = np.zeros(g, dtype=np.uint8)
    v[3, 1, 2], st[8, 0], mask[20], xs[31, 4] = np.nan, 4, 1, np.nan
    phi, valid = basis_host(xs, basis)
    acc = surface_host(v, st, mask, phi, valid, None, shift, basis=basis)
    fit = acc.finalize()
    found = surface_validate_host(fit, xs, v, st, mask)
    given = surface_validate_host(fit, xs, v, st, mask, used=acc.used)
    assert found.count == given.count == g - 4 == fit.count
    for name in ("loo_rms", "q2", "loo_max", "loo_max_geometry"):
        assert np.array_equal(getattr(found, name), getattr(given, name)), name
    assert not np.isin(found.loo_max_geometry, [3, 8, 20, 31]).any() and np.all(found.q2 <= fit.r2)
    fit.whitener = None
    with pytest.raises(ValueError, match="carries no whitener"):
        surface_validate_host(fit, xs, v, st, mask)


def validation_bounds(phi, fit, table, e, h, used):
    """Bounds on |device - host| of ``SurfaceValidation``'s fields, from the predict bound and 1 / (1 - h) <= 2 (the caller asserts it):
    ``dict(loo [G, N], loo_rms [N], loo_max [N], q2 [N], leverage)``.  ``table [G, N]`` the entries' values, ``e``, ``h``, ``used`` the host's
    own terms (surface_loo_host).  Two results of a predict call differ by 2 E; h = sum_t z_t^2 over T squares moves by
    sum 2 |z_t| dz_t + dz_t^2 and by its own summation, (T + 1) u h each side; e / (1 - h) by de / (1 - h) + |e| dh / (1 - h)^2 and two
    roundings each side; a sum of G squares by sum 2 |x| dx + dx^2 and (G + 1) u each side."""
    g, t = phi.shape
    de = 2 * predict_bounds(phi, fit.coefficients, fit.shift, table)
    dz = 2 * predict_bounds(phi, fit.whitener)
    z = np.abs(phi @ fit.whitener) + dz
    dh = (2 * z * dz + dz * dz).sum(axis=1) + 2 * (t + 1) * U * h
    keep = used[:, None]
    loo = np.where(keep, np.abs(e) / (1.0 - h)[:, None], 0.0)
    dloo = np.where(keep, 2 * de + 4 * np.abs(np.nan_to_num(e)) * dh[:, None] + 8 * U * loo, 0.0)
    ss = (loo * loo).sum(axis=0)
    dss = (2 * loo * dloo + dloo * dloo).sum(axis=0) + 2 * (g + 1) * U * ss
    count = int(used.sum())
    rms = np.sqrt(ss / count)
    # sqrt(a + da) - sqrt(a) <= da / (2 sqrt(a)) + ...: bounded by da / sqrt(a) for da <= a; the quotient and the root are rounded (4 u rms)
    drms = dss / count / np.maximum(rms, 1e-300) + 4 * U * rms
    return dict(loo=dloo, loo_rms=drms, loo_max=dloo.max(axis=0), q2=dss / fit.total_ss + 4 * U * (1.0 + ss / fit.total_ss),
                leverage=float(dh[used].max()) + 2 * (g + 1) * U)
