"""
CPU: the polynomial response surface of an evaluated ensemble (open_kinematics_amd/ensemble_stats.py: surface_terms, basis_host,
surface_host, SurfaceAccumulator, EnsembleSurface) - planted coefficients, variance shares against NumPy's lstsq and a closed form, the
orthonormality of the polynomials, merged runs, the complete-case rule, the refusals, the library's host-only entry points, and
ShardedEnsemble(reduce=True, factors=..., surface=...) on the host path in one process and over two gloo ranks.

Every tolerance is derived here from the summation order and the number format (u = 2^-53), never from an outcome.  phi (the basis row) and
d = value - shift carry the same bits in every layer (every operation of the basis is rounded on its own; d is ONE IEEE subtraction), so the
bounds start from them.  Over the n geometries of a call:

  gram[t][t'] = sum phi_t phi_t', cross[t][m] = sum phi_t d_m, sumsq[m] = sum d_m d_m: a sum of at most n products in SOME order - one after
      the other on the host, four at a time inside a matrix instruction and slab by slab on the device, chunk after chunk when merged.  The
      first-order bound of a sum of n terms holds for every order, (n - 1) u sum |term| (Higham, Accuracy and Stability, eq. 4.4), plus the
      rounding of each product (u each; none when it is fused), plus one u for the final rounding of an exact reference:
                                       |result - exact| <= E = (n + 1) u sum |term|
  two float results (host and device, merged and whole, two chunkings): each within E of the exact value, so within 2 E = 2 (n + 1) u sum |term|
      of each other.  The bound's own sum is rounded too: a factor 1 + 4 n u.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from open_kinematics_amd import ensemble_sample as sm
from open_kinematics_amd.ensemble_stats import (SURFACE_HERMITE, SURFACE_LEGENDRE, SURFACE_MAX_ENTRIES, SURFACE_MAX_TERMS, SURFACE_MONOMIAL,
                                                EnsembleSurface, SurfaceAccumulator, SurfaceBasis, basis_host, check_surface_arguments,
                                                check_surface_basis, surface_host, surface_terms)

U = 2.0 ** -53


def hermite_plan(p, kind=sm.NORMAL):
    """A sampling plan of ``p`` latents of one kind (one per coordinate of ``ceil(p / 3)`` points)."""
    return sm.SamplePlan(nominal=np.zeros(((p + 2) // 3, 3)), coords=np.arange(p), kind=kind)


def surface_bounds(phi, d):
    """(E gram [T, T], E cross [T, N], E sumsq [N]) of the module docstring for a call over the rows of ``phi [n, T]`` and ``d [n, N]`` (the rows
    of dropped geometries zero)."""
    n = phi.shape[0]
    f, a = np.abs(phi), np.abs(d)
    c = (n + 1) * U * (1.0 + 4 * n * U)
    return c * (f.T @ f), c * (f.T @ a), c * (a * a).sum(axis=0)


def within(got, want, bound):
    eg, ec, es = bound
    return np.all(np.abs(got.gram - want.gram) <= 2 * eg) and np.all(np.abs(got.cross - want.cross) <= 2 * ec) and np.all(np.abs(got.sumsq - want.sumsq) <= 2 * es)


def test_terms_and_laws():
    plan = sm.SamplePlan(nominal=np.zeros((2, 3)), coords=np.arange(4), kind=[sm.NORMAL, sm.UNIFORM, sm.NORMAL, sm.UNIFORM])
    b = surface_terms(plan)
    assert b.orthonormal and b.n_factors == 4 and b.n_terms == 1 + 2 * 4 + 6 and b.terms.dtype == np.int32 and b.law.dtype == np.float64
    assert b.law.tolist() == [[SURFACE_HERMITE, 0.0, 1.0], [SURFACE_LEGENDRE, 0.0, 1.0]] * 2
    assert b.terms[0].tolist() == [-1, 0, -1, 0]
    assert b.terms[1:5].tolist() == [[a, 1, -1, 0] for a in range(4)] and b.terms[5:9].tolist() == [[a, 2, -1, 0] for a in range(4)]
    assert b.terms[9:].tolist() == [[1, 1, 0, 1], [2, 1, 0, 1], [2, 1, 1, 1], [3, 1, 0, 1], [3, 1, 1, 1], [3, 1, 2, 1]]
    assert b.term_name(0) == "1" and b.term_name(6) == "psi2(point0.y)" and b.term_name(9) == "psi1(point0.y) psi1(point0.x)"
    assert surface_terms(plan, degree=1).n_terms == 5 and surface_terms(plan, degree=3).n_terms == 1 + 12 + 6
    assert surface_terms(plan, interactions=False).n_terms == 9
    few = surface_terms(plan, factors=[3, 1])
    assert few.n_factors == 4 and few.terms.tolist() == [[-1, 0, -1, 0], [3, 1, -1, 0], [1, 1, -1, 0], [3, 2, -1, 0], [1, 2, -1, 0], [1, 1, 3, 1]]
    assert 1 + 2 * 30 + 435 == surface_terms(hermite_plan(30)).n_terms == 496  # the C5 size
    assert not surface_terms(sm.SamplePlan(nominal=np.zeros((1, 3)), coords=[0, 1], kind=sm.TRUNCATED, bound=2.0)).orthonormal
    mixed = sm.SamplePlan(nominal=np.zeros((1, 3)), coords=[0, 1], kind=sm.NORMAL, mixing=np.eye(2))
    assert surface_terms(mixed).orthonormal and surface_terms(mixed).factor_names == ("latent0", "latent1")
    # a factor table: monomials of the standardised columns, the same bits from the same table
    rng = np.random.default_rng(2)
    table = rng.normal(size=(50, 3)) * [1.0, 5.0, 0.0] + [3.0, -1.0, 2.0]
    table[7, 0] = np.nan
    t = surface_terms(table)
    assert not t.orthonormal and np.all(t.law[:, 0] == SURFACE_MONOMIAL) and t.law[2].tolist() == [0.0, 2.0, 1.0]
    finite = table[np.isfinite(table[:, 0]), 0]
    assert t.law[0, 1] == np.mean(finite) and t.law[0, 2] == 1.0 / np.std(finite)
    assert np.array_equal(surface_terms(table.copy()).law, t.law)


def test_planted_coefficients_are_recovered():
    """A table built as shift + Phi c: an entry with a linear, a quadratic and a product term and otherwise zeros, an entry with every
    coefficient planted, under all three kinds of law."""
    rng = np.random.default_rng(3)
    g, p = 500, 5
    plan = sm.SamplePlan(nominal=np.zeros((2, 3)), coords=np.arange(p), kind=[sm.NORMAL, sm.UNIFORM, sm.NORMAL, sm.UNIFORM, sm.NORMAL])
    x = np.where(np.asarray(plan.kind) == sm.UNIFORM, rng.uniform(-1, 1, size=(g, p)), rng.normal(size=(g, p)))
    for basis in (surface_terms(plan), surface_terms(plan, degree=3), surface_terms(x * 3.0 + 1.0)):
        source = x if basis.orthonormal else x * 3.0 + 1.0
        phi, valid = basis_host(source, basis)
        t = basis.n_terms
        assert valid.all() and phi.shape == (g, t) and np.all(phi[:, 0] == 1.0)
        c = np.zeros((t, 3))
        quad = int(np.flatnonzero((basis.terms[:, 0] == 2) & (basis.terms[:, 1] == 2))[0])
        cross = int(np.flatnonzero((basis.terms[:, 0] == 3) & (basis.terms[:, 2] == 1))[0])
        c[[1, quad, cross], 0] = 0.7, -1.3, 2.1
        c[:, 1] = rng.normal(size=t)
        c[0, 2] = 4.0  # (a constant entry: nothing to explain)
        shift = np.array([[10.0, -2.0, 0.5]])
        values = (shift + phi @ c).reshape(g, 1, 3)
        fit = surface_host(values, None, None, phi, valid, None, shift, basis=basis).finalize()
        assert isinstance(fit, EnsembleSurface) and fit.count == g and fit.dropped == 0 and fit.coefficients.shape == (t, 3)
        assert np.all(np.abs(fit.coefficients - c) <= 1e-9 * np.abs(c).max(axis=0))
        assert np.all(np.abs(fit.r2[:2] - 1.0) <= 1e-9)
        # the residual sum of squares is the DIFFERENCE of two sums of g products, each within (g + 1) u of its terms and carried through a
        # solve with cond(gram) < 16 here: it is 0 to within 16 (g + 1) u sum d^2, its root to within the square root of that
        rms = np.sqrt(((values[:, 0, :] - shift) ** 2).sum(axis=0) / (g - t))
        assert np.all(fit.residual_std <= np.sqrt(16 * (g + 1) * U) * rms)
        assert np.all(np.abs(fit.predict(source) - values[:, 0, :]) <= 1e-9 * np.abs(values).max())
        assert (fit.first is not None) == basis.orthonormal
        if basis.orthonormal:
            var = 0.7 ** 2 + 1.3 ** 2 + 2.1 ** 2
            assert abs(fit.variance[0] - var) <= 1e-8 * var
            assert abs(fit.first[0, 0] - 0.49 / var) <= 1e-8 and abs(fit.first[2, 0] - 1.69 / var) <= 1e-8
            assert abs(fit.interaction[3, 1, 0] - 4.41 / var) <= 1e-8 and fit.interaction[1, 3, 0] == fit.interaction[3, 1, 0]
            assert abs(fit.total[1, 0] - 4.41 / var) <= 1e-8 and abs(fit.total[4, 0]) <= 1e-8 and np.all(np.diagonal(fit.interaction) == 0.0)


def test_indices_against_lstsq_and_the_closed_form():
    """y = 2 z0 + 3 He2(z1) + 1.5 z0 z2 + noise over 4096 IID normal latents: variance 4 + 9 + 2.25 = 15.25.  The fit is asserted against NumPy's
    lstsq of the same table at 1e-9 (cond(Phi^T Phi / G) is about 1.2 here: the normal equations lose nothing that matters); the closed form
    gets the margin the fit's own coefficient standard errors give: five of them, propagated to first order through share = c_i^2 / V, plus
    the squares that terms with a true coefficient of 0 add to V."""
    rng = np.random.default_rng(4096)
    g, sigma = 4096, 0.25
    basis = surface_terms(hermite_plan(3))
    z = rng.standard_normal((g, 3))
    phi, valid = basis_host(z, basis)
    y = 2.0 * z[:, 0] + 3.0 * (z[:, 1] ** 2 - 1.0) / np.sqrt(2.0) + 1.5 * z[:, 0] * z[:, 2] + sigma * rng.standard_normal(g)
    shift = np.array([[0.25]])
    fit = surface_host((y + 0.25).reshape(g, 1, 1), None, None, phi, valid, None, shift, basis=basis).finalize()
    ref, *_ = np.linalg.lstsq(phi, y[:, None], rcond=None)
    assert np.all(np.abs(fit.coefficients - ref) <= 1e-9 * np.abs(ref).max())
    cc = ref[:, 0] ** 2
    var = cc[1:].sum()
    pure = lambda a: sum(cc[i] for i in range(1, 10) if basis.terms[i, 0] == a and basis.terms[i, 2] < 0)  # noqa: E731
    holds = lambda a: sum(cc[i] for i in range(1, 10) if a in (basis.terms[i, 0], basis.terms[i, 2]))  # noqa: E731
    pair = int(np.flatnonzero((basis.terms[:, 0] == 2) & (basis.terms[:, 2] == 0))[0])
    assert abs(fit.variance[0] - var) <= 1e-9 * var
    for a in range(3):
        assert abs(fit.first[a, 0] - pure(a) / var) <= 1e-9 and abs(fit.total[a, 0] - holds(a) / var) <= 1e-9
    assert abs(fit.interaction[2, 0, 0] - cc[pair] / var) <= 1e-9 and fit.interaction[0, 2, 0] == fit.interaction[2, 0, 0]
    # the closed form
    resid = y - phi @ ref[:, 0]
    s2 = resid @ resid / (g - basis.n_terms)
    assert abs(fit.residual_std[0] - np.sqrt(s2)) <= 1e-9 and abs(np.sqrt(s2) - sigma) < 0.05 * sigma
    se = np.sqrt(s2 * np.diag(np.linalg.inv(phi.T @ phi)))
    c = ref[:, 0]
    v_true = 15.25

    def margin(members):
        share = sum(cc[i] for i in members) / var
        first_order = sum(abs(2.0 * c[i] * ((1.0 if i in members else 0.0) - share)) / var * 5.0 * se[i] for i in range(1, 10))
        return first_order + sum((5.0 * se[i]) ** 2 for i in range(1, 10)) / var

    lin0 = [1]
    quad1 = [int(np.flatnonzero((basis.terms[:, 0] == 1) & (basis.terms[:, 1] == 2))[0])]
    print("shares", fit.first[0, 0], fit.first[1, 0], fit.interaction[2, 0, 0], "margins", margin(lin0), margin(quad1), margin([pair]))
    assert abs(fit.first[0, 0] - 4.0 / v_true) <= margin(lin0)
    assert abs(fit.first[1, 0] - 9.0 / v_true) <= margin(quad1)
    assert abs(fit.interaction[2, 0, 0] - 2.25 / v_true) <= margin([pair])
    assert abs(fit.total[0, 0] - 6.25 / v_true) <= margin(lin0 + [pair]) and abs(fit.total[2, 0] - 2.25 / v_true) <= margin([pair])
    assert abs(fit.total[1, 0] - 9.0 / v_true) <= margin(quad1)
    assert margin(lin0) < 0.01  # the margins are worth the test
    assert abs(fit.r2[0] - (1.0 - resid @ resid / ((y - y.mean()) @ (y - y.mean())))) <= 1e-9


@pytest.mark.parametrize("kind", [SURFACE_HERMITE, SURFACE_LEGENDRE])
def test_the_polynomials_are_orthonormal(kind):
    """sum w psi_i psi_j = delta_ij to 1e-14 for degrees 0 to 3 over Gauss nodes that integrate degree 6 exactly (8 nodes: degree 15)."""
    if kind == SURFACE_HERMITE:
        nodes, weights = np.polynomial.hermite_e.hermegauss(8)
        weights = weights / np.sqrt(2.0 * np.pi)  # the standard normal density
        centre, scale = 0.0, 1.0
    else:
        nodes, weights = np.polynomial.legendre.leggauss(8)
        weights = weights / 2.0  # the uniform density on [lo, hi]
        lo, hi = -3.0, 5.0
        nodes, centre, scale = (lo + hi) / 2.0 + nodes * (hi - lo) / 2.0, (lo + hi) / 2.0, 2.0 / (hi - lo)
    basis = SurfaceBasis(*check_surface_basis([[kind, centre, scale]], [[-1, 0, -1, 0], [0, 1, -1, 0], [0, 2, -1, 0], [0, 3, -1, 0]]))
    phi, valid = basis_host(nodes[:, None], basis)
    assert valid.all()
    assert np.all(np.abs((phi * weights[:, None]).T @ phi - np.eye(4)) <= 1e-14)


def integer_case(g, s, k, p, seed):
    """Integer factors in [-2, 2] under the monomial law (0, 1) and integer d: every product and every sum is exact."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(g, p)).astype(np.float64)
    shift = rng.integers(-50, 50, size=(s, k)).astype(np.float64)
    values = shift[None] + rng.integers(-1000, 1000, size=(g, s, k))
    status = np.ones((g, s), dtype=np.uint8)
    basis = surface_terms(np.zeros((2, p)), degree=3)
    return values, status, x, basis, shift


def real_case(g, s, k, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(g, p))
    values = rng.normal(size=(s, k))[None] * 3.0 + rng.normal(size=(g, s, k)) + (x @ rng.normal(size=(p, s * k))).reshape(g, s, k)
    return values, np.ones((g, s), dtype=np.uint8), x, surface_terms(hermite_plan(p)), np.nan_to_num(values[0])


def merged(values, status, mask, phi, valid, entries, shift, basis, edges):
    acc = SurfaceAccumulator.empty(shift, basis, entries)
    for a, b in zip(edges[:-1], edges[1:]):
        acc = acc.merge(surface_host(values[a:b], status[a:b], None if mask is None else mask[a:b], phi[a:b], valid[a:b], entries, shift, basis=basis))
    return acc


@pytest.mark.parametrize("edges", [[0, 97], [0, 40, 97], [0, 1, 2, 50, 50, 97]])
def test_merged_chunks_are_the_whole(edges):
    g, s, k, p = 97, 3, 4, 4
    entries = [5, 0, 11, 2]
    values, status, x, basis, shift = integer_case(g, s, k, p, 1)
    status[5, 1], values[9, 0, 0] = 2, np.nan
    phi, valid = basis_host(x, basis)
    whole = surface_host(values, status, None, phi, valid, entries, shift, basis=basis)
    got = merged(values, status, None, phi, valid, entries, shift, basis, edges)
    for name in ("gram", "cross", "sumsq", "counts"):
        assert np.array_equal(getattr(got, name), getattr(whole, name)), name
    assert list(whole.counts) == [95, 2]
    values, status, x, basis, shift = real_case(g, s, k, p, 2)
    phi, valid = basis_host(x, basis)
    whole = surface_host(values, status, None, phi, valid, entries, shift, basis=basis)
    got = merged(values, status, None, phi, valid, entries, shift, basis, edges)
    d = values.reshape(g, s * k)[:, entries] - shift.reshape(-1)[entries]
    assert np.array_equal(got.counts, whole.counts) and within(got, whole, surface_bounds(phi, d))
    if len(edges) == 2:
        assert np.array_equal(got.gram, whole.gram)  # one chunk after the empty accumulator: the same additions
    # merging needs the same shift, entries and basis
    with pytest.raises(ValueError, match="different shifts"):
        whole.merge(surface_host(values, status, None, phi, valid, entries, shift + 1.0, basis=basis))
    with pytest.raises(ValueError, match="different entries"):
        whole.merge(surface_host(values, status, None, phi, valid, [5, 0, 11, 3], shift, basis=basis))
    with pytest.raises(ValueError, match="different bases"):
        other = surface_terms(hermite_plan(p, sm.UNIFORM))
        whole.merge(surface_host(values, status, None, phi, valid, entries, shift, basis=other))


def test_complete_cases_change_used_and_nothing_else():
    g, s, k, p = 60, 3, 4, 3
    entries = [5, 0, 11]
    values, status, x, basis, shift = real_case(g, s, k, p, 7)
    phi, valid = basis_host(x, basis)
    base = surface_host(values, status, None, phi, valid, entries, shift, basis=basis)
    assert list(base.counts) == [g, 0] and base.used.all()

    def dropped(acc, rows):
        keep = np.setdiff1d(np.arange(g), rows)
        want = surface_host(values[keep], status[keep], None, phi[keep], valid[keep], entries, shift, basis=basis)
        assert list(acc.counts) == [g - len(rows), len(rows)] and np.array_equal(np.flatnonzero(acc.used == 0), rows)
        for name in ("gram", "cross", "sumsq"):
            assert np.array_equal(getattr(acc, name), getattr(want, name)), name  # the same additions in the same order: the same bits

    st = status.copy()
    st[4, 1] = 5  # a failed state in a selected step (entry 5 = step 1, column 1)
    dropped(surface_host(values, st, None, phi, valid, entries, shift, basis=basis), [4])
    st = status.copy()
    st[4, 1] = 9  # (an advisory bit: still accepted)
    dropped(surface_host(values, st, None, phi, valid, entries, shift, basis=basis), [])
    v = values.copy()
    v[6, 0, 1] = np.nan  # entry 1 is not selected: ignored
    dropped(surface_host(v, status, None, phi, valid, entries, shift, basis=basis), [])
    v[6, 2, 3] = np.inf  # entry 11 is
    dropped(surface_host(v, status, None, phi, valid, entries, shift, basis=basis), [6])
    mask = np.zeros(g, dtype=np.uint8)
    mask[[8, 9, 10]] = 1, 2, 3  # bit 0 decides
    dropped(surface_host(values, status, mask, phi, valid, entries, shift, basis=basis), [8, 10])
    xx = x.copy()
    xx[12, 2] = np.nan
    phi2, valid2 = basis_host(xx, basis)
    assert valid2[12] == 0 and valid2.sum() == g - 1 and not phi2[12].any() and np.array_equal(np.delete(phi2, 12, axis=0), np.delete(phi, 12, axis=0))
    dropped(surface_host(values, status, None, phi2, valid2, entries, shift, basis=basis), [12])


def test_refusals():
    g, s, k, p = 40, 2, 3, 3
    values, status, x, basis, shift = real_case(g, s, k, p, 9)
    phi, valid = basis_host(x, basis)
    # rank deficiency: a duplicated factor column
    twin = np.column_stack([x, x[:, 0]])
    wide = surface_terms(hermite_plan(4), interactions=False)
    phi4, valid4 = basis_host(twin, wide)
    with pytest.raises(ValueError, match=r"term 4 \(psi1\(point1.x\)\) is rank-deficient - not independent of the terms before it \(pivot .* <= 2\^-40"):
        surface_host(values, status, None, phi4, valid4, None, shift, basis=wide).finalize()
    # too few geometries: T = 10 needs 12
    with pytest.raises(ValueError, match=r"11 geometries used, a fit of 10 terms needs at least T \+ 2 = 12"):
        surface_host(values[:11], status[:11], None, phi[:11], valid[:11], None, shift, basis=basis).finalize()
    surface_host(values[:12], status[:12], None, phi[:12], valid[:12], None, shift, basis=basis).finalize()
    # the basis
    with pytest.raises(ValueError, match=r"okx_ensemble_basis: term 0 must be the constant \(-1, 0, -1, 0\)"):
        check_surface_basis(basis.law, basis.terms[1:])
    with pytest.raises(ValueError, match=r"okx_ensemble_basis: term 2 names factor 3, outside \[-1, 3\)"):
        check_surface_basis(basis.law, [[-1, 0, -1, 0], [0, 1, -1, 0], [3, 1, -1, 0]])
    with pytest.raises(ValueError, match=r"okx_ensemble_basis: term 1 has degree 4 of factor 0 \(0 without a factor, else 1 to 3\)"):
        check_surface_basis(basis.law, [[-1, 0, -1, 0], [0, 4, -1, 0]])
    with pytest.raises(ValueError, match="okx_ensemble_basis: factor 1 has kind 3, not 0"):
        check_surface_basis([[0, 0, 1], [3, 0, 1]], [[-1, 0, -1, 0]])
    with pytest.raises(ValueError, match="okx_ensemble_basis: factor 0 has a centre or scale that is not finite"):
        check_surface_basis([[0, np.nan, 1]], [[-1, 0, -1, 0]])
    with pytest.raises(ValueError, match=f"okx_ensemble_basis: 1081 terms, 1 to {SURFACE_MAX_TERMS} allowed"):
        surface_terms(hermite_plan(45))  # 1 + 90 + 990
    assert surface_terms(hermite_plan(43)).n_terms == 990 <= SURFACE_MAX_TERMS
    with pytest.raises(ValueError, match="the degree of a response surface is 1 to 3, not 4"):
        surface_terms(hermite_plan(3), degree=4)
    with pytest.raises(ValueError, match=r"factors= must be distinct indices in \[0, 3\)"):
        surface_terms(hermite_plan(3), factors=[0, 0])
    # the entries
    with pytest.raises(ValueError, match=r"okx_ensemble_surface: entry 1 repeats entry 0 \(index 4\)"):
        surface_host(values, status, None, phi, valid, [4, 4], shift, basis=basis)
    with pytest.raises(ValueError, match=r"okx_ensemble_surface: entry 0 is 6, outside \[0, 6\)"):
        check_surface_arguments([6], 6)
    with pytest.raises(ValueError, match=f"okx_ensemble_surface: 2049 entries selected, 1 to {SURFACE_MAX_ENTRIES} allowed"):
        check_surface_arguments(None, 2049)
    with pytest.raises(ValueError, match="okx_ensemble_surface: 0 entries selected, 1 to 2048 allowed"):
        check_surface_arguments([], 6)
    with pytest.raises(ValueError, match="okx_ensemble_surface: 1025 terms, 1 to 1024 allowed"):
        check_surface_arguments(None, 6, 1025)
    with pytest.raises(ValueError, match="one row per geometry of the table"):
        surface_host(values, status, None, phi[:5], valid[:5], None, shift, basis=basis)


def test_the_library_checks_speak_the_same_words():
    """okx_ensemble_basis_check / okx_ensemble_surface_check / okx_ensemble_surface_scratch_bytes are host-only: they run without a GPU."""
    from open_kinematics_amd import _lib

    lib = _lib.load()
    basis = surface_terms(hermite_plan(3))
    law = np.ascontiguousarray(basis.law)

    def basis_check(law, terms, p=None):
        law, terms = np.ascontiguousarray(law, dtype=np.float64), np.ascontiguousarray(terms, dtype=np.int32)
        return lib.okx_ensemble_basis_check(law.ctypes.data_as(C.c_void_p), law.shape[0] if p is None else p, terms.ctypes.data_as(C.c_void_p), terms.shape[0])

    assert basis_check(law, basis.terms) == 0
    for law_, terms_ in ((law, basis.terms[1:]), (law, [[-1, 0, -1, 0], [0, 1, -1, 0], [3, 1, -1, 0]]), (law, [[-1, 0, -1, 0], [0, 4, -1, 0]]),
                         ([[0, 0, 1], [3, 0, 1]], [[-1, 0, -1, 0]]), ([[0, np.nan, 1]], [[-1, 0, -1, 0]]), (law, np.tile([[-1, 0, -1, 0]], (1025, 1)))):
        with pytest.raises(ValueError) as err:
            check_surface_basis(law_, terms_)
        assert basis_check(law_, terms_) != 0
        assert _lib.last_error() == str(err.value)

    def entry_check(entries, n_table, n_terms=10):
        e = None if entries is None else np.ascontiguousarray(entries, dtype=np.int32)
        return lib.okx_ensemble_surface_check(None if e is None else e.ctypes.data_as(C.c_void_p), n_table if e is None else e.size, n_table, n_terms)

    assert entry_check([3, 1, 2], 6) == 0 and entry_check(None, 6) == 0
    for entries, n_table, n_terms in (([4, 4], 6, 10), ([1, 6], 6, 10), (None, 2049, 10), ([], 6, 10), ([0, 5, 2, 5, 2], 6, 10), (None, 6, 1025), (None, 6, 0)):
        with pytest.raises(ValueError) as err:
            check_surface_arguments(entries, n_table, n_terms)
        assert entry_check(entries, n_table, n_terms) != 0
        assert _lib.last_error() == str(err.value)
    # the scratch size follows the plan of okx_surface.hip: used bytes, one count per workgroup of the used pass, sums of squares per (entry
    # tile, slab), one 64 x 64 tile per (item, slab); T = 130, N = 65 are 3 term tiles (6 pairs) and 2 entry tiles (6 rectangles): 12 items
    size = lambda g, t, n: lib.okx_ensemble_surface_scratch_bytes(g, 13, 5, t, n)  # noqa: E731
    assert size(300, 130, 65) == 304 + 8 * 75 + 8 * 2 * 3 * 64 + 8 * 12 * 3 * 4096  # three slabs of 128, 75 workgroups of 4 geometries
    assert size(0, 130, 65) == 8 and size(300, 1025, 65) == 0 and size(300, 130, 2049) == 0
    assert size(4096, 496, 36) == size(4096, 496, 36)  # (a function of the sizes alone)


# ---- ShardedEnsemble(reduce=True, factors=..., surface=...) on the stand-in program (host path): one process and two gloo ranks ----

SUBSET = [7, 0, 5, 2, 4]  # (two steps of the six: the stand-in rejects a quarter of the states, complete cases multiply that)
OPTIONS = dict(factors=[0, 4, 8], entries=SUBSET)  # T = 1 + 6 + 3 = 10 terms of three of the nine latents
G_REAL, G_INT = 65, 64  # 65: two ranks hold 33 and 32 geometries; 64 in three chunks: ragged chunks on every rank


def sign_factors(g):
    """[G, 3] of +1 / -1, every column balanced (G even): mean 0 and standard deviation 1 EXACTLY, so the table's law is (0, 0, 1), the basis
    values are +1 / -1 and every product with an integer d is exact."""
    i = np.arange(g)
    return np.column_stack([np.where(i % 2 == 0, 1.0, -1.0), np.where((i // 2) % 2 == 0, 1.0, -1.0), np.where((i // 4) % 2 == 0, 1.0, -1.0)])


def _sharded(which, chunks):
    """(pipe, reference inputs) of one of the two sharded cases, built the same way in every process."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs
    from test_ensemble_sample import STEPS, stand_in_plan
    from test_ensemble_sobol import integer_stand_in
    from test_ensemble_stats import COLUMNS, _stand_in

    kw = dict(chunks=chunks, metric_columns=COLUMNS, reduce=True)
    if which == "real":
        plan, relative = stand_in_plan(G_REAL)
        return ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", surface=OPTIONS, **kw), plan
    table, relative = _ensemble_inputs(G_INT, STEPS)
    return ShardedEnsemble(integer_stand_in(), table, relative, STEPS, factors=sign_factors(G_INT), surface=dict(entries=SUBSET), **kw), None


def _reference(pipe, plan):
    """surface_host over the whole table of a ONE-process run of the same ensemble."""
    from test_ensemble_sample import STEPS
    from test_ensemble_stats import COLUMNS

    g = G_REAL if plan is not None else G_INT
    values = pipe.metric_local.numpy().reshape(g, STEPS, len(COLUMNS))
    status = pipe.info_local[:, 32].numpy().reshape(g, STEPS)
    if plan is not None:
        _, latents, _, flags = sm.sample_host(plan)
        basis = surface_terms(plan, factors=OPTIONS["factors"])
    else:
        latents, flags = sign_factors(g), None
        basis = surface_terms(latents)
        assert basis.law.tolist() == [[0.0, 0.0, 1.0]] * 3
    phi, valid = basis_host(latents, basis)
    shift = pipe.local_accumulator.shift.numpy()
    want = surface_host(values, status, flags, phi, valid, SUBSET, shift, basis=basis)
    d = np.where(want.used[:, None] != 0, values.reshape(g, -1)[:, SUBSET] - shift.reshape(-1)[SUBSET], 0.0)
    return want, surface_bounds(np.where(want.used[:, None] != 0, phi, 0.0), d)


def _surface_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for which, chunks in (("real", 2), ("integer", 3)):
        pipe, _ = _sharded(which, chunks)
        pipe.step()
        first = pipe.surface_accumulator.numpy()
        pipe.step()  # a second step starts from nothing
        again = pipe.surface_accumulator.numpy()
        out[which] = {"gram": first.gram.copy(), "cross": first.cross.copy(), "sumsq": first.sumsq.copy(), "counts": first.counts.copy(),
                      "again": (again.gram.copy(), again.cross.copy(), again.sumsq.copy(), again.counts.copy()), "range": pipe.geometry_range,
                      "used": pipe.stages["surface"].local.used.clone(), "sent": pipe.surface_exchange_bytes_per_rank,
                      "coefficients": pipe.surface().coefficients if which == "real" else None}
    torch.save(out, os.path.join(out_dir, f"surface{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("chunks", [1, 3])
def test_sharded_ensemble_surface_in_one_process(chunks):
    for which in ("real", "integer"):
        pipe, plan = _sharded(which, chunks)
        pipe.step()
        got = pipe.surface_accumulator.numpy()
        want, bound = _reference(pipe, plan)
        assert np.array_equal(got.counts, want.counts) and np.array_equal(pipe.stages["surface"].local.used.numpy(), want.used)
        assert 12 < want.counts[0] < (G_REAL if plan is not None else G_INT)  # the stand-in's status bytes drop some geometries and keep most
        assert within(got, want, bound) and pipe.surface_exchange_bytes_per_rank == 0
        if chunks == 1 or which == "integer":
            for name in ("gram", "cross", "sumsq"):
                assert np.array_equal(getattr(got, name), getattr(want, name)), name  # the same additions in the same order / integers
        if which == "real":
            fit, ref = pipe.surface(), want.finalize()
            assert fit.count == ref.count and fit.basis.factor_names == tuple(plan.factor_names()) and fit.first.shape == (9, len(SUBSET))
            assert np.all(np.abs(fit.coefficients - ref.coefficients) <= 1e-9 * np.abs(ref.coefficients).max(axis=0))
        first = got.gram.copy()
        pipe.step()  # a second step starts from nothing
        assert np.array_equal(pipe.surface_accumulator.numpy().gram, first)


def test_sharded_surface_gives_every_rank_the_same_bits(tmp_path):
    from open_kinematics_amd.dist import shard_range

    world = 2
    port = 35600 + (os.getpid() + 17 * world) % 2000
    mp.spawn(_surface_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"surface{r}.pt"), weights_only=False) for r in range(world)]
    for which, chunks in (("real", 2), ("integer", 3)):
        alone, plan = _sharded(which, 1)
        alone.step()
        want, bound = _reference(alone, plan)
        one, two = got[0][which], got[1][which]
        for key in ("gram", "cross", "sumsq", "counts"):
            assert np.array_equal(one[key], two[key]), (which, key)
        t, n = want.gram.shape[0], len(SUBSET)
        for r, rank in enumerate((one, two)):
            acc = SurfaceAccumulator(rank["gram"], rank["cross"], rank["sumsq"], rank["counts"], want.shift, want.entries, basis=want.basis)
            assert np.array_equal(acc.counts, want.counts) and within(acc, want, bound)
            if which == "integer":
                assert np.array_equal(acc.gram, want.gram) and np.array_equal(acc.cross, want.cross) and np.array_equal(acc.sumsq, want.sumsq)
            for a, b in zip(rank["again"], (rank["gram"], rank["cross"], rank["sumsq"], rank["counts"])):
                assert np.array_equal(a, b)
            lo, hi = rank["range"]
            assert (lo, hi) == shard_range(G_REAL if which == "real" else G_INT, r, world) and np.array_equal(rank["used"].numpy(), want.used[lo:hi])
            assert rank["sent"] == 8 * (t * t + t * n + n + 2)
        assert one["range"][1] - one["range"][0] != two["range"][1] - two["range"][0] or which == "integer"  # 65 geometries: 33 and 32
        ref = want.finalize().coefficients if which == "real" else None
        if ref is not None:
            assert np.array_equal(one["coefficients"], two["coefficients"])
            assert np.all(np.abs(one["coefficients"] - ref) <= 1e-9 * np.abs(ref).max(axis=0))


def test_sharded_surface_refusals():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs
    from test_ensemble_sample import STEPS, stand_in_plan
    from test_ensemble_stats import COLUMNS, _stand_in

    plan, relative = stand_in_plan(8)
    kw = dict(metric_columns=COLUMNS, reduce=True)
    with pytest.raises(ValueError, match="surface= regresses the reduced ensemble on its factors: it needs reduce=True, factors and no FamilyPlan"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, surface=True, **kw)
    family = sm.FamilyPlan(plan, sm.group_by_point(plan)[0], 2)
    with pytest.raises(ValueError, match="no FamilyPlan \\(the pick-freeze rows are not an independent sample\\)"):
        ShardedEnsemble(_stand_in(), family, relative, STEPS, factors="sampled", surface=True, **kw)
    with pytest.raises(ValueError, match=r"surface= takes True or dict\(degree=, interactions=, entries=, factors=\)"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", surface={"bins": 3}, **kw)
    with pytest.raises(ValueError, match=r"surface\(\) needs surface=True"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", **kw).surface()
    with pytest.raises(RuntimeError, match="no step"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", surface=True, **kw).surface()
    with pytest.raises(ValueError, match="the response surface is refused: .* geometries used, a fit of 55 terms needs at least T \\+ 2 = 57"):
        pipe = ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", surface=True, **kw)
        pipe.step()
        pipe.surface()
    # more than 2048 entries ask for entries=
    table, rel = _ensemble_inputs(2, 600)
    with pytest.raises(ValueError, match="surface=: the table has 2400 entries, more than 2048: choose some with entries="):
        ShardedEnsemble(_stand_in(), table, rel, 600, factors=np.ones((2, 1)), surface=True, **kw)
