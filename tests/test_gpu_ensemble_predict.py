"""
GPU: okx_ensemble_predict (DeviceProgram.upload_surface / predict_ensemble), DeviceProgram.validate_surface and
ensemble_virtual.virtual_ensemble against NumPy (ensemble_stats.predict_host / surface_validate_host).

The BASIS BITS through the product: with the identity for coefficients the pass must hand out basis_host's values.
EXACT tables: integer factors in [-2, 2] under the monomial law (0, 1) give integer basis values |phi| <= 8; integer |c| <= 1023 with a
pattern of its own per (term, entry), an integer shift and integer table values keep every partial sum below 130 * 8 * 1023 + 2^11 < 2^21,
so every addition order gives the same bits and the device must equal NumPy's int64 result.  A swapped row and column, a result row of the
matrix instruction written to the wrong place or a panel read twice shows as a different integer.
ROW PURITY by torch.equal.  FLOAT tables within the bound derived in tests/test_ensemble_predict.py (u = 2^-53; nothing from an outcome).

The plan the shapes are chosen from (okx_predict.hip): tiles of 64 geometries x 64 entries, panels of 32 terms, factor rows in LDS up to
40 factors and read from memory beyond.
"""

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd.ensemble_stats import (EnsembleSurface, basis_host, predict_host, surface_host, surface_loo_host, surface_terms,
                                                surface_validate_host)
from test_ensemble_predict import fitted, loo_case, predict_bounds, validation_bounds
from test_ensemble_surface import hermite_plan
from test_gpu_ensemble_covariance import integer_case, upload
from test_gpu_ensemble_surface import P, chain_pipe, cut_basis, integer_factors, mixed_law, real_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def dp():
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.workloads import bump_sweep_problem

    program, _ = bump_sweep_problem(4)
    return DeviceProgram(program, DEV)


def surface_of(basis, coefficients, shift=None, entries=None, whitener=None):
    """An EnsembleSurface that carries what upload_surface reads."""
    c = np.ascontiguousarray(coefficients, dtype=np.float64)
    n = c.shape[1]
    return EnsembleSurface(np.arange(n) if entries is None else np.asarray(entries), 0, 0, basis, np.zeros(n) if shift is None else np.asarray(shift, dtype=np.float64),
                           c, None, None, whitener=whitener)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


@pytest.mark.parametrize("t", [1, 2, 31, 32, 33, 64, 65, 130, 323])
def test_the_basis_bits_through_the_product(dp, t):
    """Identity coefficients, N = T, no shift: out == basis_host(x) by value - all three kinds, degrees 1 to 3 and products under mixed_law; T
    under, at and over a panel of 32 and a tile of 64; NaN / inf factors (the row is NaN, valid 0)."""
    basis = cut_basis(t, mixed_law(t))
    model = dp.upload_surface(surface_of(basis, np.eye(t)))
    rng = np.random.default_rng(100 + t)
    for g in (1, 5, 300):
        x = rng.normal(size=(g, P)) * 1.5
        if g >= 5:
            x[1, 3], x[g - 1, P - 1] = np.nan, np.inf
            x[2, 0] = -np.inf
        phi, valid = basis_host(x, basis)
        out, ok = dp.predict_ensemble(model, dev(x))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(ok.cpu().numpy(), valid) and valid.sum() == (g if g < 5 else g - 3)
        assert np.all(np.isnan(got[valid == 0])) and np.array_equal(got[valid != 0], phi[valid != 0])


def test_the_basis_bits_with_factor_rows_read_from_memory(dp):
    """41 factors: one more than the rows staged in LDS.  Degree 1 (42 terms) by value, then degree 2 (903 terms) within the bound."""
    p = 41
    rng = np.random.default_rng(41)
    x = rng.normal(size=(130, p))
    x[7, 40], x[129, 0] = np.nan, np.inf
    basis = surface_terms(hermite_plan(p), degree=1)
    out, ok = dp.predict_ensemble(dp.upload_surface(surface_of(basis, np.eye(42))), dev(x))
    torch.cuda.synchronize()
    phi, valid = basis_host(x, basis)
    got = out.cpu().numpy()
    assert np.array_equal(ok.cpu().numpy(), valid) and np.all(np.isnan(got[valid == 0])) and np.array_equal(got[valid != 0], phi[valid != 0])
    basis = surface_terms(hermite_plan(p), degree=2)
    assert basis.n_terms == 903
    c, shift = rng.normal(size=(903, 70)), rng.normal(size=70)
    out, ok = dp.predict_ensemble(dp.upload_surface(surface_of(basis, c, shift)), dev(x))
    torch.cuda.synchronize()
    want, valid = predict_host(x, basis, c, shift)
    keep = valid != 0
    bound = predict_bounds(basis_host(x, basis)[0], c, shift)
    gap = np.abs(out.cpu().numpy() - want)[keep] / (2 * bound[keep])
    print(f"41 factors, T = 903: gap / bound {float(gap.max()):.3f}")
    assert np.array_equal(ok.cpu().numpy(), valid) and np.all(gap <= 1.0) and torch.isnan(out[~torch.as_tensor(keep, device=DEV)]).all()


def integer_coefficients(t, n):
    a = np.arange(t, dtype=np.int64)[:, None]
    e = np.arange(n, dtype=np.int64)[None, :]
    return (a * (2 * e + 3) + 7 * e * e + 13 * e + (a * a) % (e + 5)) % 2047 - 1023


SHAPES = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 129: (43, 3)}  # N = S K
COUNTS = (1, 31, 33, 63, 64, 65, 127, 129, 300)  # tiles of 64 geometries: under, at and over one and two; 300 is five, the last of 44


@pytest.mark.parametrize("t", [1, 5, 64, 65, 130])
def test_exact_integer_tables(dp, t):
    """(T, N, G) over {1, 5, 64, 65, 130} x {1, 63, 64, 65, 129} x COUNTS in both modes; NaN factors, NaN values, rejected states and (every
    second case) a mask."""
    basis = cut_basis(t)
    for n, (s, k) in SHAPES.items():
        c = integer_coefficients(t, n)
        shift = ((np.arange(n) * 29) % 151 - 75).astype(np.float64)
        model = dp.upload_surface(surface_of(basis, c, shift))
        for g in COUNTS:
            values, status, _ = integer_case(g, s, k, 100 * n + g)
            x = integer_factors(g, g + t)
            phi, valid = basis_host(x, basis)
            mask = None
            if (g + n) % 2:
                mask = ((np.arange(g) * 7 + n) % 11 == 0).astype(np.uint8) * 5 + ((np.arange(g) % 4 == 1) * 2).astype(np.uint8)  # bits 0 and 2; bit 1 alone
                valid = valid & ((mask & 1) == 0)
            keep = valid != 0
            fi = np.where(keep[:, None], phi, 0.0).astype(np.int64)
            assert np.array_equal(fi, np.where(keep[:, None], phi, 0.0)) and np.abs(fi).max(initial=0) <= 8
            want = fi @ c + shift.astype(np.int64)[None, :]
            assert np.abs(want).max() < 2 ** 21
            m = None if mask is None else dev(mask)
            out, ok = dp.predict_ensemble(model, dev(x), mask=m)
            v, st = upload(values, status)
            res, ok2 = dp.predict_ensemble(model, dev(x), mask=m, values=v, status=st, steps_per_geometry=s)
            torch.cuda.synchronize()
            got, rgot = out.cpu().numpy(), res.cpu().numpy()
            assert np.array_equal(ok.cpu().numpy(), valid) and np.array_equal(ok2.cpu().numpy(), valid)
            assert np.all(np.isnan(got[~keep])) and np.all(np.isnan(rgot[~keep]))
            bad = np.argwhere(got[keep] != want[keep])
            assert bad.size == 0, ("value", t, n, g, bad[:8].tolist())
            table = values.reshape(g, n)
            counts = np.isfinite(table) & np.repeat((status & 7) == 1, k, axis=1) & keep[:, None]
            assert np.array_equal(np.isnan(rgot), ~counts), ("residual: which entries count", t, n, g)
            bad = np.argwhere(rgot[counts] != (table[counts] - want[counts]))
            assert bad.size == 0, ("residual", t, n, g, bad[:8].tolist())
            if g >= 127:
                assert 0 < (~keep).sum() < g // 2 and 0 < (~counts[keep]).sum()  # the inputs are worth the test


def test_row_purity(dp):
    """The row of a geometry is a function of its factors and the model alone: chunks, the rows reversed, N = 17 against the first 17
    columns of N = 129, two identical calls - torch.equal (NaN rows compared by their valid byte)."""
    g, p = 300, 10
    _, _, mask, x, basis, _ = real_case(g, 3, 4, p, 31)
    rng = np.random.default_rng(2)
    t = basis.n_terms
    c, shift = rng.normal(size=(t, 129)), rng.normal(size=129)
    model = dp.upload_surface(surface_of(basis, c, shift))
    xs, m = dev(x), dev(mask)
    whole, ok = dp.predict_ensemble(model, xs, mask=m)
    again, ok_again = dp.predict_ensemble(model, xs, mask=m)
    torch.cuda.synchronize()
    keep = ok != 0
    assert 0 < int((~keep).sum()) < 40 and torch.isnan(whole[~keep]).all() and torch.isfinite(whole[keep]).all()
    bits = lambda a: torch.nan_to_num(a, nan=-7.0)  # noqa: E731  (NaN rows: one value, so that equal compares the rest by its bits)
    assert torch.equal(bits(whole), bits(again)) and torch.equal(ok, ok_again)
    for edges in ([0, 1, 2, 130, 130, 300], [0, 64, 128, 192, 256, 300]):
        parts = [dp.predict_ensemble(model, xs[a:b], mask=m[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        torch.cuda.synchronize()
        assert torch.equal(bits(torch.cat([q[0] for q in parts])), bits(whole)), edges
        assert torch.equal(torch.cat([q[1] for q in parts]), ok)
    back, ok_back = dp.predict_ensemble(model, xs.flip(0).contiguous(), mask=m.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(bits(back.flip(0)), bits(whole)) and torch.equal(ok_back.flip(0), ok)
    few = dp.upload_surface(surface_of(basis, c[:, :17], shift[:17]))
    narrow, _ = dp.predict_ensemble(few, xs, mask=m)
    torch.cuda.synchronize()
    assert torch.equal(bits(narrow), bits(whole[:, :17]))
    # another leading dimension of the factors and of the output changes nothing either
    wide = torch.full((g, 3 * p), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, p:2 * p] = xs
    room = torch.zeros((g, 140), dtype=torch.float64, device=DEV)
    dp.predict_ensemble(model, wide[:, p:2 * p], mask=m, out=room[:, 5:134], valid=torch.empty(g, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(room[:, 5:134]), bits(whole))


def test_views(dp):
    """Factors as a strided view in the middle of a NaN-filled tensor, out with ld_out = N + 9 and sentinels around it, coefficients with
    ld_c > N; RESIDUAL mode over a strided values view with a strided status byte (72 / 40), scattered permuted entries, rejected states,
    NaN values and a mask.  Integer tables: exact."""
    s, k, t, n = 11, 24, 65, 17
    basis = cut_basis(t)
    rng = np.random.default_rng(n)
    entries = rng.permutation(s * k)[:n].astype(np.int64)
    c = integer_coefficients(t, n)
    shift = ((np.arange(n) * 29) % 151 - 75).astype(np.float64)
    for g in (33, 300):
        values, status, _ = integer_case(g, s, k, 7 * n + g)
        x = integer_factors(g, n + g)
        mask = ((np.arange(g) * 5 + n) % 9 == 0).astype(np.uint8)
        pad = 40
        big = torch.full((pad + g * s + pad, 3, 24), float("nan"), dtype=torch.float64, device=DEV)
        info = torch.full((pad + g * s + pad, 40), 2, dtype=torch.uint8, device=DEV)
        big[pad : pad + g * s, 0, :] = dev(values.reshape(g * s, k))
        info[pad : pad + g * s, 32] = dev(status.reshape(-1))
        view, st = big[pad : pad + g * s, 0, :], info[pad : pad + g * s, 32]
        assert view.stride(0) == 72 and st.stride(0) == 40
        wide = torch.full((g + 4, 2 * P + 3), float("nan"), dtype=torch.float64, device=DEV)
        wide[2 : 2 + g, 2 : 2 + P] = dev(x)
        model = dp.upload_surface(surface_of(basis, c, shift, entries))
        cw = torch.full((t, n + 6), float("nan"), dtype=torch.float64, device=DEV)
        cw[:, :n] = model.coefficients
        model.coefficients = cw[:, :n]
        assert model.coefficients.stride(0) == n + 6
        phi, valid = basis_host(x, basis)
        valid = valid & ((mask & 1) == 0)
        keep = valid != 0
        want = np.where(keep[:, None], phi, 0.0).astype(np.int64) @ c + shift.astype(np.int64)[None, :]
        table = values.reshape(g, s * k)[:, entries]
        counts = np.isfinite(table) & ((status & 7) == 1)[:, entries // k] & keep[:, None]
        for mode in ("value", "residual"):
            room = torch.full((g, n + 9), -7.0, dtype=torch.float64, device=DEV)
            ok = torch.full((g,), 9, dtype=torch.uint8, device=DEV)
            extra = dict(values=view, status=st, steps_per_geometry=s) if mode == "residual" else {}
            out, back = dp.predict_ensemble(model, wide[2 : 2 + g, 2 : 2 + P], mask=dev(mask), out=room[:, 4 : 4 + n], valid=ok, **extra)
            torch.cuda.synchronize()
            assert back is ok and np.array_equal(ok.cpu().numpy(), valid)
            assert torch.all(room[:, :4] == -7.0) and torch.all(room[:, 4 + n :] == -7.0)
            got = out.cpu().numpy()
            if mode == "value":
                assert np.all(np.isnan(got[~keep])) and np.array_equal(got[keep], want[keep])
            else:
                assert np.array_equal(np.isnan(got), ~counts) and np.array_equal(got[counts], table[counts] - want[counts])
                assert 0 < (~counts[keep]).sum()
                host, hv = predict_host(x, basis, c, shift, mask, values, status, entries)  # the definition gives the same integers
                assert np.array_equal(hv, valid) and np.array_equal(np.isnan(host), ~counts) and np.array_equal(host[counts], got[counts])


@pytest.mark.parametrize("shape", [(300, 9, 15, 10, None), (700, 5, 13, 12, [64, 3, 47, 62, 0, 33, 12])])
def test_real_tables_within_the_bound(dp, shape):
    g, s, k, p, entries = shape
    values, status, mask, x, basis, shift = real_case(g, s, k, p, 11 + g)
    phi, valid = basis_host(x, basis)
    fit = surface_host(values, status, mask, phi, valid, entries, shift, basis=basis).finalize()
    model = dp.upload_surface(fit)
    v, st = upload(values, status)
    out, ok = dp.predict_ensemble(model, dev(x), mask=dev(mask))
    res, _ = dp.predict_ensemble(model, dev(x), mask=dev(mask), values=v, status=st, steps_per_geometry=s)
    torch.cuda.synchronize()
    table = values.reshape(g, s * k)[:, fit.entries]
    for what, got, want, bound in (("value", out, predict_host(x, basis, fit.coefficients, fit.shift, mask), predict_bounds(phi, fit.coefficients, fit.shift)),
                                   ("residual", res, predict_host(x, basis, fit.coefficients, fit.shift, mask, values, status, fit.entries),
                                    predict_bounds(phi, fit.coefficients, fit.shift, table))):
        got, (want, want_valid) = got.cpu().numpy(), want
        assert np.array_equal(ok.cpu().numpy(), want_valid) and np.array_equal(np.isnan(got), np.isnan(want))
        defined = ~np.isnan(want)
        gap = np.abs(got - want)[defined] / (2 * bound[defined])
        print(f"{what}: G = {g}, T = {basis.n_terms}, N = {table.shape[1]}, {int(defined.sum())} defined: gap / bound {float(gap.max()):.3f}")
        assert g * table.shape[1] // 2 < defined.sum() < defined.size and np.all(gap <= 1.0)


def test_a_captured_graph(dp):
    """sample_ensemble(out=) -> predict_ensemble(out=) -> reduce_ensemble(out=) captured and replayed with new contents of the model.  That
    the capture is a single chain without parallel branches is NOT asserted here: it follows from the code - every launch of the three
    entry points goes to the one stream they are given, and nothing forks a second one."""
    p, g, n = 9, 300, 36
    plan = hermite_plan(p)
    basis = surface_terms(plan, degree=2)
    rng = np.random.default_rng(4)
    c, shift = rng.normal(size=(basis.n_terms, n)), rng.normal(size=n)
    model = dp.upload_surface(surface_of(basis, c, shift))
    sample = dp.sample_ensemble(plan, 50, 50 + g, latents=True)
    table, valid = dp.predict_ensemble(model, sample.latents, mask=sample.flags)
    acc = dp.reduce_ensemble(table, steps_per_geometry=1, shift=shift.reshape(1, n), geometry_offset=50)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.sample_ensemble(plan, 50, 50 + g, latents=True, out=sample)
        dp.predict_ensemble(model, sample.latents, mask=sample.flags, out=table, valid=valid)
        dp.reduce_ensemble(table, steps_per_geometry=1, geometry_offset=50, out=acc)
    for seed in (5, 4):
        c2 = np.random.default_rng(seed).normal(size=c.shape)
        model.coefficients.copy_(dev(c2))
        for tensor in (sample.latents, table, acc.acc):
            tensor.fill_(3.0)
        valid.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        latents = sample.latents.clone()
        want, want_valid = dp.predict_ensemble(model, latents, mask=sample.flags)
        want_acc = dp.reduce_ensemble(want, steps_per_geometry=1, shift=shift.reshape(1, n), geometry_offset=50)
        torch.cuda.synchronize()
        assert torch.equal(table, want) and torch.equal(valid, want_valid) and bool(valid.all()) and torch.equal(acc.acc, want_acc.acc)
        host, _ = predict_host(latents.cpu().numpy(), basis, c2, shift)
        assert np.all(np.abs(table.cpu().numpy() - host) <= 2 * predict_bounds(basis_host(latents.cpu().numpy(), basis)[0], c2, shift))


def test_validate_surface_is_the_host_validation(dp):
    values, x, basis, shift = loo_case()
    g, s, k = values.shape
    fit = fitted(values, x, basis, shift)
    want = surface_validate_host(fit, x, values)
    assert want.max_leverage <= 0.5, want.max_leverage  # the CONDITION of the bound: 1 / (1 - h) <= 2
    model = dp.upload_surface(fit)
    v, _ = upload(values, None)
    got = dp.validate_surface(model, fit, dev(x), v, steps_per_geometry=s, chunk=150)
    e, h, used = surface_loo_host(fit, x, values)
    bound = validation_bounds(basis_host(x, basis)[0], fit, values.reshape(g, s * k), e, h, used)
    assert got.count == want.count == g
    for name in ("loo_rms", "loo_max", "q2"):
        gap = np.abs(getattr(got, name) - getattr(want, name)) / bound[name]
        print(f"validate_surface {name}: gap / bound {float(gap.max()):.3f}")
        assert np.all(gap <= 1.0), name
    assert abs(got.max_leverage - want.max_leverage) <= bound["leverage"] and abs(got.mean_leverage - want.mean_leverage) <= bound["leverage"]
    loo = np.abs(e / (1.0 - h)[:, None])
    top = np.sort(loo, axis=0)
    clear = top[-1] - top[-2] > 2 * bound["loo_max"]  # where the largest is ahead of the second by more than both may move
    assert clear.any() and np.array_equal(got.loo_max_geometry[clear], want.loo_max_geometry[clear])
    # rows the fit dropped: found again from the residuals, or given
    values[3, 1, 2], x[31, 4] = np.nan, np.nan
    status = np.ones((g, s), dtype=np.uint8)
    status[8, 0] = 4
    mask = np.zeros(g, dtype=np.uint8)
    mask[20] = 1
    phi, valid = basis_host(x, basis)
    acc = surface_host(values, status, mask, phi, valid, None, shift, basis=basis)
    fit = acc.finalize()
    want = surface_validate_host(fit, x, values, status, mask)
    model = dp.upload_surface(fit)
    v, st = upload(values, status)
    for used in (None, dev(acc.used)):
        got = dp.validate_surface(model, fit, dev(x), v, steps_per_geometry=s, status=st, mask=dev(mask), used=used)
        assert got.count == want.count == g - 4 and np.allclose(got.loo_rms, want.loo_rms, rtol=1e-9, atol=0.0)  # (the bound is asserted above)


QUANTILE_FIELDS = ("probs", "count", "lower", "upper", "quantile", "below", "above", "yield_")


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_virtual_ensemble(dp):
    """The chain fixture's plan (256 x 9, 3 points: 55 terms, 36 entries): fit on the solved geometries, then 5 000 virtual ones.  Every
    integer result is bit-equal for chunk 5000, 1024 and 777; the floating sums follow reduce_ensemble's chunk rule; the whole table held at
    once gives the same quantiles and verdicts through select_ensemble / screen_ensemble directly."""
    from open_kinematics_amd.ensemble_virtual import virtual_ensemble

    cdp, plan, pipe = chain_pipe(1)
    pipe.step()
    torch.cuda.synchronize()
    fit = pipe.surface()
    assert fit.coefficients.shape == (55, 36) and fit.whitener.shape == (55, 55)
    model = cdp.upload_surface(fit)
    big = dataclasses.replace(plan, n_total=5000, seed=11)
    centre, spread = fit.shift + fit.coefficients[0], np.sqrt(fit.variance) + 1e-9  # (an orthonormal basis: the constant's coefficient is the model's mean)
    limits = np.stack([centre - 2.0 * spread, centre + 3.0 * spread], axis=1)
    limits[5], limits[7, 0] = (-np.inf, np.inf), -np.inf
    probs = [0.001, 0.5, 0.9999]
    runs = {chunk: virtual_ensemble(cdp, model, big, chunk=chunk, probs=probs, limits=limits, scale=spread, screen=True) for chunk in (5000, 1024, 777)}
    one = runs[5000]
    assert one.drawn == 5000 and one.invalid >= one.dropped >= 0 and one.screen.tally[0] == 5000
    assert 0.05 < one.screen.joint_yield < 0.999 and one.screen.blame.sum() > 0  # the limits bite
    for chunk in (1024, 777):
        run = runs[chunk]
        assert (run.drawn, run.dropped, run.invalid) == (one.drawn, one.dropped, one.invalid)
        for name in ("count", "rejected", "argmin", "argmax", "min", "max"):
            assert same(getattr(run.stats, name), getattr(one.stats, name)), (chunk, name)
        for name in QUANTILE_FIELDS:
            assert same(getattr(run.quantiles, name), getattr(one.quantiles, name)), (chunk, name)
        for name in ("flags", "margin", "entry", "tally", "blame", "passed"):
            assert same(getattr(run.screen, name), getattr(one.screen, name)), (chunk, name)
        # reduce_ensemble's chunk rule: the sums of d = value - shift and of d d over G = 5000 geometries in another order, each within
        # (G + 1) u sum |term| of the exact sum; mean |d| <= |mean d| + std and mean d d = variance + (mean d)^2
        away = np.abs(one.stats.mean - fit.shift.reshape(1, -1))
        assert np.all(np.abs(run.stats.mean - one.stats.mean) <= 2 * 5002 * U * (away + one.stats.std))
        assert np.all(np.abs(run.stats.variance - one.stats.variance) <= 8 * 5002 * U * (one.stats.variance + away * away))
    # the whole table at once
    sample = cdp.sample_ensemble(big, 0, 5000, latents=True)
    table, valid = cdp.predict_ensemble(model, sample.latents, mask=sample.flags)
    direct = cdp.select_ensemble(table, steps_per_geometry=1, probs=probs, limits=limits).finalize()
    verdict = cdp.screen_ensemble(table, steps_per_geometry=1, limits=limits, scale=spread).finalize()
    torch.cuda.synchronize()
    assert int((valid == 0).sum()) == one.invalid and int((sample.flags & 1).sum()) == one.dropped
    for name in QUANTILE_FIELDS:
        assert same(getattr(direct, name), getattr(one.quantiles, name)), name
    for name in ("flags", "margin", "entry", "tally", "blame", "passed"):
        assert same(getattr(verdict, name), getattr(one.screen, name)), name
    want, _ = predict_host(sample.latents.cpu().numpy(), fit.basis, fit.coefficients, fit.shift, sample.flags.cpu().numpy())
    assert np.all(np.abs(table.cpu().numpy() - want)[valid.cpu().numpy() != 0]
                  <= 2 * predict_bounds(basis_host(sample.latents.cpu().numpy(), fit.basis)[0], fit.coefficients, fit.shift)[valid.cpu().numpy() != 0])
    tallies = virtual_ensemble(cdp, model, big, 1000, 3000, chunk=512, limits=limits, scale=spread, screen=True, verdicts=False)
    assert tallies.quantiles is None and tallies.screen.flags.size == 0 and tallies.drawn == 2000
    assert tallies.screen.tally[1] == int((one.screen.flags[1000:3000] == 0).sum())


def test_error_paths(dp):
    from open_kinematics_amd import _lib

    lib = dp.lib
    s, k, g, t = 3, 4, 64, 10
    n = s * k
    rng = np.random.default_rng(0)
    basis = cut_basis(t)
    model = dp.upload_surface(surface_of(basis, rng.normal(size=(t, n)), rng.normal(size=n)))
    xs = dev(rng.normal(size=(g, P)))
    v = dev(rng.normal(size=(g * s, k)))
    out, valid = dp.predict_ensemble(model, xs)
    torch.cuda.synchronize()
    kept, kept_valid = out.clone(), valid.clone()
    with pytest.raises(ValueError, match="one column per factor of the basis"):
        dp.predict_ensemble(model, xs[:, :5].contiguous())
    with pytest.raises(ValueError, match="factors must be a float64 \\[G, P\\] device tensor with unit column stride"):
        dp.predict_ensemble(model, xs.float())
    with pytest.raises(ValueError, match="mask must be a contiguous uint8"):
        dp.predict_ensemble(model, xs, mask=torch.zeros(g + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"out \[64, 12\] must be a float64 \[G, N\] device tensor"):
        dp.predict_ensemble(model, xs, out=torch.zeros((g + 1, n), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match=r"out must be \[64, 12\]"):
        dp.predict_ensemble(model, xs, out=torch.zeros((g, n + 1), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="valid must be a contiguous uint8"):
        dp.predict_ensemble(model, xs, valid=torch.zeros(g, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="steps_per_geometry is needed with values="):
        dp.predict_ensemble(model, xs, values=v)
    with pytest.raises(ValueError, match="values must hold 64 geometries"):
        dp.predict_ensemble(model, xs, values=v[: 5 * s], steps_per_geometry=s)
    with pytest.raises(ValueError, match=r"okx_ensemble_predict: entry 8 is 8, outside \[0, 8\)"):
        dp.predict_ensemble(model, xs, values=dev(rng.normal(size=(g * 4, 2))), steps_per_geometry=4)
    with pytest.raises(ValueError, match="okx_ensemble_predict: 12 entries of the table for 13 columns of the coefficients"):
        dp.predict_ensemble(model, xs, values=v, steps_per_geometry=s, coefficients=dev(rng.normal(size=(t, 13))))
    with pytest.raises(ValueError, match=r"coefficients \[10, N\] must be a float64 \[T, N\] device tensor"):
        dp.predict_ensemble(model, xs, coefficients=dev(rng.normal(size=(t + 1, 3))))
    with pytest.raises(ValueError, match="model must be the SurfaceModel of upload_surface"):
        dp.predict_ensemble(None, xs)
    with pytest.raises(ValueError, match="okx_ensemble_predict: 2049 entries, 1 to 2048 allowed"):
        dp.upload_surface(surface_of(basis, np.zeros((t, 2049))))
    with pytest.raises(ValueError, match=r"okx_ensemble_basis: term 0 must be the constant \(-1, 0, -1, 0\)"):
        dp.upload_surface(surface_of(dataclasses.replace(basis, terms=basis.terms[1:]), np.zeros((t - 1, 3))))
    bare = dp.upload_surface(surface_of(basis, rng.normal(size=(t, n))))
    with pytest.raises(ValueError, match="carries no whitener"):
        dp.validate_surface(bare, surface_of(basis, np.zeros((t, n))), xs, v, steps_per_geometry=s)
    # the host check, by the library
    e = np.array([4, 4], dtype=np.int32)
    assert lib.okx_ensemble_predict_check(e.ctypes.data_as(C.c_void_p), 2, 12, t, P) != 0 and "entry 1 repeats entry 0 (index 4)" in _lib.last_error()
    assert lib.okx_ensemble_predict_check(None, 4, 12, t, P) != 0 and "without an entry list all 12 entries are selected, not 4" in _lib.last_error()
    assert lib.okx_ensemble_predict_check(None, 4, 0, 1025, P) != 0 and "1025 terms, 1 to 1024 allowed" in _lib.last_error()
    assert lib.okx_ensemble_predict_check(None, 4, 0, t, 289) != 0 and "289 factors, 1 to 288 allowed" in _lib.last_error()
    assert lib.okx_ensemble_predict_check(None, 12, 12, t, P) == 0 and lib.okx_ensemble_predict_check(None, 2048, 0, 1024, 288) == 0
    # the entry point itself
    p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())  # noqa: E731

    def call(mode=0, n_terms=t, n_entries=n, ld=P, ld_out=n, ld_c=n, out=out, valid=valid, values=None, n_factors=P, factors=xs):
        return lib.okx_ensemble_predict(g, mode, p(factors), ld, n_factors, p(model.law), p(model.terms), n_terms, p(model.coefficients), ld_c, n_entries,
                                        p(model.shift), None, s, k, p(values), k, None, 0, None, p(out), ld_out, p(valid), None)

    for kwargs, words in ((dict(out=None), "null output table or null valid bytes"), (dict(valid=None), "null output table or null valid bytes"),
                          (dict(n_terms=0), "0 terms, 1 to 1024 allowed"), (dict(n_terms=1025), "1025 terms, 1 to 1024 allowed"),
                          (dict(n_entries=0), "0 entries, 1 to 2048 allowed"), (dict(n_entries=2049), "2049 entries, 1 to 2048 allowed"),
                          (dict(n_factors=0), "0 factors, 1 to 288 allowed"), (dict(ld=P - 1), "null factor table or ld < n_factors"),
                          (dict(factors=None), "null factor table or ld < n_factors"), (dict(ld_out=n - 1), "ld_out < n_entries"),
                          (dict(ld_c=n - 1), "null coefficient table or ld_c < n_entries"), (dict(mode=1), "OKX_PREDICT_RESIDUAL needs the table"),
                          (dict(mode=1, values=v, n_entries=5), "without an entry list all 12 entries are selected, not 5"),
                          (dict(mode=2), "mode 2, not OKX_PREDICT_VALUE (0) or OKX_PREDICT_RESIDUAL (1)")):
        assert call(**kwargs) != 0, kwargs
        assert words in _lib.last_error(), (kwargs, _lib.last_error())
    torch.cuda.synchronize()
    assert torch.equal(out, kept) and torch.equal(valid, kept_valid)  # nothing was touched by the refused calls
    assert call(mode=1, values=v) == 0  # natural order through a null entry list
    torch.cuda.synchronize()
    want, _ = dp.predict_ensemble(model, xs, values=v, steps_per_geometry=s)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
