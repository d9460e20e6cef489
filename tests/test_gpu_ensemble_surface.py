"""
GPU: okx_ensemble_basis (DeviceProgram.basis_factors), okx_ensemble_surface (DeviceProgram.surface_ensemble) and predict_surface against
NumPy (ensemble_stats.basis_host / surface_host / EnsembleSurface.predict).

The basis pass is compared BIT FOR BIT: both sides round every operation on its own.

EXACT tables for the surface pass: integer factors in [-2, 2] under the monomial law (0, 1) give integer basis values |phi| <= 8, integer
|d| = |value - shift| <= 1023 and G <= 300 make every product (< 2^13) and every partial sum (< 2^22) an integer that fp64 holds, so every
addition order gives the same bits and the device must equal NumPy's int64 tables (array_equal).  Every term and every entry carries its own
pattern over the geometries, so a swapped row and column, a result row of the matrix instruction written to the wrong place, a tile of
Phi^T D read as a tile of Phi^T Phi or a geometry counted twice shows as a different integer.

FLOAT tables against surface_host within the bounds derived in tests/test_ensemble_surface.py (u = 2^-53; nothing here comes from an
outcome): each of two results is within (G + 1) u sum |term| of the exact sum, so they are within twice that of each other.

The plan the shapes are chosen from (okx_surface.hip): 64-wide tiles of terms and of entries, panels of 32 geometries, slabs of at least
128 geometries, 256 terms per workgroup of the basis pass.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_stats import (SURFACE_HERMITE, SURFACE_LEGENDRE, SURFACE_MONOMIAL, SurfaceBasis, basis_host, surface_host,
                                                surface_terms)
from test_ensemble_covariance import shifted
from test_ensemble_surface import hermite_plan, surface_bounds
from test_gpu_ensemble_covariance import integer_case, upload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = 23  # degree 3 with interactions: 1 + 69 + 253 = 323 terms to cut the term counts from


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


def cut_basis(t, law=None, degree=3):
    """The first ``t`` terms of the degree-3 basis with interactions over P factors, in an order that mixes the kinds of terms: the constant,
    then the rest interleaved (a linear, a square, a cube, a product, ...), so that a short cut holds every kind."""
    full = surface_terms(np.zeros((2, P)), degree=degree)
    rest = full.terms[1:]
    groups = [rest[:P], rest[P:2 * P], rest[2 * P:3 * P], rest[3 * P:]]
    order = [groups[i % 4][i // 4] for i in range(4 * P)] + list(groups[3][P:])
    terms = np.array([full.terms[0]] + order, dtype=np.int32)[:t]
    if law is None:
        law = np.zeros((P, 3))
        law[:, 2] = 1.0
    return SurfaceBasis(np.ascontiguousarray(law, dtype=np.float64), np.ascontiguousarray(terms))


def mixed_law(seed):
    rng = np.random.default_rng(seed)
    law = np.zeros((P, 3))
    law[:, 0] = np.arange(P) % 3  # monomial, Hermite, Legendre in turn
    law[:, 1] = rng.normal(size=P) * 0.3
    law[:, 2] = rng.uniform(0.5, 2.0, size=P)
    assert set(law[:, 0]) == {SURFACE_MONOMIAL, SURFACE_HERMITE, SURFACE_LEGENDRE}
    return law


@pytest.mark.parametrize("t", [1, 2, 63, 64, 65, 130, 257, 323])
def test_the_basis_pass_is_basis_host_bit_for_bit(dp, t):
    """All three kinds, degrees 1 to 3 and products; T under, at and over a 64-term tile and the 256 terms of a workgroup; a table with
    ld_phi > T; the factors as a strided view; NaN / inf factors (the row is invalid and 0)."""
    basis = cut_basis(t, mixed_law(t))
    if t >= 63:
        assert {tuple(r[1::2]) for r in basis.terms.tolist()} >= {(0, 0), (1, 0), (2, 0), (3, 0), (1, 1)}
    rng = np.random.default_rng(100 + t)
    for g in (1, 5, 300):
        x = rng.normal(size=(g, P)) * 1.5
        if g >= 5:
            x[1, 3], x[g - 1, P - 1] = np.nan, np.inf
            x[2, 0] = -np.inf
        want_phi, want_valid = basis_host(x, basis)
        assert want_valid.sum() == (g if g < 5 else g - 3) and np.all(want_phi[want_valid == 0] == 0.0)
        table = dp.basis_factors(torch.as_tensor(x, device=DEV), basis)
        torch.cuda.synchronize()
        assert np.array_equal(table.valid.cpu().numpy(), want_valid)
        assert np.array_equal(table.phi.cpu().numpy().view(np.uint64), want_phi.view(np.uint64))
        # the same into a wider table (ld_phi = T + 7) from a strided view of the factors (ld = 2 P + 3): what lies around stays
        wide = torch.full((g, t + 7), -7.0, dtype=torch.float64, device=DEV)
        big = torch.full((g, 2 * P + 3), float("nan"), dtype=torch.float64, device=DEV)
        big[:, 2:2 + P] = torch.as_tensor(x, device=DEV)
        table.phi, table.valid = wide[:, 3:3 + t], torch.full((g,), 9, dtype=torch.uint8, device=DEV)
        again = dp.basis_factors(big[:, 2:2 + P], out=table)
        torch.cuda.synchronize()
        assert again is table and np.array_equal(table.valid.cpu().numpy(), want_valid)
        assert np.array_equal(wide[:, 3:3 + t].cpu().numpy().view(np.uint64), want_phi.view(np.uint64))
        assert torch.all(wide[:, :3] == -7.0) and torch.all(wide[:, 3 + t:] == -7.0)


def integer_factors(g, seed):
    """[G, P] integers in [-2, 2], a different pattern per factor; a few rows carry a NaN."""
    i = np.arange(g, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    x = ((i * (2 * p + 3) + p * p + (i * i) % (p + 3)) % 5 - 2).astype(np.float64)
    rng = np.random.default_rng(seed)
    for _ in range(g // 20):
        x[rng.integers(0, g), rng.integers(0, P)] = np.nan
    return x


def integer_tables(values, status, mask, phi, valid, entries, shift):
    """(gram, cross, sumsq, counts, used) in int64 arithmetic."""
    d, used = shifted(values, status, entries, shift)
    if mask is not None:
        used = used & ((mask & 1) == 0)
    used = used & (valid != 0)
    d = np.where(used[:, None], d, 0.0)
    f = np.where(used[:, None], phi, 0.0)
    di, fi = d.astype(np.int64), f.astype(np.int64)
    assert np.array_equal(di, d) and np.array_equal(fi, f) and np.abs(di).max(initial=0) <= 1024 and np.abs(fi).max(initial=0) <= 8
    return fi.T @ fi, fi.T @ di, (di * di).sum(axis=0), np.array([used.sum(), used.size - used.sum()]), used.astype(np.uint8)


def equal_exactly(acc, want):
    gram, cross, sumsq, counts, used = want
    got = acc.numpy()
    assert np.array_equal(got.counts, counts) and np.array_equal(got.used[: used.size], used)
    bad = np.argwhere(got.gram != gram)
    assert bad.size == 0, ("gram", bad[:8].tolist(), got.gram[tuple(bad[0])], gram[tuple(bad[0])])
    bad = np.argwhere(got.cross != cross)
    assert bad.size == 0, ("cross", bad[:8].tolist(), got.cross[tuple(bad[0])], cross[tuple(bad[0])])
    assert np.array_equal(got.sumsq, sumsq)
    assert np.array_equal(got.gram.view(np.uint64), got.gram.T.view(np.uint64))
    return counts


SHAPES = {1: (1, 1), 63: (9, 7), 65: (13, 5), 129: (43, 3)}  # N = S K
COUNTS = (1, 31, 33, 127, 129, 300)  # panels of 32 geometries, slabs of 128: 300 is three slabs, the last of 44


@pytest.mark.parametrize("t", [1, 5, 64, 65, 130])
def test_exact_integer_tables(dp, t):
    """(T, N) over {1, 5, 64, 65, 130} x {1, 63, 65, 129}: under, at and over one tile on either side, up to three by three tiles; G over the
    panel and slab boundaries.  Failed states, NaN values, NaN factors and (every second case) a mask drop geometries."""
    basis = cut_basis(t)
    for n, (s, k) in SHAPES.items():
        for g in COUNTS:
            values, status, shift = integer_case(g, s, k, 100 * n + g)
            x = integer_factors(g, g + t)
            phi, valid = basis_host(x, basis)
            mask = None
            if (g + n) % 2:
                mask = ((np.arange(g) * 7 + n) % 11 == 0).astype(np.uint8) * 5 + ((np.arange(g) % 4 == 1) * 2).astype(np.uint8)  # bits 0 and 2; bit 1 alone
            v, st = upload(values, status)
            table = dp.basis_factors(torch.as_tensor(x, device=DEV), basis)
            acc = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, shift=shift,
                                      mask=None if mask is None else torch.as_tensor(mask, device=DEV))
            torch.cuda.synchronize()
            assert acc.natural and tuple(acc.gram.shape) == (t, t) and tuple(acc.cross.shape) == (t, n)
            counts = equal_exactly(acc, integer_tables(values, status, mask, phi, valid, None, shift))
            if g >= 127:
                assert 0 < counts[1] < g * 2 // 3  # the inputs are worth the test
    # without status bytes every state is accepted
    acc = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, shift=shift)
    torch.cuda.synchronize()
    equal_exactly(acc, integer_tables(values, None, None, phi, valid, None, shift))


@pytest.mark.parametrize("n", [1, 17, 63, 65, 129])
def test_exact_scattered_entries_of_strided_views(dp, n):
    """A permuted scattered subset of N entries of a wider table that lies as a strided view (ld = 72 > K, status bytes 40 apart) in the
    MIDDLE of larger tensors filled with NaN and rejected bytes, with a mask, and phi as a view with ld_phi > T."""
    s, k, t = 11, 24, 65
    basis = cut_basis(t)
    rng = np.random.default_rng(n)
    entries = rng.permutation(s * k)[:n].astype(np.int64)
    for g in (33, 300):
        values, status, shift = integer_case(g, s, k, 7 * n + g)
        x = integer_factors(g, n + g)
        phi, valid = basis_host(x, basis)
        mask = ((np.arange(g) * 5 + n) % 9 == 0).astype(np.uint8)
        pad = 40
        big = torch.full((pad + g * s + pad, 3, 24), float("nan"), dtype=torch.float64, device=DEV)
        info = torch.full((pad + g * s + pad, 40), 2, dtype=torch.uint8, device=DEV)
        big[pad : pad + g * s, 0, :] = torch.as_tensor(values.reshape(g * s, k), device=DEV)
        info[pad : pad + g * s, 32] = torch.as_tensor(status.reshape(-1), device=DEV)
        view, st = big[pad : pad + g * s, 0, :], info[pad : pad + g * s, 32]
        assert view.stride(0) == 72 and st.stride(0) == 40
        table = dp.basis_factors(torch.as_tensor(x, device=DEV), basis)
        wide = torch.full((g, t + 9), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, 4:4 + t] = table.phi
        table.phi = wide[:, 4:4 + t]
        acc = dp.surface_ensemble(view, steps_per_geometry=s, basis_table=table, status=st, mask=torch.as_tensor(mask, device=DEV), entries=entries,
                                  shift=shift)
        torch.cuda.synchronize()
        assert not acc.natural and np.array_equal(acc.entries.cpu().numpy(), entries)
        want = integer_tables(values, status, mask, phi, valid, entries, shift)
        equal_exactly(acc, want)
        host = surface_host(values, status, mask, phi, valid, entries, shift, basis=basis)  # the definition gives the same integers
        assert np.array_equal(host.gram, want[0]) and np.array_equal(host.cross, want[1]) and np.array_equal(host.sumsq, want[2])
        assert np.array_equal(host.counts, want[3]) and np.array_equal(host.used, want[4])
        if g == 33:  # an entry that is not selected never drops a geometry: NaN everywhere else changes nothing
            spoiled = values.reshape(g, s * k).copy()
            spoiled[:, np.setdiff1d(np.arange(s * k), entries)] = np.nan
            big[pad : pad + g * s, 0, :] = torch.as_tensor(spoiled.reshape(g * s, k), device=DEV)
            again = dp.surface_ensemble(view, steps_per_geometry=s, basis_table=table, status=st, mask=torch.as_tensor(mask, device=DEV), out=acc)
            torch.cuda.synchronize()
            assert again is acc
            equal_exactly(acc, want)


def real_case(g, s, k, p, seed, degree=2):
    """(values, status, mask, x, basis, shift): normal latents under the Hermite basis of a plan, values around per-entry centres that depend on
    the latents, a few NaN, rejected states, masked geometries and NaN latents."""
    rng = np.random.default_rng(seed)
    basis = surface_terms(hermite_plan(p), degree=degree)
    x = rng.normal(size=(g, p))
    values = rng.normal(size=(s, k))[None] * 3.0 + rng.normal(size=(g, s, k)) * 0.2 + (x @ rng.normal(size=(p, s * k))).reshape(g, s, k) \
        + (x[:, 0] * x[:, 1])[:, None, None] * rng.normal(size=(s, k))[None]
    status = np.ones((g, s), dtype=np.uint8)
    mask = np.zeros(g, dtype=np.uint8)
    for _ in range(g // 40):
        values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = np.nan
        status[rng.integers(0, g), rng.integers(0, s)] = 2
        mask[rng.integers(0, g)] = 1
        x[rng.integers(0, g), rng.integers(0, p)] = np.nan
    return values, status, mask, x, basis, np.nan_to_num(values[3])


def within_bounds(got, want, bound, what):
    eg, ec, es = bound
    gaps = (np.abs(got.gram - want.gram) / np.maximum(2 * eg, 1e-300), np.abs(got.cross - want.cross) / np.maximum(2 * ec, 1e-300),
            np.abs(got.sumsq - want.sumsq) / np.maximum(2 * es, 1e-300))
    print(f"{what}: T = {got.gram.shape[0]}, N = {got.sumsq.size}, used {int(want.counts[0])}: gap / bound gram {float(gaps[0].max()):.3f}, "
          f"cross {float(gaps[1].max()):.3f}, sumsq {float(gaps[2].max()):.3f}")
    assert all(np.all(gap <= 1.0) for gap in gaps)


@pytest.mark.parametrize("shape", [(300, 9, 15, 10, None), (700, 5, 13, 12, [64, 3, 47, 62, 0, 33, 12])])
def test_real_tables_within_the_bound_and_the_same_bits_twice(dp, shape):
    g, s, k, p, entries = shape
    values, status, mask, x, basis, shift = real_case(g, s, k, p, 11 + g)
    phi, valid = basis_host(x, basis)
    want = surface_host(values, status, mask, phi, valid, entries, shift, basis=basis)
    assert g // 2 < want.counts[0] < g
    v, st = upload(values, status)
    m = torch.as_tensor(mask, device=DEV)
    table = dp.basis_factors(torch.as_tensor(x, device=DEV), basis)
    acc = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, mask=m, entries=entries, shift=shift)
    again = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, mask=m, entries=entries, shift=shift)
    torch.cuda.synchronize()
    got = acc.numpy()
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.used, want.used) and np.array_equal(got.entries, want.entries)
    d = np.where(want.used[:, None] != 0, shifted(values, status, entries, shift)[0], 0.0)
    within_bounds(got, want, surface_bounds(np.where(want.used[:, None] != 0, phi, 0.0), d), "device against surface_host")
    assert np.array_equal(got.gram.view(np.uint64), got.gram.T.view(np.uint64))  # the transpose by its bits
    for name in ("gram", "cross", "sumsq", "counts", "used"):
        assert torch.equal(getattr(acc, name), getattr(again, name)), name  # two identical calls: the same bits
    fin, ref = acc.finalize(), want.finalize()
    assert fin.count == ref.count and np.all(ref.r2 > 0.9)
    scale = np.abs(ref.coefficients).max(axis=0)
    assert np.all(np.abs(fin.coefficients - ref.coefficients) <= 1e-9 * scale)  # cond(gram / n) of an orthonormal basis over hundreds of draws is O(10)


@pytest.mark.parametrize("edges", [[0, 300], [0, 149, 300], [0, 1, 2, 130, 130, 300], [0, 64, 128, 192, 256, 300]])
def test_chunks_accumulate_to_the_whole_table(dp, edges):
    """Integer tables exactly; real tables within the bound.  An empty chunk adds nothing; the first call overwrites."""
    s, k, g, t = 13, 5, 300, 65
    basis = cut_basis(t)
    values, status, shift = integer_case(g, s, k, 21)
    x = integer_factors(g, 5)
    real = real_case(g, s, k, 10, 77)
    for values, status, mask, x, basis, shift, exact in ((values, status, None, x, basis, shift, True), real + (False,)):
        phi, valid = basis_host(x, basis)
        v, st = upload(values, status)
        m = None if mask is None else torch.as_tensor(mask, device=DEV)
        xs = torch.as_tensor(x, device=DEV)
        table = dp.basis_factors(xs, basis)
        for entries in (None, np.random.default_rng(3).permutation(s * k)[:17]):
            whole = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, mask=m, entries=entries, shift=shift)
            out = dp.surface_ensemble(v[:0], steps_per_geometry=s, basis_table=dp.basis_factors(xs[:0], basis), status=st[:0], entries=entries, shift=shift)
            torch.cuda.synchronize()
            assert out.counts.tolist() == [0, 0] and not out.gram.any() and not out.cross.any() and not out.sumsq.any()
            out.used = torch.zeros(g, dtype=torch.uint8, device=DEV)
            for tensor in (out.gram, out.cross, out.sumsq, out.counts):
                tensor.fill_(99)  # the first call overwrites
            used = []
            for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                part = dp.basis_factors(xs[a:b], basis)
                dp.surface_ensemble(v[a * s : b * s], steps_per_geometry=s, basis_table=part, status=st[a * s : b * s], mask=None if m is None else m[a:b],
                                    out=out, accumulate=i > 0)
                used.append(out.used[: b - a].clone())  # (the used bytes are those of the call)
            torch.cuda.synchronize()
            assert torch.equal(out.counts, whole.counts) and torch.equal(torch.cat(used), whole.used)
            if exact:
                for name in ("gram", "cross", "sumsq"):
                    assert torch.equal(getattr(out, name), getattr(whole, name)), name
                equal_exactly(whole, integer_tables(values, status, mask, phi, valid, entries, shift))
            else:
                keep = whole.used.cpu().numpy()[:, None] != 0
                d = np.where(keep, shifted(values, status, entries, shift)[0], 0.0)
                within_bounds(out.numpy(), whole.numpy(), surface_bounds(np.where(keep, phi, 0.0), d), f"chunks {edges} against the whole")


def test_a_captured_graph(dp):
    """With out= and a shape seen before both passes are captured and replayed with new table contents.  That the capture is a single chain
    without parallel branches is NOT asserted here: it follows from the code - every launch of both entry points goes to the one stream
    they are given, and nothing forks a second one."""
    s, k, g, t = 13, 5, 300, 65
    basis = cut_basis(t)
    values, status, shift = integer_case(g, s, k, 8)
    x = integer_factors(g, 9)
    v, st = upload(values, status)
    xs = torch.as_tensor(x, device=DEV)
    table = dp.basis_factors(xs, basis)
    out = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, shift=shift)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.basis_factors(xs, out=table)
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, status=st, out=out)
    values2, status2, _ = integer_case(g, s, k, 9)  # (the same shift table: integer_case's shift depends on the shape alone)
    x2 = integer_factors(g, 10)[::-1].copy()
    for vals, stat, fac in ((values2, status2, x2), (values, status, x)):
        v.copy_(torch.as_tensor(vals.reshape(g * s, k), device=DEV))
        st.copy_(torch.as_tensor(stat.reshape(-1), device=DEV))
        xs.copy_(torch.as_tensor(fac, device=DEV))
        for tensor in (out.gram, out.cross, out.sumsq, out.counts, out.used, table.phi, table.valid):
            tensor.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        phi, valid = basis_host(fac, basis)
        assert np.array_equal(table.phi.cpu().numpy(), phi)
        equal_exactly(out, integer_tables(vals, stat, None, phi, valid, None, shift))


def test_error_paths(dp):
    s, k, g, t = 9, 15, 64, 10
    rng = np.random.default_rng(0)
    lib = dp.lib
    import ctypes as C
    from open_kinematics_amd import _lib

    basis = cut_basis(t)
    v = torch.as_tensor(rng.normal(size=(g * s, k)), device=DEV)
    xs = torch.as_tensor(rng.normal(size=(g, P)), device=DEV)
    table = dp.basis_factors(xs, basis)
    with pytest.raises(ValueError, match=r"entry 1 repeats entry 0 \(index 4\)"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, entries=[4, 4])
    with pytest.raises(ValueError, match=r"okx_ensemble_surface: entry 0 is 135, outside \[0, 135\)"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, entries=[135])
    with pytest.raises(ValueError, match="okx_ensemble_surface: 0 entries selected, 1 to 2048 allowed"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, entries=[])
    wide = torch.zeros((g, 2049), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="2049 entries selected, 1 to 2048 allowed"):
        dp.surface_ensemble(wide, steps_per_geometry=1, basis_table=table)
    with pytest.raises(ValueError, match="one row per geometry of the table"):
        dp.surface_ensemble(v[: 5 * s], steps_per_geometry=s, basis_table=table)
    with pytest.raises(ValueError, match="accumulate=True needs the accumulator"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, accumulate=True)
    out = dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, entries=[1, 2, 3])
    with pytest.raises(ValueError, match="out= carries its own shift and entries"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, out=out, entries=[1, 2, 3])
    with pytest.raises(ValueError, match="out= was taken with another basis"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=dp.basis_factors(xs, cut_basis(t + 1)), out=out)
    with pytest.raises(ValueError, match="mask must be a contiguous uint8"):
        dp.surface_ensemble(v, steps_per_geometry=s, basis_table=table, mask=torch.zeros(g + 1, dtype=torch.uint8, device=DEV))
    # the basis: the host check's words, from the Python check and from the library
    bad = SurfaceBasis(basis.law, basis.terms[1:])
    with pytest.raises(ValueError, match=r"okx_ensemble_basis: term 0 must be the constant \(-1, 0, -1, 0\)"):
        dp.basis_factors(xs, bad)
    law, terms = np.ascontiguousarray(basis.law), np.ascontiguousarray(basis.terms[1:])
    assert lib.okx_ensemble_basis_check(law.ctypes.data_as(C.c_void_p), P, terms.ctypes.data_as(C.c_void_p), t - 1) != 0
    assert "term 0 must be the constant (-1, 0, -1, 0)" in _lib.last_error()
    with pytest.raises(ValueError, match="one column per factor of the basis"):
        dp.basis_factors(xs[:, :5], basis)
    # the entry points themselves: null outputs, short scratch, counts out of range
    need = lib.okx_ensemble_surface_scratch_bytes(g, s, k, t, 3)
    assert need > 0 and lib.okx_ensemble_surface_scratch_bytes(g, s, k, 1025, 3) == 0 and lib.okx_ensemble_surface_scratch_bytes(g, s, k, t, 2049) == 0
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = lambda x: C.c_void_p(0 if x is None else x.data_ptr())  # noqa: E731

    def call(n_terms=t, n_entries=3, gram=out.gram, scratch_bytes=need, phi=table.phi):
        return lib.okx_ensemble_surface(g, s, k, p(v), k, None, 0, None, p(phi), t, p(table.valid), n_terms, p(out.entries), n_entries, p(out.shift), 0,
                                        p(gram), p(out.cross), p(out.sumsq), p(out.counts), None, p(scratch), scratch_bytes, None)

    for kwargs, words in ((dict(gram=None), "null gram, cross, sumsq, counts or shift"), (dict(scratch_bytes=need - 8), "bytes of scratch needed"),
                          (dict(n_terms=0), "0 terms, 1 to 1024 allowed"), (dict(n_terms=1025), "1025 terms, 1 to 1024 allowed"),
                          (dict(n_entries=0), "0 entries selected, 1 to 2048 allowed"), (dict(n_entries=2049), "2049 entries selected, 1 to 2048 allowed"),
                          (dict(phi=None), "null basis table")):
        assert call(**kwargs) != 0, kwargs
        assert words in _lib.last_error(), (kwargs, _lib.last_error())
    torch.cuda.synchronize()
    assert out.counts.tolist() == [g, 0]  # nothing was touched by the refused calls


def test_predict_surface_is_the_host_prediction(dp):
    """1e-12 relative to the LARGEST prediction of the entry, not element by element: a prediction is a sum of T signed terms that may cancel
    to nearly nothing, and the two matrix products differ by their summation order (T u sum |phi_t c_t| each)."""
    g, s, k, p = 400, 3, 4, 6
    values, status, mask, x, basis, shift = real_case(g, s, k, p, 5, degree=3)
    phi, valid = basis_host(x, basis)
    surface = surface_host(values, status, mask, phi, valid, [7, 0, 3, 11], shift, basis=basis).finalize()
    at = np.random.default_rng(1).normal(size=(50, p))
    at[4, 2] = np.nan
    want = surface.predict(at)
    got = dp.predict_surface(surface, torch.as_tensor(at, device=DEV)).cpu().numpy()
    assert got.shape == (50, 4) and np.all(np.isnan(got[4])) and np.all(np.isnan(want[4]))
    rows = np.arange(50) != 4
    # the same basis bits on both sides; the two matrix products differ by their summation order: T u sum |phi_t c_t| each, far inside 1e-12 relative
    assert np.all(np.abs(got[rows] - want[rows]) <= 1e-12 * np.abs(want[rows]).max(axis=0))


# ---- the chain end to end: a sampled double-wishbone ensemble through ShardedEnsemble(reduce=True, factors="sampled", surface=True) ----

CHAIN_G, CHAIN_S = 256, 9  # 3 perturbed points: 9 latents, T = 1 + 18 + 36 = 55 terms; 4 columns: N = 36 entries


def chain_pipe(chunks=None):
    import open_kinematics_amd.dist as okd

    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_effects_rate import build

    dp, plan, rel, columns = build(CHAIN_G, CHAIN_S, DEV, n_points=3)
    pipe = okd.ShardedEnsemble(dp, plan, rel, CHAIN_S, chunks=chunks, metric_columns=columns, reduce=True, factors="sampled", surface=True, chain_len=1,
                               predictor=False)
    return dp, plan, pipe


def chain_reference(pipe, plan):
    """surface_host over the run's own metric_local, and its bounds."""
    g, s = CHAIN_G, CHAIN_S
    values = pipe.metric_local.cpu().numpy().reshape(g, s, 4)
    status = pipe.info_local[:, 32].cpu().numpy().reshape(g, s)
    flags, latents = pipe.sampled_flags.cpu().numpy(), pipe.my_factors.cpu().numpy()
    shift = pipe.local_accumulator.shift.cpu().numpy()
    basis = surface_terms(plan)
    assert basis.n_terms == 55 and basis.orthonormal
    phi, valid = basis_host(latents, basis)
    want = surface_host(values, status, flags, phi, valid, None, shift, basis=basis)
    keep = want.used[:, None] != 0
    d = np.where(keep, values.reshape(g, -1) - shift.reshape(1, -1), 0.0)
    return want, surface_bounds(np.where(keep, phi, 0.0), d), values, latents, phi


@pytest.mark.parametrize("chunks", [1, 3])
def test_the_chain_on_one_gpu(chunks):
    dp, plan, pipe = chain_pipe(chunks)
    acc = pipe.step()
    torch.cuda.synchronize()
    want, bound, values, latents, phi = chain_reference(pipe, plan)
    got = pipe.surface_accumulator.numpy()
    assert np.array_equal(got.counts, want.counts) and np.array_equal(pipe.stages["surface"].local.used.cpu().numpy(), want.used)
    assert want.counts[0] >= 57 and pipe.surface_exchange_bytes_per_rank == 0
    within_bounds(got, want, bound, f"chain in {chunks} chunk(s) against surface_host")
    fit = pipe.surface()
    assert fit.coefficients.shape == (55, 36) and fit.first.shape == (9, 36) and fit.basis.factor_names == tuple(plan.factor_names())
    # both models against NumPy's lstsq on the copied table: the surface on its used geometries, the reduce pass's straight line on all of them
    used = want.used != 0
    d = values.reshape(CHAIN_G, -1) - fit.shift[None, :]
    full, *_ = np.linalg.lstsq(phi[used], d[used], rcond=None)
    scale = np.maximum(np.abs(full).max(axis=0), 1e-300)  # (an entry that does not move at all: 0 against 0)
    gap = np.abs(fit.coefficients - full) / scale
    print(f"coefficients against lstsq: {float(gap.max()):.2e} relative; r2 from {float(np.nanmin(fit.r2)):.6f}")
    assert np.all(gap <= 1e-8)  # cond(Phi^T Phi / n) of 55 orthonormal terms over 256 LHS draws is below 100: the normal equations lose two digits of 16
    stats = acc.finalize()
    # the fixture: 256 LHS draws at sigma = 1 mm, every state converges and every metric is defined, so no geometry is dropped and the reduce
    # pass's straight line is defined for every entry - asserted, so that the comparison below can never fall away unseen
    assert used.all() and np.isfinite(stats.sensitivity).all()
    line, *_ = np.linalg.lstsq(np.column_stack([np.ones(CHAIN_G), latents]), d, rcond=None)
    slopes = stats.sensitivity.reshape(36, 9).T  # [P, N]
    line_gap = np.abs(slopes - line[1:]) / np.maximum(np.abs(line[1:]).max(axis=0), 1e-300)
    print(f"reduce slopes against lstsq: {float(line_gap.max()):.2e} relative")
    assert np.all(line_gap <= 1e-8)
    # degree 1 of the surface (times the latents' scale, 1 for Hermite (0, 1)) differs from the straight line's slope by what the quadratic
    # terms explain in-sample - the difference of the two lstsq models, not a fixed number
    first = fit.coefficients[1:10] * fit.basis.law[:, 2][:, None]
    assert np.all(np.abs((first - slopes) - (full[1:10] - line[1:])) <= 2e-8 * scale)
    first_gram = got.gram.copy()
    pipe.step()  # a second step starts from nothing
    torch.cuda.synchronize()
    assert np.array_equal(pipe.surface_accumulator.numpy().gram, first_gram)


def test_two_ranks_rehearsed_on_one_gpu(tmp_path):
    """Two ranks at 256 x 9 in two chunks on cuda:0 over gloo in fresh child processes, each under its own time limit: both ranks hold the same
    bits, and they are within the bound of surface_host over the one-GPU run's table."""
    world = 2
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_surface_rate.py"), "--rehearse", str(world), "--geometries", str(CHAIN_G),
                           "--steps-per-geometry", str(CHAIN_S), "--chunks", "2", "--points", "3", "--out", str(tmp_path), "--timeout", "240"],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    for key in ("gram", "cross", "sumsq", "counts", "entries", "shift"):
        assert torch.equal(got[0][key], got[1][key]), key
    assert np.array_equal(got[0]["coefficients"], got[1]["coefficients"])
    dp, plan, pipe = chain_pipe(1)
    pipe.step()
    torch.cuda.synchronize()
    want, bound, *_ = chain_reference(pipe, plan)
    assert torch.equal(got[0]["shift"], pipe.local_accumulator.shift.cpu())
    from open_kinematics_amd.ensemble_stats import SurfaceAccumulator

    acc = SurfaceAccumulator(*(got[0][key].numpy() for key in ("gram", "cross", "sumsq", "counts")), want.shift, want.entries, basis=want.basis)
    assert np.array_equal(acc.counts, want.counts)
    within_bounds(acc, want, bound, "two ranks against surface_host")
    for r in range(world):
        lo, hi = got[r]["range"]
        assert np.array_equal(got[r]["used"].numpy(), want.used[lo:hi]) and got[r]["sent"] == 8 * (55 * 55 + 55 * 36 + 36 + 2)
