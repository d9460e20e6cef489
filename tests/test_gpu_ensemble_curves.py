"""
GPU: okx_ensemble_curves (DeviceProgram.curves_ensemble) and ShardedEnsemble(reduce=True, curves=...) against
ensemble_stats.curves_host on the copied tables.  Counts, extremes, abscissae (fields 6 .. 11) and every NaN pattern are compared
exactly; the fit within the forward-error bound of a Cholesky solve of normal equations, 8 cond(N) eps max|y| per (geometry,
column) in u units, and the residual fields within what that moves a fitted value by (tests/test_ensemble_curves.py states both
and holds the generator of the inputs).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_stats import (CURVE_FIELDS, covariance_host, curves_host, reduce_host, screen_host, select_host)
from test_ensemble_curves import bits, compare_with_host, random_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def upload(values, status):
    g, s, k = values.shape
    return (torch.as_tensor(np.ascontiguousarray(values).reshape(g * s, k), device=DEV),
            None if status is None else torch.as_tensor(np.ascontiguousarray(status).reshape(-1), device=DEV))


def device_curves(dp, values, status, abscissa, origin, scale, degree, window, **kw):
    v, st = upload(values, status)
    got = dp.curves_ensemble(v, steps_per_geometry=values.shape[1], status=st, abscissa=abscissa, origin=origin, scale=scale, degree=degree,
                             window=window, **kw)
    torch.cuda.synchronize()
    return got


def check(dp, case, degree):
    values, status, abscissa, origin, scale, window = case
    got = device_curves(dp, values, status, abscissa, origin, scale, degree, window).finalize()
    return compare_with_host(got, values, status, abscissa, origin, scale, degree, window)


SHAPES = [(1, 1), (2, 2), (3, 4), (4, 5), (5, 24), (63, 5), (64, 4), (65, 24), (257, 1), (64, 1), (257, 4), (63, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_where_the_mapping_can_go_wrong(dp, shape):
    """S in {1, 2, 3, 4, 5, 63, 64, 65, 257} and K in {1, 2, 4, 5, 24}: 64 geometries per wavefront down to one, column lanes
    that are idle (K = 5 of 8, 24 of 32), slices that end at different steps, several steps per lane; G in {0, 1, 37, 64, 1031}
    - no geometry, one, a count that is no multiple of what a wavefront packs, several workgroups.  At G = 37 every degree with
    both kinds of abscissa; window and status bytes alternate."""
    s, k = shape
    at = SHAPES.index(shape)
    worst, tally = 0.0, np.zeros(5, dtype=np.int64)
    runs = [(g, (at + i) % 4, bool((at + i) & 1), bool((at + i) & 2), not (g == 64 and at % 2)) for i, g in enumerate((0, 1, 64, 1031))]
    runs += [(37, d, column, bool((d + at) & 1), bool(d & 2) or column) for d in range(4) for column in (False, True)]
    for g, degree, column, window, with_status in runs:
        case = random_case(s, k, g, 1000 * at + 10 * g + degree, column=column, window=window, with_status=with_status, degree=degree)
        ratio, *counts = check(dp, case, degree)
        worst = max(worst, ratio)
        if g >= 37:
            tally += counts
    print(f"curves S={s} K={k}: worst coefficient error / (cond eps max|y|) = {worst:.3f} (bound 8)")
    empty, short, refused, fitted, rows = tally
    # the inputs are worth the test: rows without a used step, short rows, refused fits, and nine rows in ten fitted
    assert empty > 0
    if s >= 8:
        assert short > 0 and refused > 0 and fitted > 0.9 * rows


def test_more_columns_than_a_wavefront_has_lanes(dp):
    """K = 70: the columns go in two blocks of 64 lanes, the second with six lanes live; the abscissa column lies in the second."""
    for degree, column in ((1, False), (3, True)):
        case = random_case(9, 70, 5, 69, column=column, degree=degree)
        assert not column or case[2] == 69
        _, _, _, _, fitted, rows = check(dp, case, degree)
        assert fitted > 0.3 * rows


def test_argument_checks_mirror_the_host(dp):
    values, status, abscissa, origin, scale, window = random_case(6, 3, 4, 1)
    v, st = upload(values, status)
    kw = dict(steps_per_geometry=6, status=st, abscissa=abscissa, scale=scale)
    for change, message in ((dict(degree=4), "degree 4, 0 to 3 allowed"), (dict(scale=0.0), "scale is 0, not finite and > 0"),
                            (dict(origin=float("nan")), "origin is NaN"), (dict(window=(2.0, 1.0)), r"window has lo > hi \(2 > 1\)"),
                            (dict(abscissa=3), r"abscissa column 3, outside \[0, 3\)"), (dict(abscissa=np.zeros(5)), "shared abscissa of 5 values, 6 steps")):
        with pytest.raises(ValueError, match=message):
            dp.curves_ensemble(v, **{**kw, **change})
    with pytest.raises(ValueError, match="unit column stride"):
        dp.curves_ensemble(v.t(), **kw)
    with pytest.raises(ValueError, match="abscissa and scale are needed"):
        dp.curves_ensemble(v, steps_per_geometry=6)
    out = dp.curves_ensemble(v, **kw)
    with pytest.raises(ValueError, match="out= carries its own"):
        dp.curves_ensemble(v, steps_per_geometry=6, out=out, degree=1)
    with pytest.raises(ValueError, match="do not fit"):
        dp.curves_ensemble(v, steps_per_geometry=6, out=out, first_row=1)


def test_strided_rows_inside_a_larger_tensor(dp):
    """Row 0 of evaluation-shaped records (ld = 3 * 24 > K) and byte 32 of 40-byte info records as views in the MIDDLE of larger
    tensors filled with NaN and rejected bytes: a read outside the view would change a count."""
    s, k, g = 16, 24, 50
    values, status, kx, origin, scale, window = random_case(s, k, g, 77 * 24 + 5, column=True, window=True)
    assert kx == 5
    pad = 40
    big = torch.full((pad + g * s + pad, 3, 24), float("nan"), dtype=torch.float64, device=DEV)
    info = torch.full((pad + g * s + pad, 40), 2, dtype=torch.uint8, device=DEV)
    big[pad : pad + g * s, 0, :] = torch.as_tensor(values.reshape(g * s, k), device=DEV)
    info[pad : pad + g * s, 32] = torch.as_tensor(status.reshape(-1), device=DEV)
    view, st = big[pad : pad + g * s, 0, :], info[pad : pad + g * s, 32]
    assert view.stride(0) == 72 and not view.is_contiguous() and st.stride(0) == 40
    got = dp.curves_ensemble(view, steps_per_geometry=s, status=st, abscissa=kx, origin=origin, scale=scale, degree=2, window=window)
    torch.cuda.synchronize()
    _, empty, _, refused, fitted, rows = compare_with_host(got.finalize(), values, status, kx, origin, scale, 2, window)
    assert empty > 0 and refused > 0 and fitted > 0.9 * rows
    # ... and a narrower table inside the same rows (columns 3 .. 7, the abscissa column inside that range)
    narrow = big[pad : pad + g * s, 0, 3:8]
    got = dp.curves_ensemble(narrow, steps_per_geometry=s, status=st, abscissa=kx - 3, origin=origin, scale=scale, degree=3, window=window)
    torch.cuda.synchronize()
    compare_with_host(got.finalize(), values[:, :, 3:8], status, kx - 3, origin, scale, 3, window)


@pytest.mark.parametrize("edges", [[0, 300], [0, 149, 300], [0, 1, 2, 130, 130, 300]])
def test_chunks_fill_the_one_table(dp, edges):
    s, k, g = 16, 4, 300
    values, status, abscissa, origin, scale, window = random_case(s, k, g, 21, column=True)
    whole = device_curves(dp, values, status, abscissa, origin, scale, 2, window)
    v, st = upload(values, status)
    out = dp.curves_prepare(s, k, g, abscissa=abscissa, origin=origin, scale=scale, degree=2, window=window)
    out.features.fill_(99.0)
    out.count.fill_(99)
    for a, b in zip(edges[:-1], edges[1:]):
        dp.curves_ensemble(v[a * s : b * s], steps_per_geometry=s, status=st[a * s : b * s], out=out, first_row=a)
    torch.cuda.synchronize()
    assert torch.equal(out.count, whole.count) and torch.equal(out.features.view(torch.int64), whole.features.view(torch.int64))
    compare_with_host(out.finalize(), values, status, abscissa, origin, scale, 2, window)


def test_determinism_and_a_captured_graph(dp):
    s, k, g = 64, 4, 1500
    values, status, abscissa, origin, scale, window = random_case(s, k, g, 8, window=True)
    v, st = upload(values, status)
    kw = dict(steps_per_geometry=s, status=st)
    first = dp.curves_ensemble(v, abscissa=abscissa, origin=origin, scale=scale, degree=3, window=window, **kw)
    second = dp.curves_ensemble(v, abscissa=abscissa, origin=origin, scale=scale, degree=3, window=window, **kw)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.count, b.count) and torch.equal(a.features.view(torch.int64), b.features.view(torch.int64))  # noqa: E731
    assert same(first, second)
    compare_with_host(first.finalize(), values, status, abscissa, origin, scale, 3, window)
    # a single-stream captured graph, replayed once after its outputs were overwritten
    out = dp.curves_prepare(s, k, g, abscissa=abscissa, origin=origin, scale=scale, degree=3, window=window)
    dp.curves_ensemble(v, out=out, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.curves_ensemble(v, out=out, **kw)
    out.features.fill_(3.0)
    out.count.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, first)


def test_the_feature_table_feeds_the_other_passes(dp):
    """screen, select, reduce and covariance on ``.table()`` with one step per geometry equal their host counterparts on
    ``curves_host``-shaped tables of the copied device features: the layout is the one those passes take."""
    from test_ensemble_screen import same as same_screen

    s, k, g = 33, 4, 400
    values, status, abscissa, origin, scale, window = random_case(s, k, g, 12, column=True)
    got = device_curves(dp, values, status, abscissa, origin, scale, 2, window)
    table = got.table()
    assert tuple(table.shape) == (g, k * CURVE_FIELDS) and table.data_ptr() == got.features.data_ptr()
    host = got.finalize().table()[:, None, :]  # [G, 1, K * 12]
    assert np.isnan(host).any() and np.isfinite(host[:, 0, 1]).mean() > 0.9
    n = k * CURVE_FIELDS
    finite = np.where(np.isfinite(host), host, np.nan)
    limits = np.stack([np.nanquantile(finite, 0.05, axis=0), np.nanquantile(finite, 0.95, axis=0)], axis=2)
    limits[0, 2 * CURVE_FIELDS :] = (-np.inf, np.inf)  # two columns are looked at
    screened = dp.screen_ensemble(table, steps_per_geometry=1, limits=limits)
    torch.cuda.synchronize()
    want = screen_host(host, None, limits)
    same_screen(screened.finalize(), want)
    assert 0 < want.tally[1] < g and want.tally[3] > 0
    quantiles = dp.select_ensemble(table, steps_per_geometry=1, probs=(0.1, 0.5, 0.9)).finalize()
    want_q = select_host(host, None, (0.1, 0.5, 0.9))
    assert np.array_equal(quantiles.count, want_q.count) and np.array_equal(bits(quantiles.lower), bits(want_q.lower)) and np.array_equal(bits(quantiles.upper), bits(want_q.upper))
    shift = np.nan_to_num(host[0], nan=0.0, posinf=0.0, neginf=0.0)
    acc = dp.reduce_ensemble(table, steps_per_geometry=1, shift=shift).numpy()
    torch.cuda.synchronize()
    want_a = reduce_host(host, None, None, shift)
    exact = [0, 1, 4, 5, 6, 7]  # count, rejected, min, max, argmin, argmax
    assert np.array_equal(acc.acc[..., exact], want_a.acc[..., exact])
    d = np.where(np.isfinite(host), host - shift[None], 0.0)
    assert np.all(np.abs(acc.acc[..., 2] - want_a.acc[..., 2]) <= 2 * g * 2.0 ** -53 * np.abs(d).sum(axis=0))
    assert np.all(np.abs(acc.acc[..., 3] - want_a.acc[..., 3]) <= 2 * (g + 1) * 2.0 ** -53 * (d * d).sum(axis=0))
    entries = [1, 2, CURVE_FIELDS + 1, 2 * CURVE_FIELDS + 7]  # gradients, a curvature, a maximum
    cov = dp.covariance_ensemble(table, steps_per_geometry=1, entries=entries, shift=shift).numpy()
    torch.cuda.synchronize()
    want_c = covariance_host(host, None, entries, shift)
    assert np.array_equal(cov.counts, want_c.counts) and np.array_equal(cov.used, want_c.used) and 0 < want_c.counts[1] < g
    dd = np.where(want_c.used[:, None] != 0, d[:, 0, entries], 0.0)
    assert np.all(np.abs(cov.gram - want_c.gram) <= 2 * (g + 2) * 2.0 ** -53 * (np.abs(dd).T @ np.abs(dd)))
    assert n == 48


def _c5(n_geom, steps):
    from test_gpu_ensemble_stats import _c5 as build

    return build(n_geom, steps)


def test_end_to_end_on_evaluation_rows():
    """48 perturbed double-wishbone geometries x 16 bump steps, solved and evaluated; the pass reads row 0 of the evaluation
    records and byte 32 of the info records in place, every geometry against its own wheel travel."""
    from open_kinematics_amd.metrics import METRIC_NAMES

    g, s = 48, 16
    dp, program, table, rel, columns = _c5(g, s)
    gpos, gparam = dp.rebind(table)
    targets = dp.ensemble_targets(gpos, rel)
    res = dp.solve_evaluated(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, output="none", chain_len=1, predictor=False)
    torch.cuda.synchronize()
    view, st = res.eval[:, 0, :], res.info_raw[:, 32]
    k = view.shape[1]
    assert view.stride(0) > k and st.stride(0) == 40
    kx, camber = METRIC_NAMES.index("wheel_travel"), METRIC_NAMES.index("camber")
    kw = dict(abscissa=kx, origin=0.0, scale=40.0, degree=2, window=(-40.0, 40.0))
    got = dp.curves_ensemble(view, steps_per_geometry=s, status=st, **kw)
    torch.cuda.synchronize()
    values, status = view.cpu().numpy().reshape(g, s, k), st.cpu().numpy().reshape(g, s)
    _, empty, short, refused, fitted, rows = compare_with_host(got.finalize(), values, status, kx, 0.0, 40.0, 2, (-40.0, 40.0))
    host = got.finalize()
    accepted = host.count[:, camber] >= 3
    assert accepted.sum() > 0.9 * g
    gradient = host.gradient[accepted, camber]
    assert np.all(np.isfinite(gradient)) and np.all(gradient != 0.0)
    # the travel column against itself is the line x: value 0 at the origin, gradient 1
    assert np.allclose(host.features[accepted, kx, :3], [0.0, 1.0, 0.0], atol=1e-9)


def _stat_tables(stats) -> dict:
    import dataclasses

    return {f.name: getattr(stats, f.name) for f in dataclasses.fields(stats)}


def _same_stats(a: dict, b: dict) -> None:
    for name in a:
        x, y = a[name], b[name]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name
        else:
            assert x == y, name


def _one_process(g, s, factors, chunks=1):
    import open_kinematics_amd.dist as okd

    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_curves_rate import curve_arguments

    dp, program, table, rel, columns = _c5(g, s)
    pipe = okd.ShardedEnsemble(dp, table, rel, s, chunks=chunks, metric_columns=columns, reduce=True, factors=factors, curves=curve_arguments(rel),
                               chain_len=1, predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    return pipe, curve_arguments(rel)


def test_sharded_ensemble_on_one_gpu():
    """64 geometries x 16 steps: curves_local() equals curves_host of the same run's metric_local and status bytes within the
    fit's bound, curve_stats() is the reduction of the device's own feature table (reduce_host's integers, extremes and indices
    exactly), and one chunk and two give the same bits."""
    g, s = 64, 16
    answers = []
    for chunks in (1, 2):
        pipe, kw = _one_process(g, s, "hardpoints", chunks)
        pipe.step()  # the second step overwrites the first
        torch.cuda.synchronize()
        local = pipe.curves_local().finalize()
        values = pipe.metric_local.cpu().numpy().reshape(g, s, 4)
        status = pipe.info_local[:, 32].cpu().numpy().reshape(g, s)
        _, _, _, _, fitted, rows = compare_with_host(local, values, status, kw["abscissa"], kw["origin"], kw["scale"], kw["degree"], kw["window"])
        assert fitted > 0.9 * rows
        stage = pipe.stages["curves"]
        want = reduce_host(local.table()[:, None, :], None, pipe.my_factors.cpu().numpy(), stage.acc.shift.cpu().numpy(), 0, pipe.factor_names)
        stats = pipe.curve_stats()
        for name in ("count", "rejected", "min", "max", "argmin", "argmax"):
            assert np.array_equal(getattr(stats, name), getattr(want.finalize(), name), equal_nan=True), name
        assert stats.sensitivity.shape == (1, 4 * CURVE_FIELDS, pipe.n_factors) and np.isfinite(stats.sensitivity[0, 1]).all()
        assert pipe.curves_exchange_bytes_per_rank == 0
        answers.append((_stat_tables(stats), local))
    _same_stats(answers[0][0], answers[1][0])
    assert np.array_equal(bits(answers[0][1].features), bits(answers[1][1].features)) and np.array_equal(answers[0][1].count, answers[1][1].count)


@pytest.mark.parametrize("world,g,chunks", [(2, 256, 2), (3, 2, 1)])
def test_ranks_rehearsed_on_one_gpu(tmp_path, world, g, chunks):
    """Two ranks at 256 x 16 in two chunks, and three ranks over two geometries (rank 2 owns none), on cuda:0 over gloo in fresh
    child processes: curves_local() is the rank's slice of the one-process feature table bit for bit, and every rank's
    curve_stats() carries the bits of the one-process result - every rank reduces the same gathered table."""
    import open_kinematics_amd.dist as okd

    s = 16
    pipe, _ = _one_process(g, s, "hardpoints" if g > 2 else None)
    want, features, count = _stat_tables(pipe.curve_stats()), pipe.curves_local().features.cpu(), pipe.curves_local().count.cpu()
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_curves_rate.py"), "--rehearse", str(world), "--geometries", str(g),
                           "--steps-per-geometry", str(s), "--chunks", str(chunks), "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    largest = max(hi - lo for lo, hi in (okd.shard_range(g, r, world) for r in range(world)))
    for r in range(world):
        lo, hi = got[r]["range"]
        assert (lo, hi) == okd.shard_range(g, r, world)
        assert torch.equal(got[r]["features"].view(torch.int64), features[lo:hi].view(torch.int64)) and torch.equal(got[r]["count"], count[lo:hi])
        _same_stats(got[r]["stats"], want)
        assert got[r]["curves_sent"] == 8 * largest * 4 * CURVE_FIELDS and got[r]["n_factors"] == pipe.n_factors
    assert (want["count"][0] > 0).any()
