"""
CPU: the curve characteristics of an ensemble along the sweep (ensemble_stats.curves_host, the definition okx_ensemble_curves is
compared with) against numpy.polynomial.polynomial.polyfit on hand-made curves, the undefined cases, every message of
check_curve_arguments, and the Curves stage of ShardedEnsemble(reduce=True, curves=...) on a CPU ensemble - one process and two
gloo ranks, the stand-in program of tests/test_dist.py.

random_case / compare_with_host are what tests/test_gpu_ensemble_curves.py feeds the device pass with and judges it by.  The
bound on the coefficients is the forward-error bound of a Cholesky solve of normal equations, in u units:

    |a_i(device) - a_i(lstsq)| <= 8 cond(N) eps max|y|,   N = V^T V of THAT (geometry, column)'s used steps, eps = 2^-52

and on the residual fields (4, 5) that bound times sum_i max|u|^i - what a coefficient error moves a fitted value by - plus
4 eps max|y| for the evaluation itself.  Counts, extremes and abscissae (fields 6 .. 11) are compared by their bits.
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from numpy.polynomial import polynomial

from conftest import REPO
from open_kinematics_amd.ensemble_stats import (CURVE_FIELDS, EnsembleCurves, check_curve_arguments, curve_normal_refused, curves_host,
                                                reduce_host)
from test_ensemble_stats import COLUMNS, _stand_in

EPS = 2.0 ** -52
BOUND = 8.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def used_steps(values, status, x, window):
    """``used [G, S, K]`` and ``xs [G, S]`` by the rule of the pass (``x``: a shared [S] table or a column index)."""
    g, s, k = values.shape
    xs = np.broadcast_to(np.asarray(x, dtype=np.float64)[None], (g, s)) if not isinstance(x, (int, np.integer)) else values[:, :, int(x)]
    lo, hi = (-np.inf, np.inf) if window is None else window
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(xs) & (xs >= lo) & (xs <= hi)
    ok = np.isfinite(values) & inside[:, :, None]
    if status is not None:
        ok &= ((status & 7) == 1)[:, :, None]
    return ok, xs


def random_case(s, k, g, seed, *, column=False, window=False, with_status=True, degree=3):
    """
    ``(values [G, S, K], status [G, S] or None, abscissa, origin, scale, window)``: a uniform grid on [-1, 1] in u, jittered by
    at most a quarter of its spacing, in a third of the cases (by the seed) moved to [0, 1] and in another third to
    [0.5, 1.5], a tenth of the steps dropped (a NaN abscissa); cubics with noise as values; about 4 % rejected states and a few
    NaN / +-inf values.  With ``column`` every geometry has its own jitter and drops in column ``kx`` of the table; then geometry 2
    (if there is one) has all its abscissae equal - a refused fit - while geometry 1 is rejected as a whole and geometry 3 keeps
    ``degree`` used steps - a short row.
    """
    rng = np.random.default_rng(seed)
    origin, scale = 3.0, 25.0
    grid = np.linspace(-1.0, 1.0, s) if s > 1 else np.zeros(1)
    spacing = 2.0 / (s - 1) if s > 1 else 1.0
    shape = (g, s) if column else (s,)
    u = grid + rng.uniform(-0.25, 0.25, size=shape) * spacing
    kind = seed % 3
    if kind == 1:
        u = 0.5 * (u + 1.0)
    elif kind == 2:
        u = 0.5 * (u + 1.0) + 0.5
    x = origin + scale * u
    x = np.where(rng.random(shape) < 0.1, np.nan, x)
    uu = np.broadcast_to(u, (g, s))[:, :, None]
    coef = rng.normal(size=(4, g, 1, k)) * np.array([5.0, 2.0, 1.0, 0.5]).reshape(4, 1, 1, 1)
    values = coef[0] + coef[1] * uu + coef[2] * uu ** 2 + coef[3] * uu ** 3 + 1e-3 * rng.normal(size=(g, s, k))
    status = np.ones((g, s), dtype=np.uint8)
    for _ in range(max(g // 25, min(g, 1))):
        values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = rng.choice([np.nan, np.inf, -np.inf])
    status[rng.random((g, s)) < 0.04] = rng.choice(np.array([0, 2, 3, 5], dtype=np.uint8))
    abscissa = x
    if column:
        kx = int(seed % k)
        values[:, :, kx] = x
        abscissa = kx
        if g > 2:
            values[2, :, kx] = origin + 0.5 * scale
    if g > 1:
        status[1] = 2
    if g > 3 and s > degree:
        status[3] = 2
        status[3, rng.choice(s, size=degree, replace=False)] = 1
    win = (origin - 0.8 * scale, origin + 1.2 * scale) if window else None
    return values, (status if with_status else None), abscissa, origin, scale, win


def compare_with_host(got: EnsembleCurves, values, status, abscissa, origin, scale, degree, window):
    """
    Device (or any other) features against ``curves_host``: count, fields 6 .. 11 and every NaN pattern exactly, the fit within
    the bounds of the module docstring.  Returns ``(worst ratio of a coefficient error to its bound without the factor 8, rows
    with no used step, short rows, refused fits, fitted rows, all rows)``.
    """
    want = curves_host(values, status, abscissa, origin, scale, degree, window)
    gf, gc = np.asarray(got.features), np.asarray(got.count)
    assert gf.shape == want.features.shape and gc.shape == want.count.shape and gc.dtype == np.int32
    assert np.array_equal(gc, want.count)
    assert np.array_equal(np.isnan(gf), np.isnan(want.features))
    assert np.array_equal(bits(gf[..., 6:]), bits(want.features[..., 6:]))
    used, xs = used_steps(values, status, abscissa, window)
    powers = np.arange(degree + 1)
    worst = 0.0
    empty = short = refused = fitted = 0
    g, s, k = values.shape
    for gi in range(g):
        for ki in range(k):
            at = np.flatnonzero(used[gi, :, ki])
            if at.size == 0:
                empty += 1
                continue
            if np.isnan(want.features[gi, ki, 0]):
                short += at.size < degree + 1
                refused += at.size >= degree + 1
                continue
            fitted += 1
            u = (xs[gi, at] - origin) / scale
            v = np.vander(u, degree + 1, increasing=True)
            unit = np.linalg.cond(v.T @ v) * EPS * np.max(np.abs(values[gi, at, ki]))
            err = np.abs(gf[gi, ki, : degree + 1] * scale ** powers - want.features[gi, ki, : degree + 1] * scale ** powers)
            ratio = float(err.max() / unit) if unit > 0.0 else (0.0 if err.max() == 0.0 else np.inf)  # (a column of zeros: no error allowed)
            if ratio > 4.0:
                print(f"curves g={gi} k={ki} n={at.size} D={degree} coefficient error / (cond eps max|y|) = {ratio:.3f}")
            worst = max(worst, ratio)
            assert np.all(err <= BOUND * unit), (gi, ki, err / unit)
            assert np.all(gf[gi, ki, degree + 1 : 4] == 0.0)
            tol = BOUND * unit * np.sum(np.max(np.abs(u)) ** powers) + 4 * EPS * np.max(np.abs(values[gi, at, ki]))
            assert np.all(np.abs(gf[gi, ki, 4:6] - want.features[gi, ki, 4:6]) <= tol), (gi, ki)
    return worst, empty, short, refused, fitted, g * k


# ---- curves_host against polyfit on hand-made curves ----

def test_an_exact_cubic_and_its_truncations():
    x = np.array([-30.0, -21.0, -10.0, -2.5, 0.0, 4.0, 11.0, 19.5, 30.0])
    origin, scale = 1.5, 30.0
    t = x - origin
    y = 2.0 - 0.04 * t + 3e-3 * t ** 2 - 5e-5 * t ** 3
    values = np.stack([y, -y, t], axis=1)[None]  # [1, 9, 3]
    for degree in range(4):
        got = curves_host(values, None, x, origin, scale, degree)
        assert got.features.shape == (1, 3, CURVE_FIELDS) and list(got.count[0]) == [9, 9, 9]
        for col in range(3):
            want = polynomial.polyfit(t, values[0, :, col], degree)
            f = got.features[0, col]
            assert np.allclose(f[: degree + 1], want, rtol=1e-10, atol=1e-12 * np.abs(want).max()) and np.all(f[degree + 1 : 4] == 0.0)
            r = values[0, :, col] - polynomial.polyval(t, want)
            assert np.isclose(f[4], np.sqrt(np.mean(r * r)), rtol=1e-9, atol=1e-13) and np.isclose(f[5], np.abs(r).max(), rtol=1e-9, atol=1e-13)
    exact = curves_host(values, None, x, origin, scale, 3)
    assert np.allclose(exact.features[0, 0, :4], [2.0, -0.04, 3e-3, -5e-5], rtol=1e-11) and exact.features[0, 0, 5] < 1e-13
    assert np.allclose(exact.value_at_origin[0], [2.0, -2.0, 0.0], atol=1e-13) and np.allclose(exact.gradient[0], [-0.04, 0.04, 1.0], rtol=1e-11)
    assert np.allclose(exact.curvature[0], [6e-3, -6e-3, 0.0], rtol=1e-10, atol=1e-15) and exact.table().shape == (1, 36)
    line = curves_host(values, None, 2, origin, scale, 1)  # the table's own column as the abscissa: t against t is a line
    assert np.allclose(line.features[0, 2, :2], [origin, 1.0], rtol=1e-12) and line.features[0, 2, 5] < 1e-13
    assert np.array_equal(line.features[0, 2, 6:8], line.features[0, 2, 10:12]) and list(line.features[0, 2, 6:8]) == [t.min(), t.max()]


def test_ties_go_to_the_lowest_step_and_window_edges_are_inclusive():
    x = np.array([5.0, 1.0, 3.0, 2.0, 4.0, 0.0])
    y = np.array([7.0, -1.0, 9.0, -1.0, 9.0, 50.0])
    got = curves_host(y[None, :, None], None, x, 0.0, 1.0, 1, window=(1.0, 5.0))
    f = got.features[0, 0]
    assert got.count[0, 0] == 5  # x = 1 and x = 5 are inside, x = 0 is not
    assert list(f[6:12]) == [-1.0, 9.0, 1.0, 3.0, 1.0, 5.0]  # the first -1 is at x = 1, the first 9 at x = 3
    keep = (x >= 1.0) & (x <= 5.0)
    assert np.allclose(f[:2], polynomial.polyfit(x[keep], y[keep], 1), rtol=1e-12)
    tied = curves_host(y[None, :, None], None, np.array([2.0, 2.0, 1.0, 1.0, 3.0, 3.0]), 0.0, 1.0, 0)
    assert list(tied.features[0, 0, 6:12]) == [-1.0, 50.0, 2.0, 3.0, 1.0, 3.0] and np.isclose(tied.features[0, 0, 0], y.mean(), rtol=1e-14)
    signed = curves_host(np.array([0.0, -0.0, 0.0])[None, :, None], None, np.array([-0.0, 0.0, 1.0]), 0.0, 1.0, 0)
    assert np.array_equal(bits(signed.features[0, 0, 6:12]), bits(np.array([0.0, 0.0, -0.0, -0.0, -0.0, 1.0])))


def test_undefined_cases():
    x = np.linspace(-1.0, 1.0, 6)
    y = np.stack([x ** 2, np.full(6, np.nan), x], axis=1)[None].repeat(4, axis=0)  # [4, 6, 3]
    status = np.ones((4, 6), dtype=np.uint8)
    status[1] = 2                # no used step
    status[2, 2:] = 4            # two used steps
    status[0, 3] = 9             # converged + advisory: counts
    got = curves_host(y, status, x, 0.0, 1.0, 2)
    assert np.array_equal(got.count, [[6, 0, 6], [0, 0, 0], [2, 0, 2], [6, 0, 6]])
    assert np.isnan(got.features[1]).all() and np.isnan(got.features[:, 1]).all()
    assert np.isnan(got.features[2, 0, :6]).all() and list(got.features[2, 0, 6:]) == [0.36, 1.0, -0.6, -1.0, -1.0, -0.6]
    assert np.allclose(got.features[0, 0, :4], [0.0, 0.0, 1.0, 0.0], atol=1e-14)
    # all-equal abscissae: the normal matrix is singular, the fit refused for D >= 1 and plain for D = 0
    same = curves_host(y, None, np.full(6, 0.7), 0.0, 1.0, 1)
    assert curve_normal_refused(np.full(6, 0.7), 1) and not curve_normal_refused(np.full(6, 0.7), 0) and not curve_normal_refused(x, 3)
    assert np.isnan(same.features[0, 0, :6]).all() and list(same.features[0, 0, 8:]) == [0.7] * 4 and same.count[0, 0] == 6
    assert np.isclose(curves_host(y, None, np.full(6, 0.7), 0.0, 1.0, 0).features[0, 0, 0], np.mean(x ** 2))
    # a NaN or an infinite abscissa is a step that is not used
    holes = x.copy()
    holes[[0, 5]] = np.nan, np.inf
    assert curves_host(y, None, holes, 0.0, 1.0, 1).count[0, 0] == 4
    # S = 1: D = 0 fits, higher degrees do not; no geometry at all
    one = y[:, :1]
    assert list(curves_host(one, None, x[:1], 0.0, 1.0, 0).features[0, 0, :6]) == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    high = curves_host(one, None, x[:1], 0.0, 1.0, 1)
    assert np.isnan(high.features[0, 0, :6]).all() and list(high.features[0, 0, 6:]) == [1.0, 1.0, -1.0, -1.0, -1.0, -1.0]
    none = curves_host(y[:0], None, x, 0.0, 1.0, 2)
    assert none.features.shape == (0, 3, 12) and none.count.shape == (0, 3) and none.table().shape == (0, 36)


MESSAGES = [
    (dict(degree=4), "okx_ensemble_curves: degree 4, 0 to 3 allowed"),
    (dict(degree=-1), "okx_ensemble_curves: degree -1, 0 to 3 allowed"),
    (dict(scale=0.0), "okx_ensemble_curves: scale is 0, not finite and > 0"),
    (dict(scale=float("inf")), "okx_ensemble_curves: scale is inf, not finite and > 0"),
    (dict(scale=float("nan")), "okx_ensemble_curves: scale is nan, not finite and > 0"),
    (dict(origin=float("nan")), "okx_ensemble_curves: origin is NaN"),
    (dict(window=(float("nan"), 1.0)), "okx_ensemble_curves: window is NaN"),
    (dict(window=(2.0, 1.0)), r"okx_ensemble_curves: window has lo > hi \(2 > 1\)"),
    (dict(abscissa=3), r"okx_ensemble_curves: abscissa column 3, outside \[0, 3\)"),
    (dict(abscissa=-1), r"okx_ensemble_curves: abscissa column -1, outside \[0, 3\)"),
    (dict(abscissa=np.zeros(5)), "okx_ensemble_curves: shared abscissa of 5 values, 6 steps"),
    (dict(abscissa=None), "okx_ensemble_curves: abscissa is needed"),
]


@pytest.mark.parametrize("change,message", MESSAGES)
def test_every_message_of_check_curve_arguments(change, message):
    kw = dict(abscissa=np.zeros(6), origin=0.0, scale=1.0, degree=2, window=None)
    kw.update(change)
    with pytest.raises(ValueError, match=message):
        check_curve_arguments(kw["abscissa"], kw["origin"], kw["scale"], kw["degree"], kw["window"], 6, 3)
    with pytest.raises(ValueError, match=message):
        curves_host(np.zeros((2, 6, 3)), None, kw["abscissa"], kw["origin"], kw["scale"], kw["degree"], kw["window"])


def test_the_header_and_the_library_agree_with_the_host():
    """OKX_CURVE_FIELDS of include/okx.h, and okx_ensemble_curves_check's words (it needs no GPU) against check_curve_arguments'."""
    import ctypes as C
    import re

    from open_kinematics_amd import _lib

    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        assert int(re.search(r"#define OKX_CURVE_FIELDS (\d+)", fh.read()).group(1)) == CURVE_FIELDS
    lib = _lib.load()
    inf = float("inf")
    assert lib.okx_ensemble_curves_check(6, 3, 6, 0, 0.0, 1.0, -inf, inf, 2) == 0 and lib.okx_ensemble_curves_check(6, 3, -1, 2, 0.0, 1.0, 1.0, 1.0, 0) == 0
    for change, message in MESSAGES[:-1]:  # (the last one is Python's: a missing argument)
        kw = dict(abscissa=np.zeros(6), origin=0.0, scale=1.0, degree=2, window=(-inf, inf))
        kw.update(change)
        shared = not isinstance(kw["abscissa"], int)
        rc = lib.okx_ensemble_curves_check(6, 3, len(kw["abscissa"]) if shared else -1, 0 if shared else kw["abscissa"], kw["origin"], kw["scale"],
                                           kw["window"][0], kw["window"][1], kw["degree"])
        assert rc == -1 and re.search(message, _lib.last_error()), (change, _lib.last_error())
    assert isinstance(lib.okx_ensemble_curves, C._CFuncPtr)


def test_accepted_arguments_come_back_normalised():
    x, kx, origin, scale, lo, hi, degree = check_curve_arguments([0, 1, 2], 1, 2, 3, None, 3, 2)
    assert x.dtype == np.float64 and list(x) == [0.0, 1.0, 2.0] and (kx, origin, scale, lo, hi, degree) == (-1, 1.0, 2.0, -np.inf, np.inf, 3)
    assert check_curve_arguments(np.int64(1), 0.0, 1.0, 0, (1.0, 1.0), 3, 2) == (None, 1, 0.0, 1.0, 1.0, 1.0, 0)


def test_random_cases_hold_their_own_bound():
    """``curves_host`` compared with itself: what the GPU test's inputs contain - rows without a used step, short rows, refused
    fits, more than nine fitted rows in ten - and that the generator's normal matrices stay well conditioned."""
    totals = np.zeros(5, dtype=np.int64)
    for seed, (s, k, column, window) in enumerate([(65, 5, True, False), (64, 4, False, True), (63, 2, True, True), (257, 1, False, False)]):
        case = random_case(s, k, 37, 40 + seed, column=column, window=window)
        values, status, abscissa, origin, scale, win = case
        got = curves_host(values, status, abscissa, origin, scale, 3, win)
        worst, *tally = compare_with_host(got, values, status, abscissa, origin, scale, 3, win)
        assert worst == 0.0
        totals += tally
    empty, short, refused, fitted, rows = totals
    assert empty > 0 and short > 0 and refused > 0 and fitted > 0.9 * rows


# ---- the Curves stage on a CPU ensemble ----

CURVES = dict(abscissa=1, origin=0.5, scale=4.0, degree=2, window=(-20.0, 20.0))
STEPS = 6


def _tables(answer) -> dict:
    import dataclasses

    return {f.name: getattr(answer, f.name) for f in dataclasses.fields(answer)}


def _curves_ensemble(n_geom: int, chunks: int, factors="hardpoints"):
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs
    from test_ensemble_stages import _program

    table, relative = _ensemble_inputs(n_geom, STEPS)
    pipe = ShardedEnsemble(_program(), table, relative, STEPS, chunks=chunks, metric_columns=COLUMNS, reduce=True, factors=factors, curves=CURVES)
    pipe.step()
    pipe.step()  # a second step starts from nothing
    return pipe


def _one_process_table(n_geom: int):
    """``(values [G, S, K], status [G, S])`` of the gathered table of the same ensemble in one process."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, STEPS)
    plain = ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS)
    full = plain.step()
    return full.numpy().reshape(n_geom, STEPS, len(COLUMNS)), plain.status_full.numpy().reshape(n_geom, STEPS)


def _same_bits(a: dict, b: dict) -> bool:
    from test_ensemble_stages import same_bits

    return same_bits(a, b)


def test_the_stage_in_one_process():
    n_geom = 5
    values, status = _one_process_table(n_geom)
    want = curves_host(values, status, **CURVES)
    assert (want.count > 2).any() and np.isfinite(want.features[..., 1]).any()
    answers = []
    for chunks in (1, 2):
        pipe = _curves_ensemble(n_geom, chunks)
        local = pipe.curves_local()
        assert np.array_equal(bits(local.features.numpy()), bits(want.features)) and np.array_equal(local.count.numpy(), want.count)
        assert pipe.curves_exchange_bytes_per_rank == 0
        # the shift is the feature row of the reduction's shift table (geometry 0's rows, undefined entries 0)
        shift = pipe.accumulator.shift.numpy()
        nominal = np.nan_to_num(curves_host(shift[None], None, **CURVES).table(), nan=0.0, posinf=0.0, neginf=0.0)
        stage = pipe.stages["curves"]
        assert np.array_equal(bits(stage.acc.shift.numpy()), bits(nominal))
        whole = reduce_host(want.table()[:, None, :], None, pipe.stages["reduce"].all_factors, nominal, 0, pipe.factor_names)
        assert _same_bits(_tables(pipe.curve_stats()), _tables(whole.finalize())), chunks
        answers.append(_tables(pipe.curve_stats()))
    assert _same_bits(answers[0], answers[1])
    stats = answers[0]
    assert stats["count"].shape == (1, len(COLUMNS) * CURVE_FIELDS) and stats["sensitivity"].shape == (1, len(COLUMNS) * CURVE_FIELDS, 3)
    with pytest.raises(ValueError, match="needs reduce=True"):
        from open_kinematics_amd.dist import ShardedEnsemble
        from test_dist import _ensemble_inputs

        ShardedEnsemble(_stand_in(), *_ensemble_inputs(2, STEPS), STEPS, metric_columns=COLUMNS, curves=CURVES)
    with pytest.raises(ValueError, match="abscissa column 9"):
        ShardedEnsemble(_stand_in(), *_ensemble_inputs(2, STEPS), STEPS, metric_columns=COLUMNS, reduce=True, curves=dict(CURVES, abscissa=9))


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for n_geom in (5, 1):
        for chunks in (1, 2):
            pipe = _curves_ensemble(n_geom, chunks)
            local = pipe.curves_local()
            out[n_geom, chunks] = {"range": pipe.geometry_range, "stats": _tables(pipe.curve_stats()), "features": local.features.clone(),
                                   "count": local.count.clone(), "sent": pipe.curves_exchange_bytes_per_rank, "n_factors": pipe.n_factors,
                                   "shift": pipe.stages["curves"].acc.shift.clone(), "factors": pipe.stages["reduce"].all_factors,
                                   "names": pipe.factor_names}
    torch.save(out, os.path.join(out_dir, f"curves{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_one_process_bits(tmp_path):
    """Five geometries shard 3 + 2; one geometry leaves rank 1 without any, and it still joins the all-gather.  Every rank reduces
    the gathered feature table, so curve_stats() is reduce_host of curves_host(...).table() of the one-process table bit for bit,
    on both ranks and with one chunk or two."""
    world = 2
    port = 35300 + (os.getpid() + 29 * world) % 2000
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"curves{r}.pt"), weights_only=False) for r in range(world)]
    k = len(COLUMNS)
    for n_geom in (5, 1):
        values, status = _one_process_table(n_geom)
        want = curves_host(values, status, **CURVES)
        for chunks in (1, 2):
            one, two = got[0][n_geom, chunks], got[1][n_geom, chunks]
            assert (one["range"], two["range"]) == ({5: (0, 3), 1: (0, 1)}[n_geom], {5: (3, 5), 1: (1, 1)}[n_geom])
            whole = reduce_host(want.table()[:, None, :], None, one["factors"], one["shift"].numpy(), 0, one["names"]).finalize()
            for rank in (one, two):
                lo, hi = rank["range"]
                assert np.array_equal(bits(rank["features"].numpy()), bits(want.features[lo:hi])) and np.array_equal(rank["count"].numpy(), want.count[lo:hi])
                assert _same_bits(rank["stats"], _tables(whole)), (n_geom, chunks)
                assert rank["sent"] == 8 * {5: 3, 1: 1}[n_geom] * k * CURVE_FIELDS and rank["n_factors"] == (3 if n_geom == 5 else 0)
            assert (whole.count[0] > 0).any() and (whole.rejected[0] > 0).any() == bool(np.isnan(want.table()).any())
