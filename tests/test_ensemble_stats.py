"""
CPU: the ensemble statistics (open_kinematics_amd/ensemble_stats.py) against the statistics the fixture generator took
from the REFERENCE's metrics of 64 perturbed geometries x 9 steps (tests/golden/ensemble_stats_dw.npz, math.fsum / exact
comparisons / numpy.linalg.lstsq), merging of partial accumulators, and ShardedEnsemble(reduce=True) over gloo ranks.

Every tolerance is derived here from the summation order and the number format (u = 2^-53), never from an outcome:

  a sum of n terms t_i added one after the other:      |fl(sum) - sum| <= n u sum|t_i|            (Higham, Accuracy and
                                                                                                   Stability, eq. 4.4, to first order)
  S1 = sum d:            E1 = n u sum|d|
  S2 = sum d^2:          E2 = (n + 1) u sum d^2     (one more rounding: the product, or none with an fma)
  mean = shift + S1 / n: E1 / n + 4 u (|shift| + |S1 / n|)       (the division, the addition, and the reference mean's own two)
  variance = (S2 - S1^2 / n) / (n - 1):
                         (E2 + 2 |S1| E1 / n + 8 u (S2 + S1^2 / n)) / (n - 1) + 8 u variance
                         (propagated through the formula; the last terms: the roundings of the formula itself and of the
                          generator's own sum of squared deviations)
  slopes (normal equations of the accumulated moments against lstsq): the Gram matrix and the right-hand sides are sums of
  G terms (relative error G u each), the solve adds (P + 1) u, and an error e of the normal equations' data moves their
  solution by cond(A^T A) e = cond(A)^2 e:   2 (G + P + 1) cond^2 u ||coefficients||_2   per entry, with
  cond = cond([1 | factors]) as the fixture stores it and the coefficients those of the shifted problem.

Two of these depart from the wording of the issue that asked for the feature, and are named here for that reason:
  * the issue words the slope bound as "cond^2 u times the slope scale".  That figure has no room for the G-term sums the
    normal equations are built from (each carries a relative error of up to G u before cond^2 amplifies it), so it cannot be
    met by ANY normal-equations solution of accumulated moments; the bound above is the issue's figure times the dimension
    factor 2 (G + P + 1) that the accumulation and the solve contribute, derived before anything was run.
  * where one accumulator is compared with ANOTHER accumulator (a merged one with the single run, the device's with
    NumPy's) the bound is 2 E: each is a rounding of the same exact sum and within E of it, so within 2 E of each other.
    Against the generator's fsum value (exact to one rounding) the bound is E itself.
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, REPO
from open_kinematics_amd.ensemble_stats import (ENS_ARGMAX, ENS_ARGMIN, ENS_COUNT, ENS_FIELDS, ENS_MAX, ENS_MIN, ENS_REJECTED,
                                                ENS_SUM, ENS_SUMSQ, EnsembleAccumulator, hardpoint_factors, reduce_host)

U = 2.0 ** -53


def load_fixture():
    fx = dict(np.load(os.path.join(GOLDEN, "ensemble_stats_dw.npz"), allow_pickle=False))
    fx["table"] = np.concatenate([fx["values"], fx["deriv"]], axis=2)  # [G, S, 15]
    return fx


def sum_bounds(values, ok, shift):
    """(E1, E2) of the accumulated sums over the accepted entries of ``values [G, S, K]``."""
    d = np.where(ok, values - shift[None], 0.0)
    n = values.shape[0]
    return n * U * np.abs(d).sum(axis=0), (n + 1) * U * (d * d).sum(axis=0)


def check_against_generator(acc: EnsembleAccumulator, fx, *, eps_shift_exact=True):
    """An accumulator of the fixture's table against the generator's statistics: the bounds of the module docstring."""
    table = fx["table"]
    g, s, k = table.shape
    a = acc.numpy().acc
    ok = np.ones(table.shape, dtype=bool)
    e1, e2 = sum_bounds(table, ok, fx["stat_shift"])
    assert np.array_equal(acc.numpy().shift, fx["stat_shift"])
    assert np.array_equal(a[..., ENS_COUNT], fx["stat_count"]) and np.all(a[..., ENS_REJECTED] == 0)
    assert np.array_equal(a[..., ENS_MIN], fx["stat_min"]) and np.array_equal(a[..., ENS_MAX], fx["stat_max"])
    assert np.array_equal(a[..., ENS_ARGMIN], fx["stat_argmin"]) and np.array_equal(a[..., ENS_ARGMAX], fx["stat_argmax"])
    assert np.all(np.abs(a[..., ENS_SUM] - fx["stat_sum_d"]) <= e1)
    assert np.all(np.abs(a[..., ENS_SUMSQ] - fx["stat_sumsq_d"]) <= e2)
    st = acc.finalize()
    s1, s2 = np.abs(fx["stat_sum_d"]), fx["stat_sumsq_d"]
    tol_mean = e1 / g + 4 * U * (np.abs(fx["stat_shift"]) + s1 / g)
    assert np.all(np.abs(st.mean - fx["stat_mean"]) <= tol_mean)
    tol_var = (e2 + 2 * s1 * e1 / g + 8 * U * (s2 + s1 * s1 / g)) / (g - 1) + 8 * U * fx["stat_variance"]
    assert np.all(np.abs(st.variance - fx["stat_variance"]) <= tol_var)
    assert np.array_equal(st.count, fx["stat_count"]) and np.array_equal(st.argmin, fx["stat_argmin"]) and np.array_equal(st.argmax, fx["stat_argmax"])
    assert np.array_equal(st.min, fx["stat_min"]) and np.array_equal(st.max, fx["stat_max"])
    return st


def check_fit_against_lstsq(st, fx):
    g, p = fx["factors"].shape
    cond = float(fx["cond"])
    coef = np.concatenate([(fx["stat_intercept"] - fx["stat_shift"])[..., None], fx["stat_sensitivity"]], axis=2)
    tol = 2 * (g + p + 1) * cond ** 2 * U * np.linalg.norm(coef, axis=2)
    assert np.all(np.abs(st.sensitivity - fx["stat_sensitivity"]) <= tol[..., None])
    assert np.all(np.abs(st.intercept - fx["stat_intercept"]) <= tol + 4 * U * np.abs(fx["stat_intercept"]))
    assert np.all(np.abs(st.r2 - fx["stat_r2"]) <= 1e-9)  # (1 - small / large in the generator: R^2 is a report, not pinned tighter)


def test_reduce_host_reproduces_the_reference_statistics():
    fx = load_fixture()
    acc = reduce_host(fx["table"], None, fx["factors"], None, 0, [str(n) for n in fx["factor_names"]])
    st = check_against_generator(acc, fx)
    check_fit_against_lstsq(st, fx)
    assert st.factor_names == [str(n) for n in fx["factor_names"]]
    # the factor moments are the unmasked ones
    p = fx["factors"].shape[1]
    fa = acc.factor_acc
    assert fa[-1] == 64 and np.allclose(fa[:p], fx["factors"].sum(axis=0), atol=64 * U * np.abs(fx["factors"]).sum(axis=0).max())


def tampered_fixture(fx, seed=3):
    """The fixture's table with NaN values, rejected status bytes, one whole step rejected and ties at the extremes."""
    rng = np.random.default_rng(seed)
    table = fx["table"].copy()
    g, s, k = table.shape
    status = np.ones((g, s), dtype=np.uint8)
    status[rng.integers(0, g, 40), rng.integers(0, s, 40)] = rng.choice(np.array([0, 3, 5, 9 + 2, 4], dtype=np.uint8), 40)
    status[rng.integers(0, g, 10), rng.integers(0, s, 10)] = 9  # converged + ill-conditioned (advisory): still accepted
    status[:, 4] = 0                                             # a whole step rejected
    idx = (rng.integers(0, g, 60), rng.integers(0, s, 60), rng.integers(0, k, 60))
    table[idx] = np.nan
    table[5, 2, 3] = np.inf
    # ties: the extreme of a column planted a second and third time at other geometries (status kept accepted there)
    for step, col in ((0, 0), (7, 9), (3, 14)):
        column = np.where(np.isfinite(table[:, step, col]) & ((status[:, step] & 7) == 1), table[:, step, col], np.nan)
        lo, hi = np.nanmin(column), np.nanmax(column)
        for where, v in ((11, lo), (50, lo), (23, hi), (61, hi)):
            table[where, step, col] = v
            status[where, step] = 1
    return table, status


def expected_extremes(table, status):
    ok = np.isfinite(table) & ((status & 7) == 1)[:, :, None]
    lo, hi = np.where(ok, table, np.inf), np.where(ok, table, -np.inf)
    some = ok.any(axis=0)
    return ok, lo.min(axis=0), hi.max(axis=0), np.where(some, lo.argmin(axis=0), -1), np.where(some, hi.argmax(axis=0), -1)


def check_same_accumulator(got: EnsembleAccumulator, want: EnsembleAccumulator, e1, e2, fe=None):
    a, b = got.numpy().acc, want.numpy().acc
    for f in (ENS_COUNT, ENS_REJECTED, ENS_MIN, ENS_MAX, ENS_ARGMIN, ENS_ARGMAX):
        assert np.array_equal(a[..., f], b[..., f]), f
    # (both are roundings of the same exact sum: each within the bound of it, so within twice the bound of each other)
    assert np.all(np.abs(a[..., ENS_SUM] - b[..., ENS_SUM]) <= 2 * e1)
    assert np.all(np.abs(a[..., ENS_SUMSQ] - b[..., ENS_SUMSQ]) <= 2 * e2)
    if fe is not None:
        assert np.all(np.abs(a[..., ENS_FIELDS:] - b[..., ENS_FIELDS:]) <= 2 * fe)


def cross_bound(table, ok, shift, factors):
    d = np.where(ok, table - shift[None], 0.0)
    return (table.shape[0] + 1) * U * np.einsum("gsk,gp->skp", np.abs(d), np.abs(factors))


@pytest.mark.parametrize("runs", [1, 2, 3, 7, 64])
def test_partial_accumulators_merge_to_the_single_run(runs):
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    g = table.shape[0]
    shift = fx["stat_shift"]
    whole = reduce_host(table, status, fx["factors"], shift, 0)
    ok, lo, hi, amin, amax = expected_extremes(table, status)
    a = whole.acc
    assert np.array_equal(a[..., ENS_COUNT], ok.sum(axis=0)) and np.array_equal(a[..., ENS_REJECTED], g - ok.sum(axis=0))
    assert np.array_equal(a[..., ENS_MIN], lo) and np.array_equal(a[..., ENS_MAX], hi)
    assert np.array_equal(a[..., ENS_ARGMIN], amin) and np.array_equal(a[..., ENS_ARGMAX], amax)
    assert amin[0, 0] == min(11, amin[0, 0]) and amin[0, 0] <= 11 and amax[0, 0] <= 23  # ties went to the lowest index
    edges = np.linspace(0, g, runs + 1).round().astype(int)
    merged = None
    for lo_g, hi_g in zip(edges[:-1], edges[1:]):
        part = reduce_host(table[lo_g:hi_g], status[lo_g:hi_g], fx["factors"][lo_g:hi_g], shift, int(lo_g))
        merged = part if merged is None else merged.merge(part)
    e1, e2 = sum_bounds(table, ok, shift)
    check_same_accumulator(merged, whole, e1, e2, cross_bound(table, ok, shift, fx["factors"]))
    assert np.allclose(merged.factor_acc, whole.factor_acc, rtol=0, atol=2 * 65 * U * np.abs(whole.factor_acc).max())
    st = merged.finalize()
    # the rejected step: nothing counts
    assert np.all(st.count[4] == 0) and np.all(st.rejected[4] == g)
    assert np.all(np.isnan(st.mean[4])) and np.all(np.isnan(st.min[4])) and np.all(np.isnan(st.max[4])) and np.all(np.isnan(st.variance[4]))
    assert np.all(st.argmin[4] == -1) and np.all(st.argmax[4] == -1)
    # sensitivities only where nothing was rejected
    assert np.array_equal(np.isnan(st.sensitivity[..., 0]), st.rejected != 0)
    # merging in torch gives what merging in NumPy gives
    both = whole.to("cpu").merge(EnsembleAccumulator.empty(9, 15, 30, shift).to("cpu"))
    assert np.array_equal(both.numpy().acc, whole.acc)
    with pytest.raises(ValueError, match="different shifts"):
        whole.merge(reduce_host(table, status, fx["factors"], shift + 1.0, 0))


def test_finalize_edge_cases_and_rank_deficiency():
    fx = load_fixture()
    one = reduce_host(fx["table"][:1])
    st = one.finalize()
    assert np.all(st.count == 1) and np.all(np.isnan(st.variance)) and np.array_equal(st.mean, fx["table"][0])
    twice = np.concatenate([fx["factors"], fx["factors"][:, :1]], axis=1)  # a repeated column: rank 30 of 31 + intercept
    with pytest.raises(ValueError, match="rank 31 of 32"):
        reduce_host(fx["table"], None, twice).finalize()
    # a shift entry that is undefined is replaced by 0
    table = fx["table"].copy()
    table[0, 0, 0] = np.nan
    assert reduce_host(table).shift[0, 0] == 0.0
    # factors="hardpoints": the perturbations of the authored points, centred
    names = [str(n) for n in fx["prog_point_names"]]
    derived = set(int(i) for i in fx["prog_dop_out"])
    authored = [i for i in range(len(names)) if i not in derived]
    f, fnames = hardpoint_factors(fx["hardpoints"][:, authored], [names[i].lower() for i in authored])
    want = dict(zip((str(n) for n in fx["factor_names"]), (fx["factors"] - fx["factors"].mean(axis=0)).T))
    assert len(fnames) == 30 and sorted(fnames) == sorted(want)
    for j, n in enumerate(fnames):
        assert np.max(np.abs(f[:, j] - want[n])) <= 1e-12, n


# ---- ShardedEnsemble(reduce=True) over gloo ranks, a stand-in program (tests/test_dist.py) ----

COLUMNS = [(3, None), (0, 0), (23, 0), (7, None)]


def _stand_in():
    """tests/test_dist.py's stand-in program with status bytes that accept most states and reject some."""
    from test_dist import _StandInProgram

    class _Program(_StandInProgram):
        def solve(self, targets, **kw):
            res = super().solve(targets, **kw)
            res.info_raw[:, 32] = torch.where((targets[:, 0].abs() * 7).to(torch.int64) % 4 == 0, 2, 1).to(torch.uint8)
            return res

    return _Program()


def _reduce_worker(rank: int, world: int, port: int, n_geom: int, steps: int, chunks: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, steps)
    factors = torch.randn((n_geom, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    pipe = ShardedEnsemble(_stand_in(), table, relative, steps, chunks=chunks, metric_columns=COLUMNS, reduce=True, factors=factors)
    acc = pipe.step()
    again = pipe.step()  # a second step starts from nothing
    plain = ShardedEnsemble(_stand_in(), table, relative, steps, chunks=chunks, metric_columns=COLUMNS)
    gathered = plain.step().clone()
    torch.save({"acc": acc.acc.clone(), "factor_acc": acc.factor_acc.clone(), "shift": acc.shift.clone(), "again": again.acc.clone(),
                "sent": pipe.exchange_bytes_per_rank, "groups": pipe.p2p_groups, "range": pipe.geometry_range,
                "no_table": pipe.metric_full is None and pipe.status_full is None,
                "metric_full": gathered, "status_full": plain.status_full.clone(), "plain_sent": plain.exchange_bytes_per_rank},
               os.path.join(out_dir, f"reduce{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_geom,chunks", [(2, 6, 2), (2, 7, 3), (3, 7, 2), (3, 2, 1)])
def test_sharded_reduction_gives_every_rank_the_same_bits(tmp_path, world, n_geom, chunks):
    """Even and ragged geometry counts, a rank without a geometry ((3, 2)): every rank ends with the same accumulator bits, equal
    to the one-process reduction of the gathered table within the summation bound; reduce=False is what it was."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    steps = 4
    port = 33500 + (os.getpid() + 7 * world + n_geom) % 2000
    mp.spawn(_reduce_worker, args=(world, port, n_geom, steps, chunks, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"reduce{r}.pt")) for r in range(world)]
    for r in range(1, world):
        for key in ("acc", "factor_acc", "shift", "again", "metric_full", "status_full"):
            assert torch.equal(torch.nan_to_num(got[0][key]), torch.nan_to_num(got[r][key])), (key, r)
    assert torch.equal(got[0]["acc"], got[0]["again"])
    assert all(g["no_table"] and g["groups"] == 0 for g in got)
    k = len(COLUMNS)
    assert all(g["sent"] == 8 * (steps * k * (ENS_FIELDS + 3) + 3 + 6 + 1) for g in got)
    # one process, no collective: reduce=False unchanged, reduce=True the same answer
    table, relative = _ensemble_inputs(n_geom, steps)
    factors = torch.randn((n_geom, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    alone = ShardedEnsemble(_stand_in(), table, relative, steps, metric_columns=COLUMNS)
    full = alone.step()
    assert torch.equal(full, got[0]["metric_full"]) and torch.equal(alone.status_full, got[0]["status_full"])
    lo, hi = got[0]["range"]
    assert got[0]["plain_sent"] == (hi - lo) * steps * (8 * k + 1)
    values = full.numpy().reshape(n_geom, steps, k)
    status = alone.status_full.numpy().reshape(n_geom, steps)
    shift = got[0]["shift"].numpy()
    assert np.array_equal(shift, np.nan_to_num(values[0]))  # geometry 0's evaluation, broadcast from rank 0
    want = reduce_host(values, status, factors.numpy(), shift, 0)
    ok = np.isfinite(values) & ((status & 7) == 1)[:, :, None]
    assert 0 < ok.sum() < ok.size  # the stand-in's status bytes accept some states and reject others
    e1, e2 = sum_bounds(values, ok, shift)
    check_same_accumulator(EnsembleAccumulator(got[0]["acc"].numpy(), shift), want, e1, e2, cross_bound(values, ok, shift, factors.numpy()))
    assert np.allclose(got[0]["factor_acc"].numpy(), want.factor_acc, rtol=0, atol=2 * (n_geom + 1) * U * np.abs(want.factor_acc).max())
    single = ShardedEnsemble(_stand_in(), table, relative, steps, metric_columns=COLUMNS, reduce=True, factors=factors)
    check_same_accumulator(single.step(), want, e1, e2, cross_bound(values, ok, shift, factors.numpy()))
    assert single.exchange_bytes_per_rank == 0
    if n_geom >= 5:
        assert single.stats().count.shape == (steps, k) and single.stats().sensitivity.shape == (steps, k, 3)
    else:  # two geometries cannot carry three slopes and an intercept
        with pytest.raises(ValueError, match="rank-deficient: rank 2 of 4"):
            single.stats()
    with pytest.raises(ValueError, match="needs metric_columns"):
        ShardedEnsemble(_stand_in(), table, relative, steps, reduce=True)
