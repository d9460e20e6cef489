"""
CPU: ensemble quantiles and spec-limit yield (open_kinematics_amd/ensemble_stats.py: select_host, the NumPy twins of the
device's count / descend rounds) on the REFERENCE's metric values of 64 perturbed geometries x 9 steps
(tests/golden/ensemble_stats_dw.npz), on a tampered copy, on hand-made columns, in chunks, and through
ShardedEnsemble(reduce=True, quantiles=...) over gloo ranks.

Order statistics and counts are integers' work: every comparison of them is exact (array_equal).  One bound, for the
interpolated quantile against numpy.quantile(..., method="linear"), u = 2^-53:

  q = x_lo + t (x_hi - x_lo), t = h - floor(h) in [0, 1) exact (h < 2^52 and its floor are doubles, their difference is one)
  evaluated:  d = fl(x_hi - x_lo)            |d - (x_hi - x_lo)| <= u (|x_lo| + |x_hi|)
              m = fl(t d)                    |m - t d| <= u |t d| <= u (|x_lo| + |x_hi|)
              q = fl(x_lo + m)               |q - (x_lo + m)| <= u (|x_lo| + |m|) <= u (|x_lo| + |x_hi|) to first order
  so each evaluation lies within 3 u (|x_lo| + |x_hi|) of the exact interpolant - NumPy's own (it evaluates the same three
  operations, from the other end for t >= 0.5) as well as this module's - and the two within 6 u (|x_lo| + |x_hi|) of each
  other.  This is the bound the issue that asked for the feature states; nothing here departs from it.
"""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from open_kinematics_amd import ensemble_stats as es
from open_kinematics_amd.ensemble_stats import (ENS_MAX, ENS_MIN, SELECT_BINS, SELECT_BITS, SELECT_ROUNDS, reduce_host, select_host,
                                                select_rounds_host)
from test_ensemble_stats import COLUMNS, _stand_in, load_fixture, tampered_fixture

U = 2.0 ** -53
PROBS = (0.0, 0.00135, 0.25, 0.5, 0.75, 0.99865, 1.0)
FIELDS = ("count", "lower", "upper", "quantile", "below", "above", "yield_")


def same(a, b, fields=FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f


def by_sort(values, status, probs):
    """lower / upper / count by indexing np.sort, entry by entry - the definition."""
    g, s, k = values.shape
    lower = np.full((s, k, len(probs)), np.nan)
    upper = lower.copy()
    count = np.zeros((s, k), dtype=np.int64)
    for i in range(s):
        for j in range(k):
            ok = np.isfinite(values[:, i, j]) & (np.ones(g, dtype=bool) if status is None else (status[:, i] & 7) == 1)
            x = np.sort(values[ok, i, j])
            count[i, j] = x.size
            for q, p in enumerate(probs):
                if x.size:
                    h = (x.size - 1) * p
                    lower[i, j, q], upper[i, j, q] = x[int(np.floor(h))], x[int(np.ceil(h))]
    return count, lower, upper


def check_exact(got, values, status, probs, limits=None):
    count, lower, upper = by_sort(values, status, probs)
    assert np.array_equal(got.count, count)
    assert np.array_equal(got.lower, lower, equal_nan=True) and np.array_equal(got.upper, upper, equal_nan=True)
    if limits is not None:
        ok = np.isfinite(values) & (True if status is None else ((status & 7) == 1)[:, :, None])
        lim = np.broadcast_to(limits, values.shape[1:] + (2,))
        assert np.array_equal(got.below, (ok & (values < lim[None, ..., 0])).sum(axis=0))
        assert np.array_equal(got.above, (ok & (values > lim[None, ..., 1])).sum(axis=0))
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.where(count > 0, 1.0 - (got.below + got.above) / count, np.nan)
        assert np.array_equal(got.yield_, want, equal_nan=True)


def hand_made_columns():
    """[37, 1, 6]: lowest key bit only | signs around +-0.0 | denormals next to 1e300 | all equal | wide integers | a tie-heavy column."""
    g = 37
    rng = np.random.default_rng(11)
    cols = np.zeros((g, 1, 6))
    base = np.float64(1.5).view(np.uint64)
    cols[:, 0, 0] = (base + rng.integers(0, 2, g).astype(np.uint64)).view(np.float64)
    cols[:, 0, 1] = rng.choice(np.array([-0.0, 0.0, -5e-324, 5e-324, -1.0, 1.0, -2.5e-310, 2.5e-310]), g)
    cols[:, 0, 2] = rng.choice(np.array([5e-324, 1e-310, 2.2e-308, 1e300, -1e300, 9.9e299, -5e-324]), g)
    cols[:, 0, 3] = -7.25
    cols[:, 0, 4] = rng.integers(-2 ** 40, 2 ** 40, g).astype(np.float64)
    cols[:, 0, 5] = rng.integers(0, 3, g).astype(np.float64)
    return cols


def test_reference_values_against_sort_and_numpy_quantile():
    fx = load_fixture()
    table = fx["table"]
    direct = select_host(table, None, PROBS)
    rounds = select_rounds_host(table, None, PROBS)
    same(direct, rounds)
    check_exact(direct, table, None, PROBS)
    assert np.array_equal(direct.lower[..., 0], fx["stat_min"]) and np.array_equal(direct.upper[..., 0], fx["stat_min"])
    assert np.array_equal(direct.lower[..., -1], fx["stat_max"]) and np.array_equal(direct.upper[..., -1], fx["stat_max"])
    acc = reduce_host(table).acc
    assert np.array_equal(direct.quantile[..., 0], acc[..., ENS_MIN]) and np.array_equal(direct.quantile[..., -1], acc[..., ENS_MAX])
    want = np.moveaxis(np.quantile(table, PROBS, axis=0, method="linear"), 0, 2)
    bound = 6 * U * (np.abs(direct.lower) + np.abs(direct.upper))
    err = np.abs(direct.quantile - want)
    print("quantile vs numpy.quantile: worst error / bound =", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


def test_tampered_table():
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    limits = np.stack([np.nanquantile(fx["table"], 0.1, axis=0), np.nanquantile(fx["table"], 0.8, axis=0)], axis=2)
    direct = select_host(table, status, PROBS, limits)
    same(direct, select_rounds_host(table, status, PROBS, limits))
    check_exact(direct, table, status, PROBS, limits)
    assert np.all(direct.count[4] == 0) and np.all(np.isnan(direct.lower[4])) and np.all(np.isnan(direct.quantile[4])) and np.all(np.isnan(direct.yield_[4]))
    assert 0 < direct.count[0, 0] < 64
    for step, col in ((0, 0), (7, 9), (3, 14)):  # the planted ties: three states hold each extreme
        assert direct.lower[step, col, 0] == direct.upper[step, col, 1] == direct.lower[step, col, 1]
        assert direct.upper[step, col, -1] == direct.lower[step, col, -2] == direct.upper[step, col, -2]


@pytest.mark.parametrize("g", [37, 2, 1])
def test_hand_made_columns(g):
    cols = hand_made_columns()[:g]
    status = np.ones((g, 1), dtype=np.uint8)
    if g == 37:
        status[[3, 30]] = 2
    got = select_rounds_host(cols, status, PROBS)
    same(got, select_host(cols, status, PROBS))
    check_exact(got, cols, status, PROBS)
    assert np.all(got.lower[0, 3] == -7.25) and np.all(got.quantile[0, 3] == -7.25)
    empty = select_rounds_host(cols[:0], None, PROBS, limits=(-1.0, 1.0))  # G = 0 is legal
    same(empty, select_host(cols[:0], None, PROBS, limits=(-1.0, 1.0)))
    assert np.all(empty.count == 0) and np.all(np.isnan(empty.lower)) and np.all(empty.below == 0) and np.all(np.isnan(empty.yield_))


def test_limits():
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    g, s, k = table.shape
    limits = np.empty((s, k, 2))
    limits[..., 0], limits[..., 1] = table[7], table[20]  # limits EQUAL to table values: strictly below / above
    swap = limits[..., 0] > limits[..., 1]
    limits[swap] = limits[swap][:, ::-1]
    limits[np.isnan(limits[..., 0]) | np.isinf(limits[..., 0]), 0] = -np.inf
    limits[np.isnan(limits[..., 1]) | np.isinf(limits[..., 1]), 1] = np.inf
    limits[2, :, 0], limits[3, :, 1], limits[5] = -np.inf, np.inf, (-np.inf, np.inf)
    got = select_rounds_host(table, status, (0.5,), limits)
    same(got, select_host(table, status, (0.5,), limits))
    check_exact(got, table, status, (0.5,), limits)
    assert np.all(got.below[2] == 0) and np.all(got.above[3] == 0) and np.all(got.yield_[5][got.count[5] > 0] == 1.0)
    assert got.below.sum() > 0 and got.above.sum() > 0
    one = select_host(table, status, (0.5,), (-0.5, 0.5))  # one window for every entry
    check_exact(one, table, status, (0.5,), np.array([-0.5, 0.5]))
    assert select_host(table, status, (0.5,)).below is None


@pytest.mark.parametrize("chunks", [1, 2, 3, 7, 64])
def test_chunks_accumulate_into_one_histogram(chunks):
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    limits = (-0.25, 0.5)
    seen = []
    single = select_rounds_host(table, status, PROBS, limits, on_round=lambda rnd, hist: seen.append(hist.copy()))
    again = []
    got = select_rounds_host(table, status, PROBS, limits, chunks=chunks, on_round=lambda rnd, hist: again.append(hist.copy()))
    same(got, single)
    assert len(seen) == len(again) == SELECT_ROUNDS and all(np.array_equal(a, b) for a, b in zip(seen, again))
    assert seen[0].shape == table.shape[1:] + (2 * len(PROBS), SELECT_BINS) and not seen[0][:, :, 2:].any()


# ---- ShardedEnsemble(reduce=True, quantiles=...) over gloo ranks, the stand-in program of tests/test_dist.py ----

Q3 = (0.00135, 0.5, 0.99865, 0.0, 1.0)
WINDOW = (-0.2, 0.3)


def _select_worker(rank: int, world: int, port: int, n_geom: int, steps: int, chunks: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, steps)
    pipe = ShardedEnsemble(_stand_in(), table, relative, steps, chunks=chunks, metric_columns=COLUMNS, reduce=True, quantiles=Q3, limits=WINDOW)
    acc = pipe.step()
    q = pipe.quantiles()
    pipe.step()
    again = pipe.quantiles()
    plain = ShardedEnsemble(_stand_in(), table, relative, steps, chunks=chunks, metric_columns=COLUMNS, reduce=True)
    torch.save({"q": {f: getattr(q, f) for f in FIELDS}, "again": {f: getattr(again, f) for f in FIELDS}, "acc": acc.acc.clone(),
                "plain_acc": plain.step().acc.clone(), "sent": pipe.exchange_bytes_per_rank, "plain_sent": plain.exchange_bytes_per_rank,
                "select_sent": pipe.select_exchange_bytes_per_rank, "plain_select_sent": plain.select_exchange_bytes_per_rank},
               os.path.join(out_dir, f"select{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_geom,chunks", [(2, 6, 2), (2, 7, 3), (3, 7, 2), (3, 2, 1)])
def test_sharded_selection_gives_every_rank_the_same_bits(tmp_path, world, n_geom, chunks):
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    steps, k = 4, len(COLUMNS)
    port = 35600 + (os.getpid() + 7 * world + n_geom) % 2000
    mp.spawn(_select_worker, args=(world, port, n_geom, steps, chunks, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"select{r}.pt"), weights_only=False) for r in range(world)]
    for r in range(world):
        for f in FIELDS:
            assert np.array_equal(got[0]["q"][f], got[r]["q"][f], equal_nan=True), (f, r)
            assert np.array_equal(got[r]["q"][f], got[r]["again"][f], equal_nan=True), (f, r)
        # the accumulator and its traffic are what they are without quantiles
        assert torch.equal(got[r]["acc"], got[r]["plain_acc"]) and got[r]["sent"] == got[r]["plain_sent"] and got[r]["plain_select_sent"] == 0
        assert got[r]["select_sent"] == SELECT_ROUNDS * 8 * steps * k * 2 * len(Q3) * SELECT_BINS
    table, relative = _ensemble_inputs(n_geom, steps)
    alone = ShardedEnsemble(_stand_in(), table, relative, steps, metric_columns=COLUMNS)
    values = alone.step().numpy().reshape(n_geom, steps, k)
    status = alone.status_full.numpy().reshape(n_geom, steps)
    want = select_host(values, status, Q3, WINDOW)
    for f in FIELDS:
        assert np.array_equal(got[0]["q"][f], getattr(want, f), equal_nan=True), f
    assert 0 < want.count.sum() < values.size
    single = ShardedEnsemble(_stand_in(), table, relative, steps, metric_columns=COLUMNS, reduce=True, quantiles=Q3, limits=WINDOW)
    acc = single.step()
    same(single.quantiles(), want)
    assert single.select_exchange_bytes_per_rank == 0
    some = want.count > 0
    assert np.array_equal(single.quantiles().lower[..., 3][some], acc.acc[..., ENS_MIN].numpy()[some])
    assert np.array_equal(single.quantiles().upper[..., 4][some], acc.acc[..., ENS_MAX].numpy()[some])
    with pytest.raises(ValueError, match="need reduce=True"):
        ShardedEnsemble(_stand_in(), table, relative, steps, metric_columns=COLUMNS, quantiles=Q3)


# ---- sizes, constants and argument errors through the library (no device needed) ----

def test_sizes_constants_and_errors_through_the_library():
    from open_kinematics_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "okx.h"), encoding="utf-8").read()
    assert int(re.search(r"#define OKX_ENS_SELECT_BITS (\d+)", header).group(1)) == SELECT_BITS
    assert int(re.search(r"OKX_ENS_SELECT_MAX_PROBS = (\d+)", header).group(1)) == es.SELECT_MAX_PROBS
    assert lib.okx_ensemble_select_rounds() == SELECT_ROUNDS == 64 // SELECT_BITS
    for s, k, q in ((9, 15, 7), (256, 4, 3), (1, 1, 1)):
        words = s * k * 2 * q * SELECT_BINS
        state, hist = es.select_begin(s, k, q)
        assert lib.okx_ensemble_select_hist_len(s, k, q) == words == hist.size
        state_bytes = lib.okx_ensemble_select_state_bytes(s, k, q)
        assert state_bytes == state.prefix.nbytes + state.rank.nbytes + state.count.nbytes + state.outside.nbytes
        assert lib.okx_ensemble_select_scratch_bytes(s, k, q) == state_bytes + 8 * words
    assert lib.okx_ensemble_select_hist_len(0, 4, 3) == 0 and lib.okx_ensemble_select_scratch_bytes(9, 0, 3) == 0

    def check(probs, limits=None):
        p = np.asarray(probs, dtype=np.float64)
        lim = None if limits is None else np.ascontiguousarray(limits, dtype=np.float64).reshape(-1, 2)
        rc = lib.okx_ensemble_select_check(p.ctypes.data_as(C.c_void_p), p.size, None if lim is None else lim.ctypes.data_as(C.c_void_p),
                                           0 if lim is None else lim.shape[0])
        return rc, _lib.last_error()

    assert check(PROBS, [[-1.0, 1.0], [-np.inf, np.inf], [2.0, 2.0]])[0] == 0
    for bad in ([0.5, 1.5], [-1e-9], [0.1, np.nan]):
        rc, text = check(bad)
        assert rc == -1 and "outside [0, 1]" in text, text
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            select_host(np.zeros((2, 1, 1)), None, bad)
    rc, text = check([0.5], [[0.0, 1.0], [2.0, 1.0]])
    assert rc == -1 and "limit 1 has lo > hi" in text, text
    with pytest.raises(ValueError, match="limit 0 has lo > hi"):
        select_host(np.zeros((2, 1, 1)), None, (0.5,), (1.0, 0.0))
    assert check([0.5], [[np.nan, 1.0]])[0] == -1 and check([], None)[0] == -2 and check(np.full(65, 0.5))[0] == -2
    # null outputs and short scratch are refused before anything is launched
    assert lib.okx_ensemble_select(0, 9, 15, None, 15, None, 0, None, 3, None, None, None, None, None, 0, None) == -1
    assert "null order-statistic or count table" in _lib.last_error()
    buf = (C.c_double * 4)()
    assert lib.okx_ensemble_select(0, 9, 15, None, 15, None, 0, buf, 3, None, buf, buf, None, buf, 32, None) == -1
    assert "bytes of scratch needed" in _lib.last_error()
