"""
CPU: covariance and correlation of selected entries of an evaluated ensemble over its complete geometries
(open_kinematics_amd/ensemble_stats.py: covariance_host, CovarianceAccumulator, EnsembleCovariance) on the REFERENCE's metric
values of 64 perturbed geometries x 9 steps (tests/golden/ensemble_stats_dw.npz), on a tampered copy, against reduce_host, in
merged runs, through the library's host-only entry points, and through ShardedEnsemble(reduce=True, covariance=...) over two
gloo ranks.

Every tolerance is derived here from the summation order and the number format (u = 2^-53), never from an outcome.  With
d = value - shift (ONE IEEE subtraction: the same bits in every layer, so the bounds start from d) over the G geometries of a
call, n of them used:

  gram[n][m] = sum d_n d_m:  a sum of at most G products in SOME order - one after the other on the host, four at a time
      inside a matrix instruction and slab by slab on the device, chunk after chunk when merged; the first-order bound of a
      sum of G terms holds for every order (Higham, Accuracy and Stability, eq. 4.4) - plus the rounding of each product (none
      when it is fused) and, on the side of the exact value, math.fsum of the ROUNDED products (one u on each) and its own
      final rounding:                  |result - exact| <= EG = (G + 2) u sum |d_n d_m|
  sum[n] = sum d_n:                    |result - exact| <= E1 = G u sum |d_n|      (as tests/test_ensemble_stats.py)
  two float results (host and device, merged and whole, two chunkings): each within the bound of the exact value, so within
      2 EG / 2 E1 of each other.
  covariance C = (gram - s_n s_m / n) / (n - 1), propagated (first order in the E, the formula's own roundings - a product,
      a division, a subtraction, a division - as 4 u on its two terms and 4 u on the result):
      EC = (EG + (|s_n| E1_m + |s_m| E1_n) / n + 4 u (|gram| + |s_n s_m| / n)) / (n - 1) + 4 u |C|
  numpy.cov of the used rows is another algorithm with its own error: it subtracts the computed mean (off by at most
      dm = n u mean|x|, its own sum, plus one rounding) and sums n products of the centred values, each centred value rounded
      once: ENP = ((n + 4) u sum |xc_n xc_m| + n dm_n dm_m + sum(|xc_n| dm_m + |xc_m| dm_n)) / (n - 1) with xc = x - mean.  The
      comparison against numpy.cov allows EC + ENP.
  the diagonal against ENS_SUMSQ of reduce_host: that table's bound is (G + 1) u sum d^2 (tests/test_ensemble_stats.py), ours
      EG: the two differ by at most their sum.
"""

import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from open_kinematics_amd.ensemble_stats import (COV_MAX_ENTRIES, ENS_COUNT, ENS_SUM, ENS_SUMSQ, CovarianceAccumulator, EnsembleCovariance,
                                                check_covariance_arguments, covariance_host, reduce_host)
from test_ensemble_stats import COLUMNS, _stand_in, load_fixture, tampered_fixture

U = 2.0 ** -53


def shifted(values, status, entries, shift):
    """(d [G, N] with the rows of dropped geometries zero, used [G]) - the definition, written out a second time."""
    g, s, k = values.shape
    e = np.arange(s * k) if entries is None else np.asarray(entries, dtype=np.int64)
    ok = np.isfinite(values)
    if status is not None:
        ok &= ((status & 7) == 1)[:, :, None]
    used = ok.reshape(g, s * k)[:, e].all(axis=1)
    with np.errstate(invalid="ignore"):
        d = values.reshape(g, s * k)[:, e] - np.asarray(shift, dtype=np.float64).reshape(-1)[e][None]
    return np.where(used[:, None], d, 0.0), used


def bounds(d):
    """(EG [N, N], E1 [N]) of a call over the geometries of ``d [G, N]``."""
    g = d.shape[0]
    a = np.abs(d)
    return (g + 2) * U * (a.T @ a) * (1.0 + 4 * g * U), g * U * a.sum(axis=0)  # (the bound's own sum is rounded too: a factor 1 + O(G u))


def exact(d):
    """(gram, sum) of ``d [G, N]`` by math.fsum - exact up to the rounding of each product and one final rounding."""
    n = d.shape[1]
    gram = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            gram[i, j] = gram[j, i] = math.fsum(d[:, i] * d[:, j])
    return gram, np.array([math.fsum(d[:, i]) for i in range(n)])


def covariance_bound(acc, eg, e1):
    """EC of the module docstring for an accumulator with bounds (EG, E1) on its tables."""
    n = float(acc.counts[0])
    s = np.abs(acc.sum)
    cov = acc.finalize().covariance
    return (eg + (np.outer(s, e1) + np.outer(e1, s)) / n + 4 * U * (np.abs(acc.gram) + np.outer(s, s) / n)) / (n - 1) + 4 * U * np.abs(cov)


def numpy_cov_bound(x):
    """ENP of the module docstring for ``numpy.cov(x.T)`` of the used rows ``x [n, N]``."""
    n = x.shape[0]
    xc = np.abs(x - x.mean(axis=0))
    dm = n * U * np.abs(x).mean(axis=0) + U * np.abs(x.mean(axis=0))
    return ((n + 4) * U * (xc.T @ xc) + n * np.outer(dm, dm) + np.outer(xc.sum(axis=0), dm) + np.outer(dm, xc.sum(axis=0))) / (n - 1)


def check_against_exact(acc, values, status, entries, shift):
    """An accumulator against the fsum tables within (EG, E1); counts and used bytes exactly.  Returns (d, used, EG, E1)."""
    d, used = shifted(values, status, entries, shift)
    eg, e1 = bounds(d)
    gram, s1 = exact(d)
    assert np.array_equal(acc.counts, [used.sum(), used.size - used.sum()])
    if acc.used is not None:
        assert np.array_equal(acc.used, used.astype(np.uint8))
    assert np.all(np.abs(acc.gram - gram) <= eg) and np.all(np.abs(acc.sum - s1) <= e1)
    assert np.array_equal(acc.gram, acc.gram.T)
    return d, used, eg, e1


def check_against_numpy_cov(acc, values, entries, used, eg, e1):
    g, s, k = values.shape
    e = np.arange(s * k) if entries is None else np.asarray(entries, dtype=np.int64)
    x = values.reshape(g, s * k)[used][:, e]
    fin = acc.finalize()
    tol = covariance_bound(acc, eg, e1) + numpy_cov_bound(x)
    want = np.atleast_2d(np.cov(x.T))
    assert np.all(np.abs(fin.covariance - want) <= tol)
    tol_mean = e1 / x.shape[0] + 4 * U * (np.abs(np.asarray(acc.shift).reshape(-1)[e]) + np.abs(acc.sum) / x.shape[0]) + x.shape[0] * U * np.abs(x).mean(axis=0)
    assert np.all(np.abs(fin.mean - x.mean(axis=0)) <= tol_mean)
    assert np.array_equal(fin.std, np.sqrt(np.maximum(np.diag(fin.covariance), 0.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = fin.covariance / np.outer(fin.std, fin.std)
    some = np.outer(fin.std, fin.std) > 0
    assert np.array_equal(fin.correlation[some], corr[some]) and np.all(np.isnan(fin.correlation[~some]))
    assert np.array_equal(fin.covariance, fin.covariance.T)
    return fin


def test_the_fixture_against_numpy_cov():
    fx = load_fixture()
    table, shift = fx["table"], fx["stat_shift"]
    acc = covariance_host(table, None, None, shift)
    assert acc.gram.shape == (135, 135) and np.array_equal(acc.entries, np.arange(135))
    d, used, eg, e1 = check_against_exact(acc, table, None, None, shift)
    assert used.all()
    fin = check_against_numpy_cov(acc, table, None, used, eg, e1)
    assert isinstance(fin, EnsembleCovariance) and fin.count == 64 and fin.dropped == 0 and np.array_equal(fin.entries, np.arange(135))
    # a permuted subset: rows and columns in the caller's order
    entries = [9 * 15 - 1, 3, 47, 15 * 4 + 2, 0, 77]
    sub = covariance_host(table, None, entries, shift)
    at = np.asarray(entries)
    assert np.array_equal(sub.gram, acc.gram[np.ix_(at, at)]) and np.array_equal(sub.sum, acc.sum[at])
    # the default shift: geometry 0 of the table
    own = covariance_host(table, None, entries)
    assert np.array_equal(own.shift, table[0])
    d, used, eg, e1 = check_against_exact(own, table, None, entries, table[0])
    check_against_numpy_cov(own, table, entries, used, eg, e1)
    # the tampered table: step 4 is rejected as a whole, so with every entry selected no geometry is complete ...
    tampered, status = tampered_fixture(fx)
    none = covariance_host(tampered, status, None, shift)
    assert list(none.counts) == [0, 64] and not none.gram.any() and not none.sum.any()
    fin = none.finalize()
    assert fin.count == 0 and np.all(np.isnan(fin.mean)) and np.all(np.isnan(fin.covariance)) and np.all(np.isnan(fin.correlation))
    # ... and with entries of three other steps some are dropped and most are used
    entries = [s * 15 + k for s in (0, 2, 7) for k in (0, 3, 9, 14)]
    part = covariance_host(tampered, status, entries, shift)
    d, used, eg, e1 = check_against_exact(part, tampered, status, entries, shift)
    assert 2 < used.sum() < 64
    check_against_numpy_cov(part, tampered, entries, used, eg, e1)


def test_complete_case_rule():
    rng = np.random.default_rng(5)
    values = rng.normal(size=(6, 3, 2))
    status = np.ones((6, 3), dtype=np.uint8)
    entries = [0, 3, 4]  # (s, k) = (0, 0), (1, 1), (2, 0)
    shift = np.zeros((3, 2))
    assert list(covariance_host(values, status, entries, shift).counts) == [6, 0]
    values[1, 1, 1] = np.nan   # a selected entry: geometry 1 is dropped
    values[2, 1, 0] = np.nan   # not selected (entry 2): geometry 2 stays
    values[3, 2, 1] = np.inf   # not selected (entry 5)
    status[4, 2] = 3           # residual exceeded at step 2, which holds the selected entry 4: dropped
    status[5, 0] = 9           # converged + ill-conditioned (advisory): accepted
    status[0, 1] = 1
    acc = covariance_host(values, status, entries, shift)
    assert list(acc.used) == [1, 0, 1, 1, 0, 1] and list(acc.counts) == [4, 2]
    rows = values.reshape(6, 6)[[0, 2, 3, 5]][:, entries]
    assert np.allclose(acc.gram, rows.T @ rows, rtol=0, atol=6 * U * (np.abs(rows).T @ np.abs(rows)).max())
    for byte in (0, 2, 3, 4, 5, 6, 7, 8, 10):  # everything but converged-and-clean in the low three bits
        status[0, 0] = byte
        assert covariance_host(values, status, entries, shift).used[0] == 0, byte
    status[0, 0] = 0
    assert covariance_host(values, status, [3, 4], shift).used[0] == 1  # step 0 holds no selected entry any more
    # fewer than two complete geometries: a mean but no covariance; none: nothing
    one = covariance_host(values[:1], None, entries, shift).finalize()
    assert one.count == 1 and np.array_equal(one.mean, values[0].reshape(-1)[entries]) and np.all(np.isnan(one.covariance)) and np.all(np.isnan(one.std))
    zero = covariance_host(values[:0], None, entries, shift)
    assert list(zero.counts) == [0, 0] and np.all(np.isnan(zero.finalize().mean))
    # a constant entry: variance 0, its correlations NaN, the others defined
    flat = rng.normal(size=(8, 1, 3))
    flat[:, 0, 1] = 2.5
    fin = covariance_host(flat, None, None, np.full((1, 3), 2.5)).finalize()
    assert fin.std[1] == 0.0 and np.all(np.isnan(fin.correlation[1])) and np.all(np.isnan(fin.correlation[:, 1])) and np.isfinite(fin.correlation[0, 2])
    with pytest.raises(ValueError, match="shift must be finite"):
        covariance_host(values, status, entries, np.full((3, 2), np.nan))


def test_cross_check_against_the_reduction():
    fx = load_fixture()
    table, shift = fx["table"], fx["stat_shift"]
    red = reduce_host(table, None, None, shift).acc
    acc = covariance_host(table, None, None, shift)
    d, used = shifted(table, None, None, shift)
    assert used.all()
    eg, e1 = bounds(d)
    e2 = (64 + 1) * U * (d * d).sum(axis=0)  # the reduction's bound on its sum of squares (tests/test_ensemble_stats.py)
    assert np.all(np.abs(np.diag(acc.gram) - red[..., ENS_SUMSQ].reshape(-1)) <= np.diag(eg) + e2)
    assert np.all(np.abs(acc.sum - red[..., ENS_SUM].reshape(-1)) <= 2 * e1)
    assert np.all(red[..., ENS_COUNT] == acc.counts[0])
    st, fin = reduce_host(table, None, None, shift).finalize(), acc.finalize()
    assert np.allclose(fin.mean, st.mean.reshape(-1), rtol=0, atol=(2 * e1 / 64 + 8 * U * np.abs(fin.mean)).max())


@pytest.mark.parametrize("edges", [[0, 64], [0, 31, 64], [0, 1, 2, 40, 40, 64], list(range(65))])
def test_chunks_merge_to_the_whole_table(edges):
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    shift = fx["stat_shift"]
    entries = [s * 15 + k for s in (0, 2, 7, 8) for k in (1, 3, 9, 14)][::-1]
    whole = covariance_host(table, status, entries, shift)
    d, used, eg, e1 = check_against_exact(whole, table, status, entries, shift)
    merged = CovarianceAccumulator.empty(shift, entries)
    for a, b in zip(edges[:-1], edges[1:]):
        merged = merged.merge(covariance_host(table[a:b], status[a:b], entries, shift))
    assert np.array_equal(merged.counts, whole.counts) and np.array_equal(merged.gram, merged.gram.T)
    assert np.all(np.abs(merged.gram - whole.gram) <= 2 * eg) and np.all(np.abs(merged.sum - whole.sum) <= 2 * e1)
    assert np.all(np.abs(merged.finalize().covariance - whole.finalize().covariance) <= 2 * covariance_bound(whole, eg, e1))
    if len(edges) == 2:  # one chunk after the empty accumulator: the same bits
        assert np.array_equal(merged.gram, whole.gram) and np.array_equal(merged.sum, whole.sum)
    # the empty accumulator is the neutral element on either side, and torch tensors merge as NumPy arrays do
    empty = CovarianceAccumulator.empty(shift, entries)
    for both in (whole.merge(empty), empty.merge(whole)):
        assert np.array_equal(both.gram, whole.gram) and np.array_equal(both.sum, whole.sum) and np.array_equal(both.counts, whole.counts)
    as_torch = lambda a: CovarianceAccumulator(*(torch.as_tensor(t) for t in (a.gram, a.sum, a.counts, a.shift, a.entries)))  # noqa: E731
    twice = as_torch(whole).merge(as_torch(whole)).numpy()
    assert np.array_equal(twice.gram, whole.gram + whole.gram) and list(twice.counts) == [2 * c for c in whole.counts]
    with pytest.raises(ValueError, match="different shifts"):
        whole.merge(covariance_host(table, status, entries, shift + 1.0))
    with pytest.raises(ValueError, match="different entries"):
        whole.merge(covariance_host(table, status, entries[::-1], shift))
    with pytest.raises(ValueError, match="different entries"):
        whole.merge(covariance_host(table, status, entries[:-1], shift))


def test_argument_errors_in_the_words_of_the_library():
    from open_kinematics_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "okx.h"), encoding="utf-8").read()
    assert f"OKX_ENS_COV_MAX_ENTRIES = {COV_MAX_ENTRIES}" in header and COV_MAX_ENTRIES == 2048

    def check(entries, n_table):
        e = np.ascontiguousarray(entries, dtype=np.int32)
        return lib.okx_ensemble_covariance_check(e.ctypes.data_as(C.c_void_p), e.size, n_table), _lib.last_error()

    assert check([4, 0, 11], 12)[0] == 0 and check(np.arange(2048)[::-1], 4096)[0] == 0
    assert lib.okx_ensemble_covariance_check(None, 12, 12) == 0
    assert np.array_equal(check_covariance_arguments(None, 12), np.arange(12)) and check_covariance_arguments([4, 0, 11], 12).dtype == np.int32
    cases = [([1, 1], 12), ([3, 1, 2, 1, 3], 12), ([5, 0, 7, 5, 0], 12),   # duplicates: the FIRST position that repeats an earlier one
             ([0, 12], 12), ([-1], 12), ([2, 5, 99, -3], 12),               # out of range
             ([], 12),                                                      # N = 0
             (np.arange(2049), 4096)]                                       # N > 2048
    for entries, n_table in cases:
        rc, text = check(entries, n_table)
        assert rc == -1, entries
        with pytest.raises(ValueError) as err:
            check_covariance_arguments(np.asarray(entries, dtype=np.int64), n_table)
        assert str(err.value) == text, (str(err.value), text)
    assert "repeats entry 1 (index 1)" in check([3, 1, 2, 1, 3], 12)[1] and "entry 3 repeats entry 0 (index 5)" in check([5, 0, 7, 5, 0], 12)[1]
    # no entry list selects the whole table: too large a table, or a count that is not the table's, is refused
    assert lib.okx_ensemble_covariance_check(None, 2049, 2049) == -1 and "1 to 2048 allowed" in _lib.last_error()
    with pytest.raises(ValueError) as err:
        check_covariance_arguments(None, 2049)
    assert str(err.value) == _lib.last_error()
    assert lib.okx_ensemble_covariance_check(None, 5, 12) == -1 and "without an entry list" in _lib.last_error()
    with pytest.raises(ValueError, match="integers"):
        check_covariance_arguments([0.5, 1.0], 12)
    with pytest.raises(ValueError, match="repeats"):
        covariance_host(np.zeros((2, 3, 4)), None, [1, 1])
    # the scratch size is a function of the sizes alone: used bytes | used counts | sums [tile][slab][64] | tiles [pair][slab][64][64]
    size = lib.okx_ensemble_covariance_scratch_bytes
    assert size(-1, 9, 15, 4) == 0 and size(10, 9, 15, 0) == 0 and size(10, 9, 15, 2049) == 0 and size(0, 9, 15, 135) == 8
    assert size(300, 26, 5, 130) == 304 + 8 * 75 + 8 * 3 * 3 * 64 + 8 * 6 * 3 * 4096      # three slabs of 128 geometries
    assert size(300, 1, 1, 1) == 304 + 8 * 75 + 8 * 1 * 3 * 64 + 8 * 1 * 3 * 4096
    assert size(4096, 256, 4, 1024) == 4096 + 8 * 1024 + 8 * 16 * 7 * 64 + 8 * 136 * 7 * 4096  # C5: 136 tile pairs x 7 slabs of 608
    # null outputs, a bad table and short scratch are refused before anything is launched
    buf = (C.c_double * 64)()
    args = lambda **kw: [kw.get(n, d) for n, d in (("g", 0), ("s", 3), ("k", 2), ("values", buf), ("ld", 2), ("status", None), ("stride", 0),  # noqa: E731
                                                    ("entries", buf), ("n", 4), ("shift", buf), ("acc", 0), ("gram", buf), ("sum", buf), ("counts", buf),
                                                    ("used", None), ("scratch", buf), ("bytes", 512), ("stream", None))]
    for kw, words in ((dict(gram=None), "null gram, sum, counts or shift"), (dict(shift=None), "null gram, sum, counts or shift"),
                      (dict(g=2, ld=1), "null table or ld < n_columns"), (dict(g=2, values=None), "null table"),
                      (dict(status=buf, stride=0), "status_stride must be positive"), (dict(g=-1), "negative geometry, step or column count"),
                      (dict(n=0), "0 entries selected, 1 to 2048 allowed"), (dict(n=2049), "2049 entries selected"),
                      (dict(n=7), "7 distinct entries of a table of 6"), (dict(entries=None, n=4), "without an entry list all 6 entries"),
                      (dict(bytes=4), "bytes of scratch needed"), (dict(scratch=None), "bytes of scratch needed")):
        assert lib.okx_ensemble_covariance(*args(**kw)) == -1, kw
        assert words in _lib.last_error(), (kw, _lib.last_error())


# ---- ShardedEnsemble(reduce=True, covariance=...) over two gloo ranks, the stand-in program of tests/test_dist.py ----

STEPS = 4
SHARDED_CASES = [(64, 1), (64, 3), (7, 2), (5, 3), (1, 1)]  # (geometries, chunks): even and ragged counts; one geometry leaves rank 1 without any
SUBSET = [13, 2, 7, 8, 0]


def sharded_table(n_geom):
    """(hardpoint table, relative targets, values [G, S, K], status [G, S]) of the stand-in ensemble, unsharded."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, STEPS)
    alone = ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS)
    values = alone.step().numpy().reshape(n_geom, STEPS, len(COLUMNS)).copy()
    return table, relative, values, alone.status_full.numpy().reshape(n_geom, STEPS).copy()


def _covariance_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    out = {}
    for n_geom, chunks in SHARDED_CASES:
        table, relative = _ensemble_inputs(n_geom, STEPS)
        kw = dict(chunks=chunks, metric_columns=COLUMNS, reduce=True)
        for name, which in (("all", True), ("subset", SUBSET)):
            pipe = ShardedEnsemble(_stand_in(), table, relative, STEPS, covariance=which, **kw)
            acc = pipe.step()
            first = pipe.covariance_accumulator.numpy()
            pipe.step()  # a second step starts from nothing
            again, fin = pipe.covariance_accumulator.numpy(), pipe.covariance()
            plain = ShardedEnsemble(_stand_in(), table, relative, STEPS, **kw)
            out[(n_geom, chunks, name)] = {"gram": first.gram.copy(), "sum": first.sum.copy(), "counts": first.counts.copy(), "entries": first.entries.copy(),
                                           "again": (again.gram.copy(), again.sum.copy(), again.counts.copy()), "covariance": fin.covariance, "mean": fin.mean,
                                           "count": fin.count, "shift": acc.shift.clone(), "used": pipe.covariance_local_used.clone(), "range": pipe.geometry_range,
                                           "same_acc": torch.equal(torch.nan_to_num(acc.acc), torch.nan_to_num(plain.step().acc)),
                                           "sent": pipe.covariance_exchange_bytes_per_rank, "plain_sent": plain.covariance_exchange_bytes_per_rank,
                                           "acc_sent": (pipe.exchange_bytes_per_rank, plain.exchange_bytes_per_rank)}
    torch.save(out, os.path.join(out_dir, f"covariance{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_covariance_gives_every_rank_the_same_bits(tmp_path):
    from open_kinematics_amd.dist import ShardedEnsemble, shard_range

    world = 2
    port = 35600 + (os.getpid() + 13 * world) % 2000
    mp.spawn(_covariance_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"covariance{r}.pt"), weights_only=False) for r in range(world)]
    k = len(COLUMNS)
    for n_geom, chunks in SHARDED_CASES:
        table, relative, values, status = sharded_table(n_geom)
        for name, entries in (("all", None), ("subset", SUBSET)):
            one, two = got[0][(n_geom, chunks, name)], got[1][(n_geom, chunks, name)]
            for key in ("gram", "sum", "counts", "entries", "covariance", "mean"):
                assert np.array_equal(one[key], two[key], equal_nan=True), (key, n_geom, chunks, name)
            shift = one["shift"].numpy()
            want = covariance_host(values, status, entries, shift)  # the one-process answer
            d, used = shifted(values, status, entries, shift)
            eg, e1 = bounds(d)
            if n_geom == 64:  # the inputs are worth the test: the stand-in's status bytes drop some geometries and keep most
                assert 2 < used.sum() < 64
            n = want.entries.size
            assert n == (STEPS * k if entries is None else len(SUBSET)) and np.array_equal(one["entries"], want.entries)
            for r, rank in enumerate((one, two)):
                assert np.array_equal(rank["counts"], want.counts) and rank["count"] == want.counts[0]
                assert np.all(np.abs(rank["gram"] - want.gram) <= 2 * eg) and np.all(np.abs(rank["sum"] - want.sum) <= 2 * e1)
                assert np.array_equal(rank["gram"], rank["gram"].T)
                for a, b in zip(rank["again"], (rank["gram"], rank["sum"], rank["counts"])):
                    assert np.array_equal(a, b)
                if want.counts[0] > 1:
                    assert np.all(np.abs(rank["covariance"] - want.finalize().covariance) <= 2 * covariance_bound(want, eg, e1))
                else:
                    assert np.all(np.isnan(rank["covariance"]))
                lo, hi = rank["range"]
                assert (lo, hi) == shard_range(n_geom, r, world) and np.array_equal(rank["used"].numpy(), want.used[lo:hi])
                # the accumulator of the reduction and its traffic are what they are without the covariance
                assert rank["same_acc"] and rank["acc_sent"][0] == rank["acc_sent"][1] and rank["plain_sent"] == 0
                assert rank["sent"] == 8 * (n * n + n + 2)
    # one process: no exchange, the host accumulator's bits (one chunk: the same additions in the same order)
    table, relative, values, status = sharded_table(64)
    single = ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS, reduce=True, covariance=SUBSET, quantiles=(0.5,))
    acc = single.step()
    want = covariance_host(values, status, SUBSET, acc.shift.numpy())
    mine = single.covariance_accumulator.numpy()
    assert np.array_equal(mine.gram, want.gram) and np.array_equal(mine.sum, want.sum) and np.array_equal(mine.counts, want.counts)
    assert single.covariance_exchange_bytes_per_rank == 0 and single.covariance().count == want.counts[0] and single.quantiles() is not None
    kw = dict(metric_columns=COLUMNS, reduce=True)
    with pytest.raises(ValueError, match="needs reduce=True"):
        ShardedEnsemble(_stand_in(), table, relative, STEPS, metric_columns=COLUMNS, covariance=True)
    with pytest.raises(ValueError, match="repeats entry 0"):
        ShardedEnsemble(_stand_in(), table, relative, STEPS, covariance=[3, 3], **kw)
    with pytest.raises(ValueError, match=r"outside \[0, 16\)"):
        ShardedEnsemble(_stand_in(), table, relative, STEPS, covariance=[16], **kw)
    with pytest.raises(ValueError, match=r"covariance\(\) needs covariance="):
        ShardedEnsemble(_stand_in(), table, relative, STEPS, **kw).covariance()
    with pytest.raises(RuntimeError, match="no step"):
        ShardedEnsemble(_stand_in(), table, relative, STEPS, covariance=True, **kw).covariance()
