"""
Poisson-bootstrap intervals of the Sobol' indices, CPU: the weights' definition (ensemble_stats.bootstrap_weights - thresholds, ranges,
counter words, statistics), the replicate accumulators' NumPy definition (ensemble_stats.sobol_bootstrap_host) against sobol_host and
against itself over chunkings, the finalization on the known response of tests/test_ensemble_sobol.py, and the SobolBootstrap stage
of ShardedEnsemble on the stand-in program of tests/test_dist.py (chunkings in one process, two ranks over gloo).

Integer tables (``integer_table``: |value - shift| <= 8, at most 67 families): every term is an integer below 2^9, every weight at
most 13 and every partial sum below 2^22, so every addition order gives the same bits and the comparisons are array_equal.
On real tables the integer fields (COUNT_r, DROPPED_r: sums of weights) are compared exactly and the others within
``weighted_bound``: 2 (n + 1) U sum |w term| over the host's own weighted terms - the bound of ``term_bound`` with the rounded
products w * term, which every route forms bit-identically, as the summands.
"""

import decimal
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from open_kinematics_amd import ensemble_sample as smp
from open_kinematics_amd import ensemble_stats as es
from open_kinematics_amd.ensemble_sample import LHS, NORMAL, FamilyPlan, SamplePlan, families_host
from open_kinematics_amd.ensemble_stats import (SOBOL_COUNT, SOBOL_DROPPED, SOBOL_FIELDS, SobolBootstrapAccumulator, bootstrap_weights, sobol_bootstrap_host,
                                                sobol_host, sobol_terms)
from test_ensemble_sobol import STEPS, bits, integer_stand_in, integer_table, stand_in_families

U = 2.0 ** -53


def weighted_bound(values, status, mask, d, shift, weights):
    """``[R, S, K, fields]``: 2 (n + 1) U sum_i |w_i,r term_i| (Higham (4.4), as ``term_bound``): two recursive sums of the same n rounded
    products, each within (n + 1) U sum |product| of their exact sum whatever its order."""
    _, terms, _ = sobol_terms(values, status, mask, d, shift)
    w = np.asarray(weights, dtype=np.float64)
    total = np.zeros((w.shape[1],) + terms.shape[1:])
    for i in range(terms.shape[0]):
        total += np.abs(w[i][:, None, None, None] * terms[i][None])
    return 2.0 * (terms.shape[0] + 1) * U * total


# ---- thresholds and header ----

def test_thresholds_are_the_poisson_cdf_and_match_the_header():
    decimal.getcontext().prec = 60
    e_inv = decimal.Decimal(-1).exp()
    cdf, term, want = decimal.Decimal(0), decimal.Decimal(1), []
    for k in range(13):
        if k:
            term /= k
        cdf += e_inv * term
        want.append(int((cdf * 2 ** 32).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    assert want == [int(t) for t in es.BOOTSTRAP_THRESHOLDS] and es.BOOTSTRAP_THRESHOLDS.dtype == np.uint32
    assert want == [0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21, 0xffffffd4,
                    0xfffffffc, 0xffffffff]
    assert es.BOOTSTRAP_MAX_WEIGHT == len(want) == 13
    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        header = fh.read()
    with open(os.path.join(REPO, "open_kinematics_amd", "csrc", "okx_bootstrap.hip"), "r", encoding="utf-8") as fh:
        unit = fh.read()
    for t in want:
        assert f"0x{t:08x}" in header and f"0x{t:08x}u" in unit
    assert int(re.search(r"OKX_ENS_BOOTSTRAP_MAX_REPLICATES = (\d+)", header).group(1)) == es.BOOTSTRAP_MAX_REPLICATES
    assert int(re.search(r"OKX_ENS_BOOTSTRAP_MAX_WEIGHT = (\d+)", header).group(1)) == es.BOOTSTRAP_MAX_WEIGHT
    assert int(re.search(r"OKX_SAMPLE_PURPOSE_BOOTSTRAP = (\d+)", header).group(1)) == smp.PURPOSE_BOOTSTRAP == 2
    assert (smp.PURPOSE_DRAW, smp.PURPOSE_STRATA) == (0, 1)
    for name in ("DRAW", "STRATA"):
        assert int(re.search(rf"OKX_SAMPLE_PURPOSE_{name} = (\d+)", header).group(1)) == getattr(smp, f"PURPOSE_{name}")


# ---- bootstrap_weights ----

def test_weights_are_a_function_of_seed_row_and_replicate():
    whole = bootstrap_weights(21, 0, 100, 8)
    assert whole.shape == (100, 8) and whole.dtype == np.uint8 and whole.max() <= 13
    for lo, hi in ((0, 0), (3, 4), (17, 100), (99, 100)):
        assert np.array_equal(bootstrap_weights(21, lo, hi, 8), whole[lo:hi])
    assert np.array_equal(bootstrap_weights(21, 0, 100, 5), whole[:, :5])  # (replicates 4 .. 7 come from a second Philox call)
    assert np.array_equal(bootstrap_weights(21, 0, 100, 1), whole[:, :1])
    far = bootstrap_weights(21, 2 ** 32 + 3, 2 ** 32 + 103, 8)  # the counter's high word
    assert far.shape == (100, 8) and not np.array_equal(far, bootstrap_weights(21, 3, 103, 8))
    assert np.array_equal(far[5:9], bootstrap_weights(21, 2 ** 32 + 8, 2 ** 32 + 12, 8))
    assert not np.array_equal(bootstrap_weights(22, 0, 100, 8), whole)
    assert not np.array_equal(bootstrap_weights(21 + 2 ** 32, 0, 100, 8), whole)  # the key's high word
    # the definition, one weight written out: word r % 4 of the call (row lo, row hi, r // 4, purpose << 8)
    row, r = 2 ** 32 + 7, 6
    words = smp.philox4x32_10((row & 0xFFFFFFFF, row >> 32, r // 4, smp.PURPOSE_BOOTSTRAP << 8), smp._seed_key(21))
    assert far[4, r] == sum(int(words[r % 4]) >= int(t) for t in es.BOOTSTRAP_THRESHOLDS)
    # not the sampler's draw of the same counter
    assert int(words[0]) != int(smp.philox4x32_10((row & 0xFFFFFFFF, row >> 32, r // 4, smp.PURPOSE_DRAW << 8), smp._seed_key(21))[0])
    for bad in (0, es.BOOTSTRAP_MAX_REPLICATES + 1):
        with pytest.raises(ValueError, match=f"{bad} replicates, 1 to 1024 allowed"):
            bootstrap_weights(21, 0, 4, bad)
    with pytest.raises(ValueError, match="bad range"):
        bootstrap_weights(21, 5, 4, 8)
    assert bootstrap_weights(21, 0, 2, es.BOOTSTRAP_MAX_REPLICATES).shape == (2, 1024)


def test_weight_statistics():
    """2^20 draws: mean and variance of Poisson(1) within five standard deviations of their estimators (1 / 1024 and sqrt(3) / 1024 -
    the fourth central moment of Poisson(1) is 4, so var(s^2) = (4 - 1) / n)."""
    w = bootstrap_weights(5, 0, 4096, 256).astype(np.float64)
    print("mean", w.mean(), "variance", w.var(), "largest", w.max())
    assert abs(w.mean() - 1.0) < 5.0 / 1024 and abs(w.var() - 1.0) < 5.0 * np.sqrt(3.0) / 1024
    assert w.max() <= 13
    # rows and replicates are not copies of each other
    assert len({w[i].tobytes() for i in range(64)}) == 64 and len({w[:, r].tobytes() for r in range(64)}) == 64


# ---- sobol_bootstrap_host ----

CASES = [(n, d, s, k) for n in (1, 2, 67) for d in (1, 3) for s, k in ((1, 1), (3, 5))]


@pytest.mark.parametrize("n,d,s,k", CASES)
def test_host_definition_on_integer_tables(n, d, s, k):
    m, r = d + 2, 11
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(n, d, s, k, 1000 * n + 10 * d + s, with_mask)
        plain = sobol_host(values, status, mask, d, shift)
        # every weight 1: each replicate IS the plain accumulator, bit for bit
        ones = sobol_bootstrap_host(values, status, mask, d, shift, seed=0, n_replicates=3, weights=np.ones((n, 3), dtype=np.uint8))
        assert ones.acc.shape == (3, s, k, SOBOL_FIELDS + 3 * d) and all(np.array_equal(bits(ones.acc[i]), bits(plain.acc)) for i in range(3))
        # the seed's weights: a plain-loop restatement of one replicate, and the weight sums
        offset = 2 ** 32 + 5
        got = sobol_bootstrap_host(values, status, mask, d, shift, seed=9, n_replicates=r, family_offset=offset, group_names=[f"g{j}" for j in range(d)])
        w = bootstrap_weights(9, offset, offset + n, r)
        _, terms, _ = sobol_terms(values, status, mask, d, shift)
        for rep in (0, r - 1):
            want = np.zeros(terms.shape[1:])
            for i in range(n):
                want += float(w[i, rep]) * terms[i]
            assert np.array_equal(got.acc[rep], want)
        assert np.array_equal(got.acc[..., SOBOL_COUNT] + got.acc[..., SOBOL_DROPPED], np.broadcast_to(w.sum(axis=0)[:, None, None], (r, s, k)))
        assert got.seed == 9 and got.n_groups == d and got.n_replicates == r and got.group_names == [f"g{j}" for j in range(d)]
        # two chunks of whole families with their family_offset, merged: the whole, exactly
        cut = (n // 2) * m
        halves = [sobol_bootstrap_host(values[a:b], status[a:b], None if mask is None else mask[a:b], d, shift, seed=9, n_replicates=r,
                                       family_offset=offset + a // m) for a, b in ((0, cut), (cut, n * m))]
        assert np.array_equal(halves[0].merge(halves[1]).acc, got.acc)
        if n >= 2:  # ... and without the offset it is another resample
            wrong = sobol_bootstrap_host(values[cut:], status[cut:], None if mask is None else mask[cut:], d, shift, seed=9, n_replicates=r, family_offset=offset)
            assert not np.array_equal(halves[1].acc, wrong.acc)
    with pytest.raises(ValueError, match="no whole families"):
        sobol_bootstrap_host(values[:-1], status[:-1], None, d, shift, seed=9, n_replicates=r)
    with pytest.raises(ValueError, match="different seeds"):
        got.merge(sobol_bootstrap_host(values, status, mask, d, shift, seed=10, n_replicates=r, family_offset=offset))
    with pytest.raises(ValueError, match="different shifts"):
        got.merge(sobol_bootstrap_host(values, status, mask, d, shift + 1.0, seed=9, n_replicates=r, family_offset=offset))
    with pytest.raises(ValueError, match="different shapes"):
        got.merge(sobol_bootstrap_host(values, status, mask, d, shift, seed=9, n_replicates=r + 1, family_offset=offset))
    with pytest.raises(ValueError, match="0 replicates, 1 to 1024 allowed"):
        sobol_bootstrap_host(values, status, mask, d, shift, seed=9, n_replicates=0)
    with pytest.raises(ValueError, match="weights must be"):
        sobol_bootstrap_host(values, status, mask, d, shift, seed=9, n_replicates=r, weights=np.ones((n + 1, r)))


def test_real_tables_count_exactly_over_chunkings():
    n, d, s, k, r = 67, 3, 3, 5, 9
    m = d + 2
    rng = np.random.default_rng(5)
    shift = rng.normal(0.0, 3.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (n * m, s, k)) * np.logspace(-3, 3, k)[None, None]
    _, status, mask, _ = integer_table(n, d, s, k, 77)
    whole = sobol_bootstrap_host(values, status, mask, d, shift, seed=3, n_replicates=r)
    assert 0 < whole.acc[..., SOBOL_DROPPED].max() and whole.acc[..., SOBOL_COUNT].min() > 0
    bound = weighted_bound(values, status, mask, d, shift, bootstrap_weights(3, 0, n, r))
    for cuts in ((0, 1, n), (0, 20, 21, 66, n), tuple(range(n + 1))):
        merged = None
        for a, b in zip(cuts, cuts[1:]):
            part = sobol_bootstrap_host(values[a * m : b * m], status[a * m : b * m], mask[a * m : b * m], d, shift, seed=3, n_replicates=r, family_offset=a)
            merged = part if merged is None else merged.merge(part)
        assert np.array_equal(merged.acc[..., :2], whole.acc[..., :2])
        assert np.all(np.abs(merged.acc - whole.acc) <= bound)


# ---- finalize: the known response ----

def known_response(stratify=LHS, n_families=4096):
    """tests/test_ensemble_sobol.py::test_indices_of_a_known_response: y = sum c_z x_z + 0.3 x_2 x_3, groups {0, 1}, {2}, {3, 4}."""
    plan = SamplePlan(np.zeros((2, 3)), np.arange(6), np.full(6, NORMAL), stratify=stratify, seed=77)
    fp = FamilyPlan(plan, np.array([0, 0, 1, 2, 2, -1]), n_families)
    lat = families_host(fp)[1]
    y = lat @ np.array([1.0, 2.0, 0.5, 1.0, 1.0, 0.0]) + 0.3 * lat[:, 2] * lat[:, 3]
    var, inter = np.array([5.0, 0.25, 2.0]), 0.09
    return y[:, None, None], var / (var.sum() + inter), (var + [0.0, inter, inter]) / (var.sum() + inter)


def test_intervals_cover_the_known_response():
    """Bootstrap seed 77, R = 256, shift 0: the 95 % percentile interval of each of the nine indices holds its closed-form value, and
    every standard deviation lies in (0, 0.05)."""
    y, want_first, want_total = known_response()
    acc = sobol_bootstrap_host(y, None, None, 3, np.zeros((1, 1)), seed=77, n_replicates=256, group_names=("a", "b", "c"))
    out = acc.finalize()
    assert out.first.shape == (256, 1, 1, 3) and out.mean.shape == (256, 1, 1) and out.level == 0.95 and out.group_names == ["a", "b", "c"]
    assert np.array_equal(out.defined, [[256]])
    for name, want in (("first", want_first), ("first_jansen", want_first), ("total", want_total)):
        lo, hi = out.interval(name)
        std = getattr(out, f"{name}_std")
        print(name, "interval", lo[0, 0], hi[0, 0], "closed form", want, "std", std[0, 0])
        assert lo.shape == (1, 1, 3) and np.all(lo[0, 0] <= want) and np.all(want <= hi[0, 0])
        assert np.all(std > 0.0) and np.all(std < 0.05)
        # the interval is np.nanquantile's, and a narrower level nests inside
        table = getattr(out, name)
        assert all(np.array_equal(a, b) for a, b in zip((lo, hi), np.nanquantile(table, [(1.0 - 0.95) / 2.0, (1.0 + 0.95) / 2.0], axis=0)))
        assert np.array_equal(std, np.nanstd(table, axis=0, ddof=1))
        lo5, hi5 = out.interval(name, 0.5)
        assert np.all(lo <= lo5) and np.all(hi5 <= hi)
    lo, hi = out.interval("mean")
    assert lo[0, 0] <= 0.0 <= hi[0, 0] and 0.0 < out.mean_std[0, 0] < 0.1
    lo, hi = out.interval("variance")
    assert lo[0, 0] <= 7.34 <= hi[0, 0]
    # replicate r is SobolAccumulator.finalize of its own tables
    one = es.SobolAccumulator(acc.acc[7], acc.shift).finalize()
    assert np.array_equal(one.first, out.first[7]) and np.array_equal(one.total, out.total[7]) and np.array_equal(one.variance, out.variance[7])
    with pytest.raises(ValueError, match="no replicates of"):
        out.interval("count")
    with pytest.raises(ValueError, match="level must lie inside"):
        acc.finalize(1.0)


def test_finalize_is_nan_aware():
    d, s, k, n, r = 2, 2, 3, 12, 16
    rng = np.random.default_rng(3)
    shift = rng.normal(0.0, 10.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (n * (d + 2), s, k))
    values[:, 1, 0] = shift[1, 0]                  # a constant column: V = 0 in every replicate
    values[4 :: d + 2, 1, 1] = np.nan              # member 0 of every family but family 0 is undefined: COUNT_r = w(r, 0)
    acc = sobol_bootstrap_host(values, None, None, d, shift, seed=1, n_replicates=r)
    w0 = bootstrap_weights(1, 0, 1, r)[0]
    assert 0 < (w0 == 0).sum() < r
    out = acc.finalize(0.9)
    assert out.level == 0.9 and np.array_equal(out.defined[0], [r] * k) and out.defined[1, 0] == 0
    assert np.all(np.isnan(out.first_std[1, 0])) and np.all(np.isnan(out.interval("total")[0][1, 0]))
    assert np.all(np.isfinite(out.first_std[0])) and np.all(np.isfinite(out.interval("first")[1][0]))
    # one family alone counts there: the entry is defined in the replicates that drew it, NaN in the others
    assert out.defined[1, 1] == (w0 > 0).sum() and np.array_equal(np.isfinite(out.mean[:, 1, 1]), w0 > 0)
    assert np.array_equal(np.isfinite(out.total[:, 1, 1, 0]), w0 > 0) and np.all(np.isfinite(out.total_std[1, 1]))
    torch_acc = SobolBootstrapAccumulator(torch.as_tensor(acc.acc), torch.as_tensor(acc.shift), acc.seed)
    assert np.array_equal(bits(torch_acc.numpy().acc), bits(acc.acc)) and torch.equal(torch_acc.merge(torch_acc).acc, 2.0 * torch_acc.acc)
    with pytest.raises(ValueError, match="acc must be"):
        SobolBootstrapAccumulator(acc.acc[0], acc.shift, 1)


# ---- the SobolBootstrap stage of ShardedEnsemble on host stand-ins ----

def test_bootstrap_stage_chunked_equals_unchunked():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_stats import COLUMNS, _stand_in

    fp, relative = stand_in_families(9)
    k, r = len(COLUMNS), 5
    shift = np.zeros((STEPS, k))
    flags = families_host(fp)[3]
    for program, exact in ((integer_stand_in, True), (_stand_in, False)):
        runs = {}
        for chunks in (1, 2, 4):
            pipe = ShardedEnsemble(program(), fp, relative, STEPS, chunks=chunks, metric_columns=COLUMNS, reduce=True, sobol=True, bootstrap=r, shift=shift)
            pipe.step()
            assert pipe.sobol_bootstrap_exchange_bytes_per_rank == 0 and pipe.sobol_bootstrap_accumulator.seed == fp.plan.seed == 9
            runs[chunks] = pipe
        one = runs[1]
        acc = one.sobol_bootstrap_accumulator.acc.numpy()
        values = one.metric_local.numpy().reshape(45, STEPS, k)
        status = one.info_local[:, 32].numpy().reshape(45, STEPS)
        want = sobol_bootstrap_host(values, status, flags, 3, shift, seed=9, n_replicates=r)
        weights = bootstrap_weights(9, 0, 9, r)
        bound = weighted_bound(values, status, flags, 3, shift, weights)
        assert acc.shape == (r, STEPS, k, SOBOL_FIELDS + 9)
        assert np.array_equal(acc[..., SOBOL_COUNT] + acc[..., SOBOL_DROPPED], np.broadcast_to(weights.sum(axis=0)[:, None, None], (r, STEPS, k)))
        assert acc[..., SOBOL_COUNT].max() > 0 and acc[..., SOBOL_DROPPED].max() > 0
        for c in (1, 2, 4):
            got = runs[c].sobol_bootstrap_accumulator.acc.numpy()
            assert np.array_equal(got[..., :2], want.acc[..., :2])
            assert np.array_equal(got, want.acc) if exact else np.all(np.abs(got - want.acc) <= bound)
            # the Sobol' stage beside it is what it is without the bootstrap
        plain = ShardedEnsemble(program(), fp, relative, STEPS, chunks=2, metric_columns=COLUMNS, reduce=True, sobol=True, shift=shift)
        plain.step()
        assert np.array_equal(bits(plain.sobol_accumulator.acc.numpy()), bits(runs[2].sobol_accumulator.acc.numpy()))
        out = one.sobol_bootstrap()
        assert out.first.shape == (r, STEPS, k, 3) and out.group_names == ["lower", "middle", "upper"] and one.sobol_bootstrap(0.5).level == 0.5
        again = one.step() and one.sobol_bootstrap_accumulator.acc.numpy()
        assert np.array_equal(again, acc)  # a second step starts from nothing
    other = ShardedEnsemble(_stand_in(), fp, relative, STEPS, metric_columns=COLUMNS, reduce=True, sobol=True, bootstrap=r, bootstrap_seed=10, shift=shift)
    other.step()
    assert other.sobol_bootstrap_accumulator.seed == 10 and not np.array_equal(other.sobol_bootstrap_accumulator.acc.numpy(), acc)


def _bootstrap_worker(rank: int, world: int, port: int, n_families: int, chunks: int, replicates: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_stats import COLUMNS, _stand_in

    fp, relative = stand_in_families(n_families)
    pipe = ShardedEnsemble(_stand_in(), fp, relative, STEPS, chunks=chunks, metric_columns=COLUMNS, reduce=True, sobol=True, bootstrap=replicates,
                           shift=np.zeros((STEPS, len(COLUMNS))))
    pipe.step()
    torch.save({"acc": pipe.sobol_bootstrap_accumulator.acc.clone(), "sobol": pipe.sobol_accumulator.acc.clone(), "range": pipe.geometry_range,
                "sent": pipe.sobol_bootstrap_exchange_bytes_per_rank, "values": pipe.metric_local.clone(), "status": pipe.info_local[:, 32].clone()},
               os.path.join(out_dir, f"boot{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_families,chunks", [(2, 9, 2), (3, 2, 1)])
def test_bootstrap_stage_over_gloo_ranks(tmp_path, world, n_families, chunks):
    """Ragged shards of whole families and a rank without a family ((3, 2)): the same replicate bits on every rank; their integer
    fields equal the one-call definition over the gathered table, the others lie within the bound."""
    from test_ensemble_stats import COLUMNS

    r, k, m = 5, len(COLUMNS), 5
    port = 35500 + (os.getpid() + 7 * world + n_families) % 2000
    mp.spawn(_bootstrap_worker, args=(world, port, n_families, chunks, r, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"boot{i}.pt")) for i in range(world)]
    assert all(torch.equal(got[0][key].view(torch.int64), g[key].view(torch.int64)) for g in got[1:] for key in ("acc", "sobol"))
    assert all(g["sent"] == 8 * r * STEPS * k * (SOBOL_FIELDS + 9) for g in got)
    assert [g["range"][0] for g in got] + [got[-1]["range"][1]] == sorted([g["range"][0] for g in got] + [n_families * m])
    values = torch.cat([g["values"] for g in got]).numpy().reshape(n_families * m, STEPS, k)
    status = torch.cat([g["status"] for g in got]).numpy().reshape(n_families * m, STEPS)
    fp, _ = stand_in_families(n_families)
    flags = families_host(fp)[3]
    shift = np.zeros((STEPS, k))
    want = sobol_bootstrap_host(values, status, flags, 3, shift, seed=9, n_replicates=r).acc
    bound = weighted_bound(values, status, flags, 3, shift, bootstrap_weights(9, 0, n_families, r))
    acc = got[0]["acc"].numpy()
    assert np.array_equal(acc[..., :2], want[..., :2]) and np.all(np.abs(acc - want) <= bound) and want[..., SOBOL_COUNT].max() > 0


# ---- argument errors ----

def test_argument_errors():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_stats import COLUMNS, _stand_in

    fp, relative = stand_in_families(3)
    kw = dict(metric_columns=COLUMNS, reduce=True)
    with pytest.raises(ValueError, match="bootstrap= resamples the families .* it needs sobol=True"):
        ShardedEnsemble(_stand_in(), fp, relative, STEPS, bootstrap=8, **kw)
    with pytest.raises(ValueError, match="bootstrap_seed needs bootstrap="):
        ShardedEnsemble(_stand_in(), fp, relative, STEPS, sobol=True, bootstrap_seed=3, **kw)
    for bad in (0, -1, es.BOOTSTRAP_MAX_REPLICATES + 1):
        with pytest.raises(ValueError, match=f"bootstrap=: {bad} replicates, 1 to 1024 allowed"):
            ShardedEnsemble(_stand_in(), fp, relative, STEPS, sobol=True, bootstrap=bad, **kw)
    plain = ShardedEnsemble(_stand_in(), fp, relative, STEPS, sobol=True, **kw)
    assert plain.sobol_bootstrap_exchange_bytes_per_rank == 0 and "sobol_bootstrap" not in plain.stages
    with pytest.raises(ValueError, match="needs sobol=True and bootstrap=R"):
        plain.sobol_bootstrap()
    ready = ShardedEnsemble(_stand_in(), fp, relative, STEPS, sobol=True, bootstrap=es.BOOTSTRAP_MAX_REPLICATES, **kw)
    assert ready.sobol_bootstrap_accumulator is None
    with pytest.raises(RuntimeError, match="no step"):
        ready.sobol_bootstrap()
    from open_kinematics_amd import _lib

    assert {"okx_ensemble_bootstrap_weights", "okx_ensemble_sobol_bootstrap", "okx_ensemble_sobol_bootstrap_scratch_bytes"} <= set(_lib.EXPORTS)
