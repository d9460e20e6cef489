"""
GPU: okx_ensemble_bin (DeviceProgram.bin_factors), okx_ensemble_effects (DeviceProgram.effects_ensemble) and
ShardedEnsemble(reduce=True, factors="sampled", effects=...) against the NumPy definitions ensemble_stats.bin_factors_host,
bin_lists_host and effects_host.

The bins are compared byte for byte in all three outputs.  The accumulator is compared exactly on the integer tables of
tests/test_ensemble_effects.py (|value - shift| <= 8: every difference, product and partial sum is an integer fp64 holds) and, on real
tables, within 2 (n + 1) U sum |term| of effects_host per cell, n the geometries of the cell's bin, the bound computed from the host's
own terms (``term_bound``; the terms are bit-identical, contraction is off in the unit): nothing here comes from an outcome.

The plan the shapes are chosen from (okx_effects.hip): the list pass places 256 geometries a round (G = 1000: four rounds, the last
partial; G = 67: one partial round); in the effects pass a lane owns one of 64 entries of a tile ((S, K) = (5, 17): 85 entries, a second,
partial tile) and walks a bin's list eight rows at a time (lists of 0, 1, ..., 500 rows: with and without the unrolled body and its tail).
"""

import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_sample import sample_host
from open_kinematics_amd.ensemble_stats import (EFFECTS_COUNT, EFFECTS_FIELDS, EFFECTS_NO_BIN, EffectsAccumulator, bin_factors_host, bin_lists_host,
                                                effects_edges, effects_host)
from test_ensemble_effects import bits, factor_table, integer_table, term_bound

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


def upload(values, status, mask, pad=3, stride=40):
    """The table with ``ld = K + pad`` and its status bytes ``stride`` apart, the rest filled with what must never be read as data."""
    g, s, k = values.shape
    wide = torch.full((g * s, k + pad), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :k] = torch.as_tensor(np.ascontiguousarray(values).reshape(g * s, k), device=DEV)
    st = None
    if status is not None:
        info = torch.full((g * s, stride), 2, dtype=torch.uint8, device=DEV)
        info[:, 32 % stride] = torch.as_tensor(np.ascontiguousarray(status).reshape(-1), device=DEV)
        st = info[:, 32 % stride]
    return wide[:, :k], st, None if mask is None else torch.as_tensor(mask, device=DEV)


def upload_factors(x, pad=2):
    """The factor table with ``ldf = F + pad``, the padding NaN."""
    g, f = x.shape
    wide = torch.full((g, f + pad), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :f] = torch.as_tensor(x, device=DEV)
    return wide[:, :f]


# ---- the bins ----

@pytest.mark.parametrize("g", [1, 2, 67, 1000])
@pytest.mark.parametrize("b", [1, 2, 16, 64])
@pytest.mark.parametrize("f", [1, 3, 65])
def test_bins_equal_the_host_byte_for_byte(dp, g, f, b):
    x, edges = factor_table(g, f, b, 10 * g + f + b)
    want = bin_factors_host(x, edges)
    order, offsets = bin_lists_host(want, b)
    factors = upload_factors(x)
    assert g == 1 or factors.stride(0) == f + 2
    got = dp.bin_factors(factors, edges)
    torch.cuda.synchronize()
    assert got.n_bins == b and np.array_equal(got.edges.cpu().numpy(), edges)
    assert np.array_equal(got.bins.cpu().numpy(), want)
    assert np.array_equal(got.offsets.cpu().numpy(), offsets)
    assert np.array_equal(got.order.cpu().numpy(), order)
    if g >= 67 and b >= 2:
        assert (want == EFFECTS_NO_BIN).sum() >= 1  # a NaN factor: the inputs are worth the test
        if f >= 2:
            assert offsets[1, 1] == g or np.isnan(x[:, 1]).any()  # all in one bin
        if f >= 3 and b >= 3:
            assert offsets[2, 1] == offsets[2, 2]  # an empty bin
    # again into the same tables: the same bytes
    got.bins.fill_(7), got.order.fill_(-9), got.offsets.fill_(-9)
    dp.bin_factors(factors, out=got)
    torch.cuda.synchronize()
    assert np.array_equal(got.bins.cpu().numpy(), want) and np.array_equal(got.order.cpu().numpy(), order) and np.array_equal(got.offsets.cpu().numpy(), offsets)


# ---- the accumulator, exact ----

EXACT = [(g, s, k, f, b) for g in (1, 2, 67, 1000) for s, k in ((1, 1), (3, 5), (5, 17)) for f, b in ((1, 1), (3, 16), (65, 2))]


@pytest.mark.parametrize("g,s,k,f,b", EXACT)
def test_exact_integer_tables(dp, g, s, k, f, b):
    x, edges = factor_table(g, f, b, g + f)
    host_bins = bin_factors_host(x, edges)
    bins = dp.bin_factors(upload_factors(x), edges)
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(g, s, k, 1000 * g + 10 * f + s, with_mask)
        want = effects_host(values, status, mask, host_bins, b, shift, edges).acc
        v, st, mk = upload(values, status, mask)
        assert v.stride(0) == k + 3 and st.stride(0) == 40
        acc = dp.effects_ensemble(v, steps_per_geometry=s, bins=bins, status=st, mask=mk, shift=shift)
        torch.cuda.synchronize()
        got = acc.numpy().acc
        bad = np.argwhere(got != want)
        assert bad.size == 0, (bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        # COUNT over the bins plus what the rule rejected is G wherever the factor has no NaN
        counted = effects_host(values, status, mask, np.zeros((g, 1), dtype=np.uint8), 1, shift).acc[0, 0, EFFECTS_COUNT]  # of all geometries
        rejected = g - counted
        for j in range(f):
            if not np.isnan(x[:, j]).any():
                assert np.array_equal(got[j, :, EFFECTS_COUNT].sum(axis=0) + rejected, np.full((s, k), float(g)))
        if g >= 67:
            assert 0 < rejected.max() < g  # the inputs are worth the test
        # two chunks cut at an odd geometry, the second accumulated onto the first: bit-equal to the whole
        cut = g // 2 if (g // 2) % 2 else g // 2 + 1
        cut = min(cut, g)
        out = EffectsAccumulator(torch.full_like(acc.acc, -7.0), acc.shift, acc.edges)
        factors = upload_factors(x)
        one, two = dp.bin_factors(factors[:cut], edges), dp.bin_factors(factors[cut:], edges)
        dp.effects_ensemble(v[: cut * s], steps_per_geometry=s, bins=one, status=st[: cut * s], mask=None if mk is None else mk[:cut], out=out)
        torch.cuda.synchronize()
        first = out.numpy().acc
        assert np.array_equal(first, effects_host(values[:cut], status[:cut], None if mask is None else mask[:cut], host_bins[:cut], b, shift, edges).acc)  # -7 overwritten
        dp.effects_ensemble(v[cut * s :], steps_per_geometry=s, bins=two, status=st[cut * s :], mask=None if mk is None else mk[cut:], out=out, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(out.numpy().acc, want)
    # no status bytes: every state accepted
    plain = dp.effects_ensemble(v, steps_per_geometry=s, bins=bins, shift=shift)
    torch.cuda.synchronize()
    assert np.array_equal(plain.numpy().acc, effects_host(values, None, None, host_bins, b, shift, edges).acc)


def test_no_geometry_leaves_zeros_or_what_was_there(dp):
    s, k, f, b = 3, 5, 3, 16
    edges = effects_edges(np.random.default_rng(0).normal(size=(50, f)), b)
    bins = dp.bin_factors(torch.empty((0, f), dtype=torch.float64, device=DEV), edges)
    torch.cuda.synchronize()
    assert tuple(bins.order.shape) == (f, 0) and tuple(bins.offsets.shape) == (f, b + 1) and not bins.offsets.any()
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    empty = torch.empty((0, k), dtype=torch.float64, device=DEV)
    acc = dp.effects_ensemble(empty, steps_per_geometry=s, bins=bins, shift=shift)
    torch.cuda.synchronize()
    assert tuple(acc.acc.shape) == (f, b, EFFECTS_FIELDS, s, k) and not acc.acc.any()
    acc.acc.fill_(5.0)
    dp.effects_ensemble(empty, steps_per_geometry=s, bins=bins, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert bool((acc.acc == 5.0).all())
    dp.effects_ensemble(empty, steps_per_geometry=s, bins=bins, out=acc)
    torch.cuda.synchronize()
    assert not acc.acc.any()


# ---- the accumulator, real data ----

def test_real_table_within_the_summation_bound_and_the_same_bits_again(dp):
    g, s, k, f, b = 1000, 3, 5, 3, 16
    rng = np.random.default_rng(5)
    shift = rng.normal(0.0, 3.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (g, s, k)) * np.logspace(-3, 3, k)[None, None]
    _, status, mask, _ = integer_table(g, s, k, 77)
    x, edges = factor_table(g, f, b, 9)
    host_bins = bin_factors_host(x, edges)
    want = effects_host(values, status, mask, host_bins, b, shift, edges).acc
    bound = term_bound(values, status, mask, host_bins, b, shift)
    v, st, mk = upload(values, status, mask)
    bins = dp.bin_factors(upload_factors(x), edges)
    acc = dp.effects_ensemble(v, steps_per_geometry=s, bins=bins, status=st, mask=mk, shift=shift)
    torch.cuda.synchronize()
    got = acc.numpy().acc
    print("largest |device - host| / bound:", float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0))))
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got[:, :, EFFECTS_COUNT], want[:, :, EFFECTS_COUNT])
    again = dp.effects_ensemble(v, steps_per_geometry=s, bins=dp.bin_factors(upload_factors(x), edges), status=st, mask=mk, shift=shift)
    torch.cuda.synchronize()
    assert torch.equal(again.acc.view(torch.int64), acc.acc.view(torch.int64))  # bit for bit, run to run
    out = acc.finalize()
    assert out.first.shape == (f, s, k) and out.mean.shape == (f, b, s, k) and np.all(np.isfinite(out.first[0]))


# ---- the chain ----

STEPS = 3


@pytest.fixture(scope="module")
def chain():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_effects_rate import build

    return build(32, STEPS, DEV, n_points=2)


def test_the_chain_on_two_points(chain):
    """hardpoint_plan on two points of data/geometry.yaml (6 latents under LHS), 32 geometries, 3 bump steps, 4 bins, one and two chunks."""
    import open_kinematics_amd.dist as okd

    device_program, plan, rel, columns = chain
    g, b, k = 32, 4, len(columns)
    assert (plan.n_latents, plan.n_total) == (6, g)
    _, latents, _, flags = sample_host(plan)
    edges = effects_edges(plan, b)
    host_bins = bin_factors_host(latents, edges)
    assert all(np.array_equal(np.bincount(host_bins[:, j], minlength=b), np.full(b, g // b)) for j in range(6))  # LHS: every bin evenly filled
    accs = []
    for chunks in (1, 2):
        pipe = okd.ShardedEnsemble(device_program, plan, rel, STEPS, metric_columns=columns, reduce=True, factors="sampled", effects=b, chunks=chunks,
                                   chain_len=1, predictor=False)
        pipe.step()
        torch.cuda.synchronize()
        assert len(pipe.pieces) == chunks and np.array_equal(pipe.sampled_flags.cpu().numpy(), flags)
        values = pipe.metric_local.cpu().numpy().reshape(g, STEPS, k)
        status = pipe.info_local[:, 32].cpu().numpy().reshape(g, STEPS)
        mine = pipe.effects_accumulator.numpy()
        shift = mine.shift
        assert np.array_equal(bits(mine.edges), bits(edges))
        want = effects_host(values, status, flags, host_bins, b, shift, edges).acc
        bound = term_bound(values, status, flags, host_bins, b, shift)
        assert np.all(np.abs(mine.acc - want) <= bound) and np.array_equal(mine.acc[:, :, EFFECTS_COUNT], want[:, :, EFFECTS_COUNT])
        out = pipe.effects()
        assert out.first.shape == (6, STEPS, k) and out.count.shape == (6, b, STEPS, k) and out.factor_names == plan.factor_names()
        assert out.total_count.max() > b and pipe.effects_exchange_bytes_per_rank == 0
        accs.append(mine.acc)
    assert np.array_equal(accs[0][:, :, EFFECTS_COUNT], accs[1][:, :, EFFECTS_COUNT])
    with pytest.raises(ValueError, match="effects= bins the factors of the reduced ensemble: it needs reduce=True and factors"):
        okd.ShardedEnsemble(device_program, plan, rel, STEPS, metric_columns=columns, reduce=True, effects=b, chain_len=1, predictor=False)


def test_error_paths_launch_nothing(dp):
    import ctypes as C

    from open_kinematics_amd import _lib

    lib = dp.lib
    s, k, f, b, g = 2, 3, 2, 4, 5
    table = torch.zeros((g * s, k), dtype=torch.float64, device=DEV)
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    acc = torch.full((f, b, EFFECTS_FIELDS, s, k), -3.0, dtype=torch.float64, device=DEV)
    x = torch.as_tensor(np.random.default_rng(1).normal(size=(g, f)), device=DEV)
    edges = effects_edges(x.cpu().numpy(), b)
    bins = dp.bin_factors(x, edges)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731

    def call(n=g, steps=s, columns=k, values=table, ld=k, factors=f, n_bins=b, order=bins.order, offsets=bins.offsets):
        return lib.okx_ensemble_effects(n, steps, columns, ptr(values), ld, None, 0, None, factors, n_bins, ptr(order), ptr(offsets), ptr(shift), 0, ptr(acc), None)

    for kw, words in ((dict(n=-1), "negative geometry, step or column count"), (dict(ld=k - 1), "null table or ld < n_columns"),
                      (dict(values=None), "null table or ld < n_columns"), (dict(factors=0), "0 factors, 1 to 288 allowed"),
                      (dict(factors=289), "289 factors, 1 to 288 allowed"), (dict(n_bins=0), "0 bins, 1 to 64 allowed"), (dict(n_bins=65), "65 bins, 1 to 64 allowed"),
                      (dict(order=None), "null order or offsets table"), (dict(offsets=None), "null order or offsets table"),
                      (dict(n=1 << 31), "too many geometries for one call"), (dict(steps=1 << 31), "too many entries for one call")):
        assert call(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_effects" in _lib.last_error(), (kw, _lib.last_error())

    def bin_call(n=g, factors=f, table=x, ldf=f, n_bins=b, offsets=bins.offsets):
        return lib.okx_ensemble_bin(n, factors, ptr(table), ldf, ptr(bins.edges), n_bins, ptr(bins.bins), ptr(bins.order), ptr(offsets), None)

    for kw, words in ((dict(n=-1), "negative geometry, step or column count"), (dict(ldf=f - 1), "null factor table or ldf < n_factors"),
                      (dict(table=None), "null factor table or ldf < n_factors"), (dict(factors=289), "289 factors, 1 to 288 allowed"),
                      (dict(n_bins=65), "65 bins, 1 to 64 allowed"), (dict(offsets=None), "null offsets table")):
        assert bin_call(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_bin" in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((acc == -3.0).all())  # nothing was launched
    assert call() == 0 and bin_call() == 0
    torch.cuda.synchronize()
    assert bool((acc[:, :, EFFECTS_COUNT].sum(dim=1) == g).all())
    # the Python layer
    with pytest.raises(ValueError, match="accumulate=True needs"):
        dp.effects_ensemble(table, steps_per_geometry=s, bins=bins, accumulate=True)
    with pytest.raises(ValueError, match="out= carries its own shift"):
        dp.effects_ensemble(table, steps_per_geometry=s, bins=bins, shift=shift, out=EffectsAccumulator(acc, shift, bins.edges))
    with pytest.raises(ValueError, match="mask must be"):
        dp.effects_ensemble(table, steps_per_geometry=s, bins=bins, mask=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="of the table's 4 geometries"):
        dp.effects_ensemble(table[: 4 * s], steps_per_geometry=s, bins=bins)
    with pytest.raises(ValueError, match="bins must be the EffectBins of bin_factors"):
        dp.effects_ensemble(table, steps_per_geometry=s, bins=bins.bins)
    with pytest.raises(ValueError, match="out= carries its own edges"):
        dp.bin_factors(x, edges, out=bins)
    with pytest.raises(ValueError, match="edges are needed"):
        dp.bin_factors(x)
    with pytest.raises(ValueError, match="decrease at edge 1"):
        dp.bin_factors(x, edges[:, ::-1].copy())
    with pytest.raises(ValueError, match=r"out must hold contiguous device tables bins \[4, 2\]"):
        dp.bin_factors(x[:4], out=bins)
