"""
The NumPy definitions of the main-effects pass (ensemble_stats.effects_edges, bin_factors_host, bin_lists_host, effects_host,
EffectsAccumulator, EnsembleEffects) against plain restatements: np.searchsorted for the bins, a triple loop in Python floats for the
accumulator, np.bincount for the indices - and ShardedEnsemble(reduce=True, factors=..., effects=...) on the stand-in program of
tests/test_dist.py.

Exact comparisons run on integer tables (|value - shift| <= 8: every difference, product and partial sum is an integer fp64 holds, so
every addition order gives the same bits); on real tables the brute-force loop adds in the definition's own order, so it is exact too.
"""

import numpy as np
import pytest
import torch

from open_kinematics_amd.ensemble_sample import IID, LHS, NORMAL, TRUNCATED, UNIFORM, SamplePlan, latents_from_units, sample_host
from open_kinematics_amd.ensemble_stats import (EFFECTS_COUNT, EFFECTS_FIELDS, EFFECTS_MAX_BINS, EFFECTS_MAX_FACTORS, EFFECTS_NO_BIN, EFFECTS_SUM,
                                                EFFECTS_SUMSQ, ENS_COUNT, ENS_SUM, ENS_SUMSQ, EffectsAccumulator, bin_factors_host, bin_lists_host,
                                                check_effects_arguments, effects_edges, effects_host, effects_terms, reduce_host)

U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- inputs the GPU tests share ----

def factor_table(g, f, b, seed):
    """``(factors [G, F], edges [F, B - 1])``: normal columns binned at their own order statistics - then, where the table is large
    enough, column 0 gets exact edge hits, both infinities, -0.0 and a NaN; column 1 (F >= 2) lies in ONE bin (below every edge) and
    column 2 (F >= 3) has repeated edges, so a bin between them is empty."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (g, f))
    edges = effects_edges(x, b)
    if f >= 3 and b >= 3:
        edges[2, 1] = edges[2, 0]
    if f >= 2 and b >= 2:
        x[:, 1] = edges[1, 0] - 1.0 - rng.random(g)
    if g >= 8 and b >= 2:
        x[1, 0], x[2, 0], x[3, 0], x[4, 0], x[5, 0], x[6, 0] = edges[0, 0], edges[0, -1], np.inf, -np.inf, -0.0, np.nan
        x[7, f - 1] = np.nan
    return x, edges


def integer_table(g, s, k, seed, with_mask=True):
    """``(values [G, S, K], status [G, S], mask [G] or None, shift [S, K])``: integers with |value - shift| <= 8.  From two geometries
    on, geometry 1 is rejected at ONE step (status byte), geometry 0 has a NaN in one column and - with a mask - the last geometry is
    masked; larger tables get a sprinkling of all three."""
    rng = np.random.default_rng(seed)
    shift = rng.integers(-5, 6, (s, k)).astype(np.float64)
    values = shift[None] + rng.integers(-8, 9, (g, s, k)).astype(np.float64)
    status = np.ones((g, s), dtype=np.uint8)
    mask = np.zeros(g, dtype=np.uint8) if with_mask else None
    if g >= 2:
        status[1, s - 1] = 2
        values[0, 0, k - 1] = np.nan
        if with_mask:
            mask[g - 1] = 1
    for _ in range(g // 12):
        status[rng.integers(0, g), rng.integers(0, s)] = rng.choice(np.array([0, 3, 5, 9], dtype=np.uint8))  # (9: advisory bit, still accepted)
        values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = rng.choice([np.inf, -np.inf, np.nan])
        if with_mask:
            mask[rng.integers(0, g)] = rng.choice(np.array([1, 2, 17], dtype=np.uint8))  # (2: bit 0 clear, the geometry counts)
    return values, status, mask, shift


def term_bound(values, status, mask, bins, n_bins, shift):
    """``[F, B, 3, S, K]``: 2 (n + 1) U sum |term| per cell, n the geometries of the cell's bin - two recursive sums of the same n terms,
    each within (n + 1) U sum |term| of the exact sum whatever its order (Higham, Accuracy and Stability, (4.4) with gamma_n <=
    (n + 1) U for n U << 1).  The terms are the host's own (``effects_terms``); COUNT's are integers: its sums are exact."""
    ok, d, _ = effects_terms(values, status, mask, shift)
    f = bins.shape[1]
    out = np.zeros((f, n_bins, EFFECTS_FIELDS) + d.shape[1:])
    for j in range(f):
        for b in range(n_bins):
            rows = bins[:, j] == b
            n = int(rows.sum())
            out[j, b, EFFECTS_SUM] = 2.0 * (n + 1) * U * np.abs(d[rows]).sum(axis=0)
            out[j, b, EFFECTS_SUMSQ] = 2.0 * (n + 1) * U * (d[rows] * d[rows]).sum(axis=0)
    return out


# ---- the bins ----

@pytest.mark.parametrize("g,f,b", [(1, 1, 1), (2, 3, 2), (67, 3, 16), (1000, 65, 2), (67, 1, 64), (1000, 3, 16)])
def test_bins_equal_searchsorted(g, f, b):
    x, edges = factor_table(g, f, b, 10 * g + f + b)
    got = bin_factors_host(x, edges)
    assert got.dtype == np.uint8 and got.shape == (g, f)
    for j in range(f):
        want = np.searchsorted(edges[j], x[:, j], side="right")
        want = np.where(np.isnan(x[:, j]), EFFECTS_NO_BIN, want)
        assert np.array_equal(got[:, j], want), j
    if g >= 8 and b >= 2:
        # on an edge: the upper bin; the infinities: the end bins; -0.0 as 0.0; NaN: in none
        assert got[1, 0] >= 1 and got[2, 0] == b - 1 and got[3, 0] == b - 1 and got[4, 0] == 0 and got[6, 0] == EFFECTS_NO_BIN
        assert got[5, 0] == bin_factors_host(np.zeros((1, 1)), edges[:1])[0, 0]
    if f >= 2 and b >= 2:
        assert np.all(got[:, 1] == 0)  # one bin holds everything
    order, offsets = bin_lists_host(got, b)
    assert order.dtype == np.int32 and offsets.dtype == np.int64 and order.shape == (f, g) and offsets.shape == (f, b + 1)
    for j in range(f):
        assert offsets[j, 0] == 0 and offsets[j, b] == (got[:, j] != EFFECTS_NO_BIN).sum() and np.all(order[j, offsets[j, b]:] == -1)
        for q in range(b):
            assert order[j, offsets[j, q] : offsets[j, q + 1]].tolist() == np.flatnonzero(got[:, j] == q).tolist()
    if f >= 3 and b >= 3 and g >= 67:
        assert offsets[2, 1] == offsets[2, 2]  # repeated edges: an empty bin


# ---- the accumulator ----

def plain_loops(values, status, mask, bins, n_bins, shift):
    """The accumulator restated with Python floats, one factor, bin, geometry and entry at a time."""
    g, s, k = values.shape
    f = bins.shape[1]
    acc = np.zeros((f, n_bins, EFFECTS_FIELDS, s, k))
    for j in range(f):
        for i in range(g):
            b = int(bins[i, j])
            if b == EFFECTS_NO_BIN or (mask is not None and int(mask[i]) & 1):
                continue
            for si in range(s):
                if status is not None and (int(status[i, si]) & 7) != 1:
                    continue
                for ki in range(k):
                    v = float(values[i, si, ki])
                    if not np.isfinite(v):
                        continue
                    d = v - float(shift[si, ki])
                    acc[j, b, EFFECTS_COUNT, si, ki] += 1.0
                    acc[j, b, EFFECTS_SUM, si, ki] += d
                    acc[j, b, EFFECTS_SUMSQ, si, ki] += d * d
    return acc


@pytest.mark.parametrize("integers", [True, False])
@pytest.mark.parametrize("g,s,k,f,b", [(1, 1, 1, 1, 1), (2, 3, 5, 3, 16), (67, 3, 5, 3, 16), (67, 2, 3, 5, 2), (40, 1, 2, 2, 64)])
def test_effects_host_equals_the_triple_loop(g, s, k, f, b, integers):
    x, edges = factor_table(g, f, b, g + f)
    bins = bin_factors_host(x, edges)
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(g, s, k, 100 * g + s, with_mask)
        if not integers:
            rng = np.random.default_rng(g)
            shift = rng.normal(0.0, 3.0, (s, k))
            values = np.where(np.isfinite(values), shift[None] + rng.normal(0.0, 1.0, (g, s, k)) * np.logspace(-3, 3, k)[None, None], values)
        got = effects_host(values, status, mask, bins, b, shift, edges)
        want = plain_loops(values, status, mask, bins, b, shift)
        assert np.array_equal(bits(got.acc), bits(want))
        assert np.array_equal(got.edges, edges) and np.array_equal(got.shift, shift) and got.acc.shape == (f, b, EFFECTS_FIELDS, s, k)
    plain = effects_host(values, None, None, bins, b, shift)
    assert np.array_equal(bits(plain.acc), bits(plain_loops(values, None, None, bins, b, shift))) and np.all(np.isnan(plain.edges))


def test_counts_add_up_to_the_reduction():
    g, s, k, f, b = 200, 3, 5, 4, 16
    x, edges = factor_table(g, f, b, 3)
    bins = bin_factors_host(x, edges)
    values, status, _, shift = integer_table(g, s, k, 8, False)
    acc = effects_host(values, status, None, bins, b, shift, edges).acc
    whole = reduce_host(values, status, None, shift).acc
    clean = [j for j in range(f) if not np.isnan(x[:, j]).any()]
    assert clean and len(clean) < f
    for j in range(f):
        total = acc[j, :, EFFECTS_COUNT].sum(axis=0)
        assert np.array_equal(total, whole[..., ENS_COUNT]) == (j in clean)
        assert np.all(total <= whole[..., ENS_COUNT])


def test_one_bin_is_the_reduction():
    g, s, k, f = 67, 3, 5, 3
    values, status, _, shift = integer_table(g, s, k, 5, False)
    bins = np.zeros((g, f), dtype=np.uint8)
    acc = effects_host(values, status, None, bins, 1, shift).acc
    whole = reduce_host(values, status, None, shift).acc
    for j in range(f):
        for field, ens in ((EFFECTS_COUNT, ENS_COUNT), (EFFECTS_SUM, ENS_SUM), (EFFECTS_SUMSQ, ENS_SUMSQ)):
            assert np.array_equal(acc[j, 0, field], whole[..., ens])
    assert effects_edges(np.zeros((4, f)), 1).shape == (f, 0)


def test_chunks_merge_to_the_whole_and_merge_checks_its_tables():
    g, s, k, f, b = 67, 3, 5, 3, 16
    x, edges = factor_table(g, f, b, 4)
    bins = bin_factors_host(x, edges)
    values, status, mask, shift = integer_table(g, s, k, 6)
    whole = effects_host(values, status, mask, bins, b, shift, edges)
    cut = 29
    one = effects_host(values[:cut], status[:cut], mask[:cut], bins[:cut], b, shift, edges)
    two = effects_host(values[cut:], status[cut:], mask[cut:], bins[cut:], b, shift, edges)
    merged = one.merge(two)
    assert np.array_equal(merged.acc, whole.acc) and merged.acc is not one.acc
    empty = EffectsAccumulator.empty(s, k, shift, edges)
    assert np.array_equal(empty.merge(whole).acc, whole.acc) and empty.n_factors == f and empty.n_bins == b
    moved = edges.copy()
    moved[0, 0] -= 1.0
    with pytest.raises(ValueError, match="different edges"):
        one.merge(effects_host(values[cut:], status[cut:], mask[cut:], bins[cut:], b, shift, moved))
    with pytest.raises(ValueError, match="different shifts"):
        one.merge(effects_host(values[cut:], status[cut:], mask[cut:], bins[cut:], b, shift + 1.0, edges))
    with pytest.raises(ValueError, match="different shapes"):
        one.merge(effects_host(values[cut:, :2], status[cut:, :2], mask[cut:], bins[cut:], b, shift[:2], edges))
    # torch tensors merge alike, and numpy() / to() carry every table
    t = one.to("cpu")
    assert isinstance(t.acc, torch.Tensor) and isinstance(t.edges, torch.Tensor)
    assert np.array_equal(t.merge(two.to("cpu")).numpy().acc, whole.acc) and one.numpy() is one
    with pytest.raises(ValueError, match=r"acc must be \[F, B, EFFECTS_FIELDS, S, K\]"):
        EffectsAccumulator(whole.acc, shift, edges[:, :-1])


# ---- finalize ----

def test_finalize_on_a_step_function_of_factor_zero():
    g, s, k, f, b = 400, 2, 3, 3, 8
    rng = np.random.default_rng(12)
    x = rng.normal(0.0, 1.0, (g, f))
    edges = effects_edges(x, b)
    bins = bin_factors_host(x, edges)
    level = rng.permutation(np.arange(b) - 3).astype(np.float64)  # an integer level per bin
    values = np.broadcast_to(level[bins[:, 0]][:, None, None], (g, s, k)) + np.arange(k)[None, None, :]
    shift = np.ones((s, k))
    out = effects_host(values, None, None, bins, b, shift, edges, ("a", "b", "c")).finalize()
    assert out.factor_names == ["a", "b", "c"] and np.array_equal(out.edges, edges)
    assert np.all(np.abs(out.first[0] - 1.0) <= 1e-12) and np.all(np.abs(out.first_corrected[0] - 1.0) <= 1e-12)
    assert np.all(out.std[0] == 0.0) and np.array_equal(out.mean[0], level[:, None, None] + np.arange(k)[None, None, :] + np.zeros((b, s, k)))
    assert np.all(out.first[1:] < 0.2) and np.all(out.first_corrected[1:] < out.first[1:])  # the other factors explain next to nothing
    assert np.array_equal(out.count.sum(axis=1), np.full((f, s, k), g)) and np.array_equal(out.total_count, np.full((f, s, k), g))
    assert np.allclose(out.total_mean[0], values.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(out.total_variance[0], values.var(axis=0, ddof=1), rtol=1e-12, atol=0)


def test_finalize_on_a_constant_table_and_on_empty_bins():
    g, s, k, f, b = 60, 1, 2, 2, 4
    rng = np.random.default_rng(2)
    x = rng.normal(0.0, 1.0, (g, f))
    edges = effects_edges(x, b)
    edges[1, 1] = edges[1, 0]  # factor 1: bin 1 is empty
    bins = bin_factors_host(x, edges)
    values = np.full((g, s, k), 3.0)
    out = effects_host(values, None, None, bins, b, np.zeros((s, k)), edges).finalize()
    assert np.all(np.isnan(out.first)) and np.all(np.isnan(out.first_corrected)) and np.all(out.total_variance == 0.0)
    assert np.all(out.count[1, 1] == 0) and np.all(np.isnan(out.mean[1, 1])) and np.all(np.isnan(out.std[1, 1])) and np.all(out.mean[0] == 3.0)
    # an empty bin is not counted in B_nonempty: the restatement below takes the bins that have a member
    values = rng.normal(0.0, 1.0, (g, s, k)) + x[:, 1, None, None] ** 2
    out = effects_host(values, None, None, bins, b, np.zeros((s, k)), edges).finalize()
    check_against_bincount(out, values, bins, b)
    # every bin holds one geometry: n == B_nonempty, nothing is left for the within-bin variance
    lone = effects_host(values[:4], None, None, np.arange(4, dtype=np.uint8)[:, None], 4, np.zeros((s, k))).finalize()
    assert np.all(np.isnan(lone.first)) and np.all(np.isnan(lone.first_corrected)) and np.all(np.isnan(lone.std)) and np.all(lone.count == 1)


def check_against_bincount(out, values, bins, n_bins):
    g, s, k = values.shape
    for j in range(bins.shape[1]):
        inside = bins[:, j] != EFFECTS_NO_BIN
        for si in range(s):
            for ki in range(k):
                y, q = values[inside, si, ki], bins[inside, j].astype(np.int64)
                n_b = np.bincount(q, minlength=n_bins).astype(np.float64)
                s_b = np.bincount(q, weights=y, minlength=n_bins)
                filled = n_b > 0
                n, mean = y.size, y.mean()
                ssb = float((n_b[filled] * (s_b[filled] / n_b[filled] - mean) ** 2).sum())
                sst = float(((y - mean) ** 2).sum())
                msw = (sst - ssb) / (n - filled.sum())
                assert abs(out.first[j, si, ki] - ssb / sst) <= 1e-10, (j, si, ki)
                assert abs(out.first_corrected[j, si, ki] - (ssb - (filled.sum() - 1) * msw) / sst) <= 1e-10, (j, si, ki)
                assert np.allclose(out.mean[j, filled, si, ki], s_b[filled] / n_b[filled], rtol=0, atol=1e-12)
                assert np.array_equal(out.count[j, :, si, ki], n_b.astype(np.int64)) and out.total_count[j, si, ki] == n


def test_first_order_indices_against_bincount():
    g, s, k, f, b = 500, 2, 3, 4, 16
    rng = np.random.default_rng(31)
    x = rng.normal(0.0, 1.0, (g, f))
    x[5, 2] = np.nan
    edges = effects_edges(np.nan_to_num(x), b)
    bins = bin_factors_host(x, edges)
    # quadratic in factor 0 (no linear sensitivity), a threshold in factor 1, linear in factor 2, noise
    values = (x[:, 0] ** 2)[:, None, None] * np.arange(1, k + 1)[None, None] + np.where(x[:, 1] > 1.0, 2.0, 0.0)[:, None, None] \
        + 0.5 * np.nan_to_num(x[:, 2])[:, None, None] + rng.normal(0.0, 0.3, (g, s, k))
    shift = values[0].copy()
    out = effects_host(values, None, None, bins, b, shift, edges).finalize()
    check_against_bincount(out, values, bins, b)
    assert np.all(out.first[0] > 0.4) and np.all(out.first[3] < 0.1) and out.total_count[2, 0, 0] == g - 1
    slope = np.polyfit(x[:, 0], values[:, 0, 0], 1)[0]
    assert abs(slope) * x[:, 0].std() < 0.2 * values[:, 0, 0].std()  # what the linear fit alone would have called "no sensitivity"


# ---- the edges ----

def plan_of(kinds, n_total=0, stratify=IID, guards=(), max_attempts=1, seed=5):
    z = len(kinds)
    rng = np.random.default_rng(z)
    nominal = rng.normal(0.0, 50.0, ((z + 2) // 3 + 1, 3))
    if guards:
        nominal.reshape(-1)[0] = 0.0
    return SamplePlan(nominal, np.arange(z, dtype=np.int32), np.asarray(kinds, dtype=np.int32), 0.5 + 2.0 * rng.random(z), None, 0.25 + rng.random(z),
                      stratify, n_total, seed, guards, max_attempts)


@pytest.mark.parametrize("b", [1, 2, 16, 64])
def test_analytic_edges_are_the_plans_inverse_cdfs(b):
    plan = plan_of([NORMAL, UNIFORM, TRUNCATED, NORMAL, TRUNCATED])
    edges = effects_edges(plan, b)
    assert edges.shape == (5, b - 1) and edges.flags["C_CONTIGUOUS"]
    for k in range(1, b):
        want = latents_from_units(plan, np.full((1, 5), k / b))[0]
        assert np.array_equal(bits(edges[:, k - 1]), bits(want))
    check_effects_arguments(b, 5, edges)  # finite and non-decreasing
    if b == 2:
        assert np.all(edges[:, 0] == 0.0)  # the medians of symmetric latents


def test_table_edges_are_order_statistics():
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.0, (67, 3))
    x[:, 2] = np.round(x[:, 2])  # ties
    for b in (1, 2, 16, 64):
        edges = effects_edges(x, b)
        assert edges.shape == (3, b - 1)
        for j in range(3):
            ranked = np.sort(x[:, j])
            assert all(e in x[:, j] for e in edges[j]) and np.all(np.diff(edges[j]) >= 0)
            for k in range(1, b):
                assert edges[j, k - 1] == ranked[int(np.ceil(k * 67 / b)) - 1]
    assert np.array_equal(effects_edges(torch.as_tensor(x), 16), effects_edges(x, 16))
    with pytest.raises(ValueError, match=r"factors \[G, F\] with G >= 1"):
        effects_edges(np.zeros((0, 3)), 4)


@pytest.mark.parametrize("b", [2, 16])
def test_lhs_fills_every_analytic_bin_evenly(b):
    g = 8 * b
    plan = plan_of([NORMAL, UNIFORM, TRUNCATED, NORMAL, UNIFORM, TRUNCATED], n_total=g, stratify=LHS, guards=((0, 0, 1.0, 0.0),), max_attempts=4)
    _, latents, _, flags = sample_host(plan)
    assert (flags >> 4).max() > 0  # some geometries were redrawn: they stay in their strata
    bins = bin_factors_host(latents, effects_edges(plan, b))
    for j in range(plan.n_latents):
        assert np.array_equal(np.bincount(bins[:, j], minlength=b), np.full(b, g // b)), j


# ---- the argument checks ----

def test_argument_checks_speak_the_librarys_words():
    ok_edges = np.asarray([[0.0, 1.0, 1.0], [-1.0, 0.0, 2.0]])
    assert check_effects_arguments(4, 2, ok_edges)[0] == 4
    for n_bins in (0, EFFECTS_MAX_BINS + 1, True, 2.5):
        with pytest.raises(ValueError, match=rf"okx_ensemble_effects: {n_bins} bins, 1 to 64 allowed"):
            check_effects_arguments(n_bins, 2)
    for n_factors in (0, EFFECTS_MAX_FACTORS + 1):
        with pytest.raises(ValueError, match=rf"okx_ensemble_effects: {n_factors} factors, 1 to 288 allowed"):
            check_effects_arguments(4, n_factors)
    with pytest.raises(ValueError, match=r"okx_ensemble_bin: edges must be \[2, 3\] \(factors, bins - 1\), got \[2, 2\]"):
        check_effects_arguments(4, 2, ok_edges[:, :2])
    for bad in (np.nan, np.inf):
        edges = ok_edges.copy()
        edges[1, 2] = bad
        with pytest.raises(ValueError, match=rf"okx_ensemble_bin: edge 2 of factor 1 is {bad:g}, not finite"):
            check_effects_arguments(4, 2, edges)
    edges = ok_edges.copy()
    edges[0, 2] = 0.5
    with pytest.raises(ValueError, match=r"okx_ensemble_bin: the edges of factor 0 decrease at edge 2 \(0.5 < 1\)"):
        check_effects_arguments(4, 2, edges)
    bins = np.asarray([[0, 3], [EFFECTS_NO_BIN, 4]], dtype=np.uint8)
    with pytest.raises(ValueError, match=r"okx_ensemble_effects: the bin of geometry 1 for factor 1 is 4, neither below 4 nor 255"):
        check_effects_arguments(4, 2, None, bins)
    with pytest.raises(ValueError, match=r"okx_ensemble_effects: bins must be uint8 \[G, 2\]"):
        check_effects_arguments(4, 2, None, bins.astype(np.int32))
    values = np.zeros((2, 1, 1))
    with pytest.raises(ValueError, match="neither below 4 nor 255"):
        effects_host(values, None, None, bins, 4)
    with pytest.raises(ValueError, match=r"bins must be uint8 \[2, F\], one row per geometry"):
        effects_host(values, None, None, np.zeros((3, 2), dtype=np.uint8), 4)
    with pytest.raises(ValueError, match="bins are needed"):
        effects_host(values)
    with pytest.raises(ValueError, match="the shift must be finite"):
        effects_host(values, None, None, np.zeros((2, 1), dtype=np.uint8), 1, np.full((1, 1), np.nan))
    with pytest.raises(ValueError, match="decrease at edge 1"):
        bin_factors_host(np.zeros((2, 1)), np.asarray([[1.0, 0.0]]))


def test_constants_match_the_header():
    import os
    import re

    from conftest import REPO
    from open_kinematics_amd import _abi, ensemble_stats as es

    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        header = dict((name, int(value)) for name, value in re.findall(r"\bOKX_((?:ENS_)?EFFECTS_[A-Z_]+) = (\d+)", fh.read()))
    assert sorted(header) == ["EFFECTS_COUNT", "EFFECTS_FIELDS", "EFFECTS_SUM", "EFFECTS_SUMSQ", "ENS_EFFECTS_MAX_BINS", "ENS_EFFECTS_MAX_FACTORS",
                              "ENS_EFFECTS_NO_BIN"]
    for name, value in header.items():
        assert getattr(_abi, name) == value, name
        assert getattr(es, name.replace("ENS_EFFECTS", "EFFECTS")) == value, name


# ---- ShardedEnsemble(reduce=True, factors=..., effects=...) on the stand-in program, one process ----

@pytest.mark.parametrize("chunks", [1, 3])
def test_sharded_ensemble_effects_on_the_stand_in(chunks):
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_sample import STEPS, stand_in_plan
    from test_ensemble_stats import COLUMNS, _stand_in

    g, b = 24, 4
    plan, relative = stand_in_plan(g)
    kw = dict(chunks=chunks, metric_columns=COLUMNS, reduce=True)
    pipe = ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", effects=b, **kw)
    acc = pipe.step()
    _, latents, _, flags = sample_host(plan)
    edges = effects_edges(plan, b)
    mine = pipe.effects_accumulator.numpy()
    assert np.array_equal(bits(mine.edges), bits(edges)) and mine.acc.shape == (9, b, EFFECTS_FIELDS, STEPS, len(COLUMNS))
    values = pipe.metric_local.numpy().reshape(g, STEPS, len(COLUMNS))
    status = pipe.info_local[:, 32].numpy().reshape(g, STEPS)
    bins = bin_factors_host(latents, edges)
    want = effects_host(values, status, flags, bins, b, acc.shift.numpy(), edges)
    assert np.array_equal(mine.acc[:, :, EFFECTS_COUNT], want.acc[:, :, EFFECTS_COUNT])
    assert np.all(np.abs(mine.acc - want.acc) <= term_bound(values, status, flags, bins, b, acc.shift.numpy()))
    if chunks == 1:
        assert np.array_equal(bits(mine.acc), bits(want.acc))
    out = pipe.effects()
    assert out.first.shape == (9, STEPS, len(COLUMNS)) and out.factor_names == plan.factor_names() and pipe.effects_exchange_bytes_per_rank == 0
    assert np.array_equal(out.count.sum(axis=1)[0], acc.acc[..., ENS_COUNT].numpy().astype(np.int64))  # LHS latents: no NaN, every geometry in a bin
    first = mine.acc.copy()
    pipe.step()  # a second step starts from nothing
    assert np.array_equal(bits(pipe.effects_accumulator.numpy().acc), bits(first))
    # a table of factors: the edges are its order statistics; given edges are taken as they are
    table = torch.as_tensor(sample_host(plan)[0])
    given = ShardedEnsemble(_stand_in(), table, relative, STEPS, factors=latents, effects={"bins": b, "edges": edges}, **kw)
    given.step()
    got, unmasked = given.effects_accumulator.numpy().acc, effects_host(values, status, None, bins, b, acc.shift.numpy(), edges).acc  # (a table: no flags)
    assert np.array_equal(got[:, :, EFFECTS_COUNT], unmasked[:, :, EFFECTS_COUNT])
    assert np.all(np.abs(got - unmasked) <= term_bound(values, status, None, bins, b, acc.shift.numpy())) and (chunks > 1 or np.array_equal(bits(got), bits(unmasked)))
    ranked = ShardedEnsemble(_stand_in(), table, relative, STEPS, factors=latents, effects=b, **kw)
    assert np.array_equal(ranked.stages["effects"].edges, effects_edges(latents, b))


def test_sharded_ensemble_effects_refuses_what_it_cannot_bin():
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_ensemble_sample import STEPS, stand_in_plan
    from test_ensemble_stats import COLUMNS, _stand_in

    plan, relative = stand_in_plan(8)
    kw = dict(metric_columns=COLUMNS, reduce=True)
    with pytest.raises(ValueError, match="effects= bins the factors of the reduced ensemble: it needs reduce=True and factors"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, effects=4, **kw)
    with pytest.raises(ValueError, match="65 bins, 1 to 64 allowed"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", effects=65, **kw)
    with pytest.raises(ValueError, match=r"effects= takes an integer or dict\(bins=, edges=\)"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", effects={"edges": None}, **kw)
    with pytest.raises(ValueError, match=r"effects\(\) needs effects=n_bins"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", **kw).effects()
    with pytest.raises(RuntimeError, match="no step"):
        ShardedEnsemble(_stand_in(), plan, relative, STEPS, factors="sampled", effects=4, **kw).effects()
