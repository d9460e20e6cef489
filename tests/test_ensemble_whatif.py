"""
The NumPy definitions of the tolerance what-ifs - ensemble_sample.exp_unit, tolerance_scenarios, tilt_weights_host and
ensemble_stats.reweigh_host, ReweighAccumulator, EnsembleWhatIf - against math.exp, hand-computed scenario rows, the reduction's own
sums and the analytic answer of a synthetic column; and ShardedEnsemble(reduce=True, factors="sampled", whatif=...) on the stand-in
program of tests/test_dist.py, in one process and over two gloo ranks.

Exact comparisons run on integer tables (|value - shift| <= 8) with integer-valued weights: every product and partial sum is an
integer fp64 holds, so every addition order gives the same bits.  On real tables two sums of the same terms differ by at most
2 (n + 1) U sum |term| per cell (``term_bounds``), n the geometries whose weight is not 0.
"""

import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from open_kinematics_amd.ensemble_sample import (IID, LHS, NORMAL, TILT_MAX_SCENARIOS, TRUNCATED, UNIFORM, SamplePlan, check_tilt, exp_unit, sample_host,
                                                 tilt_weights_host, tolerance_scenarios)
from open_kinematics_amd.ensemble_stats import (ENS_COUNT, ENS_SUM, ENS_SUMSQ, REWEIGH_COUNT, REWEIGH_FIELDS, REWEIGH_JOINT_FIELDS, REWEIGH_JOINT_GEOMETRIES,
                                                REWEIGH_JOINT_OUTSIDE, REWEIGH_JOINT_PASS, REWEIGH_JOINT_PASS_WW, REWEIGH_JOINT_SEEN, REWEIGH_JOINT_SEEN_WW,
                                                REWEIGH_JOINT_UNRESOLVED, REWEIGH_OUT_HI, REWEIGH_OUT_LO, REWEIGH_W, REWEIGH_WD, REWEIGH_WDD, REWEIGH_WW,
                                                REWEIGH_WW_OUT, ReweighAccumulator, reduce_host, reweigh_host, reweigh_scenario_terms, reweigh_terms)
from test_ensemble_effects import bits, integer_table

U = 2.0 ** -53


# ---- what the GPU tests share ----

def plan_of(kinds, bound=None, n_total=0, stratify=IID, seed=5):
    z = len(kinds)
    return SamplePlan(np.zeros(((z + 2) // 3, 3)), np.arange(z, dtype=np.int32), np.asarray(kinds, dtype=np.int32), bound, None, None, stratify, n_total, seed)


def mixed_scenarios(z, n):
    """``(plan, tilt [n, z, 5])``: latents of all three kinds in turn (``TRUNCATED`` at k = 2.5); scenario 0 is the identity, the others tighten,
    shift and window the first latents of every kind - windows that leave some geometries outside."""
    kinds = [(NORMAL, UNIFORM, TRUNCATED)[i % 3] for i in range(z)]
    plan = plan_of(kinds, bound=2.5)
    names = plan.factor_names()
    specs = [{}]
    for s in range(1, n):
        spec = {names[0]: dict(ratio=0.5 + 0.05 * (s % 7), shift=0.1 * (s % 3))}
        if s % 2 and z > 0:
            spec[names[0]]["window"] = (-1.0 - 0.1 * s, 1.5)
        if z > 1:
            spec[names[1]] = dict(ratio=0.5 + 0.02 * (s % 5), shift=-0.1)
        if z > 2:
            spec[names[2]] = dict(ratio=0.8, shift=0.05 * s, window=(-1.5, 2.0)) if s % 3 else dict(ratio=1.2)
        if z > 3 and s % 4 == 0:
            spec[names[3]] = dict(ratio=1.3)
        specs.append(spec)
    return plan, tolerance_scenarios(plan, specs[:n])


def latent_table(plan, g, seed):
    """``[g, Z]`` latents as the plan's sampler draws them; from eight geometries on one is NaN and one lies on a window's edge."""
    x = sample_host(SamplePlan(plan.nominal, plan.coords, plan.kind, plan.bound, None, None, IID, g, seed))[1]
    if g >= 8:
        x[3, 0] = np.nan
        x[5, 0] = 1.5
        x[6, plan.n_latents - 1] = np.nan
    return x


def real_table(g, s, k, seed):
    """``(values, status, mask, shift, limits, verdict)``: columns of very different scales around a shift, the status bytes, NaN / inf
    values and mask of ``integer_table``, limits with open sides and a verdict with all three flag values."""
    rng = np.random.default_rng(seed)
    shift = rng.normal(0.0, 3.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (g, s, k)) * np.logspace(-3, 3, k)[None, None]
    holes, status, mask, _ = integer_table(g, s, k, seed + 1)
    values[~np.isfinite(holes)] = holes[~np.isfinite(holes)]
    return (values, status, mask, shift) + limits_and_verdict(g, s, k, shift, np.logspace(-3, 3, k), seed)


def limits_and_verdict(g, s, k, shift, scale, seed):
    rng = np.random.default_rng(seed + 2)
    limits = np.stack([shift - scale[None] * rng.uniform(0.5, 1.5, (s, k)), shift + scale[None] * rng.uniform(0.5, 1.5, (s, k))], axis=-1)
    limits[0, 0, 0], limits[s - 1, k - 1, 1] = -np.inf, np.inf
    if k > 1:
        limits[0, 1] = -np.inf, np.inf
    return limits, rng.choice(np.array([0, 0, 1, 2], dtype=np.uint8), g)


def term_bounds(values, status, mask, weights, shift, limits):
    """``(acc bound [N, 10, S, K], joint bound [N, 7])``: 2 (n + 1) U sum |term| per cell, n the geometries of the table whose weight in
    the scenario is not 0 - two recursive sums of the same n terms, each within (n + 1) U sum |term| of the exact sum whatever its order
    (Higham, Accuracy and Stability, (4.4) with gamma_n <= (n + 1) U for n U << 1).  The terms are the host's own
    (``reweigh_scenario_terms``: the products are bit-identical on the device, contraction is off in the unit); COUNT's and GEOMETRIES'
    are integers: their sums are exact."""
    ok, d, below, above, _ = reweigh_terms(values, status, mask, shift, limits)
    w = np.asarray(weights, dtype=np.float64)
    g, n = w.shape
    acc = np.zeros((n, REWEIGH_FIELDS) + d.shape[1:])
    joint = np.zeros((n, REWEIGH_JOINT_FIELDS))
    seen = np.ones(g, dtype=bool) if mask is None else (np.asarray(mask) & 1) == 0
    for i in range(n):
        live = w[:, i] != 0.0
        scale = 2.0 * (int(live.sum()) + 1) * U
        acc[i] = scale * np.abs(reweigh_scenario_terms(ok[live], d[live], below[live], above[live], w[live, i])).sum(axis=1)
        acc[i, REWEIGH_COUNT] = 0.0
        wl = np.abs(np.where(seen, w[:, i], 0.0))
        joint[i, [REWEIGH_JOINT_SEEN, REWEIGH_JOINT_PASS, REWEIGH_JOINT_OUTSIDE, REWEIGH_JOINT_UNRESOLVED]] = 2.0 * (g + 1) * U * wl.sum()
        joint[i, [REWEIGH_JOINT_SEEN_WW, REWEIGH_JOINT_PASS_WW]] = 2.0 * (g + 1) * U * (wl * wl).sum()
    return acc, joint


def integer_weights(g, n, seed):
    """``[g, n]`` integer-valued weights 0 .. 3 (a third of them 0), scenario 0 all ones."""
    w = np.random.default_rng(seed).integers(0, 4, (g, n)).astype(np.float64)
    w[:, 0] = 1.0
    return w


# ---- exp_unit ----

def test_exp_unit_against_math_exp():
    assert exp_unit(0.0) == 1.0 and exp_unit(-0.0) == 1.0
    rng = np.random.default_rng(0)
    for lo, hi in ((-708.0, 708.0), (-40.0, 5.0), (-1.0, 1.0)):
        x = np.concatenate([rng.uniform(lo, hi, 20000), [lo, hi]])
        want = np.array([math.exp(v) for v in x])
        worst = float(np.max(np.abs(exp_unit(x) - want) / want))
        print(f"exp_unit on [{lo}, {hi}]: largest relative error {worst:.3e}")
        # the Horner bound: 14 multiply-adds at |r| <= 0.35 and the reduction's k LN2_LO, about 4e-15 in all
        assert worst <= 1e-14
    assert np.all(exp_unit(np.array([-708.0000001, -1000.0, -np.inf])) == 0.0) and exp_unit(-708.0) > 0.0
    assert exp_unit(np.nan) == 0.0 and exp_unit(np.inf) == exp_unit(708.0) and np.isfinite(exp_unit(709.0))


# ---- the builder ----

def phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def test_builder_rows_are_the_hand_computed_ones():
    plan = plan_of([NORMAL, TRUNCATED, UNIFORM, NORMAL], bound=[1.0, 2.0, 1.0, 1.0])
    names = plan.factor_names()
    assert names == ["point0.x", "point0.y", "point0.z", "point1.x"]
    tilt = tolerance_scenarios(plan, [{}, {names[0]: dict(ratio=0.5, shift=0.25)}, {names[1]: dict(ratio=0.5, shift=0.25, window=(-1.0, 1.5))},
                                      {names[2]: dict(ratio=0.25, shift=0.5)}, {names[1]: dict(ratio=0.5)}, {"point0": dict(ratio=0.5)},
                                      {names[3]: dict(ratio=2.0, window=(-3.0, 3.0))}])
    assert tilt.shape == (7, 4, 5) and tilt.dtype == np.float64 and tilt.flags["C_CONTIGUOUS"]
    untouched = [0.0, 0.0, 0.0, -np.inf, np.inf]
    assert all(tilt[0, z].tolist() == untouched for z in range(4))  # the identity
    # NORMAL, t = 1/2, m = 1/4: c = (1 - 4) / 2, b = 4 m, a = -ln t - m^2 / (2 t^2) = ln 2 - 1/8; window open
    assert tilt[1, 0].tolist() == [-math.log(0.5) - 0.125, 1.0, -1.5, -np.inf, np.inf] and tilt[1, 1].tolist() == untouched
    # TRUNCATED(2), the same a, b, c and the normaliser ln[(Phi(2) - Phi(-2)) / (Phi((1.5 - m) / t) - Phi((-1 - m) / t))]
    below = 0.5 * math.erfc(2.0 / math.sqrt(2.0))
    base = (1.0 - below) - below
    a, b, c, lo, hi = tilt[2, 1]
    assert (b, c, lo, hi) == (1.0, -1.5, -1.0, 1.5)
    assert abs(a - (math.log(2.0) - 0.125 + math.log(base / (phi(2.5) - phi(-2.5))))) <= 4 * U * abs(a)
    # ... by default the window is [-k, k]
    a, b, c, lo, hi = tilt[4, 1]
    assert (b, c, lo, hi) == (0.0, -1.5, -2.0, 2.0) and abs(a - (math.log(2.0) + math.log(base / (phi(4.0) - phi(-4.0))))) <= 4 * U * abs(a)
    # UNIFORM on [m - t, m + t] = [1/4, 3/4]: a = ln(1 / t) = ln 4
    assert tilt[3, 2].tolist() == [math.log(4.0), 0.0, 0.0, 0.25, 0.75]
    # a point name stands for its three coordinates, each by its own kind
    assert tilt[5, 0].tolist() == [math.log(2.0), 0.0, -1.5, -np.inf, np.inf] and tilt[5, 2].tolist() == [math.log(2.0), 0.0, 0.0, -0.5, 0.5]
    assert tilt[5, 1, 2] == -1.5 and tilt[5, 3].tolist() == untouched
    # a normal latent WITH a window may widen beyond sqrt(2): the weights are bounded there
    a, b, c, lo, hi = tilt[6, 3]
    assert (b, c, lo, hi) == (0.0, 0.375, -3.0, 3.0) and abs(a - (-math.log(2.0) - math.log(phi(1.5) - phi(-1.5)))) <= 4 * U * abs(a)
    assert np.array_equal(check_tilt(tilt), tilt)


def test_builder_rejections():
    plan = plan_of([NORMAL, TRUNCATED, UNIFORM], bound=[1.0, 2.0, 1.0])
    n, t, u = plan.factor_names()
    for spec, words in (({"point9.x": {}}, "names 'point9.x', which is no latent of the plan and no point of one"),
                        ({n: dict(ratio=0.0)}, "must be finite and the ratio greater than 0"), ({n: dict(ratio=-1.0)}, "ratio greater than 0"),
                        ({n: dict(ratio=float("nan"))}, "ratio greater than 0"), ({n: dict(sigma=1.0)}, r"takes ratio, shift and window \(got \['sigma'\]\)"),
                        ({t: dict(window=(-2.5, 1.0))}, r"the window \[-2.5, 1\] leaves the support \[-2, 2\] of the drawn law"),
                        ({t: dict(window=(1.0, -1.0))}, "must have lo < hi"),
                        ({u: dict(ratio=0.75, shift=0.5)}, r"the window \[-0.25, 1.25\] leaves the support \[-1, 1\] of the drawn law"),
                        ({u: dict(ratio=1.5)}, r"leaves the support \[-1, 1\]"), ({u: dict(ratio=0.5, window=(0.0, 0.5))}, "a uniform latent takes ratio and shift"),
                        ({n: dict(ratio=math.sqrt(2.0))}, "sqrt\\(2\\) without a window - the weights of a normal latent then have infinite variance"),
                        ({t: dict(ratio=1.5)}, "infinite variance")):
        with pytest.raises(ValueError, match=words):
            tolerance_scenarios(plan, [{}, spec])
    with pytest.raises(ValueError, match=f"0 scenarios, 1 to {TILT_MAX_SCENARIOS} allowed"):
        tolerance_scenarios(plan, [])
    with pytest.raises(ValueError, match=f"{TILT_MAX_SCENARIOS + 1} scenarios, 1 to {TILT_MAX_SCENARIOS} allowed"):
        tolerance_scenarios(plan, [{}] * (TILT_MAX_SCENARIOS + 1))
    assert tolerance_scenarios(plan, [{}] * TILT_MAX_SCENARIOS).shape == (TILT_MAX_SCENARIOS, 3, 5)
    good = tolerance_scenarios(plan, [{}])
    for at, value, words in (((0, 1, 0), np.inf, "scenario 0, latent 1: a, b or c is not finite"), ((0, 2, 3), np.nan, "scenario 0, latent 2: the window is NaN or has lo > hi"),
                             ((0, 0, slice(3, 5)), (1.0, 0.0), "latent 0: the window is NaN or has lo > hi")):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(ValueError, match=words):
            check_tilt(bad)
    with pytest.raises(ValueError, match=r"latents must be \[G, 3\]"):
        tilt_weights_host(np.zeros((4, 2)), good)


def test_identity_window_and_nan_weights():
    plan, tilt = mixed_scenarios(7, 5)
    x = latent_table(plan, 200, 3)
    w = tilt_weights_host(x, tilt)
    assert w.shape == (200, 5)
    whole = ~np.isnan(x).any(axis=1)
    assert np.all(w[whole, 0] == 1.0) and np.all(w[~whole] == 0.0) and (~whole).sum() == 2  # the identity: exactly 1; a NaN latent: 0 in every scenario
    for s in range(1, 5):
        lo, hi = tilt[s, :, 3], tilt[s, :, 4]
        with np.errstate(invalid="ignore"):
            inside = np.all((lo[None] <= x) & (x <= hi[None]), axis=1)
        assert np.all(w[~inside, s] == 0.0) and np.all(w[inside, s] > 0.0) and 0 < (~inside).sum() < 200
    edge = np.zeros((2, 7))
    edge[:, 1], edge[0, 0], edge[1, 0] = -0.1, 1.5, np.nextafter(1.5, 2.0)
    on_edge = tilt_weights_host(edge, tilt)
    assert np.all(on_edge[0, [1, 3]] > 0.0) and np.all(on_edge[1, [1, 3]] == 0.0) and np.all(on_edge[:, [2, 4]] > 0.0)  # the window is closed: its edge is inside
    # against libm, latent by latent in plain Python
    for g in (0, 17, 199):
        for s in (1, 2, 4):
            logw = 0.0
            for z in range(7):
                a, b, c = (float(v) for v in tilt[s, z, :3])
                logw = logw + ((c * float(x[g, z]) + b) * float(x[g, z]) + a)
            if w[g, s] > 0.0:
                assert abs(w[g, s] - math.exp(logw)) <= 1e-14 * math.exp(logw)


def test_weights_are_the_likelihood_ratio_of_the_new_law():
    """E_p[w] = 1 and E_p[w z] = m for every kind, by quadrature over the drawn law's density."""
    plan = plan_of([NORMAL, TRUNCATED, UNIFORM], bound=[1.0, 2.0, 1.0])
    n, t, u = plan.factor_names()
    tilt = tolerance_scenarios(plan, [{n: dict(ratio=0.7, shift=0.3)}, {t: dict(ratio=0.6, shift=-0.2, window=(-1.5, 1.0))}, {u: dict(ratio=0.4, shift=0.1)},
                                      {n: dict(ratio=0.7, shift=0.3, window=(-0.5, 2.0))}])
    z = np.linspace(-9.0, 9.0, 720001)
    dz = z[1] - z[0]
    normal = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    below = 0.5 * math.erfc(2.0 / math.sqrt(2.0))
    densities = [normal, np.where(np.abs(z) <= 2.0, normal / ((1.0 - below) - below), 0.0), np.where(np.abs(z) <= 1.0, 0.5, 0.0), normal]
    for s, (latent, density) in enumerate(zip((0, 1, 2, 0), densities)):
        x = np.zeros((z.size, 3))
        x[:, latent] = z
        w = tilt_weights_host(x, tilt[s : s + 1])[:, 0]
        assert abs((w * density).sum() * dz - 1.0) < 2e-4, s
    w = tilt_weights_host(np.stack([z, 0 * z, 0 * z], axis=1), tilt[:1])[:, 0]
    assert abs((w * z * normal).sum() * dz - 0.3) < 1e-6 and abs((w * z * z * normal).sum() * dz - (0.49 + 0.09)) < 1e-6


# ---- the accumulator ----

@pytest.mark.parametrize("g,s,k", [(1, 1, 1), (2, 3, 5), (67, 3, 5), (1000, 2, 3)])
def test_identity_scenario_is_the_reduction(g, s, k):
    values, status, _, shift = integer_table(g, s, k, 11 * g + s, with_mask=False)
    want = reduce_host(values, status, None, shift).acc
    got = reweigh_host(values, status, None, np.ones((g, 1)), shift)
    for field, ens in ((REWEIGH_COUNT, ENS_COUNT), (REWEIGH_W, ENS_COUNT), (REWEIGH_WW, ENS_COUNT), (REWEIGH_WD, ENS_SUM), (REWEIGH_WDD, ENS_SUMSQ)):
        assert np.array_equal(got.acc[0, field], want[..., ens]), field
    assert got.joint[0].tolist() == [g, g, g, g, 0.0, 0.0, g]
    out = got.finalize()
    stats = reduce_host(values, status, None, shift).finalize()
    some = stats.count > 0
    assert np.array_equal(out.count[0], stats.count) and np.allclose(out.mean[0][some], stats.mean[some], rtol=1e-14, atol=0)
    assert np.array_equal(out.ess[0][some], stats.count[some].astype(np.float64)) and out.mean_weight[0] == 1.0 and out.yield_ is None


def test_chunks_merge_to_the_whole_exactly_on_integer_tables():
    g, s, k, n = 67, 3, 5, 4
    values, status, mask, shift = integer_table(g, s, k, 5)
    limits, verdict = limits_and_verdict(g, s, k, shift, np.full(k, 4.0), 5)
    w = integer_weights(g, n, 1)
    whole = reweigh_host(values, status, mask, w, shift, limits, verdict)
    merged = ReweighAccumulator.empty(n, s, k, shift, whole.limits)
    for a, b in ((0, 0), (0, 1), (1, 34), (34, 67)):
        merged = merged.merge(reweigh_host(values[a:b], status[a:b], mask[a:b], w[a:b], shift, limits, verdict[a:b]))
    assert np.array_equal(bits(merged.acc), bits(whole.acc)) and np.array_equal(bits(merged.joint), bits(whole.joint))
    # the inputs are worth the test
    assert whole.acc[:, REWEIGH_OUT_LO].max() > 0 and whole.acc[:, REWEIGH_OUT_HI].max() > 0 and whole.acc[1:, REWEIGH_WW_OUT].max() > whole.acc[1:, REWEIGH_OUT_LO].max()
    assert np.all(whole.acc[0, REWEIGH_OUT_LO, 0, 1] == 0) and np.all(whole.acc[0, REWEIGH_OUT_HI, 0, 1] == 0)  # both sides open
    assert np.all(whole.acc[1, REWEIGH_COUNT] <= whole.acc[0, REWEIGH_COUNT]) and whole.acc[1, REWEIGH_COUNT].sum() < whole.acc[0, REWEIGH_COUNT].sum()  # w = 0 is not counted
    seen = (mask & 1) == 0
    assert whole.joint[0, REWEIGH_JOINT_GEOMETRIES] == seen.sum() < g
    assert whole.joint[1, REWEIGH_JOINT_PASS] == w[seen & (verdict == 0), 1].sum() and whole.joint[1, REWEIGH_JOINT_OUTSIDE] == w[seen & (verdict == 1), 1].sum()
    assert whole.joint[1, REWEIGH_JOINT_UNRESOLVED] == w[seen & (verdict == 2), 1].sum() and whole.joint[1, REWEIGH_JOINT_SEEN_WW] == (w[seen, 1] ** 2).sum()
    # a plain restatement of three cells
    for i, si, ki in ((1, 0, 0), (2, 2, 4), (3, 1, 2)):
        want = np.zeros(REWEIGH_FIELDS)
        for j in range(g):
            v = values[j, si, ki]
            if (mask[j] & 1) or (status[j, si] & 7) != 1 or not np.isfinite(v) or w[j, i] == 0.0:
                continue
            d, lo, hi = v - shift[si, ki], v < limits[si, ki, 0], v > limits[si, ki, 1]
            want += [1.0, w[j, i], w[j, i] ** 2, w[j, i] * d, w[j, i] * d * d, w[j, i] ** 2 * d, w[j, i] ** 2 * d * d, w[j, i] * lo, w[j, i] * hi, w[j, i] ** 2 * (lo or hi)]
        assert whole.acc[i, :, si, ki].tolist() == want.tolist(), (i, si, ki)
    with pytest.raises(ValueError, match="different shifts"):
        whole.merge(reweigh_host(values, status, mask, w, shift + 1.0, limits, verdict))
    with pytest.raises(ValueError, match="different limits"):
        whole.merge(reweigh_host(values, status, mask, w, shift, None, verdict))
    with pytest.raises(ValueError, match="different shapes"):
        whole.merge(reweigh_host(values, status, mask, w[:, :2], shift, limits, verdict))
    for kw, words in ((dict(weights=w[:5]), r"weights must be \[67, S\], one row per geometry"), (dict(limits=np.array([1.0, 0.0])), "a limit has lo > hi"),
                      (dict(limits=np.array([np.nan, 0.0])), "a limit is NaN"), (dict(verdict=verdict[:5]), r"verdict must be uint8 \[67\]"),
                      (dict(weights=np.ones((g, 257))), "257 scenarios, 1 to 256 allowed"), (dict(weights=None), "weights are needed")):
        with pytest.raises(ValueError, match=words):
            reweigh_host(values, status, mask, **{"weights": w, "shift": shift, **kw})


def test_real_tables_chunked_within_the_bound():
    g, s, k, n = 200, 2, 4, 6
    values, status, mask, shift, limits, verdict = real_table(g, s, k, 3)
    plan, tilt = mixed_scenarios(7, n)
    w = tilt_weights_host(latent_table(plan, g, 2), tilt)
    whole = reweigh_host(values, status, mask, w, shift, limits, verdict)
    merged = reweigh_host(values[:77], status[:77], mask[:77], w[:77], shift, limits, verdict[:77]).merge(
        reweigh_host(values[77:], status[77:], mask[77:], w[77:], shift, limits, verdict[77:]))
    bound, joint_bound = term_bounds(values, status, mask, w, shift, limits)
    assert np.all(np.abs(merged.acc - whole.acc) <= bound) and np.all(np.abs(merged.joint - whole.joint) <= joint_bound)
    assert np.array_equal(merged.acc[:, REWEIGH_COUNT], whole.acc[:, REWEIGH_COUNT])
    out = whole.finalize()
    assert out.yield_.shape == (n, s, k) and np.all((out.yield_[np.isfinite(out.yield_)] >= -1e-12) & (out.yield_[np.isfinite(out.yield_)] <= 1 + 1e-12))
    assert np.all(out.yield_[:, 0, 1][np.isfinite(out.yield_[:, 0, 1])] == 1.0)  # both sides open: nothing is outside
    assert np.allclose(out.joint_yield + out.outside + out.unresolved, 1.0, rtol=1e-12)


# ---- what the numbers mean ----

@pytest.mark.parametrize("stratify", [IID, LHS])
def test_tightened_tolerances_on_a_synthetic_column(stratify):
    """Six NORMAL latents, 4096 geometries; latents 0 and 2 tightened to t = 1/2.  Under the new law the column
    z0^2 + 0.5 z1 + 0.3 z0 z2 + 0.1 z3 has the mean t^2 = 1/4; the effective sample size of a normal latent tightened to t is
    t sqrt(2 - t^2) of the draw, so 0.4375 G for two of them."""
    g, t = 4096, 0.5
    for seed in range(8):
        plan = plan_of([NORMAL] * 6, n_total=g, stratify=stratify, seed=seed)
        names = plan.factor_names()
        tilt = tolerance_scenarios(plan, [{}, {names[0]: dict(ratio=t), names[2]: dict(ratio=t)}])
        _, z, _, flags = sample_host(plan)
        w = tilt_weights_host(z, tilt)
        column = z[:, 0] ** 2 + 0.5 * z[:, 1] + 0.3 * z[:, 0] * z[:, 2] + 0.1 * z[:, 3]
        out = reweigh_host(column[:, None, None], None, flags, w, np.zeros((1, 1)), limits=[-np.inf, 1.0]).finalize()
        mean, se, ess = out.mean[1, 0, 0], out.mean_se[1, 0, 0], out.ess[1, 0, 0]
        print(f"stratify {stratify} seed {seed}: mean {mean:.4f} ({(mean - t * t) / se:+.2f} se), ess {ess:.0f}, mean weight {out.mean_weight[1]:.4f}")
        assert abs(mean - t * t) <= 5.0 * se
        assert abs(ess - 0.4375 * g) <= 0.1 * 0.437 * g and abs(out.ess_all[1] - 0.4375 * g) <= 0.1 * 0.437 * g
        assert abs(out.mean_weight[1] - 1.0) < 0.05 and out.mean_weight[0] == 1.0 and out.ess[0, 0, 0] == g
        assert abs(out.mean[0, 0, 0] - 1.0) <= 5.0 * out.mean_se[0, 0, 0]  # as drawn: E z0^2 = 1
        assert out.yield_[1, 0, 0] > out.yield_[0, 0, 0] and out.std[1, 0, 0] < out.std[0, 0, 0]  # the tightened tolerance narrows the scatter


# ---- ShardedEnsemble(reduce=True, factors="sampled", whatif=...) on the stand-in program ----

N_GEOM = 24


def stage_inputs():
    from test_ensemble_sample import STEPS, stand_in_plan
    from test_ensemble_stats import COLUMNS

    plan, relative = stand_in_plan(N_GEOM)
    specs = [{}, {"point0": dict(ratio=0.6)}, {"point1.y": dict(ratio=0.8, shift=0.2), "point2.z": dict(ratio=1.2, window=(-2.5, 2.0))}]
    limits = np.array([[-40.0, 30.0], [-np.inf, 20.0], [-25.0, np.inf], [-30.0, 30.0]])
    return plan, relative, specs, limits, STEPS, COLUMNS


def run_stage(program, chunks, **kw):
    from open_kinematics_amd.dist import ShardedEnsemble

    plan, relative, specs, limits, steps, columns = stage_inputs()
    pipe = ShardedEnsemble(program, plan, relative, steps, chunks=chunks, metric_columns=columns, reduce=True, factors="sampled", whatif=specs, limits=limits,
                           screen=True, shift=np.zeros((steps, len(columns))), **kw)
    pipe.step()
    return pipe


def host_answer(pipe):
    plan, _, specs, limits, steps, columns = stage_inputs()
    _, latents, _, flags = sample_host(plan)
    values = pipe.metric_local.numpy().reshape(N_GEOM, steps, len(columns))
    status = pipe.info_local[:, 32].numpy().reshape(N_GEOM, steps)
    w = tilt_weights_host(latents, tolerance_scenarios(plan, specs))
    verdict = pipe.screen().flags
    shift = np.zeros((steps, len(columns)))
    return reweigh_host(values, status, flags, w, shift, limits, verdict), term_bounds(values, status, flags, w, shift, np.broadcast_to(limits, (steps, len(columns), 2)))


@pytest.mark.parametrize("integers", [False, True])
def test_whatif_stage_one_chunk_and_three(integers):
    from test_ensemble_sobol import integer_stand_in
    from test_ensemble_stats import _stand_in

    make = integer_stand_in if integers else _stand_in
    one, three = run_stage(make(), 1), run_stage(make(), 3)
    assert len(three.pieces) == 3 and one.whatif_exchange_bytes_per_rank == 0
    a, b = one.whatif_accumulator.numpy(), three.whatif_accumulator.numpy()
    want, (bound, joint_bound) = host_answer(one)
    assert np.array_equal(bits(a.acc), bits(want.acc)) and np.array_equal(bits(a.joint), bits(want.joint))  # one chunk IS the definition
    assert np.all(np.abs(b.acc - a.acc) <= bound) and np.all(np.abs(b.joint - a.joint) <= joint_bound)
    assert np.array_equal(b.acc[:, REWEIGH_COUNT], a.acc[:, REWEIGH_COUNT])
    if integers:  # the identity scenario's sums are sums of integers: every chunking carries the same bits
        assert np.array_equal(bits(b.acc[0]), bits(a.acc[0])) and np.array_equal(bits(b.joint[0]), bits(a.joint[0]))
    # the identity scenario is the reduction
    stats = one.accumulator.acc.numpy()
    assert np.array_equal(a.acc[0, REWEIGH_COUNT], stats[..., ENS_COUNT]) and np.array_equal(bits(a.acc[0, REWEIGH_WD]), bits(stats[..., ENS_SUM]))
    out = one.whatif()
    assert out.mean.shape == (3,) + stats.shape[:2] and out.joint_yield.shape == (3,) and out.geometries == N_GEOM
    verdict = one.screen().flags
    assert 0 < (verdict == 0).sum() < N_GEOM and out.joint_yield[0] == (verdict == 0).sum() / N_GEOM  # the inputs are worth the test
    first = bits(a.acc).copy()
    one.step()  # a second step starts from nothing, and the cached weights are the same
    assert np.array_equal(bits(one.whatif_accumulator.numpy().acc), first)


def test_whatif_stage_refusals():
    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_sample import FamilyPlan
    from test_ensemble_stats import _stand_in

    plan, relative, specs, limits, steps, columns = stage_inputs()
    kw = dict(metric_columns=columns, reduce=True)
    with pytest.raises(ValueError, match="whatif= reweighs the ensemble of a SamplePlan by its latents: it needs reduce=True, factors='sampled' and no FamilyPlan"):
        ShardedEnsemble(_stand_in(), plan, relative, steps, whatif=specs, **kw)
    with pytest.raises(ValueError, match="it needs reduce=True, factors='sampled' and no FamilyPlan"):
        ShardedEnsemble(_stand_in(), FamilyPlan(plan, [0] * 9, 2), relative, steps, factors="sampled", whatif=specs, **kw)
    with pytest.raises(ValueError, match="names 'point7', which is no latent of the plan"):
        ShardedEnsemble(_stand_in(), plan, relative, steps, factors="sampled", whatif=[{"point7": dict(ratio=0.5)}], **kw)
    with pytest.raises(ValueError, match="the scenario table has 4 latents, the plan 9"):
        ShardedEnsemble(_stand_in(), plan, relative, steps, factors="sampled", whatif=np.zeros((1, 4, 5)) + np.array([0, 0, 0, -1.0, 1.0]), **kw)
    with pytest.raises(ValueError, match=r"whatif\(\) needs whatif=scenarios"):
        ShardedEnsemble(_stand_in(), plan, relative, steps, factors="sampled", **kw).whatif()
    pipe = ShardedEnsemble(_stand_in(), plan, relative, steps, factors="sampled", whatif=tolerance_scenarios(plan, specs), **kw)  # the table itself; no limits
    with pytest.raises(RuntimeError, match="no step"):
        pipe.whatif()
    pipe.step()
    assert pipe.whatif().yield_ is None and np.all(pipe.whatif().joint_yield == 1.0)  # no verdict: every geometry passes


def _whatif_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    import torch.distributed as dist

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_ensemble_sobol import integer_stand_in
    from test_ensemble_stats import _stand_in

    out = {}
    for name, make in (("real", _stand_in), ("integer", integer_stand_in)):
        pipe = run_stage(make(), 2)
        acc = pipe.whatif_accumulator.numpy()
        out[name] = {"acc": acc.acc, "joint": acc.joint, "sent": pipe.whatif_exchange_bytes_per_rank, "range": pipe.geometry_range, "mean": pipe.whatif().mean}
    torch.save(out, os.path.join(out_dir, f"whatif{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_whatif_stage_over_two_ranks_equals_one(tmp_path):
    import torch.multiprocessing as mp
    from test_ensemble_sobol import integer_stand_in
    from test_ensemble_stats import _stand_in

    world = 2
    port = 41300 + (os.getpid() + 17 * world) % 2000
    mp.spawn(_whatif_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"whatif{r}.pt"), weights_only=False) for r in range(world)]
    steps, k = stage_inputs()[4], len(stage_inputs()[5])
    for name, make in (("real", _stand_in), ("integer", integer_stand_in)):
        alone = run_stage(make(), 1)
        a = alone.whatif_accumulator.numpy()
        _, (bound, joint_bound) = host_answer(alone)
        one, two = got[0][name], got[1][name]
        assert (one["range"], two["range"]) == ((0, 12), (12, 24)) and one["sent"] == two["sent"] == 8 * 3 * (REWEIGH_FIELDS * steps * k + REWEIGH_JOINT_FIELDS)
        assert np.array_equal(bits(one["acc"]), bits(two["acc"])) and np.array_equal(bits(one["joint"]), bits(two["joint"]))  # the same bits on both ranks
        assert np.array_equal(bits(one["mean"]), bits(two["mean"]))
        assert np.all(np.abs(one["acc"] - a.acc) <= bound) and np.all(np.abs(one["joint"] - a.joint) <= joint_bound)
        assert np.array_equal(one["acc"][:, REWEIGH_COUNT], a.acc[:, REWEIGH_COUNT])
        if name == "integer":
            assert np.array_equal(bits(one["acc"][0]), bits(a.acc[0])) and np.array_equal(bits(one["joint"][0]), bits(a.joint[0]))


def test_constants_match_the_header():
    import re

    from open_kinematics_amd import _abi, ensemble_sample as sm, ensemble_stats as es

    with open(os.path.join(REPO, "include", "okx.h"), "r", encoding="utf-8") as fh:
        header = dict((name, int(value)) for name, value in re.findall(r"\bOKX_((?:ENS_TILT|TILT|REWEIGH)_[A-Z_]+) = (\d+)", fh.read()))
    assert len(header) == 2 + 11 + 8
    for name, value in header.items():
        assert getattr(_abi, name) == value, name
        if name.startswith("REWEIGH"):
            assert getattr(es, name) == value, name
    assert (sm.TILT_MAX_SCENARIOS, sm.TILT_PARAMS, es.REWEIGH_MAX_SCENARIOS) == (header["ENS_TILT_MAX_SCENARIOS"], header["TILT_PARAMS"], header["ENS_TILT_MAX_SCENARIOS"])
