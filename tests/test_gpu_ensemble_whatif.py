"""
GPU: okx_ensemble_tilt_weights (DeviceProgram.tilt_weights), okx_ensemble_reweigh (DeviceProgram.reweigh_ensemble) and
ShardedEnsemble(reduce=True, factors="sampled", whatif=...) against the NumPy definitions ensemble_sample.tilt_weights_host and
ensemble_stats.reweigh_host.

The weights are compared bit for bit.  The accumulator is compared exactly on the integer tables of tests/test_ensemble_effects.py
with integer-valued weights uploaded directly (|value - shift| <= 8, weights 0 .. 3: every product and partial sum is an integer fp64
holds) and, on real tables with tilted weights, within 2 (n + 1) U sum |term| of reweigh_host per cell, the bound computed from the
host's own terms (``term_bounds`` of tests/test_ensemble_whatif.py; the terms are bit-identical, contraction is off in the unit):
nothing here comes from an outcome.

The plan the shapes are chosen from (okx_tilt.hip): a lane owns one of 64 entries of a tile ((S, K) = (1, 1): one entry, 63 lanes idle;
(5, 17): 85 entries, a second, partial tile); the scenarios are tiled by 8 (N = 1 and 3: one partial tile; 9: a full tile and a tile of
one; 17: two full tiles and one of one); a slab is never shorter than 32 geometries, so G = 1 is one slab, G = 33 two slabs (17 + 16:
a slab boundary), G = 97 four (25, 25, 25, 22: the merge's tail loop) and G = 1000 thirty-two of 32 with a last one of 8 (the merge's
unrolled rounds); G = 0 launches only the merge.  The weights pass is one thread per (geometry, scenario) in workgroups of 256:
G N from 1 to 17 000, whole and partial workgroups.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_sample import sample_host, tilt_weights_host, tolerance_scenarios
from open_kinematics_amd.ensemble_stats import (ENS_COUNT, ENS_SUM, REWEIGH_COUNT, REWEIGH_FIELDS, REWEIGH_JOINT_FIELDS, REWEIGH_JOINT_GEOMETRIES, REWEIGH_W,
                                                REWEIGH_WD, ReweighAccumulator, reweigh_host)
from test_ensemble_effects import bits, integer_table
from test_ensemble_whatif import integer_weights, latent_table, limits_and_verdict, mixed_scenarios, real_table, term_bounds

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


def padded(table, pad, dtype=torch.float64):
    """``table [rows, n]`` on the device with ``pad`` more columns of NaN per row, which must never be read as data: the view ``[:, :n]``."""
    rows, n = table.shape
    wide = torch.full((rows, n + pad), float("nan"), dtype=dtype, device=DEV)
    wide[:, :n] = torch.as_tensor(np.ascontiguousarray(table), device=DEV)
    return wide[:, :n]


def upload(values, status, mask, verdict, pad=3, stride=40):
    """The table with ``ld = K + pad`` and its status bytes ``stride`` apart, the rest filled with what must never be read as data."""
    g, s, k = values.shape
    v = padded(values.reshape(g * s, k), pad)
    st = None
    if status is not None:
        info = torch.full((g * s, stride), 2, dtype=torch.uint8, device=DEV)
        info[:, 32 % stride] = torch.as_tensor(np.ascontiguousarray(status).reshape(-1), device=DEV)
        st = info[:, 32 % stride]
    up = lambda a: None if a is None else torch.as_tensor(a, device=DEV)  # noqa: E731
    return v, st, up(mask), up(verdict)


# ---- the weights ----

@pytest.mark.parametrize("g", [1, 67, 1000])
@pytest.mark.parametrize("z", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 3, 9, 17])
def test_weights_equal_the_host_bit_for_bit(dp, g, z, n):
    plan, tilt = mixed_scenarios(z, n)
    x = latent_table(plan, g, 100 * g + z + n)
    want = tilt_weights_host(x, tilt)
    latents = padded(x, 2)
    out = padded(np.full((g, n), -7.0), 3)
    assert g == 1 or (latents.stride(0), out.stride(0)) == (z + 2, n + 3)
    got = dp.tilt_weights(latents, tilt, out=out)
    torch.cuda.synchronize()
    assert got is out and np.array_equal(bits(out.cpu().numpy()), bits(want))
    wide = torch.as_strided(out, (g, n + 3), (n + 3, 1))
    assert bool(torch.isnan(wide[:, n:]).all())  # nothing was written beside the rows
    fresh = dp.tilt_weights(latents, dp.tilt_prepare(tilt))
    torch.cuda.synchronize()
    assert fresh.is_contiguous() and np.array_equal(bits(fresh.cpu().numpy()), bits(want))
    if g >= 67:  # the inputs are worth the test: a NaN latent, geometries outside a window, weights on both sides of 1
        assert np.all(want[3] == 0.0) and np.all(want[[0, 1, 2], 0] == 1.0)
        if n >= 3:
            assert 0 < (want[:, 1:] == 0.0).sum() < want[:, 1:].size and want.max() > 1.0 and 0.0 < want[want > 0.0].min() < 1.0


# ---- the accumulator, exact ----

TABLES = [(1, 1), (5, 17)]
GEOMETRIES = [0, 1, 33, 97, 1000]


def run(dp, tables, weights, shift, limits, **kw):
    v, st, mk, vd = tables
    return dp.reweigh_ensemble(v, steps_per_geometry=shift.shape[0], weights=weights, status=st, mask=mk, verdict=vd, shift=shift, limits=limits, **kw)


@pytest.mark.parametrize("g", GEOMETRIES)
@pytest.mark.parametrize("s,k", TABLES)
@pytest.mark.parametrize("n", [1, 3, 9])
def test_exact_on_integer_tables(dp, g, s, k, n):
    values, status, mask, shift = integer_table(g, s, k, 1000 * g + 10 * n + s)
    limits, verdict = limits_and_verdict(g, s, k, shift, np.full(k, 4.0), g + n)
    w = integer_weights(g, n, g + 7)
    want = reweigh_host(values, status, mask, w, shift, limits, verdict)
    tables = upload(values, status, mask, verdict)
    weights = padded(w, 3)
    assert g <= 1 or (tables[0].stride(0), tables[1].stride(0), weights.stride(0)) == (k + 3, 40, n + 3)
    acc = run(dp, tables, weights, shift, limits)
    torch.cuda.synchronize()
    got = acc.numpy()
    assert got.acc.shape == (n, REWEIGH_FIELDS, s, k) and got.joint.shape == (n, REWEIGH_JOINT_FIELDS)
    bad = np.argwhere(got.acc != want.acc)
    assert bad.size == 0, (bad[:8].tolist(), got.acc[tuple(bad[0])], want.acc[tuple(bad[0])])
    assert np.array_equal(got.joint, want.joint), (got.joint, want.joint)
    if g >= 33:  # the inputs are worth the test
        assert 0 < got.joint[0, REWEIGH_JOINT_GEOMETRIES] < g and got.acc[0, REWEIGH_COUNT].min() < got.joint[0, REWEIGH_JOINT_GEOMETRIES] and set(verdict) == {0, 1, 2}
    # two chunks cut at an odd geometry, the second accumulated onto the first: exact too
    cut = min(g, g // 2 + (1 - (g // 2) % 2))
    v, st, mk, vd = tables
    out = ReweighAccumulator(torch.full_like(acc.acc, -7.0), torch.full_like(acc.joint, -7.0), acc.shift, acc.limits)
    dp.reweigh_ensemble(v[: cut * s], steps_per_geometry=s, weights=weights[:cut], status=st[: cut * s], mask=mk[:cut], verdict=vd[:cut], out=out)
    torch.cuda.synchronize()
    first = reweigh_host(values[:cut], status[:cut], mask[:cut], w[:cut], shift, limits, verdict[:cut])
    assert np.array_equal(out.numpy().acc, first.acc) and np.array_equal(out.numpy().joint, first.joint)  # -7 overwritten
    dp.reweigh_ensemble(v[cut * s :], steps_per_geometry=s, weights=weights[cut:], status=st[cut * s :], mask=mk[cut:], verdict=vd[cut:], out=out, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.numpy().acc, want.acc) and np.array_equal(out.numpy().joint, want.joint)
    # no status bytes, mask, limits or verdict: every state accepted, nothing outside, every geometry passes
    plain = dp.reweigh_ensemble(v, steps_per_geometry=s, weights=weights, shift=shift)
    torch.cuda.synchronize()
    bare = reweigh_host(values, None, None, w, shift)
    assert plain.limits is None and np.array_equal(plain.numpy().acc, bare.acc) and np.array_equal(plain.numpy().joint, bare.joint)


def test_no_geometry_leaves_zeros_or_what_was_there(dp):
    s, k, n = 3, 5, 9
    shift = np.zeros((s, k))
    empty = torch.empty((0, k), dtype=torch.float64, device=DEV)
    weights = torch.empty((0, n), dtype=torch.float64, device=DEV)
    assert tuple(dp.tilt_weights(torch.empty((0, 3), dtype=torch.float64, device=DEV), mixed_scenarios(3, n)[1]).shape) == (0, n)
    acc = dp.reweigh_ensemble(empty, steps_per_geometry=s, weights=weights, shift=shift)
    torch.cuda.synchronize()
    assert not acc.acc.any() and not acc.joint.any()
    acc.acc.fill_(5.0), acc.joint.fill_(6.0)
    dp.reweigh_ensemble(empty, steps_per_geometry=s, weights=weights, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert bool((acc.acc == 5.0).all()) and bool((acc.joint == 6.0).all())
    dp.reweigh_ensemble(empty, steps_per_geometry=s, weights=weights, out=acc)
    torch.cuda.synchronize()
    assert not acc.acc.any() and not acc.joint.any()


# ---- the accumulator, real data ----

@pytest.mark.parametrize("g", [1, 33, 97, 1000])
@pytest.mark.parametrize("s,k,n", [(1, 1, 3), (5, 17, 9)])
def test_real_tables_within_the_summation_bound_and_the_same_bits_again(dp, g, s, k, n):
    values, status, mask, shift, limits, verdict = real_table(g, s, k, g + n)
    plan, tilt = mixed_scenarios(7, n)
    x = latent_table(plan, g, g)
    w = tilt_weights_host(x, tilt)
    want = reweigh_host(values, status, mask, w, shift, limits, verdict)
    bound, joint_bound = term_bounds(values, status, mask, w, shift, limits)
    tables = upload(values, status, mask, verdict)
    weights = dp.tilt_weights(padded(x, 2), tilt, out=padded(np.zeros((g, n)), 3))
    acc = run(dp, tables, weights, shift, limits)
    torch.cuda.synchronize()
    got = acc.numpy()
    print("largest |device - host| / bound:", float(np.max(np.abs(got.acc - want.acc) / np.where(bound > 0, bound, 1.0))),
          float(np.max(np.abs(got.joint - want.joint) / np.where(joint_bound > 0, joint_bound, 1.0))))
    assert np.all(np.abs(got.acc - want.acc) <= bound) and np.all(np.abs(got.joint - want.joint) <= joint_bound)
    assert np.array_equal(got.acc[:, REWEIGH_COUNT], want.acc[:, REWEIGH_COUNT]) and np.array_equal(got.joint[:, REWEIGH_JOINT_GEOMETRIES], want.joint[:, REWEIGH_JOINT_GEOMETRIES])
    again = run(dp, tables, dp.tilt_weights(padded(x, 2), tilt), shift, limits)
    torch.cuda.synchronize()
    assert torch.equal(again.acc.view(torch.int64), acc.acc.view(torch.int64)) and torch.equal(again.joint.view(torch.int64), acc.joint.view(torch.int64))
    # three chunks accumulated: within the bound of the whole, COUNT exact
    v, st, mk, vd = tables
    out = None
    for a, b in ((0, g // 3), (g // 3, g // 3), (g // 3, g)):
        part = dict(steps_per_geometry=s, weights=weights[a:b], status=st[a * s : b * s], mask=mk[a:b], verdict=vd[a:b])
        out = dp.reweigh_ensemble(v[a * s : b * s], shift=shift, limits=limits, **part) if out is None else dp.reweigh_ensemble(v[a * s : b * s], out=out, accumulate=True, **part)
    torch.cuda.synchronize()
    chunked = out.numpy()
    assert np.all(np.abs(chunked.acc - want.acc) <= bound) and np.all(np.abs(chunked.joint - want.joint) <= joint_bound)
    assert np.array_equal(chunked.acc[:, REWEIGH_COUNT], want.acc[:, REWEIGH_COUNT])
    if g >= 97:
        result = acc.finalize()
        assert result.mean.shape == (n, s, k) and np.all(result.ess[np.isfinite(result.ess)] <= g + 1e-9) and result.geometries == int(want.joint[0, REWEIGH_JOINT_GEOMETRIES])


# ---- the chain ----

STEPS = 4


def test_the_chain_on_two_points():
    """hardpoint_plan on two points of data/geometry.yaml (6 latents under LHS), 256 geometries, 4 bump steps, two chunks, the screen's
    verdict and limits one standard deviation around the mean of a first, plain reduction (so that a good share lies outside)."""
    import open_kinematics_amd.dist as okd

    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_effects_rate import build

    g = 256
    device_program, plan, rel, columns = build(g, STEPS, DEV, n_points=2)
    k = len(columns)
    kw = dict(metric_columns=columns, reduce=True, factors="sampled", chain_len=1, predictor=False)
    plain = okd.ShardedEnsemble(device_program, plan, rel, STEPS, **kw)
    stats = plain.step().finalize()
    limits = np.stack([stats.mean - stats.std, stats.mean + stats.std], axis=-1)
    limits[~np.isfinite(limits).all(axis=-1)] = -np.inf, np.inf
    names = plan.factor_names()
    specs = [{}, {names[0]: dict(ratio=0.5), names[2]: dict(ratio=0.5)}, {names[3].rsplit(".", 1)[0]: dict(ratio=0.8, shift=0.1)}]
    tilt = tolerance_scenarios(plan, specs)
    pipe = okd.ShardedEnsemble(device_program, plan, rel, STEPS, whatif=specs, limits=limits, screen=True, chunks=2, **kw)
    pipe.step()
    torch.cuda.synchronize()
    assert len(pipe.pieces) == 2 and pipe.whatif_exchange_bytes_per_rank == 0
    _, latents, _, flags = sample_host(plan)
    assert np.array_equal(pipe.sampled_flags.cpu().numpy(), flags) and np.array_equal(bits(pipe.sampled_latents.cpu().numpy()), bits(latents))
    values = pipe.metric_local.cpu().numpy().reshape(g, STEPS, k)
    status = pipe.info_local[:, 32].cpu().numpy().reshape(g, STEPS)
    verdict = pipe.screen().flags
    mine = pipe.whatif_accumulator.numpy()
    w = tilt_weights_host(latents, tilt)
    want = reweigh_host(values, status, flags, w, mine.shift, limits, verdict)
    bound, joint_bound = term_bounds(values, status, flags, w, mine.shift, limits)
    assert np.all(np.abs(mine.acc - want.acc) <= bound) and np.all(np.abs(mine.joint - want.joint) <= joint_bound)
    assert np.array_equal(mine.acc[:, REWEIGH_COUNT], want.acc[:, REWEIGH_COUNT])
    # the identity scenario reproduces the reduction: the count exactly, the sum of d (so the mean) within the bound
    reduced = pipe.accumulator.numpy().acc
    assert np.array_equal(mine.acc[0, REWEIGH_COUNT], reduced[..., ENS_COUNT]) and np.array_equal(mine.acc[0, REWEIGH_W], reduced[..., ENS_COUNT])
    assert np.all(np.abs(mine.acc[0, REWEIGH_WD] - reduced[..., ENS_SUM]) <= bound[0, REWEIGH_WD])
    out = pipe.whatif()
    assert out.mean.shape == (3, STEPS, k) and out.geometries == int(((flags & 1) == 0).sum()) and out.mean_weight[0] == 1.0
    assert 0.0 <= np.nanmin(out.yield_[0]) < 1.0 and (verdict != 0).sum() > 0  # the inputs are worth the test
    # two normal latents tightened to 1/2: the weights' variance is 1 / 0.4375 - 1, so their mean over 256 draws scatters by 0.07
    assert np.all(out.ess[1] < out.ess[0]) and abs(out.mean_weight[1] - 1.0) < 0.25
    with pytest.raises(ValueError, match="it needs reduce=True, factors='sampled' and no FamilyPlan"):
        okd.ShardedEnsemble(device_program, plan, rel, STEPS, metric_columns=columns, reduce=True, whatif=specs, chain_len=1, predictor=False)


def test_a_captured_graph_replays(dp):
    import gc

    # (the ShardedEnsembles of the test above wait for the cycle collector; were it to run inside the capture, their release would
    #  free device memory, which no capture survives.  Likewise the program's compile job, which loads code objects when it finishes.)
    gc.collect()
    dp.wait_ready()
    g, s, k, n = 97, 5, 17, 9
    values, status, mask, shift, limits, verdict = real_table(g, s, k, 4)
    plan, tilt = mixed_scenarios(7, n)
    latents = padded(latent_table(plan, g, 8), 2)
    prepared = dp.tilt_prepare(tilt)
    v, st, mk, vd = upload(values, status, mask, verdict)
    kw = dict(steps_per_geometry=s, status=st, mask=mk, verdict=vd)
    weights = dp.tilt_weights(latents, prepared)
    acc = dp.reweigh_ensemble(v, weights=weights, shift=shift, limits=limits, **kw)   # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    first, first_joint, first_weights = acc.acc.clone(), acc.joint.clone(), weights.clone()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.tilt_weights(latents, prepared, out=weights)
        dp.reweigh_ensemble(v, weights=weights, out=acc, **kw)
    weights.fill_(77.0), acc.acc.fill_(-1.0), acc.joint.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(weights.view(torch.int64), first_weights.view(torch.int64))
    assert torch.equal(acc.acc.view(torch.int64), first.view(torch.int64)) and torch.equal(acc.joint.view(torch.int64), first_joint.view(torch.int64))


# ---- the error paths ----

def test_error_paths_launch_nothing(dp):
    from open_kinematics_amd import _lib

    lib = dp.lib
    s, k, n, g, z = 2, 3, 4, 5, 3
    table = torch.zeros((g * s, k), dtype=torch.float64, device=DEV)
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    acc = torch.full((n, REWEIGH_FIELDS, s, k), -3.0, dtype=torch.float64, device=DEV)
    joint = torch.full((n, REWEIGH_JOINT_FIELDS), -3.0, dtype=torch.float64, device=DEV)
    weights = torch.ones((g, n), dtype=torch.float64, device=DEV)
    need = int(lib.okx_ensemble_reweigh_scratch_bytes(g, s, k, n))
    assert need == 8 * n * (REWEIGH_FIELDS * s * k + REWEIGH_JOINT_FIELDS) and lib.okx_ensemble_reweigh_scratch_bytes(0, s, k, n) == 0
    scratch = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off if t is not None else 0)  # noqa: E731

    def call(geometries=g, steps=s, columns=k, values=table, ld=k, w=weights, ldw=n, scenarios=n, out=acc, per=joint, room=need, off=0):
        return lib.okx_ensemble_reweigh(geometries, steps, columns, ptr(values), ld, None, 0, None, ptr(shift), ptr(w), ldw, scenarios, None, None, 0, ptr(out), ptr(per),
                                        ptr(scratch, off), room, None)

    for kw, words in ((dict(geometries=-1), "negative geometry, step or column count"), (dict(ld=k - 1), "null table or ld < n_columns"),
                      (dict(values=None), "null table or ld < n_columns"), (dict(scenarios=0), "0 scenarios, 1 to 256 allowed"),
                      (dict(scenarios=257), "257 scenarios, 1 to 256 allowed"), (dict(w=None), "null weight table or ldw < n_scenarios"),
                      (dict(ldw=n - 1), "null weight table or ldw < n_scenarios"), (dict(out=None), "null accumulator or shift table"),
                      (dict(per=None), "null accumulator or shift table"), (dict(steps=1 << 31), "too many entries for one call"),
                      (dict(room=need - 1), f"{need} bytes of scratch needed (okx_ensemble_reweigh_scratch_bytes), {need - 1} given"),
                      (dict(off=4), "the scratch buffer must be 8-byte aligned")):
        assert call(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_reweigh" in _lib.last_error(), (kw, _lib.last_error())

    plan, tilt = mixed_scenarios(z, n)
    table_dev = dp.tilt_prepare(tilt)
    latents = torch.zeros((g, z), dtype=torch.float64, device=DEV)
    out = torch.full((g, n), -3.0, dtype=torch.float64, device=DEV)

    def weigh(geometries=g, x=latents, ldz=z, n_latents=z, scenarios=n, rows=table_dev, to=out, ldw=n):
        return lib.okx_ensemble_tilt_weights(geometries, ptr(x), ldz, n_latents, ptr(rows), scenarios, ptr(to), ldw, None)

    for kw, words in ((dict(geometries=-1), "negative geometry, step or column count"), (dict(x=None), "null latent table or ldz < n_latents"),
                      (dict(ldz=z - 1), "null latent table or ldz < n_latents"), (dict(n_latents=0), "0 latents, 1 to 288 allowed"),
                      (dict(n_latents=289, ldz=289), "289 latents, 1 to 288 allowed"), (dict(scenarios=257, ldw=257), "257 scenarios, 1 to 256 allowed"),
                      (dict(rows=None), "null scenario table"), (dict(to=None), "null weight table or ldw < n_scenarios"), (dict(ldw=n - 1), "null weight table or ldw < n_scenarios")):
        assert weigh(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_tilt_weights" in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((acc == -3.0).all()) and bool((joint == -3.0).all()) and bool((out == -3.0).all())  # nothing was launched
    assert call() == 0 and weigh() == 0
    torch.cuda.synchronize()
    assert bool((acc[:, REWEIGH_COUNT] == g).all()) and bool((joint[:, REWEIGH_JOINT_GEOMETRIES] == g).all())
    assert np.array_equal(bits(out.cpu().numpy()), bits(tilt_weights_host(np.zeros((g, z)), tilt)))
    # the host check of the scenario table
    for at, value, words in (((1, 0, 1), np.nan, "scenario 1, latent 0: a, b or c is not finite"), ((0, 2, 4), np.nan, "scenario 0, latent 2: the window is NaN or has lo > hi"),
                             ((2, 1, slice(3, 5)), (1.0, 0.0), "scenario 2, latent 1: the window is NaN or has lo > hi")):
        bad = tilt.copy()
        bad[at] = value
        assert lib.okx_ensemble_tilt_check(bad.ctypes.data_as(C.c_void_p), n, z) != 0 and words in _lib.last_error(), _lib.last_error()
        with pytest.raises(ValueError, match=words.replace("(", r"\(")):
            dp.tilt_prepare(bad)
    assert lib.okx_ensemble_tilt_check(tilt.ctypes.data_as(C.c_void_p), n, z) == 0
    # the Python layer
    with pytest.raises(ValueError, match="accumulate=True needs"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, accumulate=True)
    with pytest.raises(ValueError, match="out= carries its own shift and limits"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, shift=shift, out=ReweighAccumulator(acc, joint, shift))
    with pytest.raises(ValueError, match="mask must be"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, mask=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="verdict must be a contiguous uint8"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, verdict=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"weights must be a float64 \[4, N\] device tensor"):
        dp.reweigh_ensemble(table[: 4 * s], steps_per_geometry=s, weights=weights)
    with pytest.raises(ValueError, match="a limit has lo > hi"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, limits=[1.0, 0.0])
    with pytest.raises(ValueError, match=r"out must hold contiguous device tables acc \[4, 10, S, K\]"):
        dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, out=ReweighAccumulator(acc[:3], joint[:3], shift))
    with pytest.raises(ValueError, match="latents must be a float64"):
        dp.tilt_weights(latents.cpu(), tilt)
    with pytest.raises(ValueError, match=r"scenarios must be a contiguous float64 \[N, 2, 5\] table"):
        dp.tilt_weights(latents[:, :2].contiguous(), table_dev)
    with pytest.raises(ValueError, match=r"out must be a float64 \[5, 4\] device tensor"):
        dp.tilt_weights(latents, table_dev, out=out[:4])
