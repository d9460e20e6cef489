"""
GPU: okx_ensemble_screen (DeviceProgram.screen_ensemble) and ShardedEnsemble(reduce=True, limits=..., screen=True) against
ensemble_stats.screen_host on the copied tables.  Every comparison is exact (array_equal; the margins by their BITS): flags,
entries, tallies, blame counts and survivor lists are integers' work, and a margin is a subtraction, a division and a
comparison of table values, each rounded on its own - a fused operation or a reciprocal would show as a differing bit.
"""

import os
import statistics
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_stats import SCREEN_OUTSIDE, SCREEN_UNRESOLVED, screen_host
from test_ensemble_screen import FIELDS, hand_made, same, two_sigma
from test_ensemble_stats import load_fixture, tampered_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7


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


def device_screen(dp, values, status, limits, scale=None, **kw):
    v, st = upload(values, status)
    got = dp.screen_ensemble(v, steps_per_geometry=values.shape[1], status=st, limits=limits, scale=scale, **kw)
    torch.cuda.synchronize()
    return got


def check(dp, values, status, limits, scale=None, offset=0):
    got = device_screen(dp, values, status, limits, scale, geometry_offset=offset).finalize()
    want = screen_host(values, status, limits, scale, offset)
    same(got, want)
    return want


def random_case(s, k, g, seed):
    """Normal values around per-entry centres, limits at the distance that lets about two thirds of the geometries pass all
    S K entries, a tenth of the entries open on one side or both, a random scale, a few NaN and rejected states."""
    rng = np.random.default_rng(seed)
    n = s * k
    z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * (2.0 / 3.0) ** (1.0 / n))
    centre = rng.normal(size=(s, k)) * 3.0
    values = centre[None] + rng.normal(size=(g, s, k))
    limits = np.stack([centre - z, centre + z], axis=2)
    kind = rng.random((s, k))
    limits[kind < 0.04, 0] = -np.inf
    limits[(kind >= 0.04) & (kind < 0.08), 1] = np.inf
    if n > 2:
        limits[(kind >= 0.08) & (kind < 0.1)] = (-np.inf, np.inf)
    scale = rng.uniform(0.3, 3.0, size=(s, k))
    status = np.ones((g, s), dtype=np.uint8)
    for _ in range(g // 25):
        values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = rng.choice([np.nan, np.inf, -np.inf])
        status[rng.integers(0, g), rng.integers(0, s)] = rng.choice(np.array([0, 2, 3, 5], dtype=np.uint8))
    return values, status, limits, scale


def test_the_tables_of_the_cpu_test(dp):
    fx = load_fixture()
    table = fx["table"]
    limits, sd = two_sigma(table)
    want = check(dp, table, None, limits, sd)
    assert list(want.tally) == [64, 36, 28, 0] and (want.blame.sum(axis=2) > 0).sum() == 23
    check(dp, table, None, limits)
    check(dp, table, None, limits, sd, offset=1000)
    tampered, status = tampered_fixture(fx)
    want = check(dp, tampered, status, limits, sd)
    assert want.tally[3] == 64
    opened = limits.copy()
    opened[4] = (-np.inf, np.inf)
    want = check(dp, tampered, status, opened, sd)
    assert 0 < want.tally[3] < 64 and want.tally[1] > 0 and want.tally[2] > 0
    for name, (values, st, lim, scale, flags, margin, entry) in sorted(hand_made().items()):
        want = check(dp, values, st, lim, scale)
        assert list(want.flags) == flags and list(want.entry) == entry, name
        for g in (0, 1):
            check(dp, values[:g], None if st is None else st[:g], lim, scale, offset=7)
    v = upload(table, None)[0]
    with pytest.raises(ValueError, match="lo > hi"):
        dp.screen_ensemble(v, steps_per_geometry=9, limits=(1.0, -1.0))
    with pytest.raises(ValueError, match="not finite and > 0"):
        dp.screen_ensemble(v, steps_per_geometry=9, limits=limits, scale=0.0)
    with pytest.raises(ValueError, match="unit column stride"):
        dp.screen_ensemble(v.t(), steps_per_geometry=9, limits=limits)
    with pytest.raises(ValueError, match="limits are needed"):
        dp.screen_ensemble(v, steps_per_geometry=9)


@pytest.mark.parametrize("entries", [(1, 1), (1, 2), (9, 7), (16, 4), (13, 5), (9, 15), (37, 7), (820, 5)])
def test_shapes_where_the_mapping_can_go_wrong(dp, entries):
    """S K in {1, 2, 63, 64, 65, 135, 4 * 64 + 3} - 64, 32, 1 geometries per wavefront, under, at and over one wavefront's
    stride - and 4100, where the blame counters leave LDS for per-wavefront runs; G in {0, 1, 37, 64} and a count that spans
    several workgroups and is no multiple of the geometries a wavefront packs."""
    s, k = entries
    for g in (0, 1, 37, 64, 1031 if s * k < 4000 else 131):
        values, status, limits, scale = random_case(s, k, g, 1000 * s * k + g)
        want = check(dp, values, status, limits, scale, offset=3 * g)
        if g > 1000:  # the inputs are worth the test: about a third fail
            assert 0.1 < 1.0 - want.joint_yield < 0.6 and want.tally[2] > 0 and want.tally[3] > 0
    check(dp, values, None, limits)  # no status bytes, no scale
    if s * k > 4000:  # every failure at ONE entry: one run per wavefront
        values = np.zeros((131, s, k))
        values[::2, 700, 3] = 5.0
        one = np.full((s, k, 2), np.inf)
        one[..., 0] = -np.inf
        one[700, 3] = (-1.0, 1.0)
        want = check(dp, values, None, one)
        assert want.blame[700, 3, 1] == 66 and want.blame.sum() == 66


def test_strided_rows_inside_a_larger_tensor(dp):
    """Row 0 of evaluation-shaped records (ld = 3 * 24 > K) and byte 32 of 40-byte info records as views in the MIDDLE of larger
    tensors filled with NaN and rejected bytes: a read outside the view would change a verdict."""
    s, k, g = 8, 24, 50
    values, status, limits, scale = random_case(s, k, g, 77)
    pad = 40
    big = torch.full((pad + g * s + pad, 3, 24), float("nan"), dtype=torch.float64, device=DEV)
    info = torch.full((pad + g * s + pad, 40), 2, dtype=torch.uint8, device=DEV)
    big[pad : pad + g * s, 0, :] = torch.as_tensor(values.reshape(g * s, k), device=DEV)
    info[pad : pad + g * s, 32] = torch.as_tensor(status.reshape(-1), device=DEV)
    view, st = big[pad : pad + g * s, 0, :], info[pad : pad + g * s, 32]
    assert view.stride(0) == 72 and not view.is_contiguous() and st.stride(0) == 40
    got = dp.screen_ensemble(view, steps_per_geometry=s, status=st, limits=limits, scale=scale)
    torch.cuda.synchronize()
    want = screen_host(values, status, limits, scale)
    same(got.finalize(), want)
    assert 0 < want.tally[1] < g and want.tally[3] > 0
    # ... and a narrower table inside the same rows (K = 5 of 24 columns)
    narrow = big[pad : pad + g * s, 0, 3:8]
    got = dp.screen_ensemble(narrow, steps_per_geometry=s, status=st, limits=limits[:, 3:8], scale=scale[:, 3:8])
    torch.cuda.synchronize()
    same(got.finalize(), screen_host(values[:, :, 3:8], status, limits[:, 3:8], scale[:, 3:8]))


def test_survivor_list_and_capacity(dp):
    s, k, g = 13, 5, 700
    values, status, limits, scale = random_case(s, k, g, 5)
    want = screen_host(values, status, limits, scale, 10_000)
    n = want.passed.size
    assert 100 < n < g
    v, st = upload(values, status)
    for cap in (0, 1, n // 2, n - 1, n, n + 50):
        out = dp.screen_prepare(s, k, limits, scale, g, capacity=cap)
        out.pass_index.fill_(SENTINEL)
        dp.screen_ensemble(v, steps_per_geometry=s, status=st, geometry_offset=10_000, out=out, first_row=0)
        torch.cuda.synchronize()
        index = out.pass_index.cpu().numpy()
        assert int(out.pass_count) == n and index.shape == (cap,)
        assert np.array_equal(index[: min(n, cap)], want.passed[:cap]) and np.all(index[min(n, cap):] == SENTINEL)
        assert np.array_equal(out.flags.cpu().numpy(), want.flags) and np.array_equal(out.tally.cpu().numpy(), want.tally)


@pytest.mark.parametrize("edges", [[0, 300], [0, 149, 300], [0, 1, 2, 130, 130, 300]])
def test_chunks_accumulate_to_the_one_call(dp, edges):
    s, k, g = 16, 4, 300
    values, status, limits, scale = random_case(s, k, g, 21)
    whole = device_screen(dp, values, status, limits, scale, geometry_offset=500)
    v, st = upload(values, status)
    out = dp.screen_prepare(s, k, limits, scale, g)
    out.pass_index.fill_(SENTINEL)
    for tensor in (out.tally, out.blame, out.pass_count):
        tensor.fill_(99)  # the first call overwrites
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        dp.screen_ensemble(v[a * s : b * s], steps_per_geometry=s, status=st[a * s : b * s], geometry_offset=500 + a, out=out, accumulate=i > 0,
                           first_row=a)
    torch.cuda.synchronize()
    for name in ("flags", "margin", "entry", "tally", "blame", "pass_count"):
        assert torch.equal(getattr(out, name), getattr(whole, name)), name  # (no NaN margin: torch.equal compares values)
    n = int(whole.pass_count)
    assert torch.equal(out.pass_index[:n], whole.pass_index[:n]) and bool((out.pass_index[n:] == SENTINEL).all())
    same(out.finalize(), screen_host(values, status, limits, scale, 500))


def test_determinism_and_a_captured_graph(dp):
    s, k, g = 16, 4, 1500
    values, status, limits, scale = random_case(s, k, g, 8)
    v, st = upload(values, status)
    tensors = lambda r: (r.flags, r.margin, r.entry, r.tally, r.blame, r.pass_index, r.pass_count)  # noqa: E731
    first = dp.screen_ensemble(v, steps_per_geometry=s, status=st, limits=limits, scale=scale)
    second = dp.screen_ensemble(v, steps_per_geometry=s, status=st, limits=limits, scale=scale)
    torch.cuda.synchronize()
    want = screen_host(values, status, limits, scale)
    n = want.passed.size
    for a, b in zip(tensors(first), tensors(second)):
        assert torch.equal(a[:n], b[:n]) if a is first.pass_index else torch.equal(a, b)  # (slots beyond the count are never written)
    same(first.finalize(), want)
    # a single-stream captured graph, replayed once after its outputs were overwritten
    out = dp.screen_prepare(s, k, limits, scale, g)
    dp.screen_ensemble(v, steps_per_geometry=s, status=st, out=out)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.screen_ensemble(v, steps_per_geometry=s, status=st, out=out)
    for t in tensors(out):
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(tensors(out), tensors(first)):
        if a is out.pass_index:
            assert torch.equal(a[:n], b[:n])  # (slots beyond the count are never written)
        else:
            assert torch.equal(a, b)


def _c5(n_geom, steps):
    from test_gpu_ensemble_stats import _c5 as build

    return build(n_geom, steps)


def band(values, status, lo=0.05, hi=0.95):
    """Limits and scale from a table itself: the [lo, hi] quantile band per entry of what counts, its std (1 where it is 0)."""
    masked = np.where(np.isfinite(values) & ((status & 7) == 1)[:, :, None], values, np.nan)
    limits = np.stack([np.nanquantile(masked, lo, axis=0), np.nanquantile(masked, hi, axis=0)], axis=2)
    scale = np.nanstd(masked, axis=0)
    scale[~(scale > 0)] = 1.0
    return limits, scale


def _sharded_reference(g, s):
    """(dp, hardpoints, relative targets, columns, values [G, S, K], status [G, S]) of the reduced ensemble on one GPU."""
    import open_kinematics_amd.dist as okd

    dp, program, table, rel, columns = _c5(g, s)
    plain = okd.ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, chain_len=1, predictor=False)
    plain.step()
    torch.cuda.synchronize()
    values = plain.metric_local.cpu().numpy().reshape(g, s, len(columns))
    status = plain.info_local[:, 32].cpu().numpy().reshape(g, s)
    return dp, table, rel, columns, values, status, plain


def test_sharded_ensemble_on_one_gpu():
    """64 geometries x 16 steps of the double wishbone, solved and evaluated: screen() and screen_local() equal screen_host of the
    same run's metric_local and status bytes, with one chunk and with two; the accumulator is what it is without the screen."""
    import open_kinematics_amd.dist as okd

    g, s = 64, 16
    dp, table, rel, columns, values, status, plain = _sharded_reference(g, s)
    limits, scale = band(values, status, 0.02, 0.98)
    want = screen_host(values, status, limits, scale)
    assert 0 < want.tally[1] < g
    kw = dict(metric_columns=columns, reduce=True, limits=limits, screen=True, screen_scale=scale, chain_len=1, predictor=False)
    for chunks in (1, 2):
        pipe = okd.ShardedEnsemble(dp, table, rel, s, chunks=chunks, **kw)
        for _ in range(2):  # the second step overwrites the first
            acc = pipe.step()
            torch.cuda.synchronize()
            assert np.array_equal(pipe.metric_local.cpu().numpy().reshape(g, s, 4), values, equal_nan=True)
            got, local = pipe.screen(), pipe.screen_local()
            for f in ("flags", "tally", "blame", "passed"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (f, chunks)
            assert got.margin is None and np.array_equal(local["margin"].cpu().numpy().view(np.uint64), want.margin.view(np.uint64))
            assert np.array_equal(local["entry"].cpu().numpy(), want.entry) and int(local["pass_count"]) == want.passed.size
            assert np.array_equal(local["pass_index"].cpu().numpy()[: want.passed.size], want.passed)
            assert torch.equal(acc.acc, plain.accumulator.acc)
        assert pipe.screen_exchange_bytes_per_rank == 0 and pipe.exchange_bytes_per_rank == 0
    # what stays in HBM feeds what follows without a host copy: the worst survivors by margin
    worst = torch.topk(local["margin"], 3, largest=False).indices.cpu().numpy()
    assert set(worst) == set(np.argsort(want.margin, kind="stable")[:3])


@pytest.mark.parametrize("world,g,chunks", [(2, 256, 2), (3, 2, 1)])
def test_ranks_rehearsed_on_one_gpu(tmp_path, world, g, chunks):
    """Two ranks at 256 x 16 in two chunks, and three ranks over two geometries (rank 2 owns none), on cuda:0 over gloo in fresh
    child processes: every rank holds screen_host's bits of the one-process table."""
    import open_kinematics_amd.dist as okd

    s = 16
    dp, table, rel, columns, values, status, plain = _sharded_reference(g, s)
    limits, scale = band(values, status, 0.01, 0.99) if g > 2 else (np.tile(np.array([-0.5, 0.5]), (s, 4, 1)), np.ones((s, 4)))
    want = screen_host(values, status, limits, scale)
    if g > 2:
        assert 0 < want.tally[1] < g
    path = os.path.join(tmp_path, "limits.npz")
    np.savez(path, limits=limits, scale=scale)
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_screen_rate.py"), "--rehearse", str(world), "--geometries", str(g),
                           "--steps-per-geometry", str(s), "--chunks", str(chunks), "--limits", path, "--out", str(tmp_path)],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    largest = max(hi - lo for lo, hi in (okd.shard_range(g, r, world) for r in range(world)))
    for r in range(world):
        for f in ("flags", "tally", "blame", "passed"):
            assert np.array_equal(got[r]["screen"][f], getattr(want, f)), (f, r)
        lo, hi = got[r]["range"]
        assert (lo, hi) == okd.shard_range(g, r, world)
        loc = got[r]["local"]
        assert np.array_equal(loc["margin"].numpy().view(np.uint64), want.margin[lo:hi].view(np.uint64)) and np.array_equal(loc["entry"].numpy(), want.entry[lo:hi])
        mine = want.passed[(want.passed >= lo) & (want.passed < hi)]
        assert int(loc["pass_count"]) == mine.size and np.array_equal(loc["pass_index"].numpy()[: mine.size], mine)
        assert got[r]["screen_sent"] == 8 * (4 + 2 * s * 4) + largest and got[r]["sent"] == 8 * s * 4 * 8


def test_end_to_end_on_evaluation_rows():
    """A small real ensemble - perturbed hardpoints of the double wishbone over a bump sweep - solved and evaluated; the screen
    reads row 0 of the evaluation records and byte 32 of the info records in place."""
    g, s = 48, 8
    dp, program, table, rel, columns = _c5(g, s)
    gpos, gparam = dp.rebind(table)
    targets = dp.ensemble_targets(gpos, rel)
    res = dp.solve_evaluated(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, output="none", chain_len=1, predictor=False)
    torch.cuda.synchronize()
    view, st = res.eval[:, 0, :], res.info_raw[:, 32]
    k = view.shape[1]
    assert view.stride(0) > k and st.stride(0) == 40
    values, status = view.cpu().numpy().reshape(g, s, k), st.cpu().numpy().reshape(g, s)
    limits = np.full((s, k, 2), np.inf)
    limits[..., 0] = -np.inf
    # three metric columns are limited - the first that are finite wherever the state counts and vary at every step -, the
    # others (several of them NaN for this suspension) are not looked at
    counts = (status & 7) == 1
    some = [c for c in range(19) if np.isfinite(values[:, :, c][counts]).all() and np.nanstd(np.where(counts, values[:, :, c], np.nan), axis=0).min() > 0][:3]
    assert len(some) == 3
    limits[:, some], scale = band(values[:, :, some], status, 0.03, 0.97)
    full_scale = np.ones((s, k))
    full_scale[:, some] = scale
    got = dp.screen_ensemble(view, steps_per_geometry=s, status=st, limits=limits, scale=full_scale)
    torch.cuda.synchronize()
    want = screen_host(values, status, limits, full_scale)
    same(got.finalize(), want)
    assert 0 < want.tally[1] < g and set(want.entry % k) <= set(some)
    assert (want.flags & SCREEN_UNRESOLVED).any() == bool((~((status & 7) == 1)).any()) and (want.flags & SCREEN_OUTSIDE).any()
