"""
GPU: okx_ensemble_select (DeviceProgram.select_ensemble and its round-level calls) and ShardedEnsemble(reduce=True,
quantiles=...) against ensemble_stats.select_host - NumPy's sort - on the copied tables.  Order statistics, counts and
limit counts are compared EXACTLY (array_equal: they are selected by integer counting), the device histogram of every
round with the NumPy round's; the one floating-point bound, of the interpolated quantile, is derived in
tests/test_ensemble_select.py and checked there.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd import ensemble_stats as es
from open_kinematics_amd.ensemble_stats import ENS_MAX, ENS_MIN, select_host
from test_ensemble_select import FIELDS, PROBS, hand_made_columns, same
from test_ensemble_stats import load_fixture, tampered_fixture
from test_gpu_metrics import _roles
from test_metrics_oracle import load_metrics_golden

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


def upload(values, status):
    g, s, k = values.shape
    return (torch.as_tensor(values.reshape(g * s, k), device=DEV),
            None if status is None else torch.as_tensor(np.ascontiguousarray(status).reshape(-1), device=DEV))


def device_select(dp, values, status, probs, limits=None):
    v, st = upload(values, status)
    got = dp.select_ensemble(v, steps_per_geometry=values.shape[1], status=st, probs=probs, limits=limits)
    torch.cuda.synchronize()
    return got


def rounds_on_device(dp, values, status, probs, limits, chunks=1, histograms=None):
    """The round-level calls over ``chunks`` runs of geometries; ``histograms``: a list that takes every round's histogram."""
    g, s, k = values.shape
    v, st = upload(values, status)
    run = dp.select_prepare(s, k, probs, limits, rounds=True)
    run.hist.fill_(7)  # begin zeroes it
    dp.select_begin(run)
    edges = [g * i // chunks for i in range(chunks + 1)]
    for rnd in range(dp.select_rounds):
        for a, b in zip(edges[:-1], edges[1:]):
            dp.select_count(run, rnd, v[a * s : b * s], steps_per_geometry=s, status=None if st is None else st[a * s : b * s])
        if histograms is not None:
            histograms.append(run.hist.cpu().numpy())
        dp.select_descend(run, rnd)
    dp.select_finish(run)
    torch.cuda.synchronize()
    assert not run.hist.any()  # the last descend leaves it zero
    return run


def test_fixture_against_numpy_round_by_round(dp):
    """The fixture's reference values uploaded as they are; every round's device histogram equals the NumPy round's."""
    fx = load_fixture()
    table = fx["table"]
    limits = np.stack([np.quantile(table, 0.1, axis=0), np.quantile(table, 0.8, axis=0)], axis=2)
    want = select_host(table, None, PROBS, limits)
    same(device_select(dp, table, None, PROBS, limits).finalize(), want)
    assert dp.select_rounds == es.SELECT_ROUNDS
    mine, theirs = [], []
    run = rounds_on_device(dp, table, None, PROBS, limits, histograms=mine)
    same(run.finalize(), want)
    same(es.select_rounds_host(table, None, PROBS, limits, on_round=lambda rnd, hist: theirs.append(hist.copy())), want)
    assert len(mine) == len(theirs) == es.SELECT_ROUNDS
    for rnd, (a, b) in enumerate(zip(mine, theirs)):
        assert a.shape == b.shape and np.array_equal(a, b), rnd
    got = run.finalize()
    assert np.array_equal(got.lower[..., 0], fx["stat_min"]) and np.array_equal(got.upper[..., -1], fx["stat_max"])
    acc = dp.reduce_ensemble(upload(table, None)[0], steps_per_geometry=table.shape[1])
    torch.cuda.synchronize()
    assert np.array_equal(got.lower[..., 0], acc.numpy().acc[..., ENS_MIN]) and np.array_equal(got.upper[..., -1], acc.numpy().acc[..., ENS_MAX])
    with pytest.raises(ValueError, match="unit column stride"):
        dp.select_ensemble(upload(table, None)[0].t(), steps_per_geometry=table.shape[1], probs=PROBS)
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        dp.select_ensemble(upload(table, None)[0], steps_per_geometry=table.shape[1], probs=(0.5, 1.25))
    with pytest.raises(ValueError, match="lo > hi"):
        dp.select_ensemble(upload(table, None)[0], steps_per_geometry=table.shape[1], probs=(0.5,), limits=(1.0, -1.0))


def test_tampered_table_and_hand_made_columns(dp):
    fx = load_fixture()
    table, status = tampered_fixture(fx)
    limits = np.stack([np.nanquantile(fx["table"], 0.1, axis=0), np.nanquantile(fx["table"], 0.8, axis=0)], axis=2)
    got = device_select(dp, table, status, PROBS, limits).finalize()
    same(got, select_host(table, status, PROBS, limits))
    assert np.all(got.count[4] == 0) and np.all(np.isnan(got.lower[4])) and np.all(np.isnan(got.yield_[4]))
    # limits equal to table values (strictness) and open sides
    eq = np.empty(table.shape[1:] + (2,))
    eq[..., 0], eq[..., 1] = np.nan_to_num(table[7], nan=-1.0, posinf=-1.0), np.nan_to_num(table[7], nan=-1.0, posinf=-1.0)
    eq[2, :, 0], eq[3, :, 1] = -np.inf, np.inf
    same(device_select(dp, table, status, (0.5,), eq).finalize(), select_host(table, status, (0.5,), eq))
    cols = hand_made_columns()
    for g in (37, 2, 1, 0):
        status = np.ones((g, 1), dtype=np.uint8)
        if g == 37:
            status[[3, 30]] = 2
        got = device_select(dp, cols[:g], status, PROBS, (-1.0, 1.0)).finalize()
        same(got, select_host(cols[:g], status, PROBS, (-1.0, 1.0)))
    assert np.all(got.count == 0) and np.all(np.isnan(got.lower)) and np.all(got.below == 0)  # G = 0


@pytest.mark.parametrize("entries", [(1, 1), (5, 3), (16, 4), (13, 5), (9, 15)])
def test_shapes_where_tiles_and_slabs_can_go_wrong(dp, entries):
    """S K in {1, 15, 64, 65, 135} (under, at and over a tile of 64 entries) with G in {1, 2, 37, 300, 1031} (one lane of a
    wavefront's four geometries in flight, a ragged last slab, several slabs), about 2 % of the states rejected."""
    s, k = entries
    rng = np.random.default_rng(100 + s * k)
    for g in (1, 2, 37, 300, 1031):
        values = rng.normal(size=(g, s, k))
        values.reshape(-1)[rng.integers(0, values.size, max(1, values.size // 100))] = np.nan
        status = np.where(rng.random((g, s)) < 0.01, 2, 1).astype(np.uint8)
        limits = rng.normal(size=(s, k, 1)) + np.array([-0.5, 0.5])
        same(device_select(dp, values, status, (0.00135, 0.5, 0.99865), limits).finalize(), select_host(values, status, (0.00135, 0.5, 0.99865), limits))
    # many probabilities: the tile narrows below a wavefront (2 Q = 80 selections)
    many = tuple(np.linspace(0.0, 1.0, 40))
    same(device_select(dp, values, status, many).finalize(), select_host(values, status, many))


@pytest.mark.parametrize("kind", ["corner", "axle"])
def test_strided_views_of_evaluation_rows(golden, kind):
    """Row 0 of a corner (ld = 24 (1 + T)) and of an axle (ld = 64 (1 + T)) evaluation as a strided view, the status byte taken
    from 40-byte info records: the same bits as the packed copy, equal to NumPy's."""
    from open_kinematics_amd.batch import DeviceProgram

    if kind == "corner":
        arrays, program = golden("c1_dw_corner")
        program = program.with_line_mode("pinned")
        dp = DeviceProgram(program, DEV)
        roles, _ = _roles(program, load_metrics_golden("c1_dw_corner"))
        dp.enable_evaluation(roles)
        ev = dp.solve_evaluated(arrays["targets_abs"][:96], output="none").eval
    else:
        import yaml

        from open_kinematics_amd.input import build_suspension, build_sweep
        from open_kinematics_amd.metrics import axle_evaluation_roles
        from open_kinematics_amd.sweep import sweep_program

        arrays, _ = golden("c3_axle_grid")
        axle = build_suspension(yaml.safe_load(str(arrays["geometry_yaml"])))
        program, table = sweep_program(axle, build_sweep(yaml.safe_load(str(arrays["sweep_yaml"])), axle))
        dp = DeviceProgram(program, DEV)
        dp.enable_evaluation(axle_evaluation_roles(axle, program)[0])
        ev = dp.solve_evaluated(np.asarray(table)[:96], output="none").eval
    torch.cuda.synchronize()
    b, rows, width = ev.shape
    assert width == (24 if kind == "corner" else 64) and b == 96
    s = 8
    g = b // s
    view = ev[:, 0, :]
    assert view.stride(0) == rows * width and not view.is_contiguous()
    info = torch.zeros((b, 40), dtype=torch.uint8, device=DEV)
    info[:, 32] = 1
    info[::7, 32] = 2
    probs, limits = (0.1, 0.5, 1.0), (-1.0, 1.0)
    a = dp.select_ensemble(view, steps_per_geometry=s, status=info[:, 32], probs=probs, limits=limits)
    packed = dp.select_ensemble(view.contiguous(), steps_per_geometry=s, status=info[:, 32].contiguous(), probs=probs, limits=limits)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(a.order), torch.nan_to_num(packed.order)) and torch.equal(torch.isnan(a.order), torch.isnan(packed.order))
    assert torch.equal(a.count, packed.count) and torch.equal(a.outside, packed.outside)
    want = select_host(view.cpu().numpy().reshape(g, s, width), info[:, 32].cpu().numpy().reshape(g, s), probs, limits)
    same(a.finalize(), want)
    assert 0 < want.count.max() <= g


def test_values_at_the_end_of_their_allocation(dp):
    """The table as the tail of a large allocation of its own: no read lies beyond values[G S - 1][K - 1]."""
    rng = np.random.default_rng(5)
    for g, s, k in ((37, 5, 3), (1, 1, 1), (300, 13, 5)):
        values = rng.normal(size=(g, s, k))
        status = np.where(rng.random((g, s)) < 0.05, 4, 1).astype(np.uint8)
        block = torch.empty(32 * 1024 * 1024 // 8, dtype=torch.float64, device=DEV)  # (large enough to be an allocation of its own)
        tail = block[block.numel() - g * s * k :].view(g * s, k)
        tail.copy_(torch.as_tensor(values.reshape(g * s, k)))
        assert tail.data_ptr() + 8 * g * s * k == block.data_ptr() + 8 * block.numel()
        bytes_ = torch.empty(32 * 1024 * 1024, dtype=torch.uint8, device=DEV)
        st = bytes_[bytes_.numel() - g * s :]
        st.copy_(torch.as_tensor(status.reshape(-1)))
        got = dp.select_ensemble(tail, steps_per_geometry=s, status=st, probs=PROBS, limits=(-0.5, 0.5))
        torch.cuda.synchronize()
        same(got.finalize(), select_host(values, status, PROBS, (-0.5, 0.5)))


def test_determinism_chunks_and_a_captured_graph(dp):
    rng = np.random.default_rng(8)
    g, s, k = 300, 16, 4
    values = rng.normal(size=(g, s, k))
    values[rng.integers(0, g, 50), rng.integers(0, s, 50), rng.integers(0, k, 50)] = np.inf
    status = np.where(rng.random((g, s)) < 0.02, 3, 1).astype(np.uint8)
    limits = (-1.0, 0.75)
    v, st = upload(values, status)
    first = dp.select_ensemble(v, steps_per_geometry=s, status=st, probs=PROBS, limits=limits)
    second = dp.select_ensemble(v, steps_per_geometry=s, status=st, probs=PROBS, limits=limits)
    torch.cuda.synchronize()
    tensors = lambda r: (r.order, r.count, r.outside)  # noqa: E731
    assert all(torch.equal(a, b) for a, b in zip(tensors(first), tensors(second)))  # (no NaN here: every entry has states that count)
    same(first.finalize(), select_host(values, status, PROBS, limits))
    for chunks in (1, 2, 8):
        run = rounds_on_device(dp, values, status, PROBS, limits, chunks=chunks)
        assert all(torch.equal(a, b) for a, b in zip(tensors(run), tensors(first))), chunks
    # a captured graph, replayed after its outputs were zeroed
    out = dp.select_prepare(s, k, PROBS, limits)
    dp.select_ensemble(v, steps_per_geometry=s, status=st, out=out)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.select_ensemble(v, steps_per_geometry=s, status=st, out=out)
    for _ in range(2):
        for t in tensors(out):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(tensors(out), tensors(first)))


def _c5(n_geom, steps):
    from test_gpu_ensemble_stats import _c5 as build

    return build(n_geom, steps)


def test_sharded_ensemble_on_one_gpu():
    """64 geometries x 16 steps of the double wishbone, solved and evaluated: quantiles() equals select_host of the same run's
    metric_local and status bytes; p = 0 / 1 equal the accumulator's extremes."""
    import open_kinematics_amd.dist as okd

    g, s = 64, 16
    dp, program, table, rel, columns = _c5(g, s)
    probs = (0.0, 0.00135, 0.5, 0.99865, 1.0)
    limits = np.array([[-0.5, 0.5], [-np.inf, 0.0], [0.0, np.inf], [-1.0, 1.0]])
    kw = dict(chain_len=1, predictor=False)
    pipe = okd.ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, quantiles=probs, limits=limits, **kw)
    acc = pipe.step()
    torch.cuda.synchronize()
    got = pipe.quantiles()
    values = pipe.metric_local.cpu().numpy().reshape(g, s, 4)
    status = pipe.info_local[:, 32].cpu().numpy().reshape(g, s)
    same(got, select_host(values, status, probs, limits))
    a = acc.numpy().acc
    assert np.all(got.count > 0) and np.array_equal(got.count, a[..., 0].astype(np.int64))
    assert np.array_equal(got.lower[..., 0], a[..., ENS_MIN]) and np.array_equal(got.upper[..., -1], a[..., ENS_MAX])
    assert pipe.select_exchange_bytes_per_rank == 0 and pipe.exchange_bytes_per_rank == 0
    plain = okd.ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, **kw)
    assert torch.equal(plain.step().acc, acc.acc)  # the accumulator is what it is without quantiles
    pipe.step()
    torch.cuda.synchronize()
    same(pipe.quantiles(), got)
    two = okd.ShardedEnsemble(dp, table, rel, s, chunks=2, metric_columns=columns, reduce=True, quantiles=probs, limits=limits, **kw)
    two.step()
    same(two.quantiles(), got)


def _rehearse(tmp_path, world, g, s):
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_select_rate.py"), "--rehearse", str(world), "--geometries", str(g),
                           "--steps-per-geometry", str(s), "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    for r in range(1, world):  # the same bits on every rank
        for f in FIELDS:
            assert np.array_equal(got[0]["q"][f], got[r]["q"][f], equal_nan=True), (f, r)
    return got


@pytest.mark.parametrize("world,g", [(2, 256), (3, 2)])
def test_ranks_rehearsed_on_one_gpu(tmp_path, world, g):
    """Two ranks at 256 x 16, and three ranks over two geometries (rank 2 owns none and contributes a zero histogram), on
    cuda:0 over gloo in fresh child processes: every rank holds the one-process result's bits."""
    import open_kinematics_amd.dist as okd

    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_select_rate import PROBS as TOOL_PROBS, window

    s = 16
    got = _rehearse(tmp_path, world, g, s)
    assert [r["range"] for r in got] == [okd.shard_range(g, r, world) for r in range(world)]
    dp, program, table, rel, columns = _c5(g, s)
    pipe = okd.ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, quantiles=TOOL_PROBS, limits=window(s, 4),
                               chain_len=1, predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    alone = pipe.quantiles()
    for f in FIELDS:
        assert np.array_equal(got[0]["q"][f], getattr(alone, f), equal_nan=True), f
    assert got[0]["select_sent"] == es.SELECT_ROUNDS * 8 * s * 4 * 2 * len(TOOL_PROBS) * es.SELECT_BINS and got[0]["sent"] == 8 * s * 4 * 8
