"""
GPU: okx_ensemble_front (DeviceProgram.front_ensemble, its merge, and ShardedEnsemble(reduce=True, front=...)) against
ensemble_stats.front_host on the copied tables.  Every comparison is exact - int32 / int64 tables as integers, front values by
their bits; tests/test_ensemble_front.py holds the generator of the inputs and the special rows.
"""

import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd.ensemble_stats import CURVE_FIELDS, CURVE_MAX, CURVE_MIN, CURVE_X_AT_MAX, curves_host, front_host, screen_host
from test_ensemble_front import (assert_worth, bits, front_case, same_front, signed_zero_rows, special_rows, target_rounding_rows, worth)

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


def upload(values, status=None, mask=None, *, ld=None, info=False):
    """``(values [G * S, K] view, status [G * S] view or None, mask [G] or None)`` on the device.  ``ld``: the rows lie in a wider
    tensor whose other columns hold NaN; ``info``: the status byte is byte 32 of 40-byte records whose other bytes are 2."""
    g, s, k = values.shape
    wide = torch.full((g * s, k if ld is None else ld), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :k] = torch.as_tensor(np.ascontiguousarray(values).reshape(g * s, k), device=DEV)
    st = None
    if status is not None:
        st = torch.as_tensor(np.ascontiguousarray(status).reshape(-1), device=DEV)
        if info:
            records = torch.full((g * s, 40), 2, dtype=torch.uint8, device=DEV)
            records[:, 32] = st
            st = records[:, 32]
    return wide[:, :k], st, None if mask is None else torch.as_tensor(mask, device=DEV)


def device_front(dp, case, *, ld=None, info=False, index=None, geometry_offset=0, **kw):
    values, status, objectives, mask = case
    v, st, mk = upload(values, status, mask, ld=ld, info=info)
    ids = None if index is None else torch.as_tensor(index, device=DEV)
    got = dp.front_ensemble(v, steps_per_geometry=values.shape[1], objectives=objectives, status=st, mask=mk, index=ids, geometry_offset=geometry_offset, **kw)
    torch.cuda.synchronize()
    return got


@functools.lru_cache(maxsize=None)
def reference(g, m, levels, layout):
    """The case and ``front_host`` of it, computed once and shared (the arrays are not written)."""
    s, k, _, with_status, _, with_mask, with_index = LAYOUTS[layout](m)
    case = front_case(g, m, levels, s=s, k=k, mixed=layout % 2 == 1, with_status=with_status, with_mask=with_mask)
    index = np.random.default_rng(g + layout).permutation(g).astype(np.int64) * 5 - 3 if with_index else None
    return case, index, front_host(*case, index, 10_000 * layout)


# (S, K, ld, status, status as byte 32 of info records, mask, ids through d_index) by the objective count
LAYOUTS = [lambda m: (1, m, m, False, False, False, False),
           lambda m: (5, 4, 7, True, False, True, False),
           lambda m: (3, 24, 24, True, True, False, True),
           lambda m: (1, m, m, True, True, True, True),
           lambda m: ((1, 1, 1) if m == 1 else (5, 4, 7)) + (False, False, True, True)]


def compare(dp, g, m, levels, layout):
    s, k, ld, _, info, _, _ = LAYOUTS[layout](m)
    case, index, want = reference(g, m, levels, layout)
    got = device_front(dp, case, ld=ld, info=info, index=index, geometry_offset=10_000 * layout)
    assert got.dominated.dtype == torch.int32 and got.tally.dtype == torch.int64 and got.front_index.dtype == torch.int64
    assert same_front(got.finalize(), want), (g, m, levels, layout)
    return worth(want)


# every G with two values of M, every M with three values of G
TWO_M = {0: (1, 5), 1: (2, 8), 2: (1, 3), 63: (2, 5), 64: (1, 8), 65: (2, 3), 255: (1, 5), 256: (2, 8), 257: (2, 3), 1031: (1, 8), 4099: (2, 5)}
THREE_G = {1: (37, 257, 1031), 2: (65, 256, 1031), 3: (63, 257, 1031), 5: (63, 256, 1031), 8: (65, 255, 4099)}


@pytest.mark.parametrize("g", list(TWO_M))
def test_every_geometry_count(dp, g):
    """G in {0, 1, 2, 63, 64, 65, 255, 256, 257, 1031, 4099}: no geometry, fewer than a wavefront, a tile of 64 a-vectors and a
    workgroup of 256 b lanes filled, one short and one over; 1031 and 4099 have several workgroups along b, an a range split
    over blockIdx.y in pieces of one tile (1031) and two (4099), a last tile with NaN padding and several compaction
    workgroups.  Table shape, status bytes, mask and ids change from run to run."""
    runs = []
    for at, m in enumerate(TWO_M[g]):
        for levels in (4, 16, 0):
            got = compare(dp, g, m, levels, (g + at + levels) % len(LAYOUTS))
            if g >= 37:
                runs.append(got)
    if g >= 37:
        assert_worth(runs, 4)


@pytest.mark.parametrize("m", list(THREE_G))
def test_every_objective_count(dp, m):
    """M in {1, 2, 3, 5, 8}: every padded row length (1, 2, 4, 6, 8 doubles) of the all-pairs kernel's template."""
    runs = []
    for at, g in enumerate(THREE_G[m]):
        for levels in (4, 16, 0):
            runs.append(compare(dp, g, m, levels, (m + at + levels // 4) % len(LAYOUTS)))
    assert_worth(runs, 4)


def test_every_table_shape(dp):
    """(S, K, ld) in {(1, 1, 1), (1, M, M), (5, 4, 7), (3, 24, 24)} with status NULL, contiguous and byte 32 of okx_info records at
    stride 40, the mask NULL and given, ids by offset and through d_index - every layout at one size."""
    runs = []
    for layout in range(len(LAYOUTS)):
        for m in (1, 3):
            runs.append(compare(dp, 300, m, 4, layout))
    assert_worth(runs, 4)


def test_special_rows(dp):
    """All rows equal, a strict chain and an antichain (the compaction's worst case: everyone is written) at G = 1031; the -0.0
    tie and the TARGET difference that is rounded once."""
    g = 1031
    for name, (values, objectives, dominated) in special_rows(g).items():
        got = device_front(dp, (values, None, objectives, None)).finalize()
        assert np.array_equal(got.dominated, dominated), name
        assert same_front(got, front_host(values, None, objectives)) and got.tally[2] == (1 if name == "chain" else g)
    values, objectives, dominated = signed_zero_rows()
    got = device_front(dp, (values, None, objectives, None)).finalize()
    assert list(got.dominated) == dominated and same_front(got, front_host(values, None, objectives))
    assert np.array_equal(bits(got.values), bits(values[:2, 0, :]))  # the zeros keep their signs
    rows, near, d_near, far, d_far = target_rounding_rows()
    for objectives, dominated in ((near, d_near), (far, d_far)):
        got = device_front(dp, (rows, None, objectives, None)).finalize()
        assert list(got.dominated) == dominated and same_front(got, front_host(rows, None, objectives))


def test_capacity(dp):
    """No list at all (NULL pointers), capacity 0, one slot short and exact: the tally reports the full count, the slots that are
    there hold the first members, and nothing beyond them is touched."""
    g, m = 300, 3
    case, _, want = reference(g, m, 16, 0)
    n = int(want.tally[2])
    assert 3 < n < g
    v, _, _ = upload(case[0])
    for capacity in (0, n - 1, n, g):
        out = dp.front_prepare(1, m, g, case[2], capacity)
        spare = torch.full((g + 8,), SENTINEL, dtype=torch.int64, device=DEV), torch.full((g + 8, m), float(SENTINEL), dtype=torch.float64, device=DEV)
        out.front_index, out.front_values = spare[0][:capacity], spare[1][:capacity]  # (views: what lies behind them is watched too)
        dp.front_ensemble(v, steps_per_geometry=1, out=out)
        torch.cuda.synchronize()
        held = min(n, capacity)
        assert out.tally.tolist() == want.tally.tolist() and np.array_equal(out.dominated.cpu().numpy(), want.dominated)
        assert np.array_equal(spare[0][:held].cpu().numpy(), want.index[:held]) and np.array_equal(bits(spare[1][:held].cpu().numpy()), bits(want.values[:held]))
        assert bool((spare[0][held:] == SENTINEL).all()) and bool((spare[1][held:] == float(SENTINEL)).all())
        if capacity < n:
            with pytest.raises(RuntimeError, match=f"truncated: {n} members, capacity {capacity}"):
                out.finalize()
        else:
            assert same_front(out.finalize(), want)
    none = dp.front_ensemble(v, steps_per_geometry=1, objectives=case[2], capacity=0)
    torch.cuda.synchronize()
    assert none.capacity == 0 and none.tally.tolist() == want.tally.tolist()  # (NULL lists with a capacity: test_argument_checks_launch_nothing)


@pytest.mark.parametrize("edges", [[0, 150, 300], [0, 1, 64, 299, 300], [0, 37, 37, 100, 163, 200, 257, 300]])
def test_chunks_merge_on_the_device(dp, edges):
    """Chunked runs merged with merge() - the same kernel over the runs' front rows, no host read - equal the single call, in
    this order of the chunks and in the reverse one."""
    g = 300
    found = []
    for m, levels, layout in ((2, 4, 1), (5, 0, 2), (3, 16, 3)):
        s, k, ld, _, info, _, _ = LAYOUTS[layout](m)
        case, _, _ = reference(g, m, levels, layout)
        values, status, objectives, mask = case
        want = front_host(values, status, objectives, mask)
        found.append(worth(want))
        v, st, mk = upload(values, status, mask, ld=ld, info=info)
        parts = [dp.front_ensemble(v[a * s : b * s], steps_per_geometry=s, objectives=objectives, status=None if st is None else st[a * s : b * s],
                                   mask=None if mk is None else mk[a:b], geometry_offset=a) for a, b in zip(edges[:-1], edges[1:])]
        for order in (parts, parts[::-1]):
            total = order[0]
            for part in order[1:]:
                total = total.merge(part)
            torch.cuda.synchronize()
            got = total.finalize()
            assert got.dominated is None and np.array_equal(got.tally, want.tally)
            by_id = np.argsort(got.index, kind="stable")
            assert np.array_equal(got.index[by_id], want.index) and np.array_equal(bits(got.values[by_id]), bits(want.values))
    assert_worth(found, 4)
    short = dp.front_ensemble(v[: 150 * s], steps_per_geometry=s, objectives=objectives, status=st[: 150 * s], mask=mk[:150], capacity=1)
    with pytest.raises(RuntimeError, match="truncated"):
        short.merge(parts[-1]).finalize()


def test_determinism_and_a_captured_graph(dp):
    """One linear stream capture of the three launches, replayed on NEW data in the same tensors."""
    g, m, s, k = 1500, 3, 5, 4
    values, status, objectives, mask = front_case(g, m, 16, s=s, k=k, mixed=True, with_status=True, with_mask=True)
    v, st, mk = upload(values, status, mask)
    runs = [dp.front_ensemble(v, steps_per_geometry=s, objectives=objectives, status=st, mask=mk) for _ in range(2)]
    torch.cuda.synchronize()
    want = front_host(values, status, objectives, mask)
    n = int(want.tally[2])
    assert torch.equal(runs[0].dominated, runs[1].dominated) and torch.equal(runs[0].front_index[:n], runs[1].front_index[:n])
    assert same_front(runs[0].finalize(), want) and same_front(runs[1].finalize(), want)
    out = dp.front_prepare(s, k, g, objectives)
    dp.front_ensemble(v, steps_per_geometry=s, status=st, mask=mk, out=out)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.front_ensemble(v, steps_per_geometry=s, status=st, mask=mk, out=out)
    # new data: the geometries in reverse order, with another mask
    new_values, new_status, new_mask = np.ascontiguousarray(values[::-1]), np.ascontiguousarray(status[::-1]), np.roll(mask, 1)
    v.copy_(torch.as_tensor(new_values.reshape(g * s, k), device=DEV))
    st.copy_(torch.as_tensor(new_status.reshape(-1), device=DEV))
    mk.copy_(torch.as_tensor(new_mask, device=DEV))
    for t in (out.dominated, out.tally, out.front_index):
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    again = front_host(new_values, new_status, objectives, new_mask)
    assert not np.array_equal(again.dominated, want.dominated) and same_front(out.finalize(), again)


def _c5(n_geom, steps):
    from test_gpu_ensemble_stats import _c5 as build

    return build(n_geom, steps)


def test_end_to_end_from_solved_states_to_the_front():
    """37 perturbed double-wishbone geometries x 9 bump steps, solved and evaluated; curves_ensemble -> screen_ensemble on the
    features -> front_ensemble with the screen's flags as mask and two curve features as objectives, no host read in between,
    equal curves_host -> screen_host -> front_host on the copied table.  Limits and objectives use the features that are
    exact table bits (extremes and where they occur), so that the whole chain is comparable bit for bit."""
    from open_kinematics_amd.metrics import METRIC_NAMES

    g, s = 37, 9
    dp, program, table, rel, columns = _c5(g, s)
    gpos, gparam = dp.rebind(table)
    targets = dp.ensemble_targets(gpos, rel)
    res = dp.solve_evaluated(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, output="none", chain_len=1, predictor=False)
    torch.cuda.synchronize()
    view, st = res.eval[:, 0, :], res.info_raw[:, 32]
    k = view.shape[1]
    values, status = view.cpu().numpy().reshape(g, s, k), st.cpu().numpy().reshape(g, s)
    kx, camber, steer = METRIC_NAMES.index("wheel_travel"), METRIC_NAMES.index("camber"), METRIC_NAMES.index("roadwheel_angle")
    curve_kw = dict(abscissa=kx, origin=0.0, scale=40.0, degree=2, window=(-40.0, 40.0))
    host_curves = curves_host(values, status, **curve_kw)
    features = host_curves.table()[:, None, :]
    # keep the middle of the ensemble by its largest camber; the objectives: the smallest camber span upward and a small bump steer
    entry = camber * CURVE_FIELDS + CURVE_MAX
    limits = np.full((1, k * CURVE_FIELDS, 2), (-np.inf, np.inf))
    limits[0, entry] = np.nanquantile(features[:, 0, entry], 0.15), np.nanquantile(features[:, 0, entry], 0.85)
    objectives = [(0, camber * CURVE_FIELDS + CURVE_MIN, "max"), (0, steer * CURVE_FIELDS + CURVE_MAX, "min")]
    # the device chain: three passes, each reading what the one before left in HBM
    curves = dp.curves_ensemble(view, steps_per_geometry=s, status=st, **curve_kw)
    screened = dp.screen_ensemble(curves.table(), steps_per_geometry=1, limits=limits)
    front = dp.front_ensemble(curves.table(), steps_per_geometry=1, objectives=objectives, mask=screened.flags)
    torch.cuda.synchronize()
    want_screen = screen_host(features, None, limits)
    want = front_host(features, None, objectives, want_screen.flags)
    assert np.array_equal(screened.finalize().flags, want_screen.flags) and 0 < want_screen.tally[1] < g
    assert same_front(front.finalize(), want)
    assert 1 <= want.tally[2] <= want.tally[1] < g, want.tally


def test_sharded_ensemble_on_one_gpu():
    """ShardedEnsemble(reduce=True, curves=..., screen=True, front=...) on one GPU, 64 geometries x 16 steps in one chunk and in
    two, against the host chain on the run's own copied table: both sources, with and without the screen's mask."""
    import open_kinematics_amd.dist as okd

    g, s = 64, 16
    dp, program, table, rel, columns = _c5(g, s)
    x = np.asarray(rel, dtype=np.float64)[:, -1]
    half = float(max(np.max(np.abs(x)), 1.0))
    curve_kw = dict(abscissa=x, origin=0.0, scale=half, degree=2, window=(-0.8 * half, 0.8 * half))
    variants = {"curves": dict(objectives=[(0, CURVE_MAX, "min"), (2, CURVE_MIN, "max"), (1, CURVE_X_AT_MAX, "target", 0.0)], source="curves", screened=True),
                "table": dict(objectives=[(0, 1, "max"), (s - 1, 2, "target", 0.0)], screened=False)}
    limits = None
    for name, spec in variants.items():
        answers = []
        for chunks in (1, 2):
            kw = dict(metric_columns=columns, reduce=True, chain_len=1, predictor=False, chunks=chunks, curves=curve_kw)
            if limits is None:  # the limits from the run's own table: the 10 % - 90 % band of camber at the last step
                plain = okd.ShardedEnsemble(dp, table, rel, s, **kw)
                plain.step()
                column = plain.metric_local.cpu().numpy().reshape(g, s, 4)[:, s - 1, 0]
                limits = np.full((s, 4, 2), (-np.inf, np.inf))
                limits[s - 1, 0] = np.nanquantile(column, 0.1), np.nanquantile(column, 0.9)
            pipe = okd.ShardedEnsemble(dp, table, rel, s, **kw, limits=limits, screen=True, front=spec)
            pipe.step()
            pipe.step()  # the second step overwrites the first
            torch.cuda.synchronize()
            values = pipe.metric_local.cpu().numpy().reshape(g, s, 4)
            status = pipe.info_local[:, 32].cpu().numpy().reshape(g, s)
            mask = screen_host(values, status, limits).flags if spec["screened"] else None
            if name == "curves":
                features = curves_host(values, status, **curve_kw).table()[:, None, :]
                want = front_host(features, None, [(0, c * CURVE_FIELDS + f) + tuple(rest) for c, f, *rest in spec["objectives"]], mask)
            else:
                want = front_host(values, status, spec["objectives"], mask)
            got = pipe.front()
            assert same_front(got, want, dominated=chunks == 1), (name, chunks)
            assert 1 <= want.tally[2] <= want.tally[1] <= g and pipe.front_exchange_bytes_per_rank == 0
            assert pipe.front_local().front_values.device.type == "cuda"
            answers.append(got)
        assert np.array_equal(answers[0].index, answers[1].index) and np.array_equal(bits(answers[0].values), bits(answers[1].values))


def test_argument_checks_launch_nothing(dp):
    """Every refusal of okx_ensemble_front_check and of the launch, through ctypes: OKX_ERR_INVALID with a message, and the
    tally keeps its sentinel - nothing ran.  Then the wrapper's own refusals."""
    from open_kinematics_amd import _lib

    lib = dp.lib
    g, s, k = 8, 3, 3
    values = torch.zeros((g * s, k), dtype=torch.float64, device=DEV)
    dominated = torch.full((g,), SENTINEL, dtype=torch.int32, device=DEV)
    tally = torch.full((3,), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.empty(int(lib.okx_ensemble_front_scratch_bytes(g, 8)), dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    inf, nan = float("inf"), float("nan")

    def launch(n_geom=g, entries=(1, 6, 5), sense=(0, 1, 2), target=(0.0, 0.0, 0.5), **kw):
        e, sn = np.asarray(entries, dtype=np.int32), np.asarray(sense, dtype=np.int32)
        t = None if target is None else np.asarray(target, dtype=np.float64)
        a = dict(values=ptr(values), ld=k, status_stride=0, mask_stride=0, dominated=ptr(dominated), tally=ptr(tally), capacity=0, scratch=ptr(scratch),
                 scratch_bytes=scratch.numel())
        a.update(kw)
        return lib.okx_ensemble_front(n_geom, s, k, a["values"], a["ld"], a.get("status"), a["status_stride"], e.ctypes.data_as(C.c_void_p),
                                      sn.ctypes.data_as(C.c_void_p), None if t is None else t.ctypes.data_as(C.c_void_p), len(entries), a.get("mask"),
                                      a["mask_stride"], None, 0, a["dominated"], a["tally"], None, None, a["capacity"], a["scratch"], a["scratch_bytes"],
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

    refusals = [(dict(n_geom=65537), "65537 geometries, at most 65536"), (dict(n_geom=-1), "negative geometry"),
                (dict(entries=(), sense=()), "0 objectives, 1 to 8 allowed"), (dict(entries=(0,) * 9, sense=(0,) * 9, target=None), "9 objectives, 1 to 8 allowed"),
                (dict(entries=(9,), sense=(0,)), r"entry 0 is 9, outside \[0, 9\)"), (dict(entries=(1, 6, 1)), r"entry 2 repeats entry 0 \(index 1\)"),
                (dict(sense=(0, 3, 0)), "sense 1 is 3, not 0"), (dict(target=None), "objective 2 aims at a target and no target"),
                (dict(target=(0.0, 0.0, nan)), "target 2 is nan, not finite"), (dict(target=(0.0, 0.0, -inf)), "target 2 is -inf, not finite"),
                (dict(tally=None), "null tally"), (dict(dominated=None), "null dominated"), (dict(values=None), "null table or ld < n_columns"),
                (dict(ld=2), "null table or ld < n_columns"), (dict(status=ptr(dominated), status_stride=0), "status_stride must be positive"),
                (dict(mask=ptr(dominated), mask_stride=0), "mask_stride must be positive"), (dict(capacity=-1), "negative capacity"),
                (dict(scratch=None), "bytes of scratch needed"), (dict(scratch_bytes=8 * 64 * 4 - 1), r"2048 bytes of scratch needed \(okx_ensemble_front_scratch_bytes\), 2047 given")]
    for change, message in refusals:
        assert launch(**change) == -1 and re.search(message, _lib.last_error()), (change, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((tally == SENTINEL).all()) and bool((dominated == SENTINEL).all())
    # the same call, accepted: no list (NULL pointers) with a capacity that would hold one
    assert launch(capacity=g) == 0
    torch.cuda.synchronize()
    assert tally.tolist() == [g, g, g] and bool((dominated == 0).all())  # (all rows equal: everyone is on the front)
    # no geometry: a zero tally, no scratch needed
    tally.fill_(SENTINEL)
    assert launch(n_geom=0, values=None, dominated=None, scratch=None, scratch_bytes=0) == 0
    torch.cuda.synchronize()
    assert tally.tolist() == [0, 0, 0]
    kw = dict(steps_per_geometry=s)
    with pytest.raises(ValueError, match="objectives are needed"):
        dp.front_ensemble(values, **kw)
    with pytest.raises(ValueError, match=r"entry 0 is \(step 3, column 0\)"):
        dp.front_ensemble(values, objectives=[(3, 0, "min")], **kw)
    with pytest.raises(ValueError, match="unit column stride"):
        dp.front_ensemble(values.t(), objectives=[(0, 0, "min")], **kw)
    with pytest.raises(ValueError, match="mask must be a uint8"):
        dp.front_ensemble(values, objectives=[(0, 0, "min")], mask=torch.zeros(g + 1, dtype=torch.uint8, device=DEV), **kw)
    with pytest.raises(ValueError, match="index must be a contiguous int64"):
        dp.front_ensemble(values, objectives=[(0, 0, "min")], index=torch.zeros(g, dtype=torch.int32, device=DEV), **kw)
    out = dp.front_ensemble(values, objectives=[(0, 0, "min")], **kw)
    with pytest.raises(ValueError, match="out= carries its own"):
        dp.front_ensemble(values, objectives=[(0, 0, "min")], out=out, **kw)
    with pytest.raises(ValueError, match="negative geometry count or capacity"):
        dp.front_ensemble(values, objectives=[(0, 0, "min")], capacity=-1, **kw)
    with pytest.raises(ValueError, match="65537 geometries, at most 65536"):
        dp.front_prepare(1, 1, 65537, [(0, 0, "min")])
