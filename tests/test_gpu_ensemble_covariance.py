"""
GPU: okx_ensemble_covariance (DeviceProgram.covariance_ensemble) and ShardedEnsemble(reduce=True, covariance=...) against NumPy.

EXACT tables first: integer values with |d| = |value - shift| <= 2^10 over G <= 2^12 geometries - every product (< 2^20) and
every partial sum (< 2^32) is an integer that fp64 holds, so every addition order gives the same bits and the device must
equal the int64 Gram matrix of NumPy (array_equal).  Every entry carries its own integer pattern over the geometries, so a
swapped row and column in an off-diagonal tile, a row of the matrix instruction's result written to the wrong place or a
geometry counted twice shows as a different integer.

FLOAT tables against ensemble_stats.covariance_host within the bounds derived in tests/test_ensemble_covariance.py (u = 2^-53;
nothing here comes from an outcome): each of the two results is within EG = (G + 2) u sum |d_n d_m| (E1 = G u sum |d_n|) of the
exact sum, so they are within 2 EG (2 E1) of each other; counts and used bytes are integers' work and compared exactly.

The plan the shapes are chosen from (okx_covariance.hip; tests/test_ensemble_covariance.py pins it through the scratch size):
64-entry tiles, panels of 32 geometries, slabs of at least 128 geometries, four results per lane in rows (lane >> 4) + 4 reg.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_stats import CovarianceAccumulator, covariance_host
from test_ensemble_covariance import bounds, covariance_bound, shifted
from test_ensemble_stats import load_fixture, tampered_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.0


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


def integer_case(g, s, k, seed):
    """(values, status, shift) [G, S, K] of integers with |value - shift| <= 1023, a different pattern per entry; a tenth of the
    geometries carry a NaN or a rejected status byte somewhere."""
    rng = np.random.default_rng(seed)
    e = np.arange(s * k, dtype=np.int64)[None, :]
    i = np.arange(g, dtype=np.int64)[:, None]
    d = (i * (2 * e + 3) + 7 * e * e + 13 * e + (i * i) % (e + 5)) % 2047 - 1023
    shift = ((e * 37) % 201 - 100).astype(np.float64).reshape(s, k)
    values = d.reshape(g, s, k).astype(np.float64) + shift[None]
    status = np.ones((g, s), dtype=np.uint8)
    for _ in range((g + 9) // 10 if g > 2 else 0):
        if rng.random() < 0.5:
            values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = rng.choice([np.nan, np.inf])
        else:
            status[rng.integers(0, g), rng.integers(0, s)] = rng.choice(np.array([0, 2, 3, 5], dtype=np.uint8))
    if g >= 7:
        status[rng.integers(0, g, g // 7), rng.integers(0, s, g // 7)] = 9  # (advisory bit: still accepted)
    return values, status, shift


def integer_tables(values, status, entries, shift):
    """(gram, sum, counts, used) in int64 arithmetic."""
    d, used = shifted(values, status, entries, shift)
    di = d.astype(np.int64)
    assert np.array_equal(di, d) and np.abs(di).max(initial=0) <= 1024
    return di.T @ di, di.sum(axis=0), np.array([used.sum(), used.size - used.sum()]), used.astype(np.uint8)


def equal_exactly(acc, values, status, entries, shift):
    gram, s1, counts, used = integer_tables(values, status, entries, shift)
    got = acc.numpy()
    assert np.array_equal(got.counts, counts) and np.array_equal(got.used[: used.size], used)
    bad = np.argwhere(got.gram != gram)
    assert bad.size == 0, (bad[:8].tolist(), got.gram[tuple(bad[0])], gram[tuple(bad[0])])
    assert np.array_equal(got.sum, s1)
    return counts


SHAPES = {1: (1, 1), 2: (1, 2), 15: (3, 5), 16: (4, 4), 17: (17, 1), 63: (9, 7), 64: (16, 4), 65: (13, 5), 130: (26, 5)}
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 300)  # 300: three slabs of 128 geometries, the last of 44: no multiple of the 32-geometry panel


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_exact_integer_tables(dp, n):
    """N in {1, 2, 15, 16, 17, 63, 64, 65, 130}: under, at and over one 16-wide instruction tile and one 64-entry tile, three tiles
    (six tile pairs); G from nothing over under, at and over one 4-geometry instruction step and two panels to several slabs."""
    s, k = SHAPES[n]
    for g in COUNTS:
        values, status, shift = integer_case(g, s, k, 100 * n + g)
        v, st = upload(values, status)
        acc = dp.covariance_ensemble(v, steps_per_geometry=s, status=st, shift=shift)  # entries=None: no entry list is passed
        torch.cuda.synchronize()
        assert acc.natural and tuple(acc.gram.shape) == (n, n)
        counts = equal_exactly(acc, values, status, None, shift)
        if g >= 63:
            assert 0 < counts[1] < g // 2  # the inputs are worth the test
        if g == 300:  # no status bytes: every state accepted
            equal_exactly(dp.covariance_ensemble(v, steps_per_geometry=s, shift=shift), values, None, None, shift)
    # the default shift is geometry 0 of the table (its undefined entries 0)
    values, status, shift = integer_case(65, s, k, n)
    values[0, 0, 0] = np.nan
    v, st = upload(values, status)
    acc = dp.covariance_ensemble(v, steps_per_geometry=s, status=st)
    own = np.nan_to_num(values[0], nan=0.0, posinf=0.0, neginf=0.0)
    assert np.array_equal(acc.shift.cpu().numpy(), own)


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_exact_scattered_subsets_of_strided_views(dp, n):
    """A permuted scattered subset of N entries of a wider table that lies as a strided view (ld = 3 * 24 > K, status bytes 40
    apart) in the MIDDLE of larger tensors filled with NaN and rejected bytes: a read outside the view drops a geometry."""
    s, k = 11, 24
    rng = np.random.default_rng(n)
    entries = rng.permutation(s * k)[:n].astype(np.int64)
    for g in (5, 65, 300):
        values, status, shift = integer_case(g, s, k, 7 * n + g)
        pad = 40
        big = torch.full((pad + g * s + pad, 3, 24), float("nan"), dtype=torch.float64, device=DEV)
        info = torch.full((pad + g * s + pad, 40), 2, dtype=torch.uint8, device=DEV)
        big[pad : pad + g * s, 0, :] = torch.as_tensor(values.reshape(g * s, k), device=DEV)
        info[pad : pad + g * s, 32] = torch.as_tensor(status.reshape(-1), device=DEV)
        view, st = big[pad : pad + g * s, 0, :], info[pad : pad + g * s, 32]
        assert view.stride(0) == 72 and not view.is_contiguous() and st.stride(0) == 40
        acc = dp.covariance_ensemble(view, steps_per_geometry=s, status=st, entries=entries, shift=shift)
        torch.cuda.synchronize()
        assert not acc.natural and np.array_equal(acc.entries.cpu().numpy(), entries)
        counts = equal_exactly(acc, values, status, entries, shift)
        if g == 300 and n >= 15:
            assert 0 < counts[1] < g and counts[0] > 0
        # an entry that is not selected never drops a geometry: NaN everywhere else changes nothing
        if g == 65:
            others = np.setdiff1d(np.arange(s * k), entries)
            spoiled = values.reshape(g, s * k).copy()
            spoiled[:, others] = np.nan
            big[pad : pad + g * s, 0, :] = torch.as_tensor(spoiled.reshape(g * s, k), device=DEV)
            again = dp.covariance_ensemble(view, steps_per_geometry=s, status=st, out=acc)
            torch.cuda.synchronize()
            assert again is acc
            equal_exactly(acc, values, status, entries, shift)
    # a narrower table inside the same rows (K = 5 of 24 columns), every entry of it
    narrow = big[pad : pad + g * s, 0, 3:8]
    acc = dp.covariance_ensemble(narrow, steps_per_geometry=s, status=st, shift=shift[:, 3:8])
    torch.cuda.synchronize()
    equal_exactly(acc, values[:, :, 3:8], status, None, shift[:, 3:8])


@pytest.mark.parametrize("edges", [[0, 300], [0, 149, 300], [0, 1, 2, 130, 130, 300], [0, 64, 128, 192, 256, 300]])
def test_chunks_accumulate_to_the_whole_table_bit_for_bit(dp, edges):
    s, k, g = 13, 5, 300
    values, status, shift = integer_case(g, s, k, 21)
    v, st = upload(values, status)
    for entries in (None, np.random.default_rng(3).permutation(s * k)[:17]):
        whole = dp.covariance_ensemble(v, steps_per_geometry=s, status=st, entries=entries, shift=shift)
        out = dp.covariance_ensemble(v[:0], steps_per_geometry=s, status=st[:0], entries=entries, shift=shift)
        out.used = torch.zeros(g, dtype=torch.uint8, device=DEV)
        for tensor in (out.gram, out.sum, out.counts):
            tensor.fill_(99)  # the first call overwrites
        used = []
        for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            dp.covariance_ensemble(v[a * s : b * s], steps_per_geometry=s, status=st[a * s : b * s], out=out, accumulate=i > 0)
            used.append(out.used[: b - a].clone())  # (the used bytes are those of the call)
        torch.cuda.synchronize()
        for name in ("gram", "sum", "counts"):
            assert torch.equal(getattr(out, name), getattr(whole, name)), name
        assert torch.equal(torch.cat(used), whole.used)
        equal_exactly(whole, values, status, entries, shift)


def test_the_register_tiled_form_behind_its_developer_switch(dp, monkeypatch):
    """OKX_DEV=cov_valu runs the v_fma_f64 form of the partial Gram kernel (kept to be measured against): the same integers."""
    monkeypatch.setenv("OKX_DEV", "cov_valu")
    for n, g in ((17, 65), (130, 300)):
        s, k = SHAPES[n]
        values, status, shift = integer_case(g, s, k, 100 * n + g)
        v, st = upload(values, status)
        acc = dp.covariance_ensemble(v, steps_per_geometry=s, status=st, shift=shift)
        torch.cuda.synchronize()
        equal_exactly(acc, values, status, None, shift)


def float_check(dp, values, status, entries, shift):
    v, st = upload(values, status)
    acc = dp.covariance_ensemble(v, steps_per_geometry=values.shape[1], status=st, entries=entries, shift=shift)
    again = dp.covariance_ensemble(v, steps_per_geometry=values.shape[1], status=st, entries=entries, shift=shift)
    torch.cuda.synchronize()
    got, want = acc.numpy(), covariance_host(values, status, entries, shift)
    d, used = shifted(values, status, entries, shift)
    eg, e1 = bounds(d)
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.used, want.used) and np.array_equal(got.entries, want.entries)
    gap, gap1 = np.abs(got.gram - want.gram), np.abs(got.sum - want.sum)
    print(f"N = {got.sum.size}, used {int(want.counts[0])}: gram gap / bound {float((gap / np.maximum(2 * eg, 1e-300)).max()):.3f}, "
          f"sum gap / bound {float((gap1 / np.maximum(2 * e1, 1e-300)).max()):.3f}")
    assert np.all(gap <= 2 * eg) and np.all(gap1 <= 2 * e1)
    assert np.array_equal(got.gram.view(np.uint64), got.gram.T.view(np.uint64))  # the transpose by its bits
    for a, b in ((acc.gram, again.gram), (acc.sum, again.sum), (acc.counts, again.counts), (acc.used, again.used)):
        assert torch.equal(a, b)  # two identical calls: the same bits
    if want.counts[0] > 1:
        fin, ref = acc.finalize(), want.finalize()
        assert fin.count == ref.count and fin.dropped == ref.dropped
        assert np.all(np.abs(fin.covariance - ref.covariance) <= 2 * covariance_bound(want, eg, e1))
        assert np.array_equal(np.isnan(fin.correlation), np.isnan(ref.correlation))
    return want


def test_the_fixture_and_its_tampered_form(dp):
    fx = load_fixture()
    table, shift = fx["table"], fx["stat_shift"]
    want = float_check(dp, table, None, None, shift)
    assert list(want.counts) == [64, 0]
    float_check(dp, table, None, [134, 3, 47, 62, 0, 77], shift)
    tampered, status = tampered_fixture(fx)
    none = float_check(dp, tampered, status, None, shift)  # step 4 is rejected as a whole: no geometry is complete
    assert list(none.counts) == [0, 64]
    some = float_check(dp, tampered, status, [s * 15 + k for s in (0, 2, 7) for k in (0, 3, 9, 14)], shift)
    assert 2 < some.counts[0] < 64
    # larger than one slab and one tile: normal values around per-entry centres, a few NaN and rejected states
    rng = np.random.default_rng(11)
    g, s, k = 700, 9, 15
    values = rng.normal(size=(s, k))[None] * 3.0 + rng.normal(size=(g, s, k)) * rng.uniform(0.1, 2.0, size=(s, k))[None]
    status = np.ones((g, s), dtype=np.uint8)
    for _ in range(30):
        values[rng.integers(0, g), rng.integers(0, s), rng.integers(0, k)] = np.nan
        status[rng.integers(0, g), rng.integers(0, s)] = 2
    want = float_check(dp, values, status, None, np.nan_to_num(values[3]))
    assert 600 < want.counts[0] < g


def test_a_captured_graph(dp):
    s, k, g = 13, 5, 300
    values, status, shift = integer_case(g, s, k, 8)
    v, st = upload(values, status)
    first = dp.covariance_ensemble(v, steps_per_geometry=s, status=st, shift=shift)
    out = dp.covariance_ensemble(v, steps_per_geometry=s, status=st, shift=shift)  # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.covariance_ensemble(v, steps_per_geometry=s, status=st, out=out)
    tensors = lambda r: (r.gram, r.sum, r.counts, r.used)  # noqa: E731
    for t in tensors(out):
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(tensors(out), tensors(first)):
        assert torch.equal(a, b)
    equal_exactly(out, values, status, None, shift)


def test_error_paths(dp):
    s, k, g = 9, 15, 64
    fx = load_fixture()
    v, _ = upload(fx["table"], None)
    shift = fx["stat_shift"]
    with pytest.raises(ValueError, match=r"entry 1 repeats entry 0 \(index 4\)"):
        dp.covariance_ensemble(v, steps_per_geometry=s, entries=[4, 4])
    with pytest.raises(ValueError, match=r"entry 0 is 135, outside \[0, 135\)"):
        dp.covariance_ensemble(v, steps_per_geometry=s, entries=[135])
    with pytest.raises(ValueError, match="0 entries selected, 1 to 2048 allowed"):
        dp.covariance_ensemble(v, steps_per_geometry=s, entries=[])
    wide = torch.zeros((2, 2049), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="2049 entries selected, 1 to 2048 allowed"):
        dp.covariance_ensemble(wide, steps_per_geometry=1)
    with pytest.raises(ValueError, match="unit column stride"):
        dp.covariance_ensemble(v.t(), steps_per_geometry=s)
    with pytest.raises(ValueError, match="bad steps_per_geometry"):
        dp.covariance_ensemble(v, steps_per_geometry=7)
    with pytest.raises(ValueError, match="status must be a uint8"):
        dp.covariance_ensemble(v, steps_per_geometry=s, status=torch.ones(5, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="accumulate=True needs the accumulator"):
        dp.covariance_ensemble(v, steps_per_geometry=s, accumulate=True)
    out = dp.covariance_ensemble(v, steps_per_geometry=s, entries=[1, 2, 3], shift=shift)
    with pytest.raises(ValueError, match="out= carries its own shift and entries"):
        dp.covariance_ensemble(v, steps_per_geometry=s, out=out, shift=shift)
    with pytest.raises(ValueError, match="out= carries its own shift and entries"):
        dp.covariance_ensemble(v, steps_per_geometry=s, out=out, entries=[1, 2, 3])
    with pytest.raises(ValueError, match="out must hold contiguous device tables"):
        dp.covariance_ensemble(v[:, :5], steps_per_geometry=s, out=out)
    host = covariance_host(fx["table"], None, [1, 2, 3], shift)
    with pytest.raises(ValueError, match="out must hold contiguous device tables"):
        dp.covariance_ensemble(v, steps_per_geometry=s, out=host)
    torch.cuda.synchronize()
    assert np.array_equal(out.numpy().counts, [g, 0])  # nothing was touched by the refused calls


def _c5(n_geom, steps):
    from test_gpu_ensemble_stats import _c5 as build

    return build(n_geom, steps)


def _sharded_reference(g, s):
    import open_kinematics_amd.dist as okd

    dp, program, table, rel, columns = _c5(g, s)
    plain = okd.ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, chain_len=1, predictor=False)
    plain.step()
    torch.cuda.synchronize()
    return dp, table, rel, columns, plain


def test_sharded_ensemble_on_one_gpu():
    """64 geometries x 16 steps of the double wishbone, solved and evaluated: with one chunk the covariance accumulator is the bits
    of covariance_ensemble over the same run's metric_local, with two it is within the bound; the reduction is what it is without."""
    import open_kinematics_amd.dist as okd

    g, s = 64, 16
    dp, table, rel, columns, plain = _sharded_reference(g, s)
    values, status, shift = plain.metric_local, plain.info_local[:, 32], plain.local_accumulator.shift
    entries = [s * 4 - 1, 0, 5, 18, 33]
    kw = dict(metric_columns=columns, reduce=True, chain_len=1, predictor=False)
    host_v, host_st = values.cpu().numpy().reshape(g, s, 4), status.cpu().numpy().reshape(g, s)
    for which in (True, entries):
        want = dp.covariance_ensemble(values, steps_per_geometry=s, status=status, shift=shift, entries=None if which is True else which)
        d, used = shifted(host_v, host_st, None if which is True else which, shift.cpu().numpy())
        eg, e1 = bounds(d)
        assert used.sum() > 2
        for chunks in (1, 2):
            pipe = okd.ShardedEnsemble(dp, table, rel, s, chunks=chunks, covariance=which, **kw)
            for _ in range(2):  # the second step overwrites the first
                acc = pipe.step()
                torch.cuda.synchronize()
                got = pipe.covariance_accumulator
                assert torch.equal(got.counts, want.counts) and torch.equal(pipe.covariance_local_used, want.used)
                if chunks == 1:
                    assert torch.equal(got.gram, want.gram) and torch.equal(got.sum, want.sum)
                else:
                    assert np.all(np.abs((got.gram - want.gram).cpu().numpy()) <= 2 * eg) and np.all(np.abs((got.sum - want.sum).cpu().numpy()) <= 2 * e1)
                assert torch.equal(acc.acc, plain.accumulator.acc)
                fin = pipe.covariance()
                assert fin.count == int(want.counts[0]) and np.array_equal(fin.covariance, fin.covariance.T)
            assert pipe.covariance_exchange_bytes_per_rank == 0


def test_two_ranks_rehearsed_on_one_gpu(tmp_path):
    """Two ranks at 256 x 16 in two chunks on cuda:0 over gloo in fresh child processes, each under its own time limit: both ranks
    hold the same bits, those of the one-GPU merge of the same chunks in the same order."""
    g, s, chunks, world = 256, 16, 2, 2
    dp, table, rel, columns, plain = _sharded_reference(g, s)
    values, status, shift = plain.metric_local, plain.info_local[:, 32], plain.local_accumulator.shift
    entries = [63, 0, 5, 18, 33, 34, 35, 60, 2]
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_covariance_rate.py"), "--rehearse", str(world), "--geometries", str(g),
                           "--steps-per-geometry", str(s), "--chunks", str(chunks), "--entries", ",".join(map(str, entries)), "--out", str(tmp_path),
                           "--timeout", "240"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    for key in ("gram", "sum", "counts", "entries", "shift"):
        assert torch.equal(got[0][key], got[1][key]), key
    assert np.array_equal(got[0]["covariance"], got[1]["covariance"], equal_nan=True)
    assert torch.equal(got[0]["shift"], shift.cpu())
    # the one-GPU merge: every rank's chunks accumulated in order, the ranks' tables added in rank order
    merged = None
    for r in range(world):
        part = None
        for piece in got[0]["pieces"]:
            a, b = piece[r]
            if b <= a:
                continue
            if part is None:
                part = dp.covariance_ensemble(values[a * s : b * s], steps_per_geometry=s, status=status[a * s : b * s], entries=entries, shift=shift)
            else:
                dp.covariance_ensemble(values[a * s : b * s], steps_per_geometry=s, status=status[a * s : b * s], out=part, accumulate=True)
        part = CovarianceAccumulator(part.gram, part.sum, part.counts, part.shift, part.entries)
        merged = part if merged is None else merged.merge(part)
    torch.cuda.synchronize()
    assert torch.equal(merged.gram.cpu(), got[0]["gram"]) and torch.equal(merged.sum.cpu(), got[0]["sum"]) and torch.equal(merged.counts.cpu(), got[0]["counts"])
    whole = dp.covariance_ensemble(values, steps_per_geometry=s, status=status, entries=entries, shift=shift)
    assert torch.equal(whole.counts.cpu(), got[0]["counts"]) and int(whole.counts[0]) > 2
    for r in range(world):
        lo, hi = got[r]["range"]
        assert torch.equal(got[r]["used"], whole.used[lo:hi].cpu()) and got[r]["sent"] == 8 * (9 * 9 + 9 + 2)
