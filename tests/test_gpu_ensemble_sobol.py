"""
GPU: okx_ensemble_sample_families (DeviceProgram.sample_families), okx_ensemble_sobol (DeviceProgram.sobol_ensemble) and
ShardedEnsemble(reduce=True, sobol=True) against the NumPy definitions ensemble_sample.families_host and ensemble_stats.sobol_host.

The draw is compared by EQUAL BITS in all four outputs.  The estimator is compared exactly on the integer tables of
tests/test_ensemble_sobol.py (|value - shift| <= 8: every difference, product and partial sum is an integer fp64 holds, so every
addition order - slabs included - gives the same bits) and, on real tables, within 2 (n + 1) U sum |term| of sobol_host, the
bound computed from the host's own terms (``term_bound``; the terms are bit-identical, contraction is off in the unit): nothing
here comes from an outcome.

The plan the shapes are chosen from (okx_sobol.hip): a lane owns one of 64 entries of a tile, group tiles of 4, 8, 12 or 16 (D = 1,
3 and 40: one tile of 4 and three tiles of 16, the last with 8 groups), slabs of at least 32 families (N = 1000: 32 slabs).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available
from open_kinematics_amd.ensemble_sample import IID, LHS, families_host
from open_kinematics_amd.ensemble_stats import SOBOL_COUNT, SOBOL_DROPPED, SOBOL_FIELDS, SobolAccumulator, sobol_host
from test_ensemble_sobol import bits, check_exact_zeros, family_plan, integer_table, term_bound

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


# ---- the draw ----

def device_families(dp, fp, lo=0, hi=None, **kw):
    run = dp.sample_families(fp, lo, hi, latents=True, delta=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (run.hardpoints, run.latents, run.delta, run.flags)]


def same(got, want) -> bool:
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3]) \
        and all(np.asarray(g).shape == np.asarray(w).shape for g, w in zip(got, want))


@pytest.mark.parametrize("stratify", [IID, LHS])
@pytest.mark.parametrize("z,mixing", [(1, False), (6, False), (6, True), (65, False), (65, True)])
def test_draw_equals_the_definition(dp, stratify, z, mixing):
    """Z = 65: a second round of the 64 lanes over the latents (and, without mixing, over the coordinates)."""
    for n in (1, 5):
        fp = family_plan(z, n, stratify=stratify, mixing=mixing)
        want = families_host(fp)
        total = fp.n_total
        if n == 5:
            assert 0 < want[3].sum() < total  # the guard fails for some rows
        assert same(device_families(dp, fp), want)
        cut = min(total - 1, fp.family_size + 1)  # no multiple of the family size (one family: inside it)
        for lo, hi in ((0, cut), (cut, total)):
            assert same(device_families(dp, fp, lo, hi), [t[lo:hi] for t in want])
    assert dp.sample_families(fp, 3, 3).hardpoints.shape == (0, fp.n_points, 3)


# ---- the estimator, exact ----

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


EXACT = [(n, d, s, k) for n in (1, 2, 67) for d in (1, 3) for s, k in ((1, 1), (3, 5))] + [(1000, 3, 3, 5), (2, 40, 1, 1), (67, 40, 3, 5), (1000, 40, 1, 5)]


@pytest.mark.parametrize("n,d,s,k", EXACT)
def test_exact_integer_tables(dp, n, d, s, k):
    m = d + 2
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(n, d, s, k, 1000 * n + 10 * d + s, with_mask)
        want = sobol_host(values, status, mask, d, shift).acc
        v, st, mk = upload(values, status, mask)
        assert v.stride(0) == k + 3 and st.stride(0) == 40
        acc = dp.sobol_ensemble(v, steps_per_geometry=s, n_groups=d, status=st, mask=mk, shift=shift)
        torch.cuda.synchronize()
        got = acc.numpy().acc
        bad = np.argwhere(got != want)
        assert bad.size == 0, (bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        assert np.all(got[..., SOBOL_COUNT] + got[..., SOBOL_DROPPED] == n)
        if n >= 67:
            assert 0 < got[..., SOBOL_DROPPED].max() < n  # the inputs are worth the test
        # two chunks of whole families, the second accumulated onto the first: bit-equal to the whole
        cut = (n // 2) * m * s
        out = SobolAccumulator(torch.full_like(acc.acc, -7.0), acc.shift)
        dp.sobol_ensemble(v[:cut], steps_per_geometry=s, n_groups=d, status=st[:cut], mask=None if mk is None else mk[: cut // s], out=out)
        dp.sobol_ensemble(v[cut:], steps_per_geometry=s, n_groups=d, status=st[cut:], mask=None if mk is None else mk[cut // s :], out=out, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(out.numpy().acc, want)
    # no status bytes: every state accepted
    plain = dp.sobol_ensemble(v, steps_per_geometry=s, n_groups=d, shift=shift)
    torch.cuda.synchronize()
    assert np.array_equal(plain.numpy().acc, sobol_host(values, None, None, d, shift).acc)


def test_no_family_leaves_zeros_or_what_was_there(dp):
    s, k, d = 3, 5, 3
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    empty = torch.empty((0, k), dtype=torch.float64, device=DEV)
    acc = dp.sobol_ensemble(empty, steps_per_geometry=s, n_groups=d, shift=shift)
    torch.cuda.synchronize()
    assert tuple(acc.acc.shape) == (s, k, SOBOL_FIELDS + 3 * d) and not acc.acc.any()
    acc.acc.fill_(5.0)
    dp.sobol_ensemble(empty, steps_per_geometry=s, n_groups=d, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert bool((acc.acc == 5.0).all())


# ---- the estimator, real data ----

def test_real_table_within_the_summation_bound(dp):
    n, d, s, k = 1000, 3, 3, 5
    rng = np.random.default_rng(5)
    shift = rng.normal(0.0, 3.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (n * (d + 2), s, k)) * np.logspace(-3, 3, k)[None, None]
    _, status, mask, _ = integer_table(n, d, s, k, 77)
    want = sobol_host(values, status, mask, d, shift).acc
    bound = term_bound(values, status, mask, d, shift)
    v, st, mk = upload(values, status, mask)
    acc = dp.sobol_ensemble(v, steps_per_geometry=s, n_groups=d, status=st, mask=mk, shift=shift)
    torch.cuda.synchronize()
    got = acc.numpy().acc
    print("largest |device - host| / bound:", float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0))))
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got[..., :2], want[..., :2])
    again = dp.sobol_ensemble(v, steps_per_geometry=s, n_groups=d, status=st, mask=mk, shift=shift)
    torch.cuda.synchronize()
    assert torch.equal(again.acc.view(torch.int64), acc.acc.view(torch.int64))  # bit for bit, run to run
    out = acc.finalize()
    assert out.first.shape == (s, k, d) and np.all(np.isfinite(out.total))


# ---- the chain ----

STEPS = 3


def chain(n_families=8):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_sobol_rate import build

    return build(n_families, STEPS, DEV, n_points=2)


@pytest.mark.parametrize("chunks", [1, 2])
def test_the_chain_on_two_points(chunks):
    """hardpoint_plan on two points of data/geometry.yaml grouped by point (Z = 6, D = 2, M = 4), 8 families, 3 bump steps."""
    import open_kinematics_amd.dist as okd

    device_program, fp, rel, columns = chain()
    assert (fp.n_latents, fp.n_groups, fp.family_size, fp.n_total) == (6, 2, 4, 32)
    pipe = okd.ShardedEnsemble(device_program, fp, rel, STEPS, metric_columns=columns, reduce=True, sobol=True, chunks=chunks, chain_len=1, predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    assert all(a % 4 == 0 and b % 4 == 0 for row in pipe.pieces for a, b in row) and len(pipe.pieces) == chunks
    k = len(columns)
    values = pipe.metric_local.cpu().numpy().reshape(32, STEPS, k)
    status = pipe.info_local[:, 32].cpu().numpy().reshape(32, STEPS)
    flags = pipe.sampled_flags.cpu().numpy()
    assert np.array_equal(flags, families_host(fp)[3])
    shift = pipe.sobol_accumulator.shift.cpu().numpy()
    want = sobol_host(values, status, flags, 2, shift).acc
    bound = term_bound(values, status, flags, 2, shift)
    got = pipe.sobol_accumulator.numpy().acc
    assert np.all(np.abs(got - want) <= bound) and np.array_equal(got[..., :2], want[..., :2])
    out = pipe.sobol()
    assert np.all(out.count + out.dropped == 8) and out.count.max() == 8 and out.first.shape == (STEPS, k, 2)
    assert out.group_names == list(fp.names()) and len(set(out.group_names)) == 2
    # the exact zeros, with the drawn latents as the table
    lat = device_program.sample_families(fp, latents=True).latents
    zeros = device_program.sobol_ensemble(lat, steps_per_geometry=1, n_groups=2)
    torch.cuda.synchronize()
    check_exact_zeros(zeros.numpy().acc[0], fp.group)


def test_a_captured_graph_replays(dp):
    fp = family_plan(6, 40, stratify=LHS, guard=True)
    d, z = fp.n_groups, fp.n_latents
    run = dp.sample_families(fp, latents=True)   # (warm: the plan's tables are on the device, the scratch buffer exists)
    shift = torch.zeros((1, z), dtype=torch.float64, device=DEV)
    acc = dp.sobol_ensemble(run.latents, steps_per_geometry=1, n_groups=d, mask=run.flags, shift=shift)
    torch.cuda.synchronize()
    first = acc.acc.clone()
    want = families_host(fp)
    host = sobol_host(want[1][:, None, :], None, want[3], d, np.zeros((1, z))).acc
    assert np.all(np.abs(first.cpu().numpy() - host) <= term_bound(want[1][:, None, :], None, want[3], d, np.zeros((1, z)))) and host[..., SOBOL_COUNT].max() > 0
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.sample_families(fp, out=run)
        dp.sobol_ensemble(run.latents, steps_per_geometry=1, n_groups=d, mask=run.flags, out=acc)
    run.latents.fill_(3.0)
    run.flags.fill_(255)
    acc.acc.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.acc.view(torch.int64), first.view(torch.int64)) and np.array_equal(bits(run.latents.cpu().numpy()), bits(want[1]))
    assert np.array_equal(run.flags.cpu().numpy(), want[3])


def test_error_paths_launch_nothing(dp):
    import ctypes as C

    from open_kinematics_amd import _lib

    lib = dp.lib
    s, k, d, n = 2, 3, 2, 4
    table = torch.zeros((n * (d + 2) * s, k), dtype=torch.float64, device=DEV)
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    acc = torch.full((s, k, SOBOL_FIELDS + 3 * d), -3.0, dtype=torch.float64, device=DEV)
    need = int(lib.okx_ensemble_sobol_scratch_bytes(n, d, s, k))
    assert need == 8 * 1 * (SOBOL_FIELDS + 3 * d) * s * k
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(n_families=n, n_groups=d, steps=s, columns=k, values=table, ld=k, out=acc, room=need):
        return lib.okx_ensemble_sobol(n_families, n_groups, steps, columns, C.c_void_p(values.data_ptr() if values is not None else 0), ld, None, 0, None,
                                      C.c_void_p(shift.data_ptr()), 0, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), room, None)

    for kw, words in ((dict(n_families=-1), "negative geometry, step or column count"), (dict(ld=k - 1), "null table or ld < n_columns"),
                      (dict(values=None), "null table or ld < n_columns"), (dict(n_groups=0), "0 groups, 1 to 288 allowed"),
                      (dict(n_groups=289), "289 groups, 1 to 288 allowed"), (dict(room=need - 1), "(okx_ensemble_sobol_scratch_bytes)"),
                      (dict(steps=1 << 31), "too many entries for one call")):
        assert call(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_sobol" in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((acc == -3.0).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((acc[..., SOBOL_COUNT] == n).all())
    # the Python layer
    with pytest.raises(ValueError, match="no whole families of 4"):
        dp.sobol_ensemble(table[: 7 * s], steps_per_geometry=s, n_groups=d)
    with pytest.raises(ValueError, match="accumulate=True needs"):
        dp.sobol_ensemble(table, steps_per_geometry=s, n_groups=d, accumulate=True)
    with pytest.raises(ValueError, match="out= carries its own shift"):
        dp.sobol_ensemble(table, steps_per_geometry=s, n_groups=d, shift=shift, out=SobolAccumulator(acc, shift))
    with pytest.raises(ValueError, match="mask must be"):
        dp.sobol_ensemble(table, steps_per_geometry=s, n_groups=d, mask=torch.zeros(3, dtype=torch.uint8, device=DEV))
    fp = family_plan(6, 4, stratify=LHS)
    with pytest.raises(ValueError, match=r"geometries \[0, 21\) lie outside the 4 families of 5"):
        dp.sample_families(fp, 0, 21)
    with pytest.raises(ValueError, match="bad range"):
        dp.sample_families(fp, 5, 4)
    # the host-only check, in the library's words
    base = fp.plan
    guards = dp._sample_tables(base)["guards"]
    group = np.asarray([0, 0, 2, 2, 2, -1], dtype=np.int32)

    def check(group=fp.group, n_groups=3, max_attempts=1):
        return lib.okx_ensemble_sample_families_check(0, 0, 4, base.n_points, base.coords.ctypes.data_as(C.c_void_p), base.n_coords,
                                                      base.kind.ctypes.data_as(C.c_void_p), base.bound.ctypes.data_as(C.c_void_p), base.n_latents, 0,
                                                      group.ctypes.data_as(C.c_void_p), n_groups, guards, len(base.guards), base.stratify, max_attempts)

    assert check() == 0
    for kw, words in ((dict(group=group), "group 1 has no latent"), (dict(max_attempts=2), "max_attempts is 2; a family is drawn once"),
                      (dict(n_groups=289), "289 groups, 1 to 288 allowed"), (dict(n_groups=2), "group 2 is 2, outside [-1, 2)")):
        assert check(**kw) != 0 and words in _lib.last_error(), (kw, _lib.last_error())


# ---- two ranks rehearsed on one GPU ----

def test_two_ranks_rehearsed_on_one_gpu(tmp_path):
    """Both ranks on cuda:0, gloo in place of RCCL (fresh child processes): 8 families of 4 shard 4 + 4, two chunks each.  The same
    accumulator bits on both ranks; on the integer table they equal the one-process answer exactly."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from ensemble_sobol_rate import integer_rows

    n, world = 8, 2
    proc = subprocess.run([sys.executable, os.path.join(REPO, "tools", "ensemble_sobol_rate.py"), "--rehearse", str(world), "--families", str(n),
                           "--steps-per-geometry", str(STEPS), "--points", "2", "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]
    assert [g["range"] for g in got] == [(0, 16), (16, 32)] and got[0]["pieces"] == [[(0, 8), (16, 24)], [(8, 16), (24, 32)]]
    k, d = 4, 2
    assert got[0]["sent"] == got[1]["sent"] == 8 * STEPS * k * (SOBOL_FIELDS + 3 * d)
    for key in ("acc", "integer_acc"):
        assert torch.equal(got[0][key].view(torch.int64), got[1][key].view(torch.int64)), key
    values, status = integer_rows(0, 32 * STEPS, k)
    flags = torch.cat([g["flags"] for g in got]).numpy()
    want = sobol_host(values.reshape(32, STEPS, k), status.reshape(32, STEPS), flags, d, np.zeros((STEPS, k))).acc
    assert np.array_equal(got[0]["integer_acc"].numpy(), want) and 0 < want[..., SOBOL_DROPPED].max() < n
    device_program, fp, rel, columns = chain(n)
    import open_kinematics_amd.dist as okd

    pipe = okd.ShardedEnsemble(device_program, fp, rel, STEPS, metric_columns=columns, reduce=True, sobol=True, shift=np.zeros((STEPS, k)), chain_len=1,
                               predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    alone = pipe.sobol_accumulator.numpy().acc
    bound = term_bound(pipe.metric_local.cpu().numpy().reshape(32, STEPS, k), pipe.info_local[:, 32].cpu().numpy().reshape(32, STEPS), flags, d,
                       np.zeros((STEPS, k)))
    assert np.all(np.abs(got[0]["acc"].numpy() - alone) <= bound) and np.array_equal(got[0]["acc"].numpy()[..., :2], alone[..., :2])
