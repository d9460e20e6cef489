"""
GPU: okx_ensemble_bootstrap_weights (DeviceProgram.bootstrap_weights), okx_ensemble_sobol_bootstrap (DeviceProgram.sobol_bootstrap_ensemble)
and ShardedEnsemble(reduce=True, sobol=True, bootstrap=R) against the NumPy definitions ensemble_stats.bootstrap_weights and
ensemble_stats.sobol_bootstrap_host.

The weights are compared byte for byte.  The replicate accumulators are compared exactly on the integer tables of
tests/test_ensemble_sobol.py (|value - shift| <= 8 and w <= 13: every term, every product w * term and every partial sum is an
integer fp64 holds, so every addition order - slabs included - gives the same bits) and, on real tables, exactly in COUNT_r and
DROPPED_r and within ``weighted_bound`` of sobol_bootstrap_host in the other fields: 2 (n + 1) U sum |w term| over the host's own
weighted terms (tests/test_ensemble_bootstrap.py; the products are bit-identical, contraction is off in the unit).  Nothing here
comes from an outcome.

The plan the shapes are chosen from (okx_bootstrap.hip): a lane owns one of 64 entries of a tile; group tiles of GT = 4 (D = 1, 3: one
tile, partial; D = 40: ten tiles) beside the common fields' tile; replicate tiles of RT = 8 (R = 1, 8, 9, 19: a partial tile, one
full tile, one full and one of 1, two full and one of 3); slabs of at least 32 families, as many as 2048 workgroups over all tiles
ask for (N = 1000 gives 32 slabs at every shape below: at most 33 tiles per slab, S K <= 64).
"""

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd.ensemble_stats import (SOBOL_COUNT, SOBOL_DROPPED, SOBOL_FIELDS, SobolBootstrapAccumulator, bootstrap_weights, sobol_bootstrap_host)
from test_ensemble_bootstrap import weighted_bound
from test_ensemble_sobol import bits, family_plan, integer_table
from test_gpu_ensemble_sobol import chain, upload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RT = 8


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


# ---- the weights ----

@pytest.mark.parametrize("offset", [0, 2 ** 32 + 3])
def test_weights_equal_the_definition(dp, offset):
    for n in (0, 1, 67, 1000):
        for r in (1, 4, 5, 67):
            got = dp.bootstrap_weights(n, r, 21, row_offset=offset)
            torch.cuda.synchronize()
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, r)
            assert np.array_equal(got.cpu().numpy(), bootstrap_weights(21, offset, offset + n, r)), (n, r)
    # out=: the bytes around the table stay what they were
    wide = torch.full((69, 5), 255, dtype=torch.uint8, device=DEV)
    dp.bootstrap_weights(67, 5, 2 ** 40 + 21, row_offset=offset, out=wide[1:68])
    torch.cuda.synchronize()
    assert np.array_equal(wide[1:68].cpu().numpy(), bootstrap_weights(2 ** 40 + 21, offset, offset + 67, 5)) and bool((wide[0] == 255).all() and (wide[68] == 255).all())


# ---- the replicate accumulators, exact ----

EXACT = [(n, d, s, k) for n in (1, 2, 67) for d in (1, 3) for s, k in ((1, 1), (3, 5))] + [(1000, 1, 1, 1), (1000, 3, 3, 5), (1, 40, 3, 5), (2, 40, 1, 1),
                                                                                             (67, 40, 3, 5), (1000, 40, 1, 1)]
REPLICATES = (1, RT, RT + 1, 2 * RT + 3)


@pytest.mark.parametrize("n,d,s,k", EXACT)
def test_exact_integer_tables(dp, n, d, s, k):
    m = d + 2
    offset = 2 ** 32 + 5
    for with_mask in (False, True):
        values, status, mask, shift = integer_table(n, d, s, k, 1000 * n + 10 * d + s, with_mask)
        v, st, mk = upload(values, status, mask)
        assert v.stride(0) == k + 3 and st.stride(0) == 40
        for r in REPLICATES:
            want = sobol_bootstrap_host(values, status, mask, d, shift, seed=9, n_replicates=r, family_offset=offset).acc
            acc = dp.sobol_bootstrap_ensemble(v, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=9, family_offset=offset, status=st, mask=mk, shift=shift)
            torch.cuda.synchronize()
            got = acc.numpy().acc
            bad = np.argwhere(got != want)
            assert got.shape == (r, s, k, SOBOL_FIELDS + 3 * d) and bad.size == 0, (r, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            weights = bootstrap_weights(9, offset, offset + n, r)
            assert np.array_equal(got[..., SOBOL_COUNT] + got[..., SOBOL_DROPPED], np.broadcast_to(weights.sum(axis=0)[:, None, None], (r, s, k)))
            if n >= 67:
                assert 0 < got[..., SOBOL_DROPPED].max()  # the inputs are worth the test
        # two chunks of whole families, the second accumulated onto the first with its family_offset: bit-equal to the whole
        r = REPLICATES[-1]
        cut = (n // 2) * m * s
        out = SobolBootstrapAccumulator(torch.full_like(acc.acc, -7.0), acc.shift, 9)
        kw = dict(steps_per_geometry=s, n_groups=d, n_replicates=r, seed=9, out=out)
        dp.sobol_bootstrap_ensemble(v[:cut], family_offset=offset, status=st[:cut], mask=None if mk is None else mk[: cut // s], **kw)
        dp.sobol_bootstrap_ensemble(v[cut:], family_offset=offset + n // 2, status=st[cut:], mask=None if mk is None else mk[cut // s :], accumulate=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(out.numpy().acc, want)
    # no status bytes: every state accepted
    plain = dp.sobol_bootstrap_ensemble(v, steps_per_geometry=s, n_groups=d, n_replicates=RT + 1, seed=9, shift=shift)
    torch.cuda.synchronize()
    assert np.array_equal(plain.numpy().acc, sobol_bootstrap_host(values, None, None, d, shift, seed=9, n_replicates=RT + 1).acc)


def test_no_family_leaves_zeros_or_what_was_there(dp):
    s, k, d, r = 3, 5, 3, 9
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    empty = torch.empty((0, k), dtype=torch.float64, device=DEV)
    acc = dp.sobol_bootstrap_ensemble(empty, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, shift=shift)
    torch.cuda.synchronize()
    assert tuple(acc.acc.shape) == (r, s, k, SOBOL_FIELDS + 3 * d) and not acc.acc.any()
    acc.acc.fill_(5.0)
    dp.sobol_bootstrap_ensemble(empty, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert bool((acc.acc == 5.0).all())


# ---- the replicate accumulators, real data ----

def test_real_table_within_the_summation_bound(dp):
    n, d, s, k, r = 1000, 3, 3, 5, 2 * RT + 3
    rng = np.random.default_rng(5)
    shift = rng.normal(0.0, 3.0, (s, k))
    values = shift[None] + rng.normal(0.0, 1.0, (n * (d + 2), s, k)) * np.logspace(-3, 3, k)[None, None]
    _, status, mask, _ = integer_table(n, d, s, k, 77)
    want = sobol_bootstrap_host(values, status, mask, d, shift, seed=4, n_replicates=r, family_offset=11).acc
    bound = weighted_bound(values, status, mask, d, shift, bootstrap_weights(4, 11, 11 + n, r))
    v, st, mk = upload(values, status, mask)
    kw = dict(steps_per_geometry=s, n_groups=d, n_replicates=r, seed=4, family_offset=11, status=st, mask=mk, shift=shift)
    acc = dp.sobol_bootstrap_ensemble(v, **kw)
    torch.cuda.synchronize()
    got = acc.numpy().acc
    print("largest |device - host| / bound:", float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0))))
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got[..., :2], want[..., :2]) and 0 < got[..., SOBOL_DROPPED].max()
    again = dp.sobol_bootstrap_ensemble(v, **kw)
    torch.cuda.synchronize()
    assert torch.equal(again.acc.view(torch.int64), acc.acc.view(torch.int64))  # bit for bit, run to run
    out = acc.finalize()
    assert out.first.shape == (r, s, k, d) and np.all(np.isfinite(out.total_std)) and np.all(out.defined == r)
    # the plain pass over the same table is untouched by its neighbour's scratch and results
    plain = dp.sobol_ensemble(v, steps_per_geometry=s, n_groups=d, status=st, mask=mk, shift=shift)
    torch.cuda.synchronize()
    from open_kinematics_amd.ensemble_stats import sobol_host
    from test_ensemble_sobol import term_bound

    assert np.all(np.abs(plain.numpy().acc - sobol_host(values, status, mask, d, shift).acc) <= term_bound(values, status, mask, d, shift))


# ---- the chain ----

STEPS = 3


def test_the_sharded_stage_on_two_points():
    """hardpoint_plan on two points of data/geometry.yaml (Z = 6, D = 2, M = 4), 8 families, 3 bump steps, two chunks, bootstrap=5."""
    import open_kinematics_amd.dist as okd

    device_program, fp, rel, columns = chain()
    kw = dict(metric_columns=columns, reduce=True, sobol=True, chunks=2, chain_len=1, predictor=False)
    pipe = okd.ShardedEnsemble(device_program, fp, rel, STEPS, bootstrap=5, **kw)
    pipe.step()
    torch.cuda.synchronize()
    assert len(pipe.pieces) == 2 and pipe.sobol_bootstrap_exchange_bytes_per_rank == 0
    k, r = len(columns), 5
    boot = pipe.sobol_bootstrap_accumulator
    assert boot.seed == fp.plan.seed and tuple(boot.acc.shape) == (r, STEPS, k, SOBOL_FIELDS + 6)
    # one call over the rank's whole table
    one = device_program.sobol_bootstrap_ensemble(pipe.metric_local, steps_per_geometry=STEPS, n_groups=2, n_replicates=r, seed=fp.plan.seed,
                                                  status=pipe.info_local[:, 32], mask=pipe.sampled_flags, shift=boot.shift)
    torch.cuda.synchronize()
    values = pipe.metric_local.cpu().numpy().reshape(32, STEPS, k)
    status = pipe.info_local[:, 32].cpu().numpy().reshape(32, STEPS)
    flags = pipe.sampled_flags.cpu().numpy()
    shift = boot.shift.cpu().numpy()
    weights = bootstrap_weights(fp.plan.seed, 0, 8, r)
    bound = weighted_bound(values, status, flags, 2, shift, weights)
    got, whole = boot.numpy().acc, one.numpy().acc
    assert np.array_equal(got[..., :2], whole[..., :2]) and np.all(np.abs(got - whole) <= bound)
    want = sobol_bootstrap_host(values, status, flags, 2, shift, seed=fp.plan.seed, n_replicates=r).acc
    assert np.array_equal(got[..., :2], want[..., :2]) and np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got[..., SOBOL_COUNT] + got[..., SOBOL_DROPPED], np.broadcast_to(weights.sum(axis=0)[:, None, None], (r, STEPS, k)))
    out = pipe.sobol_bootstrap()
    assert out.first.shape == (r, STEPS, k, 2) and out.group_names == list(fp.names())
    # sobol() is what it is without the bootstrap, bit for bit
    plain = okd.ShardedEnsemble(device_program, fp, rel, STEPS, **kw)
    plain.step()
    torch.cuda.synchronize()
    assert torch.equal(plain.sobol_accumulator.acc.view(torch.int64), pipe.sobol_accumulator.acc.view(torch.int64))
    a, b = plain.sobol(), pipe.sobol()
    assert all(np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))) for name in ("first", "first_jansen", "total", "mean", "variance"))


def test_a_captured_graph_replays(dp):
    import gc

    # (a ShardedEnsemble and its stages refer to each other, so the one of the test above - and the device program it holds - waits
    #  for the cycle collector; were that to run inside the capture, the program's release would free device memory, which no
    #  capture survives.  Likewise the program's compile job, which loads code objects when it finishes.)
    gc.collect()
    dp.wait_ready()
    fp = family_plan(6, 40, stratify=1, guard=True)
    d, z, r = fp.n_groups, fp.n_latents, RT + 1
    run = dp.sample_families(fp, latents=True)   # (warm: the plan's tables are on the device)
    shift = torch.zeros((1, z), dtype=torch.float64, device=DEV)
    kw = dict(steps_per_geometry=1, n_groups=d, n_replicates=r, seed=3, mask=run.flags)
    acc = dp.sobol_bootstrap_ensemble(run.latents, shift=shift, **kw)   # (warm: the scratch buffer exists)
    weights = dp.bootstrap_weights(40, r, 3)
    torch.cuda.synchronize()
    first, first_weights = acc.acc.clone(), weights.clone()
    assert first[..., SOBOL_COUNT].max() > 0
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.sample_families(fp, out=run)
        dp.sobol_bootstrap_ensemble(run.latents, out=acc, **kw)
        dp.bootstrap_weights(40, r, 3, out=weights)
    run.latents.fill_(3.0)
    run.flags.fill_(255)
    acc.acc.fill_(-1.0)
    weights.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.acc.view(torch.int64), first.view(torch.int64)) and torch.equal(weights, first_weights)
    assert np.array_equal(weights.cpu().numpy(), bootstrap_weights(3, 0, 40, r))


def test_error_paths_launch_nothing(dp):
    import ctypes as C

    from open_kinematics_amd import _lib

    lib = dp.lib
    s, k, d, n, r = 2, 3, 2, 4, 9
    table = torch.zeros((n * (d + 2) * s, k), dtype=torch.float64, device=DEV)
    shift = torch.zeros((s, k), dtype=torch.float64, device=DEV)
    acc = torch.full((r, s, k, SOBOL_FIELDS + 3 * d), -3.0, dtype=torch.float64, device=DEV)
    need = int(lib.okx_ensemble_sobol_bootstrap_scratch_bytes(n, d, s, k, r))
    # one slab of partials, the weights padded to two replicate tiles, a counting byte per (family, entry)
    assert need == 8 * r * (SOBOL_FIELDS + 3 * d) * s * k + n * 2 * RT + (n * s * k + 7) // 8 * 8
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(n_families=n, offset=0, n_groups=d, steps=s, columns=k, values=table, ld=k, replicates=r, room=need):
        return lib.okx_ensemble_sobol_bootstrap(n_families, offset, n_groups, steps, columns, C.c_void_p(values.data_ptr() if values is not None else 0), ld, None,
                                                0, None, C.c_void_p(shift.data_ptr()), C.c_uint64(1), replicates, 0, C.c_void_p(acc.data_ptr()),
                                                C.c_void_p(scratch.data_ptr()), room, None)

    for kw, words in ((dict(n_families=-1), "negative geometry, step or column count"), (dict(offset=-1), "negative family_offset"),
                      (dict(ld=k - 1), "null table or ld < n_columns"), (dict(values=None), "null table or ld < n_columns"),
                      (dict(n_groups=0), "0 groups, 1 to 288 allowed"), (dict(n_groups=289), "289 groups, 1 to 288 allowed"),
                      (dict(replicates=0), "0 replicates, 1 to 1024 allowed"), (dict(replicates=1025), "1025 replicates, 1 to 1024 allowed"),
                      (dict(room=need - 1), "(okx_ensemble_sobol_bootstrap_scratch_bytes)"), (dict(steps=1 << 31), "too many entries for one call")):
        assert call(**kw) != 0
        assert words in _lib.last_error() and "okx_ensemble_sobol_bootstrap" in _lib.last_error(), (kw, _lib.last_error())
    weights = torch.full((4, 3), 99, dtype=torch.uint8, device=DEV)
    for args, words in (((-1, 0, 1, 3), "negative row count or offset"), ((4, -1, 1, 3), "negative row count or offset"),
                        ((4, 0, 1, 0), "0 replicates, 1 to 1024 allowed"), ((4, 0, 1, 1025), "1025 replicates, 1 to 1024 allowed")):
        assert lib.okx_ensemble_bootstrap_weights(args[0], args[1], C.c_uint64(args[2]), args[3], C.c_void_p(weights.data_ptr()), None) != 0
        assert words in _lib.last_error() and "okx_ensemble_bootstrap_weights" in _lib.last_error(), (args, _lib.last_error())
    assert lib.okx_ensemble_bootstrap_weights(4, 0, C.c_uint64(1), 3, None, None) != 0 and "null weight table" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((acc == -3.0).all()) and bool((weights == 99).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    want = bootstrap_weights(1, 0, n, r).sum(axis=0).astype(np.float64)
    assert np.array_equal(acc[..., SOBOL_COUNT].cpu().numpy(), np.broadcast_to(want[:, None, None], (r, s, k)))
    # the Python layer
    with pytest.raises(ValueError, match="no whole families of 4"):
        dp.sobol_bootstrap_ensemble(table[: 7 * s], steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1)
    with pytest.raises(ValueError, match="accumulate=True needs"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, accumulate=True)
    out = SobolBootstrapAccumulator(acc, shift, 1)
    with pytest.raises(ValueError, match="out= carries its own shift"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, shift=shift, out=out)
    with pytest.raises(ValueError, match="out= was taken with seed 1, not 2"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=2, out=out)
    with pytest.raises(ValueError, match="out must hold"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r + 1, seed=1, out=out)
    with pytest.raises(ValueError, match="1025 replicates, 1 to 1024 allowed"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=1025, seed=1)
    with pytest.raises(ValueError, match="negative family_offset"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, family_offset=-1)
    with pytest.raises(ValueError, match="mask must be"):
        dp.sobol_bootstrap_ensemble(table, steps_per_geometry=s, n_groups=d, n_replicates=r, seed=1, mask=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="0 replicates, 1 to 1024 allowed"):
        dp.bootstrap_weights(4, 0, 1)
    with pytest.raises(ValueError, match="out must be"):
        dp.bootstrap_weights(4, 3, 1, out=weights[:3])
