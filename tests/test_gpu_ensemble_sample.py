"""
GPU: okx_ensemble_sample (DeviceProgram.sample_ensemble, and ShardedEnsemble taking a SamplePlan) against
ensemble_sample.sample_host.  Every comparison is EQUAL BITS in all four outputs - hardpoints, latents, delta as uint64 words,
flags as bytes.  The shapes are where the mapping (one wavefront per geometry, lanes along latents, coordinates and the flat
row) can go wrong: rows shorter than a wavefront, of exactly 64 and 65 entries, of several rounds, and the caps.
tests/test_ensemble_sample.py holds the plans' generator and checks the definition itself.
"""

import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available
from open_kinematics_amd.ensemble_sample import GUARD_DISTINCT, GUARD_OFF_LINE, IID, LHS, NORMAL, TRUNCATED, UNIFORM, SamplePlan, sample_host
from test_ensemble_sample import bits, make_plan, same_sample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G_ALL = (0, 1, 2, 37, 63, 64, 65, 1031)


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


# the arguments of test_ensemble_sample.make_plan by case; g: the geometry counts (default G_ALL)
CASES = {
    "one coordinate": dict(p=1, f=1, kinds=(NORMAL,), stratify=IID),
    "one point, two latents mixed": dict(p=1, f=3, z=2, mixing=True, stratify=LHS, max_attempts=4, half_failing=True),
    "seven points": dict(p=7, f=5, stratify=LHS),
    "one latent moves five coordinates": dict(p=7, f=5, z=1, mixing=True, kinds=(TRUNCATED,), stratify=IID, max_attempts=4, half_failing=True),
    "a row of 96 and 60 latents": dict(p=32, f=60, stratify=IID, max_attempts=4, half_failing=True),
    "a guard that half fails, one attempt": dict(p=32, f=60, stratify=LHS, max_attempts=1, half_failing=True),
    "288 latents into 60 coordinates": dict(p=32, f=60, z=288, mixing=True, stratify=LHS),
    "the caps, no mixing": dict(p=96, f=288, stratify=LHS, max_attempts=4, half_failing=True),
    "the caps, dense mixing": dict(p=96, f=288, z=288, mixing=True, stratify=IID, g=(1, 65, 130)),
    "uniform only": dict(p=7, f=21, kinds=(UNIFORM,), stratify=LHS, g=(65,)),
    "normal only, mixed": dict(p=22, f=64, z=65, mixing=True, kinds=(NORMAL,), stratify=IID, g=(64, 65)),
    "truncated only": dict(p=22, f=65, kinds=(TRUNCATED,), stratify=IID, max_attempts=4, half_failing=True, g=(64, 65)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The plan of a case and ``sample_host`` of its largest range, computed once and shared (the arrays are not written)."""
    spec = dict(CASES[name])
    sizes = spec.pop("g", G_ALL)
    plan = make_plan(**spec, n_total=max(sizes), seed=11 + len(name))
    return plan, sizes, sample_host(plan, 0, max(sizes))


def device_sample(dp, plan, lo, hi, **kw):
    run = dp.sample_ensemble(plan, lo, hi, latents=True, delta=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (run.hardpoints, run.latents, run.delta, run.flags)]


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_definition(dp, name):
    plan, sizes, want = reference(name)
    if CASES[name].get("half_failing"):
        assert (want[3] != 0).any() and (want[3] == 0).any()  # redraws or failures happen, and not everywhere
    for g in sizes:
        got = device_sample(dp, plan, 0, g)
        assert same_sample(got, [t[:g] for t in want]), (name, g)
        assert got[0].shape == (g, plan.n_points, 3) and got[3].dtype == np.uint8


def test_optional_outputs_and_neighbouring_rows(dp):
    """latents, delta and flags NULL; the table is written for its n rows and not one entry beyond."""
    from open_kinematics_amd.ensemble_device import EnsembleSample

    plan, _, want = reference("a row of 96 and 60 latents")
    n = 65
    room = torch.full((n + 1, plan.n_points, 3), -7.0, dtype=torch.float64, device=DEV)
    run = dp.sample_ensemble(plan, 0, n, out=EnsembleSample(room[:n], None, None, None))
    torch.cuda.synchronize()
    assert run.latents is None and run.delta is None and run.flags is None
    assert np.array_equal(bits(room[:n].cpu().numpy()), bits(want[0][:n])) and bool((room[n] == -7.0).all())
    plain = dp.sample_ensemble(plan, 0, n)
    assert plain.latents is None and plain.delta is None and np.array_equal(plain.flags.cpu().numpy(), want[3][:n])
    flags_only = torch.full((n + 64,), 255, dtype=torch.uint8, device=DEV)
    dp.sample_ensemble(plan, 0, n, out=EnsembleSample(room[:n], None, None, flags_only[:n]))
    assert np.array_equal(flags_only[:n].cpu().numpy(), want[3][:n]) and bool((flags_only[n:] == 255).all())
    with pytest.raises(ValueError, match="out must hold"):
        dp.sample_ensemble(plan, 0, n + 1, out=run)


def test_the_high_counter_word(dp):
    """geometry_offset = 2^32 - 3, 8 geometries (IID): the global index crosses into the second counter word."""
    plan = make_plan(7, 5, max_attempts=4, half_failing=True)
    lo = 2 ** 32 - 3
    want = sample_host(plan, lo, lo + 8)
    assert same_sample(device_sample(dp, plan, lo, lo + 8), want)
    assert not np.array_equal(bits(want[1][3:]), bits(sample_host(plan, 0, 5)[1]))  # (g = 2^32 + i does not draw as g = i)


@pytest.mark.parametrize("name", ["one point, two latents mixed", "a row of 96 and 60 latents", "288 latents into 60 coordinates"])
def test_one_call_equals_three_ragged_chunks(dp, name):
    plan, _, want = reference(name)
    cuts = (0, 37, 101, 200)
    whole = device_sample(dp, plan, 0, cuts[-1])
    parts = [device_sample(dp, plan, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    glued = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    assert same_sample(glued, whole) and same_sample(whole, [t[: cuts[-1]] for t in want])


def test_distinct_and_off_line_guards_on_device(dp):
    """Three nearly collinear, nearly coincident points: the two geometric guards reject a good share of the draws."""
    nominal = np.asarray([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 4.0, 5.0]])
    guards = ((GUARD_DISTINCT, 0, 1, 0.4), (GUARD_OFF_LINE, 0, 2, 1, 0.05), (GUARD_OFF_LINE, 3, 0, 2, 1.0))
    plan = SamplePlan(nominal, np.arange(9), NORMAL, scale=0.2, seed=5, guards=guards, max_attempts=3)
    want = sample_host(plan, 0, 300)
    kept = want[3] >> 4
    assert {0, 1, 2} <= set(kept.tolist()) and 0 < (want[3] & 1).sum() < 300
    assert same_sample(device_sample(dp, plan, 0, 300), want)


def test_a_captured_launch_replays(dp):
    from open_kinematics_amd.ensemble_device import EnsembleSample

    plan, _, want = reference("one latent moves five coordinates")
    n = 65
    run = dp.sample_ensemble(plan, 100, 100 + n, latents=True, delta=True)  # (warm: the plan's tables are on the device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        dp.sample_ensemble(plan, 100, 100 + n, out=run)
    for t in (run.hardpoints, run.latents, run.delta):
        t.fill_(3.0)
    run.flags.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (run.hardpoints, run.latents, run.delta, run.flags)]
    assert same_sample(got, [t[100 : 100 + n] for t in want]) and isinstance(run, EnsembleSample)


@functools.lru_cache(maxsize=None)
def c5(n_geom, steps):
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.workloads import ensemble_plan, geometry_path

    program, plan, rel = ensemble_plan(n_geom, 1.0, 3, n_steps=steps, stratify=LHS)
    device_program = DeviceProgram(program, DEV)
    device_program.enable_evaluation(corner_roles(load_geometry(geometry_path("geometry.yaml")), program))
    bump = program.n_targets - 1
    columns = [("camber", None), ("camber", bump), ("roadwheel_angle", bump), (21, bump)]
    return device_program, plan, rel, columns


def test_the_chain_from_the_sampler_equals_the_chain_from_the_host_table():
    """sample_ensemble -> rebind -> solve_evaluated on 64 geometries x 4 steps: the same bits as the chain fed the host-drawn table."""
    g, s = 64, 4
    device_program, plan, rel, _ = c5(g, s)
    table = sample_host(plan)[0]
    answers = []
    for hardpoints in (device_program.sample_ensemble(plan).hardpoints, torch.as_tensor(table, device=DEV)):
        gpos, gparam = device_program.rebind(hardpoints)
        targets = device_program.ensemble_targets(gpos, rel)
        res = device_program.solve_evaluated(targets, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=s, output="none", chain_len=1, predictor=False)
        torch.cuda.synchronize()
        answers.append((gpos.cpu().numpy(), res.eval.cpu().numpy(), res.info_raw.cpu().numpy()))
    assert np.array_equal(bits(answers[0][0]), bits(answers[1][0])) and np.array_equal(bits(answers[0][1]), bits(answers[1][1]))
    assert np.array_equal(answers[0][2], answers[1][2])


@pytest.mark.parametrize("chunks", [1, 2])
def test_sharded_ensemble_with_a_plan_equals_the_materialised_route(chunks):
    import open_kinematics_amd.dist as okd

    g, s = 64, 4
    device_program, plan, rel, columns = c5(g, s)
    table, latents, _, flags = sample_host(plan)
    assert not np.any(flags & 1)
    kw = dict(metric_columns=columns, reduce=True, chain_len=1, predictor=False, chunks=chunks)
    drawn = okd.ShardedEnsemble(device_program, plan, rel, s, factors="sampled", **kw)
    made = okd.ShardedEnsemble(device_program, torch.as_tensor(table, device=DEV), rel, s, factors=latents, **kw)
    for pipe in (drawn, made):
        pipe.step()
    torch.cuda.synchronize()
    a, b = drawn.accumulator, made.accumulator
    assert drawn.my_pos.device.type == "cuda" and torch.equal(drawn.my_pos.view(torch.int64), made.my_pos.view(torch.int64))
    assert torch.equal(drawn.my_factors.view(torch.int64), made.my_factors.view(torch.int64))
    assert torch.equal(a.acc.view(torch.int64), b.acc.view(torch.int64)) and torch.equal(a.factor_acc.view(torch.int64), b.factor_acc.view(torch.int64))
    assert torch.equal(drawn.metric_local.view(torch.int64), made.metric_local.view(torch.int64))
    assert drawn.factor_names == plan.factor_names() and len(drawn.factor_names) == 30 and made.factor_names is None


def test_argument_checks_launch_nothing(dp):
    plan, _, _ = reference("seven points")
    with pytest.raises(ValueError, match=r"geometries \[1000, 1032\) lie outside the 1031 strata"):
        dp.sample_ensemble(plan, 1000, 1032)
    with pytest.raises(ValueError, match="bad range"):
        dp.sample_ensemble(plan, 5, 4)
    empty = dp.sample_ensemble(plan, 7, 7, latents=True)
    assert empty.hardpoints.shape == (0, 7, 3) and empty.latents.shape == (0, 5)


def test_a_plans_tables_leave_with_the_plan(dp):
    """The device copies of a plan's tables are held while the plan lives, not for the life of the DeviceProgram."""
    import gc

    plan = make_plan(7, 5, seed=77)
    first = dp.sample_ensemble(plan, 0, 4).hardpoints.cpu().numpy()
    held = len(dp._sample_plans)
    assert np.array_equal(bits(dp.sample_ensemble(plan, 0, 4).hardpoints.cpu().numpy()), bits(first)) and len(dp._sample_plans) == held
    del plan
    gc.collect()
    assert len(dp._sample_plans) == held - 1
