"""
ShardedEnsemble(reduce=True) with ALL FOUR stages switched on in one ensemble - reduction with hardpoint factors, quantiles with
limits, the joint screen and the covariance of a subset - over two gloo ranks, the stand-in program of tests/test_dist.py: every
answer and every byte count equals, bit for bit and on both ranks, that of an ensemble which switches on that stage alone.

Five geometries in two chunks shard 3 + 2 (every rank's second chunk accumulates onto its first); one geometry leaves rank 1
without any, and it must still join every collective in order.
"""

import dataclasses
import os
import sys
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from test_ensemble_covariance import SUBSET
from test_ensemble_screen import STEPS, sharded_limits
from test_ensemble_stats import COLUMNS, _stand_in

PROBS = (0.1, 0.5, 0.9)
CASES = [5, 1]  # geometries
CHUNKS = 2
ANSWERS = ("stats", "quantiles", "screen", "covariance")
SENT = ("exchange_bytes_per_rank", "select_exchange_bytes_per_rank", "screen_exchange_bytes_per_rank", "covariance_exchange_bytes_per_rank")


def _program():
    """The stand-in with what ``factors="hardpoints"`` asks of a program: point 0 is authored, points 1 and 2 are derived."""
    dp = _stand_in()

    class program(dp.program):  # noqa: N801 - attribute bag like ConstraintProgram
        dop_out = [1, 2]
        point_keys = [types.SimpleNamespace(name=n) for n in ("LOWER", "MIDDLE", "UPPER")]

    dp.program = program
    return dp


def _stage_arguments():
    limits, scale = sharded_limits()
    return {"stats": {}, "quantiles": dict(quantiles=PROBS, limits=limits), "screen": dict(limits=limits, screen=True, screen_scale=scale),
            "covariance": dict(covariance=SUBSET)}


def _tables(answer) -> dict:
    """The array fields of an answer (a dataclass of NumPy arrays, numbers, lists or None)."""
    return {f.name: getattr(answer, f.name) for f in dataclasses.fields(answer)}


def same_bits(a: dict, b: dict) -> bool:
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")):
                return False
        elif x != y:
            return False
    return True


def _ensembles(n_geom: int):
    """``(the ensemble with every stage, {answer: the ensemble with that stage alone})``, each stepped once."""
    from open_kinematics_amd.dist import ShardedEnsemble
    from test_dist import _ensemble_inputs

    table, relative = _ensemble_inputs(n_geom, STEPS)
    kw = dict(chunks=CHUNKS, metric_columns=COLUMNS, reduce=True, factors="hardpoints")
    arguments = _stage_arguments()
    together = ShardedEnsemble(_program(), table, relative, STEPS, **kw, quantiles=PROBS, limits=arguments["screen"]["limits"], screen=True,
                               screen_scale=arguments["screen"]["screen_scale"], covariance=SUBSET)
    alone = {name: ShardedEnsemble(_program(), table, relative, STEPS, **kw, **arguments[name]) for name in ANSWERS}
    for pipe in (together, *alone.values()):
        pipe.step()
    return together, alone


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for n_geom in CASES:
        together, alone = _ensembles(n_geom)
        out[n_geom] = {"range": together.geometry_range, "n_factors": together.n_factors,
                       "together": {name: _tables(getattr(together, name)()) for name in ANSWERS},
                       "alone": {name: _tables(getattr(alone[name], name)()) for name in ANSWERS},
                       "sent": {name: (getattr(together, name), getattr(alone[answer], name)) for name, answer in zip(SENT, ANSWERS)}}
    torch.save(out, os.path.join(out_dir, f"stages{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_all_stages_together_equal_each_stage_alone(tmp_path):
    world = 2
    port = 37700 + (os.getpid() + 17 * world) % 2000
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"stages{r}.pt"), weights_only=False) for r in range(world)]
    k = len(COLUMNS)
    for n_geom in CASES:
        one, two = got[0][n_geom], got[1][n_geom]
        assert (one["range"], two["range"]) == ({5: (0, 3), 1: (0, 1)}[n_geom], {5: (3, 5), 1: (1, 1)}[n_geom])
        p = one["n_factors"]
        assert p == two["n_factors"] == (3 if n_geom == 5 else 0)  # (one geometry: no coordinate varies)
        for rank in (one, two):
            for name in ANSWERS:
                assert same_bits(rank["together"][name], rank["alone"][name]), (n_geom, name)
                assert same_bits(rank["together"][name], one["together"][name]), (n_geom, name)  # the same bits on both ranks
            for name in SENT:
                assert rank["sent"][name][0] == rank["sent"][name][1] > 0, (n_geom, name)
            n = len(SUBSET)
            assert [rank["sent"][name][0] for name in SENT] == [8 * (STEPS * k * (8 + p) + (p + p * (p + 1) // 2 + 1 if p else 0)),
                                                                16 * 8 * STEPS * k * 2 * len(PROBS) * 16, 8 * (4 + 2 * STEPS * k) + (3 if n_geom == 5 else 1),
                                                                8 * (n * n + n + 2)]
        # the inputs are worth the test: states that count and states that do not, verdicts on the five geometries
        stats, screen = one["together"]["stats"], one["together"]["screen"]
        assert stats["count"].sum() + stats["rejected"].sum() == n_geom * STEPS * k and stats["count"].sum() > 0
        assert screen["tally"][0] == n_geom and screen["flags"].shape == (n_geom,)
        if n_geom == 5:
            assert stats["rejected"].sum() > 0 and stats["sensitivity"].shape == (STEPS, k, 3)


def test_one_process_runs_the_same_stages():
    """A world of one, no process group: together equals alone here too, and nothing is sent."""
    together, alone = _ensembles(5)
    for name, sent in zip(ANSWERS, SENT):
        assert same_bits(_tables(getattr(together, name)()), _tables(getattr(alone[name], name)())), name
        assert getattr(together, sent) == getattr(alone[name], sent) == 0
