"""
What the on-device ensemble reduction costs (okx_ensemble_reduce, ShardedEnsemble(reduce=True)) on BASELINE config 5 -
4096 perturbed geometries x 256 bump steps, bench.py's four metric columns, 30 hardpoint factors - on ONE GPU:

  (a) the evaluated ensemble's step with reduce=False (the gathered column table) and with reduce=True, alternated;
  (b) reduce=False plus what its user must add for the same answer: metric_full.cpu() and NumPy mean / var / min / max /
      argmin / argmax / lstsq;
  (c) the pass alone (device events around 4000 launches after warm-up), with its bytes over the HBM peak and its FMAs
      over the fp64 vector peak beside it.

  python tools/ensemble_reduce_rate.py --out profiles/r08/ensemble_reduce_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes), each writing its merged accumulator to
``<out>/rank<r>.pt`` - the two-rank rehearsal tests/test_gpu_ensemble_stats.py compares.
"""

from __future__ import annotations

import os
import statistics
import sys

import ensemble_rate_common as common
from ensemble_rate_common import rank, step_ms

HBM_PEAK = 6.3e12          # B/s (README roofline)
FP64_VECTOR_PEAK = 78.6e12  # FLOP/s, MI355X vector fp64


def build(n_geom: int, steps: int, device):
    import torch

    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.workloads import ensemble_problem, geometry_path

    program, table, rel = ensemble_problem(n_geom, steps)
    dp = DeviceProgram(program, device)
    dp.enable_evaluation(corner_roles(load_geometry(geometry_path("geometry.yaml")), program))
    bump = program.n_targets - 1
    columns = [("camber", None), ("camber", bump), ("roadwheel_angle", bump), (21, bump)]
    return dp, torch.as_tensor(table, device=device), rel, columns


def rank_main(args) -> None:
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        dp, table, rel, columns = build(args.geometries, args.steps_per_geometry, device)
        pipe = ShardedEnsemble(dp, table, rel, args.steps_per_geometry, metric_columns=columns, reduce=True, factors="hardpoints",
                               chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        torch.save({"acc": acc.acc.cpu(), "factor_acc": acc.factor_acc.cpu(), "shift": acc.shift.cpu(), "sent": pipe.exchange_bytes_per_rank,
                    "range": pipe.geometry_range}, os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 34500, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry])


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import EnsembleAccumulator

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    kw = dict(chain_len=1, predictor=False)
    plain = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, **kw)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, factors="hardpoints", **kw)
    factors_host = reduced.my_factors.cpu().numpy()

    def host_statistics():
        full = plain.step()
        v = full.cpu().numpy().reshape(g, s, -1)
        out = (v.mean(axis=0), v.var(axis=0, ddof=1), v.min(axis=0), v.max(axis=0), v.argmin(axis=0), v.argmax(axis=0))
        design = np.concatenate([np.ones((g, 1)), factors_host], axis=1)
        return out, np.linalg.lstsq(design, v.reshape(g, -1), rcond=None)[0]

    for _ in range(args.warmup):
        plain.step()
        reduced.step()
    rounds = []
    for _ in range(5):  # alternated: the same tree, the same call
        rounds.append((step_ms(plain.step, args.steps), step_ms(reduced.step, args.steps)))
    host_ms = [step_ms(host_statistics, 3) for _ in range(3)]

    # (c) the pass alone
    values, status = reduced.metric_local, reduced.info_local[:, 32]
    out = EnsembleAccumulator(torch.empty_like(reduced.local_accumulator.acc), reduced.local_accumulator.shift, None)

    def one_pass():
        dp.reduce_ensemble(values, steps_per_geometry=s, status=status, factors=reduced.my_factors, out=out, factor_moments=False)

    for _ in range(20):
        one_pass()
    passes = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            one_pass()
        b.record()
        torch.cuda.synchronize()
        passes.append(a.elapsed_time(b) / args.launches * 1e3)
    k, p = len(columns), reduced.n_factors
    bytes_moved = 8 * g * s * k + g * s + 8 * g * p  # the ALGORITHMIC bytes: table, status bytes, factor table, each once
    # what the pass moves beside them: the partial accumulators written by stage 1 and read by stage 2, and the factor table
    # once per tile of 64 entries instead of once (from L2 after the first tile)
    scratch_bytes = int(dp.lib.okx_ensemble_scratch_bytes(g, s, k, p))
    tiles = (s * k + 63) // 64
    fmas = g * s * k * (p + 1)
    pass_us = statistics.median(passes)
    off = statistics.median(r[0] for r in rounds)
    on = statistics.median(r[1] for r in rounds)
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns, {p} factors, one GPU",
        "a_step_ms": {"reduce_false": off, "reduce_true": on, "extra_percent": (on / off - 1.0) * 100.0, "rounds": rounds,
                      "steps_per_round": args.steps, "aim": "reduce=True at most 5 % above reduce=False"},
        "b_step_plus_host_statistics_ms": {"median": statistics.median(host_ms), "runs": host_ms,
                                           "what": "reduce=False step + metric_full.cpu() + NumPy mean / var / min / max / argmin / argmax / lstsq"},
        "c_pass_alone_us": {"median": pass_us, "runs": passes, "launches_per_run": args.launches, "bytes": bytes_moved,
                            "bytes_note": "algorithmic bytes only (table + status + factors, each once); the floors and the achieved GB/s are of these",
                            "scratch_bytes_written_and_read_again": scratch_bytes, "factor_table_reads": tiles,
                            "hbm_floor_us": bytes_moved / HBM_PEAK * 1e6, "fp64_fma": fmas,
                            "fp64_floor_us": 2 * fmas / FP64_VECTOR_PEAK * 1e6,
                            "achieved_GBps": bytes_moved / (pass_us * 1e-6) / 1e9, "achieved_fp64_TFLOPs": 2 * fmas / (pass_us * 1e-6) / 1e12},
        "accumulator_bytes_per_rank": 8 * (s * k * (8 + p) + p + p * (p + 1) // 2 + 1),
        "per_state_exchange_bytes_per_rank_it_replaces": g * s * (8 * k + 1),
    }


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, steps=400, warmup=20, launches=4000)
    return common.run(ap.parse_args(), measure, None, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
