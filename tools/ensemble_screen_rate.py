"""
What the on-device joint screen costs (okx_ensemble_screen, ShardedEnsemble(reduce=True, limits=..., screen=True)) on BASELINE
config 5 - 4096 perturbed geometries x 256 bump steps, bench.py's four metric columns, limits on every entry (the 0.2 % - 99.8 %
band of the table itself, the per-entry std as the scale) - on ONE GPU, device events, 20 repetitions after warm-up:

  (a) the screen pass alone (begin + verdict + compaction);
  (b) in the same run, on the same table: okx_ensemble_reduce and round 0 of okx_ensemble_select_count - passes that read
      the same bytes once;
  (c) what the user must otherwise do: metric_local.cpu() (timed alone), then the NumPy screen (ensemble_stats.screen_host);
  (d) the ShardedEnsemble step with and without screen=True, alternated.

The expectation: (a) is no slower than the reduce pass of (b) measured beside it - the same table moves and less arithmetic is
done - within the run-to-run spread this file reports.

  python tools/ensemble_screen_rate.py --out profiles/r10/ensemble_screen_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes), each writing its screen to ``<out>/rank<r>.pt`` - the
rehearsal tests/test_gpu_ensemble_screen.py compares; ``--limits FILE.npz`` (``limits [S, K, 2]``, ``scale [S, K]``) replaces
the fixed window.
"""

from __future__ import annotations

import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import alternated, rank, spread, step_ms
from ensemble_reduce_rate import HBM_PEAK, build
from ensemble_select_rate import window

FIELDS = ("flags", "tally", "blame", "passed")


def rank_main(args) -> None:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        dp, table, rel, columns = build(args.geometries, args.steps_per_geometry, device)
        limits, scale = window(args.steps_per_geometry, len(columns)), None
        if args.limits:
            with np.load(args.limits) as fh:
                limits, scale = fh["limits"], fh["scale"]
        pipe = ShardedEnsemble(dp, table, rel, args.steps_per_geometry, chunks=args.chunks or None, metric_columns=columns, reduce=True, limits=limits,
                               screen=True, screen_scale=scale, chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        got, local = pipe.screen(), pipe.screen_local()
        torch.save({"screen": {f: getattr(got, f) for f in FIELDS}, "local": {k: v.cpu() for k, v in local.items()}, "acc": acc.acc.cpu(),
                    "sent": pipe.exchange_bytes_per_rank, "screen_sent": pipe.screen_exchange_bytes_per_rank, "range": pipe.geometry_range},
                   os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 38500, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry,
                                                        "--chunks", args.chunks, "--limits", args.limits])


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import EnsembleAccumulator, screen_host

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    k = len(columns)
    kw = dict(chain_len=1, predictor=False)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, **kw)
    reduced.step()
    torch.cuda.synchronize()
    values, status = reduced.metric_local, reduced.info_local[:, 32]
    host_v = values.cpu().numpy().reshape(g, s, k)
    host_st = status.cpu().numpy().reshape(g, s)
    masked = np.where(np.isfinite(host_v) & ((host_st & 7) == 1)[:, :, None], host_v, np.nan)
    limits = np.stack([np.nanquantile(masked, 0.002, axis=0), np.nanquantile(masked, 0.998, axis=0)], axis=2)
    scale = np.nanstd(masked, axis=0)
    scale[~(scale > 0)] = 1.0
    screened = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, limits=limits, screen=True, screen_scale=scale, **kw)
    for _ in range(args.warmup):
        reduced.step()
        screened.step()
    torch.cuda.synchronize()
    values, status = screened.metric_local, screened.info_local[:, 32]
    reps = args.reps

    # (a) the pass alone, (b) the yardsticks beside it - alternated block by block so that a drift hits all three alike
    scr = dp.screen_ensemble(values, steps_per_geometry=s, status=status, limits=limits, scale=scale)
    one_screen = lambda: dp.screen_ensemble(values, steps_per_geometry=s, status=status, out=scr)  # noqa: E731
    acc = EnsembleAccumulator(torch.empty_like(reduced.local_accumulator.acc), reduced.local_accumulator.shift, None)
    one_reduce = lambda: dp.reduce_ensemble(values, steps_per_geometry=s, status=status, out=acc)  # noqa: E731
    run = dp.select_prepare(s, k, (0.5,), limits, rounds=True)
    dp.select_begin(run)
    one_count = lambda: dp.select_count(run, 0, values, steps_per_geometry=s, status=status)  # noqa: E731
    runs = alternated({"screen": one_screen, "reduce": one_reduce, "count": one_count}, reps)
    med = {name: statistics.median(r) for name, r in runs.items()}

    # (c) what the user must otherwise do on one GPU
    copy_ms, host_ms = [], []
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = values.cpu()  # the copy alone: the table, without its status bytes
        t1 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        if rep >= 3:  # (the NumPy part is not what the comparison is about: three runs of it)
            continue
        want = screen_host(host.numpy().reshape(g, s, k), status.cpu().numpy().reshape(g, s), limits, scale)
        host_ms.append((time.perf_counter() - t1) * 1e3)
    got = scr.finalize()
    exact = all(np.array_equal(getattr(got, f), getattr(want, f)) for f in FIELDS + ("entry",)) and \
        bool(np.array_equal(got.margin.view(np.uint64), want.margin.view(np.uint64)))

    # (d) the sharded ensemble's step with and without the screen, alternated
    rounds = [(step_ms(reduced.step, args.steps), step_ms(screened.step, args.steps)) for _ in range(5)]
    off, on = statistics.median(r[0] for r in rounds), statistics.median(r[1] for r in rounds)

    table_bytes = 8 * g * s * k + g * s
    copy = statistics.median(copy_ms)
    slack = max(spread(runs["screen"]), spread(runs["reduce"]))
    holds = bool(med["screen"] <= med["reduce"] + slack)
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns, limits on all {s * k} entries, one GPU",
        "joint_yield": got.joint_yield, "tally": [int(x) for x in got.tally], "entries_blamed": int((got.blame.sum(axis=2) > 0).sum()),
        "a_screen_pass_us": {"median": med["screen"], "interquartile": spread(runs["screen"]), "runs": runs["screen"], "table_bytes": table_bytes,
                             "hbm_floor_us": table_bytes / HBM_PEAK * 1e6},
        "b_same_bytes_once_us": {"reduce_pass": {"median": med["reduce"], "interquartile": spread(runs["reduce"]), "runs": runs["reduce"]},
                                 "select_count_round_0": {"median": med["count"], "interquartile": spread(runs["count"]), "runs": runs["count"]},
                                 "screen_over_reduce": med["screen"] / med["reduce"]},
        "expectation_screen_no_slower_than_reduce": {"screen_us": med["screen"], "reduce_us": med["reduce"], "allowed_spread_us": slack, "holds": holds,
                                                     "misses_by_us": 0.0 if holds else med["screen"] - med["reduce"] - slack},
        "c_host_path_ms": {"copy_alone_median": copy, "copy_runs": copy_ms, "numpy_screen_median": statistics.median(host_ms),
                           "what": "metric_local.cpu() alone; then the status bytes' copy and ensemble_stats.screen_host"},
        "device_equals_screen_host_exactly": bool(exact),
        "d_step_ms": {"reduce_only": off, "with_screen": on, "extra_ms": on - off, "extra_percent": (on / off - 1.0) * 100.0, "rounds": rounds,
                      "steps_per_round": args.steps},
        "screen_exchange_bytes_per_rank_at_world_two": 8 * (4 + 2 * s * k) + (g + 1) // 2,
    }


def summary(r: dict) -> str:
    a, b, c, d, e = r["a_screen_pass_us"], r["b_same_bytes_once_us"], r["c_host_path_ms"], r["d_step_ms"], r["expectation_screen_no_slower_than_reduce"]
    lines = [r["workload"], f"joint yield {r['joint_yield']:.4f}  tally (seen, passed, outside, unresolved) {r['tally']}  entries blamed {r['entries_blamed']}",
             f"(a) screen pass          {a['median']:8.1f} us  (interquartile {a['interquartile']:.1f}; the table's bytes at the HBM peak: {a['hbm_floor_us']:.1f} us)",
             f"(b) reduce pass          {b['reduce_pass']['median']:8.1f} us  (interquartile {b['reduce_pass']['interquartile']:.1f})   screen / reduce = {b['screen_over_reduce']:.2f}",
             f"    select count round 0 {b['select_count_round_0']['median']:8.1f} us  (interquartile {b['select_count_round_0']['interquartile']:.1f})",
             f"    expectation, screen no slower than reduce within the spread ({e['allowed_spread_us']:.1f} us): "
             + ("holds" if e["holds"] else f"MISSED by {e['misses_by_us']:.1f} us"),
             f"(c) copy alone           {c['copy_alone_median'] * 1e3:8.1f} us  NumPy screen {c['numpy_screen_median']:.1f} ms",
             f"    device == screen_host exactly: {r['device_equals_screen_host_exactly']}",
             f"(d) step                 {d['reduce_only']:.3f} ms reduce only, {d['with_screen']:.3f} ms with the screen (+{d['extra_ms']:.3f} ms, {d['extra_percent']:.1f} %)"]
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, steps=50, warmup=10, reps=20, chunks=0)
    ap.add_argument("--limits", default="")
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
