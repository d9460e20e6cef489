"""
What the on-device ensemble selection costs (okx_ensemble_select, ShardedEnsemble(reduce=True, quantiles=...)) on BASELINE
config 5 - 4096 perturbed geometries x 256 bump steps, bench.py's four metric columns, Q = 3 probabilities (0.00135, 0.5,
0.99865), limits on - on ONE GPU, device events, 20 repetitions after warm-up:

  (a) the select pass alone, whole and round by round (count + descend of every round through the round-level calls);
  (b) okx_ensemble_reduce on the same table in the same run: the yardstick kernel;
  (c) what the user must otherwise do: metric_local.cpu() (timed alone), numpy.quantile and the limit counts;
  (d) the ShardedEnsemble step with and without quantiles, alternated.

  python tools/ensemble_select_rate.py --out profiles/r09/ensemble_select_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes), each writing its quantiles to ``<out>/rank<r>.pt`` -
the rehearsal tests/test_gpu_ensemble_select.py compares.
"""

from __future__ import annotations

import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import events, rank, step_ms
from ensemble_reduce_rate import HBM_PEAK, build

PROBS = (0.00135, 0.5, 0.99865)
FIELDS = ("count", "lower", "upper", "quantile", "below", "above", "yield_")


def window(steps: int, n_columns: int):
    """A spec window per column, open on one side for the last: (lo, hi) [K, 2]."""
    import numpy as np

    lim = np.tile(np.array([[-0.5, 0.5]]), (n_columns, 1))
    lim[-1, 1] = np.inf
    return lim


def rank_main(args) -> None:
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        dp, table, rel, columns = build(args.geometries, args.steps_per_geometry, device)
        pipe = ShardedEnsemble(dp, table, rel, args.steps_per_geometry, metric_columns=columns, reduce=True, quantiles=PROBS,
                               limits=window(args.steps_per_geometry, len(columns)), chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        q = pipe.quantiles()
        torch.save({"q": {f: getattr(q, f) for f in FIELDS}, "acc": acc.acc.cpu(), "sent": pipe.exchange_bytes_per_rank,
                    "select_sent": pipe.select_exchange_bytes_per_rank, "range": pipe.geometry_range}, os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 36500, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry])


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import EnsembleAccumulator, select_host

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    k, q = len(columns), len(PROBS)
    limits = window(s, k)
    kw = dict(chain_len=1, predictor=False)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, **kw)
    selected = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, quantiles=PROBS, limits=limits, **kw)
    for _ in range(args.warmup):
        reduced.step()
        selected.step()
    torch.cuda.synchronize()
    values, status = selected.metric_local, selected.info_local[:, 32]
    reps = args.reps

    # (a) the pass alone
    sel = dp.select_ensemble(values, steps_per_geometry=s, status=status, probs=PROBS, limits=limits)
    one_select = lambda: dp.select_ensemble(values, steps_per_geometry=s, status=status, out=sel)  # noqa: E731
    for _ in range(5):
        one_select()
    select_runs = events(one_select, reps)
    select_us = statistics.median(select_runs)
    run = dp.select_prepare(s, k, PROBS, limits, rounds=True)
    n_rounds = dp.select_rounds
    per_round = []
    for _ in range(3):  # warm
        dp.select_begin(run)
        for rnd in range(n_rounds):
            dp.select_count(run, rnd, values, steps_per_geometry=s, status=status)
            dp.select_descend(run, rnd)
    torch.cuda.synchronize()
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * n_rounds + 1)] for _ in range(reps)]
    for rep in range(reps):
        dp.select_begin(run)
        marks[rep][0].record()
        for rnd in range(n_rounds):
            dp.select_count(run, rnd, values, steps_per_geometry=s, status=status)
            marks[rep][2 * rnd + 1].record()
            dp.select_descend(run, rnd)
            marks[rep][2 * rnd + 2].record()
        torch.cuda.synchronize()
    for rnd in range(n_rounds):
        per_round.append({"round": rnd,
                          "count_us": statistics.median(m[2 * rnd].elapsed_time(m[2 * rnd + 1]) * 1e3 for m in marks),
                          "descend_us": statistics.median(m[2 * rnd + 1].elapsed_time(m[2 * rnd + 2]) * 1e3 for m in marks)})
    dp.select_finish(run)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(run.order), torch.nan_to_num(sel.order)) and torch.equal(run.count, sel.count) and torch.equal(run.outside, sel.outside)

    # (b) the yardstick: okx_ensemble_reduce on the same table
    out = EnsembleAccumulator(torch.empty_like(reduced.local_accumulator.acc), reduced.local_accumulator.shift, None)
    one_reduce = lambda: dp.reduce_ensemble(values, steps_per_geometry=s, status=status, out=out)  # noqa: E731
    for _ in range(5):
        one_reduce()
    reduce_runs = events(one_reduce, reps)
    reduce_us = statistics.median(reduce_runs)

    # (c) what the user must otherwise do on one GPU
    copy_ms, host_ms = [], []
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = values.cpu()  # the copy alone: the table, without its status bytes
        t1 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        if rep >= 3:  # (the NumPy part is not what the condition is about: three runs of it)
            continue
        host_status = status.cpu()
        v = host.numpy().reshape(g, s, k)
        ok = ((host_status.numpy().reshape(g, s) & 7) == 1)[:, :, None] & np.isfinite(v)
        masked = np.where(ok, v, np.nan)
        band = np.nanquantile(masked, PROBS, axis=0, method="linear")
        below, above = (masked < limits[None, None, :, 0]).sum(axis=0), (masked > limits[None, None, :, 1]).sum(axis=0)
        host_ms.append((time.perf_counter() - t1) * 1e3)
    got = sel.finalize()
    want = select_host(v, host_status.numpy().reshape(g, s), PROBS, limits)
    exact = all(np.array_equal(getattr(got, f), getattr(want, f), equal_nan=True) for f in FIELDS)
    agree = bool(np.allclose(np.moveaxis(band, 0, 2), got.quantile, rtol=1e-12, atol=0, equal_nan=True)) and \
        bool(np.array_equal(below, got.below)) and bool(np.array_equal(above, got.above))

    # (d) the sharded ensemble's step with and without quantiles, alternated
    rounds = [(step_ms(reduced.step, args.steps), step_ms(selected.step, args.steps)) for _ in range(5)]
    off, on = statistics.median(r[0] for r in rounds), statistics.median(r[1] for r in rounds)

    table_bytes = 8 * g * s * k + g * s
    hist_bytes = 8 * run.hist.numel()
    copy = statistics.median(copy_ms)
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns, Q = {q} {list(PROBS)}, limits on, one GPU",
        "bits_per_round": 64 // n_rounds, "rounds": n_rounds, "histogram_bytes": hist_bytes,
        "a_select_pass_us": {"median": select_us, "runs": select_runs, "per_round": per_round,
                             "table_bytes_per_round": table_bytes, "hbm_floor_us": n_rounds * table_bytes / HBM_PEAK * 1e6},
        "b_reduce_pass_us": {"median": reduce_us, "runs": reduce_runs, "select_over_reduce": select_us / reduce_us},
        "c_host_path_ms": {"copy_alone_median": copy, "copy_runs": copy_ms, "numpy_quantile_and_limit_counts_median": statistics.median(host_ms),
                           "what": "metric_local.cpu() alone; then the status bytes' copy, numpy.nanquantile(method='linear') and the limit counts"},
        "condition_select_below_copy_alone": {"select_ms": select_us * 1e-3, "copy_ms": copy, "holds": bool(select_us * 1e-3 < copy)},
        "device_equals_select_host_exactly": bool(exact), "device_agrees_with_numpy_quantile": agree,
        "d_step_ms": {"reduce_only": off, "with_quantiles": on, "extra_ms": on - off, "extra_percent": (on / off - 1.0) * 100.0,
                      "rounds": rounds, "steps_per_round": args.steps},
        "select_exchange_bytes_per_rank_at_world_above_one": n_rounds * hist_bytes,
    }


def summary(r: dict) -> str:
    a, b, c, d = r["a_select_pass_us"], r["b_reduce_pass_us"], r["c_host_path_ms"], r["d_step_ms"]
    lines = [r["workload"], f"{r['bits_per_round']} bits per round, {r['rounds']} rounds, histogram {r['histogram_bytes']} B",
             f"(a) select pass      {a['median']:10.1f} us   (rounds x table bytes at the HBM peak: {a['hbm_floor_us']:.1f} us)"]
    lines += [f"      round {p['round']:2d}: count {p['count_us']:8.1f} us  descend {p['descend_us']:6.1f} us" for p in a["per_round"]]
    lines += [f"(b) reduce pass      {b['median']:10.1f} us   select / reduce = {b['select_over_reduce']:.2f}",
              f"(c) copy alone       {c['copy_alone_median'] * 1e3:10.1f} us   numpy.quantile + limit counts {c['numpy_quantile_and_limit_counts_median']:.1f} ms",
              f"    select below the copy alone: {r['condition_select_below_copy_alone']['holds']}",
              f"    device == select_host exactly: {r['device_equals_select_host_exactly']}; agrees with numpy.quantile: {r['device_agrees_with_numpy_quantile']}",
              f"(d) step             {d['reduce_only']:.3f} ms reduce only, {d['with_quantiles']:.3f} ms with quantiles (+{d['extra_ms']:.3f} ms, {d['extra_percent']:.1f} %)"]
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, steps=50, warmup=10, reps=20)
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
