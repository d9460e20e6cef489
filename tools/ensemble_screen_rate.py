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

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

sys.path.insert(0, os.path.join(REPO, "tools"))

from ensemble_reduce_rate import HBM_PEAK, build  # noqa: E402
from ensemble_select_rate import window  # noqa: E402

FIELDS = ("flags", "tally", "blame", "passed")


def rank_main(args) -> None:
    import numpy as np
    import torch
    import torch.distributed as dist

    from open_kinematics_amd.dist import ShardedEnsemble

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(args.port)
    dist.init_process_group("gloo", rank=args.rank, world_size=args.rehearse)
    device = torch.device("cuda:0")
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
    dist.barrier()
    dist.destroy_process_group()


def rehearse(args) -> int:
    port = 38500 + os.getpid() % 2000
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rehearse", str(args.rehearse), "--rank", str(r), "--port", str(port),
                               "--geometries", str(args.geometries), "--steps-per-geometry", str(args.steps_per_geometry), "--chunks", str(args.chunks),
                               "--limits", args.limits, "--out", args.out])
             for r in range(args.rehearse)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=args.timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            return 124
    return max(abs(c) for c in codes)


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

    def events(fn, n=reps):
        """Median and runs [us] of ``fn`` between device events, one pair per repetition."""
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out), out

    def spread(runs):
        q = statistics.quantiles(runs, n=4)
        return q[2] - q[0]

    # (a) the pass alone, (b) the yardsticks beside it - alternated block by block so that a drift hits all three alike
    scr = dp.screen_ensemble(values, steps_per_geometry=s, status=status, limits=limits, scale=scale)
    one_screen = lambda: dp.screen_ensemble(values, steps_per_geometry=s, status=status, out=scr)  # noqa: E731
    acc = EnsembleAccumulator(torch.empty_like(reduced.local_accumulator.acc), reduced.local_accumulator.shift, None)
    one_reduce = lambda: dp.reduce_ensemble(values, steps_per_geometry=s, status=status, out=acc)  # noqa: E731
    run = dp.select_prepare(s, k, (0.5,), limits, rounds=True)
    dp.select_begin(run)
    one_count = lambda: dp.select_count(run, 0, values, steps_per_geometry=s, status=status)  # noqa: E731
    for fn in (one_screen, one_reduce, one_count):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    runs = {"screen": [], "reduce": [], "count": []}
    for _ in range(4):
        for name, fn in (("screen", one_screen), ("reduce", one_reduce), ("count", one_count)):
            runs[name] += events(fn, max(1, reps // 4))[1]
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
    def step_ms(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", type=int, default=4096)
    ap.add_argument("--steps-per-geometry", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", type=int, default=0)
    ap.add_argument("--rank", type=int, default=-1)
    ap.add_argument("--port", type=int, default=0)
    ap.add_argument("--chunks", type=int, default=0)
    ap.add_argument("--limits", default="")
    ap.add_argument("--timeout", type=float, default=500.0)
    args = ap.parse_args()
    if args.rehearse and args.rank >= 0:
        rank_main(args)
        return 0
    if args.rehearse:
        return rehearse(args)
    result = measure(args)
    text = json.dumps(result, indent=1)
    print(text)
    print(summary(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")
        with open(os.path.splitext(args.out)[0] + ".txt", "w", encoding="utf-8") as fh:
            fh.write(summary(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
